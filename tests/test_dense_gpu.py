"""Device dense <-> sparse — csr_from_dense / csc_from_dense, assign_to_dense / to_dense, csmat_binop_dense_raw with the add and
mul closures, `&A + &D` (sprs/src/sparse/csmat.rs:499-549, to_dense.rs, binop.rs:273-433, csmat.rs:1951-1987) — bit for bit
against tests/dense_ref.py: every comparison is on uint64 views, no tolerance anywhere.

The small cases also run against the kernel emulator (tests/test_dense_emu_cpu.py); the large and the torch cases need a real
device."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import dense_ref as R
from conftest import IDX_COMBOS, ROOT
from helpers import fresh_blocks, ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
CSR, CSC = R.CSR, R.CSC
WIDTHS = IDX_COMBOS + [(np.uint64, np.uint32), (np.uint16, np.uint16)]
COMBOS = [(CSR, False), (CSR, True), (CSC, False), (CSC, True)]        # (storage, column-major dense)
NAN_PAYLOAD = 0x7FF8000000ABCDEF
SENTINEL = 0x7FF4DEADBEEF0001                                          # a NaN no computation produces


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "dense_fixtures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tile():
    import sprs_amd
    return int(sprs_amd.get_option("dense_tile"))


def f64(bits_):
    return np.array([bits_], dtype=np.uint64).view(np.float64)[0]


def fmat(d):
    return R.mat(d["storage"], d["shape"], d["indptr"], d["indices"], d["data"])


def eye(dim, storage=CSR):
    return R.mat(storage, (dim, dim), list(range(dim + 1)), list(range(dim)), [1.0] * dim)


def dev(m, idx=np.uint64, ptr=np.uint64, validate=True):
    from sprs_amd.device import DeviceCsMat
    m = R.to_owned(m)
    return DeviceCsMat.from_host(m[1], m[2].astype(ptr), m[3].astype(idx), m[4], storage=m[0], validate=validate)


def host(res):
    shape, ip, ix, dt = res.to_host()
    return (res.storage(), shape, ip, ix, dt)


def dmat(arr, col_major=False, pad=None, fill=0.0):
    """the array on the device; pad: extra elements behind every line, holding `fill`"""
    from sprs_amd.prod import DeviceMat
    arr = np.asarray(arr, dtype=np.float64)
    if pad is None:
        return DeviceMat.from_host(arr, col_major)
    width = arr.shape[0] if col_major else arr.shape[1]
    return DeviceMat.from_host(arr, col_major, ld=width + pad, fill=fill)


def padding(d):
    """the elements of a padded DeviceMat that are not its matrix, as bits"""
    lines, width = (d.cols, d.rows) if d.col_major else (d.rows, d.cols)
    return d.vec.to_host().view(np.uint64).reshape(lines, d.ld)[:, width:]


def check_cs(res, want):
    got = host(res)
    assert R.same_mat(got, want)
    assert int(got[2][0]) == 0 and int(got[2][-1]) == got[3].size == got[4].size == res.nnz()   # a proper indptr, exact nnz


def from_dense(d, eps, storage, idx=np.uint64, ptr=np.uint64, stream=None):
    from sprs_amd.device import DeviceCsMat
    fresh_blocks()
    f = DeviceCsMat.csr_from_dense if storage == CSR else DeviceCsMat.csc_from_dense
    return f(d, eps, idx, ptr, stream)


def special_dense(shape, seed, eps=1e-5, kept=0.3):
    """a fraction `kept` of ordinary values, the rest 0.0, and -0.0, NaN, +-inf, the smallest denormal and +-eps among them"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(shape)
    m[rng.random(shape) >= kept] = 0.0
    for v in (-0.0, np.nan, f64(NAN_PAYLOAD), np.inf, -np.inf, 5e-324, eps, -eps):
        m[rng.random(shape) < 0.03] = v
    return m


# ---- from_dense ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_from_dense_golden(fx, storage, colmaj, idx, ptr):
    """test_csr_from_dense / test_csc_from_dense (csmat.rs:2494-2540), every layout and width pair"""
    c = fx["from_dense"]
    res = from_dense(dmat(np.eye(c["eye_dim"]), colmaj), c["eye_epsilon"], storage, idx, ptr)
    check_cs(res, eye(c["eye_dim"], storage))
    res = from_dense(dmat(np.array(c["m"]), colmaj), c["epsilon"], storage, idx, ptr)
    check_cs(res, fmat(c["csr_expected" if storage == CSR else "csc_expected"]))
    assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize


def shapes(tile):
    return [(1, 3 * tile + 1), (3 * tile + 1, 1), (7, (tile // 7) | 1), (0, 5), (5, 0), (4, tile // 2)]


@pytest.mark.parametrize("storage,colmaj", COMBOS)
@pytest.mark.parametrize("which", range(6))
def test_from_dense_shapes(tile, which, storage, colmaj):
    """one line of 3T + 1, 3T + 1 lines of one, odd widths, no rows, no columns, lines that end on tile edges; specials among
    the values"""
    shape = shapes(tile)[which]
    m = special_dense(shape, which)
    check_cs(from_dense(dmat(m, colmaj), 1e-5, storage), R.from_dense_vec(m, 1e-5, storage))


@pytest.mark.parametrize("epsilon", [0.0, -1.0, float("nan"), 1e-5, float("inf")])
def test_from_dense_epsilons(tile, epsilon):
    m = special_dense((5, tile // 2 + 3), 7)
    for storage, colmaj in COMBOS[:3]:
        want = R.from_dense_vec(m, epsilon, storage)
        check_cs(from_dense(dmat(m, colmaj), epsilon, storage), want)
        assert not np.isnan(want[4]).any() and (np.abs(want[4]) > R.clamp(epsilon)).all()


@pytest.mark.parametrize("fill", [f64(NAN_PAYLOAD), 1e300])
@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_from_dense_padding_is_not_read(tile, storage, colmaj, fill):
    """ld = width + 3 (odd lines start on 8-byte boundaries): nothing of the padding reaches the result"""
    for shape in ((9, tile // 4 + 1), (6, tile // 3)):
        m = special_dense(shape, 11)
        res = from_dense(dmat(m, colmaj, pad=3, fill=fill), 1e-5, storage)
        check_cs(res, R.from_dense_vec(m, 1e-5, storage))
        assert not (host(res)[4].view(np.uint64) == np.float64(fill).view(np.uint64)).any()


@pytest.mark.parametrize("storage,colmaj", [(CSR, False), (CSC, True), (CSR, True)])
def test_from_dense_kept_patterns(tile, storage, colmaj):
    """nothing kept, everything kept, only the last element of every tile and the first of the next"""
    shape = (3, tile + 7)
    n = shape[0] * shape[1]
    for kind in ("none", "all", "edges"):
        flat = np.zeros(n)
        if kind == "all":
            flat[:] = np.arange(1, n + 1)
        if kind == "edges":
            e = np.arange(tile, n, tile)
            flat[e - 1] = -(e - 1.0)
            flat[e] = e
        m = flat.reshape((shape[1], shape[0])).T if colmaj else flat.reshape(shape)      # flat is the device's element order
        want = R.from_dense_vec(m, 0.0, storage)
        check_cs(from_dense(dmat(m, colmaj), 0.0, storage), want)
        assert R.nnz(want) == {"none": 0, "all": n, "edges": 2 * ((n - 1) // tile)}[kind]


def test_from_dense_run_of_empty_lines(tile):
    """2T + 5 lines without a kept element, then one full line"""
    m = np.zeros((2 * tile + 6, 3))
    m[-1, :] = (1.0, -2.0, 3.0)
    m[3, 1] = -0.0
    for storage, colmaj in ((CSR, False), (CSC, False)):
        check_cs(from_dense(dmat(m, colmaj), 0.0, storage), R.from_dense_vec(m, 0.0, storage))
    mt = np.ascontiguousarray(m.T)
    check_cs(from_dense(dmat(mt, True), 0.0, CSC), R.from_dense_vec(mt, 0.0, CSC))


@pytest.mark.parametrize("storage,colmaj", [(CSR, False), (CSR, True)])
def test_from_dense_index_overflow(storage, colmaj):
    """u16 indices: a kept column 3 of 70000 is fine, a kept column 69999 is where I::from_usize panics"""
    from sprs_amd import _ffi
    m = np.zeros((1, 70000))
    m[0, 3] = 2.5
    res = from_dense(dmat(m, colmaj), 0.0, storage, np.uint16, np.uint16)
    check_cs(res, R.from_dense_vec(m, 0.0, storage))
    assert res.index_bytes() == 2
    m[0, 69999] = 1.0
    with pytest.raises(_ffi.SprsHipError) as e:
        from_dense(dmat(m, colmaj), 0.0, storage, np.uint16, np.uint16)
    assert e.value.status == _ffi.INDEX_OVERFLOW
    check_cs(from_dense(dmat(m, colmaj), 0.0, storage, np.uint32, np.uint16), R.from_dense_vec(m, 0.0, storage))


def test_from_dense_nnz_overflow():
    """u16 indptr: 65535 kept elements fit, 65536 do not (Iptr::from_usize)"""
    from sprs_amd import _ffi
    m = np.ones((2, 32768))
    with pytest.raises(_ffi.SprsHipError) as e:
        from_dense(dmat(m), 0.0, CSR, np.uint16, np.uint16)
    assert e.value.status == _ffi.INDEX_OVERFLOW
    m[1, 5] = 0.0
    check_cs(from_dense(dmat(m), 0.0, CSR, np.uint16, np.uint16), R.from_dense_vec(m, 0.0, CSR))


# ---- assign_to_dense / to_dense ------------------------------------------------------------------------------------------------

def edge_matrix(tile, storage, seed=3):
    """rows: one that ends on a tile edge, one that spans three tiles, runs of empty ones; -0.0 and a NaN payload stored"""
    lens = [5, 0, 0, 0, tile - 5, 0, 2 * tile + 10] + [0] * 12 + [7, 0, 3]
    shape, ip, ix, dt = ragged_csr(np.asarray(lens, dtype=np.int64), 2 * tile + 16, seed=seed, positive=False)
    dt = np.array(dt)
    dt[::97] = -0.0
    dt[5::211] = f64(NAN_PAYLOAD)
    dt[7::389] = np.inf
    m = R.mat(CSR, shape, ip, ix, dt)
    return m if storage == CSR else R.transpose(m)


def sentinel_mat(shape, colmaj, pad):
    s = f64(SENTINEL)
    return dmat(np.full(shape, s), colmaj, pad=pad, fill=s)


def all_sentinel(bits_):
    return (np.asarray(bits_) == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_to_dense_golden(fx, storage, colmaj):
    """to_dense.rs:56-92"""
    from sprs_amd import to_dense
    c = fx["to_dense"]
    out = dmat(np.zeros((3, 3)), colmaj)
    to_dense.assign_to_dense(out, dev(eye(3, storage)))
    assert R.same_dense(out.to_host(), np.eye(3))
    for name in ("mat1", "mat3"):
        m = fmat(fx[name])
        m = m if storage == CSR else R.to_other_storage(m)
        want = np.array(c[name + "_expected"])
        assert R.same_dense(dev(m).to_dense().to_host(), want)
        out = sentinel_mat(m[1], colmaj, 2)
        dev(m).to_dense(out=out)
        assert R.same_dense(out.to_host(), want) and all_sentinel(padding(out))


@pytest.mark.parametrize("idx,ptr", [WIDTHS[0], WIDTHS[2], WIDTHS[4]])
@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_assign_and_to_dense_at_tile_edges(tile, storage, colmaj, idx, ptr):
    from sprs_amd import to_dense
    m = edge_matrix(tile, storage)
    if idx == np.uint16:
        m = edge_matrix(64, storage)                 # (indices below 2^16)
    d = dev(m, idx, ptr)
    for pad in (None, 3):
        out = sentinel_mat(m[1], colmaj, pad)
        to_dense.assign_to_dense(out, d)
        want = R.assign_to_dense_vec(np.full(m[1], f64(SENTINEL)), m)
        assert R.same_dense(out.to_host(), want)     # stored positions hold the value's bits, every other one the sentinel
        assert pad is None or all_sentinel(padding(out))
        out = sentinel_mat(m[1], colmaj, pad)
        to_dense.to_dense(d, out)
        assert R.same_dense(out.to_host(), R.to_dense_vec(m))
        assert pad is None or all_sentinel(padding(out))
    got = d.to_dense()
    assert not got.col_major and R.same_dense(got.to_host(), R.to_dense_vec(m))


@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_assign_unchecked_index_stays_inside(storage, colmaj):
    """an unchecked handle whose last slice holds an inner index above the inner dimension: the entry is skipped, a guard region
    behind the array and every non-stored element stay as they were"""
    from sprs_amd import to_dense
    from sprs_amd.device import DeviceVec
    from sprs_amd.prod import DeviceMat
    good = R.mat(storage, (4, 4), [0, 1, 2, 3, 5], [1, 0, 3, 2, 3], [1.0, 2.0, 3.0, 4.0, 5.0])
    bad = R.mat(storage, (4, 4), good[2], [1, 0, 3, 2, 6], good[4])
    want = R.assign_to_dense_vec(np.full((4, 4), f64(SENTINEL)), R.mat(storage, (4, 4), [0, 1, 2, 3, 4], [1, 0, 3, 2], good[4][:4]))
    guard = 64
    for zero_first in (False, True):
        big = DeviceVec.from_host(np.full(16 + guard, f64(SENTINEL)))
        out = DeviceMat(4, 4, DeviceVec(16, ptr=big.ptr, owner=big), colmaj)
        (to_dense.to_dense if zero_first else lambda d, o: to_dense.assign_to_dense(o, d))(dev(bad, validate=False), out)
        after = big.to_host()
        assert all_sentinel(after[16:].view(np.uint64))
        exp = want.copy()
        if zero_first:
            exp.view(np.uint64)[exp.view(np.uint64) == np.uint64(SENTINEL)] = 0
        assert R.same_dense(out.to_host(), exp)


def test_to_dense_dimension_mismatch():
    from sprs_amd import _ffi
    d, out = dev(eye(3)), dmat(np.zeros((3, 4)))
    for f in (_ffi.lib.sprs_hip_csmat_assign_to_dense_f64, _ffi.lib.sprs_hip_csmat_to_dense_f64):
        assert f(d._h, C.c_void_p(out.vec.ptr), 3, 4, out.layout, 4, None) == _ffi.DIM_MISMATCH
        assert _ffi.lib.sprs_hip_last_error() == b"Dimension mismatch"
        assert f(d._h, C.c_void_p(out.vec.ptr), 4, 3, out.layout, 4, None) == _ffi.DIM_MISMATCH


# ---- binop_dense -----------------------------------------------------------------------------------------------------------------

ADD_COEFFS = [(1.0, 1.0), (-1.0, 1.0), (2.5, -0.5), (0.0, 1.0), (float("inf"), 1.0)]
MUL_COEFFS = [1.0, -1.0, 0.0, float("inf")]


def rhs_for(shape, seed):
    """-0.0, inf and ONE NaN payload among ordinary values"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal(shape)
    r[rng.random(shape) < 0.1] = -0.0
    r[rng.random(shape) < 0.05] = np.inf
    r[rng.random(shape) < 0.03] = -np.inf
    r[shape[0] // 2, shape[1] // 3] = f64(NAN_PAYLOAD)
    return r


def check_binop(got, lhs, rhs, op, alpha, beta):
    """bits, except where the NaNs of both operand chains meet: there only `is NaN`"""
    want = R.binop_dense_vec(lhs, rhs, op, alpha, beta)
    with np.errstate(invalid="ignore"):
        chain_l = np.float64(alpha) * R.to_dense_vec(lhs)
        chain_r = np.float64(beta) * rhs if op == R.ADD else rhs
    both = np.isnan(chain_l) & np.isnan(chain_r)
    assert got.shape == want.shape
    assert np.array_equal(R.bits(got)[~both], R.bits(want)[~both])
    assert np.isnan(got[both]).all()


def run_binop(lhs, rhs, op, alpha, beta, pad_r=None, pad_o=None, d=None):
    from sprs_amd import binop
    colmaj = lhs[0] == CSC
    out = sentinel_mat(lhs[1], colmaj, pad_o)
    binop.csmat_binop_dense_raw(d if d is not None else dev(lhs), dmat(rhs, colmaj, pad=pad_r, fill=f64(SENTINEL)), op, out, alpha, beta)
    assert pad_o is None or all_sentinel(padding(out))
    return out.to_host()


def test_binop_dense_golden(fx):
    """csr_add_dense_rowmaj, csr_mul_dense_rowmaj, binop_standard_layouts (binop.rs:600-690)"""
    from sprs_amd import binop
    c = fx["csr_add_dense_rowmaj"]
    got = binop.add_dense_mat_same_ordering(dev(eye(3)), dmat(np.zeros((3, 3))), c["alpha"], c["beta"])
    assert R.same_dense(got.to_host(), np.eye(3))
    want = np.array(c["mat1_plus_mat_dense1"])
    a, b = dev(fmat(fx["mat1"])), dmat(np.array(fx["mat_dense1"]))
    assert R.same_dense(binop.add_dense_mat_same_ordering(a, b, 1.0, 1.0).to_host(), want)
    assert R.same_dense((a + b).to_host(), want)
    got = binop.mul_dense_mat_same_ordering(dev(eye(3)), dmat(np.ones((3, 3))), fx["csr_mul_dense_rowmaj"]["alpha"])
    assert R.same_dense(got.to_host(), np.eye(3)) and not got.col_major
    c = fx["binop_standard_layouts"]
    for pair in c["pairs"]:
        shape = tuple(c["shape"])
        outer = shape[0] if pair["storage"] == CSR else shape[1]
        zero = R.mat(pair["storage"], shape, [0] * (outer + 1), [], [])
        colmaj = pair["order"] == "F"
        got = binop.mul_dense_mat_same_ordering(dev(zero), dmat(np.full(shape, c["rhs_fill"]), colmaj), 1.0)
        assert got.col_major == colmaj and R.same_dense(got.to_host(), np.zeros(shape))


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_binop_dense_coefficients_and_specials(storage):
    lhs = R.from_dense(special_dense((13, 37), 21, kept=0.4), 0.0, storage)
    lhs = (lhs[0], lhs[1], lhs[2], lhs[3], np.where(np.arange(lhs[4].size) % 7 == 0, -0.0, lhs[4]))
    lhs[4][3] = f64(NAN_PAYLOAD ^ 0x1100)
    rhs = rhs_for((13, 37), 22)
    d = dev(lhs)
    for alpha, beta in ADD_COEFFS:
        check_binop(run_binop(lhs, rhs, R.ADD, alpha, beta, d=d), lhs, rhs, R.ADD, alpha, beta)
    for alpha in MUL_COEFFS:
        check_binop(run_binop(lhs, rhs, R.MUL, alpha, 1.0, d=d), lhs, rhs, R.MUL, alpha, 1.0)
        check_binop(run_binop(lhs, rhs, R.MUL, alpha, float("nan"), d=d), lhs, rhs, R.MUL, alpha, 1.0)     # beta is ignored


def test_binop_dense_performs_the_operation_on_zeros():
    z = R.mat(CSR, (2, 3), [0, 0, 1], [1], [0.0])
    r = np.array([[-0.0, np.inf, 1.0], [-0.0, -0.0, -np.inf]])
    got = run_binop(z, r, R.ADD, -1.0, 1.0)
    assert R.bits(got)[0, 0] == 0x8000000000000000 and R.bits(got)[1, 1] == 0x8000000000000000     # -1 * 0 + 1 * (-0.0) = -0.0
    got = run_binop(z, r, R.ADD, 1.0, 1.0)
    assert R.bits(got)[0, 0] == 0 and R.bits(got)[1, 1] == 0
    got = run_binop(z, r, R.MUL, 1.0, 1.0)
    assert np.isnan(got[0, 1]) and np.isnan(got[1, 2]) and R.bits(got)[0, 0] == 0x8000000000000000
    check_binop(got, z, r, R.MUL, 1.0, 1.0)


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("pad_r,pad_o", [(3, 5), (2, None), (None, 1)])
def test_binop_dense_padded_at_tile_edges(tile, storage, pad_r, pad_o):
    """the tile-edge matrix; ld and out_ld padded and unequal; out's padding keeps its sentinel (run_binop)"""
    lhs = edge_matrix(tile, storage, seed=5)
    rhs = rhs_for(lhs[1], 31)
    check_binop(run_binop(lhs, rhs, R.ADD, 2.5, -0.5, pad_r, pad_o), lhs, rhs, R.ADD, 2.5, -0.5)
    check_binop(run_binop(lhs, rhs, R.MUL, -1.0, 1.0, pad_r, pad_o), lhs, rhs, R.MUL, -1.0, 1.0)


def _rne(x):
    return float(x)       # Fraction -> float rounds to nearest even


def test_binop_dense_is_unfused():
    """an element where fma(alpha, l, beta * r) and fma(beta, r, alpha * l) both differ from (alpha * l) + (beta * r)"""
    rng = np.random.default_rng(5)
    alpha, beta = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -29
    found = None
    for _ in range(10000):
        l, r = float(rng.standard_normal()), float(rng.standard_normal())
        unfused = alpha * l + beta * r
        f1 = _rne(Fraction(alpha) * Fraction(l) + Fraction(beta * r))
        f2 = _rne(Fraction(beta) * Fraction(r) + Fraction(alpha * l))
        if f1 != unfused and f2 != unfused:
            found = (l, r, unfused, f1, f2)
            break
    assert found is not None
    l, r, unfused, f1, f2 = found
    assert np.float64(f1).view(np.uint64) != np.float64(unfused).view(np.uint64) != np.float64(f2).view(np.uint64)
    lhs = R.mat(CSR, (2, 3), [0, 1, 2], [2, 0], [l, l])
    rhs = np.full((2, 3), r)
    got = run_binop(lhs, rhs, R.ADD, alpha, beta)
    assert R.bits(got)[0, 2] == np.float64(unfused).view(np.uint64) == R.bits(got)[1, 0]
    check_binop(got, lhs, rhs, R.ADD, alpha, beta)


def test_binop_dense_contract():
    """dimensions, then storage against layout, then aliasing — at the C boundary"""
    from sprs_amd import _ffi
    f = _ffi.lib.sprs_hip_csmat_binop_dense_f64
    d = dev(R.from_dense(np.eye(3, 5), 0.0, CSR))
    rhs, out = dmat(np.ones((3, 5))), dmat(np.zeros((3, 5)))
    rp, op_ = C.c_void_p(rhs.vec.ptr), C.c_void_p(out.vec.ptr)
    assert f(d._h, rp, 5, 3, _ffi.COL_MAJOR, 5, _ffi.BINOP_ADD, 1.0, 1.0, op_, 5, None) == _ffi.DIM_MISMATCH      # both wrong
    assert _ffi.lib.sprs_hip_last_error() == b"Dimension mismatch"
    assert f(d._h, rp, 3, 5, _ffi.COL_MAJOR, 3, _ffi.BINOP_ADD, 1.0, 1.0, op_, 3, None) == _ffi.STORAGE_MISMATCH
    assert _ffi.lib.sprs_hip_last_error() == b"Storage mismatch"
    assert f(d._h, rp, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_MUL, 1.0, 1.0, rp, 5, None) == _ffi.INVALID_ARG          # out == rhs
    assert b"overlaps" in _ffi.lib.sprs_hip_last_error()
    assert f(d._h, rp, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_MUL, 1.0, 1.0, C.c_void_p(rhs.vec.ptr + 8 * 14), 5, None) == _ffi.INVALID_ARG
    assert f(d._h, rp, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_ADD, 1.0, 1.0, op_, 5, None) == _ffi.OK
    assert R.same_dense(out.to_host(), np.ones((3, 5)) + np.eye(3, 5))


# ---- `&A + &D` -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage,colmaj", COMBOS)
def test_add_operator(tile, storage, colmaj):
    lhs = R.from_dense(special_dense((11, tile // 8 + 5), 41, kept=0.3), 0.0, storage)
    rhs = rhs_for(lhs[1], 42)
    free = np.argwhere(R.to_dense_vec(lhs) == 0)[0]
    rhs[tuple(free)] = -0.0                          # -0.0 where lhs stores nothing: 1 * 0 + 1 * (-0.0) = +0.0
    for pad in (None, 3):
        got = dev(lhs) + dmat(rhs, colmaj, pad=pad, fill=f64(SENTINEL))
        assert got.col_major == colmaj and got.ld == (lhs[1][0] if colmaj else lhs[1][1])
        want = R.add_dense(lhs, np.array(rhs, order="F" if colmaj else "C"), "F" if colmaj else "C")
        both = np.isnan(R.to_dense_vec(lhs)) & np.isnan(rhs)
        assert np.array_equal(R.bits(got.to_host())[~both], R.bits(want)[~both]) and np.isnan(got.to_host()[both]).all()
        assert R.bits(got.to_host())[tuple(free)] == 0


# ---- device-only cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_large_3001_by_4099():
    """1 % kept; all five entries against the numpy twins"""
    from sprs_amd import binop, to_dense
    rng = np.random.default_rng(77)
    shape = (3001, 4099)
    m = rng.standard_normal(shape)
    m[rng.random(shape) >= 0.01] = 0.0
    rhs = rng.standard_normal(shape)
    for storage, colmaj in COMBOS:
        want = R.from_dense_vec(m, 0.0, storage)
        a = from_dense(dmat(m, colmaj), 0.0, storage, np.uint32, np.uint64)
        check_cs(a, want)
        assert R.same_dense(a.to_dense().to_host(), m)
        out = sentinel_mat(shape, colmaj, 1)
        to_dense.assign_to_dense(out, a)
        assert R.same_dense(out.to_host(), R.assign_to_dense_vec(np.full(shape, f64(SENTINEL)), want))
        assert R.same_dense((a + dmat(rhs, colmaj)).to_host(), R.binop_dense_vec(want, rhs, R.ADD, 1.0, 1.0))
        if (storage == CSR) != colmaj:
            got = binop.add_dense_mat_same_ordering(a, dmat(rhs, colmaj, pad=1), 2.5, -0.5)
            assert R.same_dense(got.to_host(), R.binop_dense_vec(want, rhs, R.ADD, 2.5, -0.5))
            got = binop.mul_dense_mat_same_ordering(a, dmat(rhs, colmaj), -3.0)
            assert R.same_dense(got.to_host(), R.binop_dense_vec(want, rhs, R.MUL, -3.0))


@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_non_blocking_stream(tile):
    """the dense operand is a torch tensor written on a non-blocking stream and used there with no host synchronise in between"""
    import torch
    from sprs_amd import binop
    from sprs_amd.device import DeviceVec
    from sprs_amd.prod import DeviceMat
    m = special_dense((37, tile // 4 + 3), 91)
    devc = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=devc)
    with torch.cuda.stream(s):
        t = torch.zeros(m.size, dtype=torch.float64, device=devc)
        o = torch.zeros(m.size, dtype=torch.float64, device=devc)
        torch.cuda._sleep(20_000_000)                # keep the stream busy: the copy below lands late
        t.copy_(torch.from_numpy(m.reshape(-1)).to(devc, non_blocking=True))
        d = DeviceMat(m.shape[0], m.shape[1], DeviceVec.borrow(t))
        a = from_dense(d, 1e-5, CSR, stream=s)
        back = a.to_dense(out=DeviceMat(m.shape[0], m.shape[1], DeviceVec.borrow(o)), stream=s)
        total = binop.add_dense_mat_same_ordering(a, back, 1.0, 1.0, stream=s)
        s.synchronize()
    want = R.from_dense_vec(m, 1e-5, CSR)
    check_cs(a, want)
    assert R.same_dense(o.cpu().numpy().reshape(m.shape), R.to_dense_vec(want))
    assert R.same_dense(total.to_host(), R.binop_dense_vec(want, R.to_dense_vec(want), R.ADD, 1.0, 1.0))
