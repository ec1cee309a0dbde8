"""GPU parity tests of the f32 triangular solves (sprs_hip_trisolve_f32 behind the four *_dense_rhs functions of sprs_amd.linalg on
a DeviceCsMatF32) against the np.float32 restatement tests/f32_solve_ref.py: every solution bit for bit (np.array_equal on the
float32 arrays), the level counts, the singular reports and the asserts as errors.  The systems are those of
tests/test_trisolve_gpu.py and tests/test_trisolve_seams_gpu.py with data and b cast to f32; what is new is that the bits must be
those of f32 ARITHMETIC (an f64 solve rounded at the end gives other bits) and that values are handed over as 4-byte words.
(tests/test_solve_f32_emu_cpu.py runs this file through the CPU emulator of the kernels as well.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import f32_solve_ref as ref
import trisolve_ref as ref64
from test_gauss_seidel_gpu import _random_system
from test_trisolve_gpu import EMU, KINDS, _singular_system, arrays, gpu_fn
from test_trisolve_seams_gpu import BLOCK, _cus, _without, block_system, level_positions

pytestmark = pytest.mark.gpu

F = np.float32
ALL_ONES_F32 = np.frombuffer(np.uint32(0xFFFFFFFF).tobytes(), dtype=np.float32)[0]


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    if not hasattr(sprs_amd._ffi.lib, "sprs_hip_trisolve_f32"):
        pytest.fail("the library has no sprs_hip_trisolve_f32")
    return sprs_amd


def arrays32(a, kind):
    ip, ix, dt = arrays(a, kind)
    return ip, ix, dt.astype(np.float32)


def device_mat(kind, n, ip, ix, dt, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMatF32, CSC, CSR
    assert dt.dtype == np.float32
    return DeviceCsMatF32.from_host((n, n), ip.astype(ptr), ix.astype(idx), dt, storage=CSC if kind.endswith("csc") else CSR)


def gpu_solve(kind, n, ip, ix, dt, b, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceVecF32
    assert b.dtype == np.float32
    a = device_mat(kind, n, ip, ix, dt, idx, ptr)
    x = DeviceVecF32.from_host(b)
    res = gpu_fn(kind)(a, x)
    out = x.to_host()
    assert out.dtype == np.float32
    return out, res


def same_bits(x, y):
    return x.dtype == y.dtype == np.float32 and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def check_against_restatement(kind, a, b, idx=np.uint64, ptr=np.uint64):
    n = a.shape[0]
    ip, ix, dt = arrays32(a, kind)
    b = b.astype(np.float32)
    x_ref = ref.SOLVES[kind](n, ip, ix, dt, b)
    assert np.isfinite(x_ref).all()
    x, res = gpu_solve(kind, n, ip, ix, dt, b, idx, ptr)
    assert np.array_equal(x, x_ref)
    assert res.levels == ref.levels(kind, n, ip, ix)
    return x


def f64_then_cast(kind, a, b):
    """the f64 solve of the SAME f32-valued system, rounded to f32 at the end: what a to_f64() detour would give"""
    ip, ix, dt = arrays32(a, kind)
    return ref64.SOLVES[kind](a.shape[0], ip, ix, dt.astype(np.float64), b.astype(np.float32).astype(np.float64)).astype(np.float32)


def test_golden_systems(hip):
    """the reference's own unit tests (trisolve.rs:368-442) cast to f32: small integers and halves, exact in f32 too"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trisolve_fixtures.json")
    systems = json.load(open(path))["systems"]
    assert sorted(s["solve"] for s in systems) == sorted(KINDS)
    for s in systems:
        n = s["shape"][0]
        ip, ix = np.array(s["indptr"], dtype=np.uint64), np.array(s["indices"], dtype=np.uint64)
        dt, b = np.array(s["data"], dtype=np.float32), np.array(s["b"], dtype=np.float32)
        want = np.array(s["x"], dtype=np.float32)
        assert np.array_equal(ref.SOLVES[s["solve"]](n, ip, ix, dt, b), want), s["solve"]      # the restatement first, on the CPU
        x, _ = gpu_solve(s["solve"], n, ip, ix, dt, b)
        assert np.array_equal(x, want), s["solve"]


SIZES = (1, 63, 64, 65, 500)


def _system(n):
    a = _random_system(n, 11 + n, 0 if n == 1 else 4, 100 if n == 500 else 0)
    return a, np.random.default_rng(n).standard_normal(n)


def _cases():
    out = []
    for kind in KINDS:
        for n in SIZES:
            widths = [(np.uint64, np.uint64)] + ([(np.uint32, np.uint64), (np.uint32, np.uint32)] if n == 65 else [])
            for idx, ptr in widths:
                out.append(pytest.param(kind, n, idx, ptr, id="%s-%d-%s-%s" % (kind, n, np.dtype(idx).name, np.dtype(ptr).name)))
    return out


@pytest.mark.parametrize("kind,n,idx,ptr", _cases())
def test_random_systems(hip, kind, n, idx, ptr):
    """full non-symmetric matrices: the other triangle is there and must be ignored; at n = 500 row n // 2 has more than one
    batch of eight on both sides of the diagonal"""
    a, b = _system(n)
    if n == 500:
        row = a.indices[a.indptr[n // 2]:a.indptr[n // 2 + 1]]
        assert (row < n // 2).sum() > 8 and (row > n // 2).sum() > 8
    check_against_restatement(kind, a, b, idx, ptr)


def test_the_arithmetic_is_f32(hip):
    """on at least one of the random systems the f32 chain and the f64 chain rounded at the end differ in bits (CPU), and the
    device gives the f32 chain's"""
    differing = []
    for kind in KINDS:
        for n in SIZES:
            a, b = _system(n)
            ip, ix, dt = arrays32(a, kind)
            if not same_bits(ref.SOLVES[kind](n, ip, ix, dt, b.astype(np.float32)), f64_then_cast(kind, a, b)):
                differing.append((kind, n))
    assert differing, "every f32 solve equals the rounded f64 solve: these systems cannot tell the two apart"
    kind, n = differing[-1]
    a, b = _system(n)
    x = check_against_restatement(kind, a, b)
    assert not same_bits(x, f64_then_cast(kind, a, b))


def test_walk_direction(hip):
    """usolve_csr subtracts row r's products by ascending column, usolve_csc by descending column: one matrix, two bit patterns"""
    n = 70
    a = _random_system(n, 3, 4)
    b = np.random.default_rng(n).standard_normal(n)
    got = {kind: check_against_restatement(kind, a, b) for kind in ("usolve_csr", "usolve_csc")}
    assert not same_bits(got["usolve_csr"], got["usolve_csc"])
    assert np.allclose(got["usolve_csr"], got["usolve_csc"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("kind", ["lsolve_csr", "usolve_csr"])
def test_bidiagonal_chain(hip, kind):
    """every unknown waits for its neighbour: n levels, hand-offs between ADJACENT 4-byte words inside a wave and across waves"""
    import scipy.sparse as sp
    n = 200
    a = (sp.diags(np.full(n, 2.0)) + sp.diags(np.full(n - 1, -1.0), -1 if kind[0] == "l" else 1)).tocsr()
    ip, ix, dt = arrays32(a, kind)
    b = np.arange(1, n + 1, dtype=np.float32)
    x, res = gpu_solve(kind, n, ip, ix, dt, b)
    assert res.levels == n
    assert np.array_equal(x, ref.SOLVES[kind](n, ip, ix, dt, b))


@pytest.mark.parametrize("kind", KINDS)
def test_dense_triangle(hip, kind):
    """rows of up to 130 entries (17 batches of eight), every unknown its own level"""
    import scipy.sparse as sp
    n = 130
    rng = np.random.default_rng(130)
    d = rng.uniform(-1.0, 1.0, (n, n))
    d = np.tril(d) if kind[0] == "l" else np.triu(d)
    d[np.arange(n), np.arange(n)] = np.abs(d).sum(axis=1) + 1.0
    check_against_restatement(kind, sp.csr_matrix(d), rng.standard_normal(n))
    ip, ix, _ = arrays(sp.csr_matrix(d), kind)
    assert ref.levels(kind, n, ip, ix) == n


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_nan_in_rhs(hip, kind):
    """b[100] is the f32 NaN that memset 0xFF leaves (0xFFFFFFFF): unknown 100 publishes it, and the unknowns that wait for it
    must see a value, not "pending" (without the substitution the spin guard ends the call with an error)"""
    n, at = 200, 100
    a = block_system(n, 200)
    ip, ix, dt = arrays32(a, kind)
    b = np.random.default_rng(201).standard_normal(n).astype(np.float32)
    b[at] = ALL_ONES_F32
    assert b.view(np.uint32)[at] == 2**32 - 1
    x_ref = ref.SOLVES[kind](n, ip, ix, dt, b)
    nans = np.isnan(x_ref)
    assert nans[at] and 1 < nans.sum() < n                   # others depend on it; the other blocks stay finite
    x, res = gpu_solve(kind, n, ip, ix, dt, b)
    assert np.array_equal(np.isnan(x), nans)
    assert same_bits(x[~nans], x_ref[~nans])
    assert res.levels == ref.levels(kind, n, ip, ix)


def test_subnormal_quotient_and_f32_rounding(hip):
    """a 4 x 4 lower system: x0 = 2^-100 / 2^33 is subnormal in f32 (kept, not flushed, and used by row 3), and row 2's
    1 - 0.6f * x1 rounds differently as two f32 operations than as the f64 expression rounded once"""
    tiny = float(np.finfo(np.float32).tiny)
    ip = np.array([0, 1, 2, 4, 7], dtype=np.uint64)
    ix = np.array([0, 1, 1, 2, 0, 2, 3], dtype=np.uint64)
    dt = np.array([2.0 ** 33, 3.0, 0.6, 1.0, 2.0 ** 120, 0.7, 7.0], dtype=np.float32)
    b = np.array([2.0 ** -100, 1.0, 1.0, 5.0], dtype=np.float32)
    x_ref = ref.lsolve_csr_dense_rhs(4, ip, ix, dt, b)
    assert 0.0 < float(x_ref[0]) < tiny and x_ref[0] == F(2.0 ** -133)                        # a subnormal quotient
    x1, v = x_ref[1], dt[2]
    two_f32_ops = F(F(1.0) - F(v * x1))
    one_rounding = F(np.float64(1.0) - np.float64(v) * np.float64(x1))
    assert two_f32_ops != one_rounding and x_ref[2] == two_f32_ops
    assert x_ref[3] == F(F(F(5.0) - F(dt[4] * x_ref[0])) - F(dt[5] * x_ref[2])) / F(7.0) and np.isfinite(x_ref).all()
    assert F(dt[4] * x_ref[0]) == F(2.0 ** -13)                                                # the subnormal was an operand
    x, _ = gpu_solve("lsolve_csr", 4, ip, ix, dt, b)
    assert same_bits(x, x_ref)
    # the same system as CSC (the scatter form): the same order here, the same bits
    import scipy.sparse as sp
    m = sp.csr_matrix((dt, ix.astype(np.int64), ip.astype(np.int64)), shape=(4, 4)).tocsc()
    m.sort_indices()
    cip, cix, cdt = m.indptr.astype(np.uint64), m.indices.astype(np.uint64), m.data.astype(np.float32)
    x_csc_ref = ref.lsolve_csc_dense_rhs(4, cip, cix, cdt, b)
    x, _ = gpu_solve("lsolve_csc", 4, cip, cix, cdt, b)
    assert same_bits(x, x_csc_ref) and 0.0 < float(x[0]) < tiny


@pytest.mark.parametrize("kind", KINDS)
def test_singular_matrices(hip, kind):
    """a stored 0.0f, a stored -0.0f, a diagonal that is not stored (structural on CSC), two at once: index, reason and text of
    the reference, as tests/test_trisolve_gpu.py checks them for f64"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVecF32
    n = 80
    b = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    for missing, zeros, minus in (([37], [], False), ([], [41], False), ([], [41], True), ([12], [70], False), ([70], [12], False),
                                  ([0], [], False), ([], [n - 1], False)):
        csr, csc = _singular_system(n, missing, zeros)
        ip, ix, dt = csc if kind.endswith("csc") else csr
        dt = dt.astype(np.float32)
        if minus:
            dt = np.where(dt == 0.0, F(-0.0), dt).astype(np.float32)
            assert np.signbit(dt[dt == 0.0]).all() and (dt == 0.0).sum() == 1
        with pytest.raises(ref.Singular) as want:
            ref.SOLVES[kind](n, ip, ix, dt, b)
        assert want.value.index == (max if kind[0] == "u" else min)(missing + zeros)
        a = device_mat(kind, n, ip, ix, dt)
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(a, DeviceVecF32.from_host(b))
        assert e.value.status == _ffi.SINGULAR_MATRIX
        assert e.value.index == want.value.index
        assert str(want.value) in str(e.value)                       # "Singular matrix at index {} ({reason})", errors.rs:87-92
        structural = kind.endswith("csc") and want.value.index in missing
        assert e.value.reason == ("structural" if structural else "numeric")
        assert ("structural" in want.value.reason) == structural


def test_nan_diagonal_is_not_singular(hip):
    """`diag == 0` is false for a NaN (trisolve.rs:64): the solve returns Ok with NaNs where the reference has them"""
    n = 40
    csr, _ = _singular_system(n, [], [20])
    ip, ix, dt = csr
    dt = np.where(dt == 0.0, np.nan, dt).astype(np.float32)
    b = np.ones(n, dtype=np.float32)
    x_ref = ref.lsolve_csr_dense_rhs(n, ip, ix, dt, b)
    x, _ = gpu_solve("lsolve_csr", n, ip, ix, dt, b)
    assert np.isnan(x_ref[20]) and np.array_equal(np.isnan(x), np.isnan(x_ref))
    ok = ~np.isnan(x_ref)
    assert same_bits(x[ok], x_ref[ok])


def test_contract_violations(hip):
    """check_solver_dimensions (trisolve.rs:10-21), the storage asserts, a vector of the other precision, uplo at the C level, n = 0"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32
    one = np.ones(2, dtype=np.float32)
    rect = DeviceCsMatF32.from_host((2, 3), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), one)
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn("lsolve_csr")(rect, DeviceVecF32.zeros(2))
    assert e.value.status == _ffi.DIM_MISMATCH and "Non square matrix passed to solver" in str(e.value)
    eye = DeviceCsMatF32.from_host((4, 4), np.arange(5, dtype=np.uint64), np.arange(4, dtype=np.uint64), np.ones(4, dtype=np.float32))
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn("usolve_csr")(eye, DeviceVecF32.zeros(5))
    assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    x = DeviceVecF32.zeros(4)
    assert _ffi.lib.sprs_hip_trisolve_f32(eye._h, 7, C.c_void_p(x.ptr), 4, None, None) == _ffi.INVALID_ARG
    assert _ffi.lib.sprs_hip_trisolve_f32(eye._h, _ffi.LOWER, None, 4, None, None) == _ffi.INVALID_ARG
    assert _ffi.lib.sprs_hip_trisolve_f32(None, _ffi.LOWER, C.c_void_p(x.ptr), 4, None, None) == _ffi.INVALID_ARG
    for kind in ("lsolve_csc", "usolve_csc"):
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(eye, x)
        assert e.value.status == _ffi.STORAGE_MISMATCH and "Storage mismatch" in str(e.value)
    csc = eye.to_other_storage()
    for kind in ("lsolve_csr", "usolve_csr"):
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(csc, x)
        assert e.value.status == _ffi.STORAGE_MISMATCH
    # mixed precision: never reaches the library
    with pytest.raises(TypeError):
        gpu_fn("lsolve_csr")(eye, DeviceVec.zeros(4))
    with pytest.raises(TypeError):
        gpu_fn("lsolve_csr")(DeviceCsMat.eye(4), DeviceVecF32.zeros(4))
    # n == 0: nothing to do
    empty = DeviceCsMatF32.from_host((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float32))
    assert gpu_fn("lsolve_csr")(empty, DeviceVecF32(0)).levels == 0


def test_diag_solve(hip):
    """linalg::diag_solve::<f32>: one IEEE f32 division per element (a subnormal quotient kept); mixed precision refused"""
    from sprs_amd.device import DeviceVec, DeviceVecF32
    from sprs_amd.linalg import diag_solve
    rng = np.random.default_rng(77)
    n = 1000
    d = rng.standard_normal(n).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    d[3], x[3] = F(2.0 ** 33), F(2.0 ** -100)
    d[5], x[5] = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        want = x / d
    assert 0.0 < float(want[3]) < float(np.finfo(np.float32).tiny) and np.isinf(want[5])
    xd = DeviceVecF32.from_host(x)
    assert diag_solve(DeviceVecF32.from_host(d), xd) is xd
    assert same_bits(xd.to_host(), want)
    with pytest.raises(TypeError):
        diag_solve(DeviceVec.zeros(4), DeviceVecF32.zeros(4))
    with pytest.raises(hip.SprsHipError) as e:
        diag_solve(DeviceVecF32.zeros(4), DeviceVecF32.zeros(5))
    assert e.value.status == hip._ffi.DIM_MISMATCH


# ---- past one chunk per wave (tests/test_trisolve_seams_gpu.py): real device only -----------------------------------------------------

_SHARED = {}


def redraw_system():
    if "redraw" not in _SHARED:
        n = 256 * _cus() + 129
        _SHARED["redraw"] = (n, block_system(n, 256), (np.random.default_rng(257).standard_normal(n) * 7.0 + 0.25).astype(np.float32))
    return _SHARED["redraw"]


@pytest.mark.skipif(EMU, reason="more than 256 x CUs rows of hand-offs: real device only")
@pytest.mark.parametrize("kind", KINDS)
def test_solve_redraws(hip, kind):
    """n = 256 x CUs + 129: every wave draws a second chunk of the level order"""
    n, a, b = redraw_system()
    assert n > 256 * _cus()
    ip, ix, dt = arrays32(a, kind)
    x_ref = ref.SOLVES[kind](n, ip, ix, dt, b)
    assert np.isfinite(x_ref).all()
    x, res = gpu_solve(kind, n, ip, ix, dt, b, np.uint32, np.uint64)
    assert np.array_equal(x, x_ref)
    assert res.levels == ref.levels(kind, n, ip, ix)


@pytest.mark.skipif(EMU, reason="more than 256 x CUs rows of hand-offs: real device only")
@pytest.mark.parametrize("kind", ["lsolve_csc", "usolve_csr"])
def test_singular_rows_in_two_chunks(hip, kind):
    """a diagonal that is not stored in the first chunk of the order, a stored 0.0f in a chunk that only a second draw reaches: the
    lower solve reports the smaller index, the upper one the larger"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVecF32
    n, a, b = redraw_system()
    grid_rows = 256 * _cus()
    upper = kind.startswith("u")
    pos = level_positions(kind, a)
    near = 5 * BLOCK + (BLOCK - 1 if upper else 0)
    far = (n // BLOCK - 3) * BLOCK + (0 if upper else BLOCK - 1)
    assert pos[near] < 64 and pos[far] >= grid_rows, "the two rows are not in the first chunk and in a redrawn one"
    ip, ix, dt = _without(a, [near], [far])["csc" if kind.endswith("csc") else "csr"]
    dt = dt.astype(np.float32)
    with pytest.raises(ref.Singular) as want:
        ref.SOLVES[kind](n, ip, ix, dt, b)
    assert want.value.index == (max if upper else min)(near, far)
    handle = device_mat(kind, n, ip, ix, dt)
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn(kind)(handle, DeviceVecF32.from_host(b))
    assert e.value.status == _ffi.SINGULAR_MATRIX
    assert e.value.index == want.value.index
    assert str(want.value) in str(e.value)
    structural = kind.endswith("csc") and want.value.index == near
    assert e.value.reason == ("structural" if structural else "numeric")
