"""Device permutations — PermOwned, `&P * x`, permute_rows, permute_cols, transform_mat_papt, transform_mat_paq
(sprs/src/sparse/permutation.rs) — bit for bit: indptr, indices and the uint64 view of the values, no tolerance anywhere.

The small cases also run against the kernel emulator (tests/test_perm_emu_cpu.py); the large and the torch cases need a real
device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import perm_ref as R
from conftest import IDX_COMBOS, ROOT, as_csr
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
CSR, CSC = R.CSR, R.CSC
WIDTHS = IDX_COMBOS + [(np.uint16, np.uint16)]
NAN_PAYLOAD = 0x7FF8000000ABCDEF


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "perm_fixtures.json")) as f:
        return json.load(f)


def _mat(m, storage=CSR, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    shape, ip, ix, dt = m
    return DeviceCsMat.from_host(tuple(shape), np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64),
                                 storage=storage)


def _perm(p, dtype=np.uint64):
    """None -> the Identity variant is made by the caller; a list / array -> PermOwned::new"""
    from sprs_amd.permutation import DevicePerm
    return DevicePerm(np.asarray(p, dtype=dtype))


def _check(res, want, storage=CSR):
    got = res.to_host()
    assert res.storage() == storage
    assert R.same_mat(got, want)
    assert int(got[1][0]) == 0 and int(got[1][-1]) == got[2].size == got[3].size     # a proper indptr, exact nnz


def _special(dt, seed):
    """-0.0, explicit 0.0, inf and a NaN with a payload among the values"""
    rng = np.random.default_rng(seed)
    dt = np.array(dt, dtype=np.float64)
    dt[rng.random(dt.size) < 0.04] = -0.0
    dt[rng.random(dt.size) < 0.04] = 0.0
    dt[rng.random(dt.size) < 0.02] = np.inf
    dt.view(np.uint64)[rng.random(dt.size) < 0.02] = NAN_PAYLOAD
    if dt.size >= 4:
        dt[:3] = [-0.0, 0.0, np.inf]
        dt.view(np.uint64)[3] = NAN_PAYLOAD
    return dt


# ---- 1. the reference's own tests (permutation.rs:587-782) -------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_golden(fx, storage, idx, ptr):
    """every expectation for the CSC matrix the reference builds and for its CSR form (mat.to_other_storage())"""
    from sprs_amd import permutation as P
    form = (lambda m: m) if storage == CSC else (lambda m: R.to_other(m, CSC))
    up = lambda m: _mat(form(m), storage, idx, ptr)
    c = fx["transform_mat_papt"]
    res = P.transform_mat_papt(up(as_csr(c["mat"])), _perm(c["perm"], idx))
    _check(res, form(as_csr(c["expected"])), storage)
    assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize
    c = fx["transform_mat_paq"]
    a, p, q = up(as_csr(c["mat"])), _perm(c["row_perm"], idx), _perm(c["col_perm"], idx)
    _check(P.transform_mat_paq(a, p, q), form(as_csr(c["expected"])), storage)
    _check(P.permute_rows(P.permute_cols(a, q), p), form(as_csr(c["expected"])), storage)
    c = fx["permute_rows"]
    _check(P.permute_rows(up(as_csr(c["mat"])), _perm(c["perm"], idx)), form(as_csr(c["expected"])), storage)
    c = fx["permute_cols"]
    # mat.transpose_view(): the same arrays in the other storage; the result is compared through its transpose
    mat_t, want_t = R.transpose(form(as_csr(c["mat"]))), R.transpose(form(as_csr(c["expected"])))
    _check(P.permute_cols(_mat(mat_t, 1 - storage, idx, ptr), _perm(c["perm"], idx)), want_t, 1 - storage)


@pytest.mark.parametrize("dtype", [np.uint64, np.uint32, np.uint16])
def test_golden_perm_mul_and_validity(fx, dtype):
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.device import DeviceVec
    c = fx["perm_mul"]
    p = _perm(c["perm"], dtype)
    assert (p * DeviceVec.from_host(np.array(c["x"], dtype=np.float64))).to_host().tolist() == c["y"]
    assert p.dim == 5 and p.index_bytes() == np.dtype(dtype).itemsize and not p.is_identity_variant()
    assert p.vec().dtype == dtype and p.vec().tolist() == c["perm"] and p.inv_vec().tolist() == R.perm_new(c["perm"])[1]
    for good in fx["perm_validity"]["valid"]:
        assert _perm(good, dtype).vec().tolist() == good
    for bad in fx["perm_validity"]["invalid"]:
        with pytest.raises(SprsHipError) as e:
            _perm(bad, dtype)
        assert e.value.status == _ffi.BAD_STRUCTURE and str(e.value).endswith("invalid permutation")


# ---- 2. the length ladder ----------------------------------------------------------------------------------------------------

KINDS = ["random", "reversal", "shift", "finite_identity", "identity_variant"]


@pytest.fixture(scope="module")
def ladder():
    """one square matrix whose non-empty rows have the lengths 1 .. 130 and 2^k - 1, 2^k, 2^k + 1 (k = 8 .. 17; under the
    emulator up to 12): every class of the relabelling path and both sides of each boundary (16, 32, 64 and the 2^12 of
    option perm_cap are powers of two).  Empty rows in between; the first and the last row are empty."""
    import sprs_amd
    n, kmax = (5000, 12) if EMULATED else (140000, 17)
    cap = int(sprs_amd.get_option("perm_cap"))
    want = list(range(1, 131)) + [(1 << k) + d for k in range(8, kmax + 1) for d in (-1, 0, 1)]
    if cap & (cap - 1):
        want += [cap - 1, cap, cap + 1]
    assert max(want) <= n
    rng = np.random.default_rng(2024)
    lens = np.zeros(n, dtype=np.int64)
    at = 1 + 3 * np.arange(len(want))               # two empty rows after every non-empty one, then empty rows to the end
    lens[at] = rng.permutation(want)
    assert lens[0] == 0 and lens[-1] == 0
    shape, ip, ix, dt = ragged_csr(lens, n, seed=5, positive=False)
    assert ix.size < 10 ** 6
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), _special(dt, 5))
    perms = {"random": rng.permutation(n), "reversal": np.arange(n)[::-1].copy(), "shift": np.roll(np.arange(n), -1),
             "finite_identity": np.arange(n), "identity_variant": None}
    other = np.random.default_rng(77).permutation(n)
    return m, perms, other, {}


def _ladder_dev(ladder, storage):
    cache = ladder[3]
    if storage not in cache:
        cache[storage] = _mat(ladder[0], storage, np.uint32, np.uint64)
    return cache[storage]


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("kind", KINDS)
def test_length_ladder(ladder, kind, storage):
    from sprs_amd import permutation as P
    from sprs_amd.permutation import DevicePerm
    m, perms, other, _ = ladder
    n = m[0][0]
    a = _ladder_dev(ladder, storage)
    hp = perms[kind]
    dp = DevicePerm.identity(n, np.uint32) if hp is None else _perm(hp, np.uint32)
    dq = _perm(other, np.uint32)
    assert dp.is_identity() == (kind in ("finite_identity", "identity_variant"))
    papt = P.transform_mat_papt(a, dp)
    _check(papt, R.transform_mat_papt_vec(m, storage, hp), storage)
    if kind in ("finite_identity", "identity_variant"):
        assert R.same_mat(papt.to_host(), m)        # the result's arrays are A's
    _check(P.transform_mat_paq(a, dp, dq), R.transform_mat_paq_vec(m, storage, hp, other), storage)
    _check(P.transform_mat_paq(a, dq, dp), R.transform_mat_paq_vec(m, storage, other, hp), storage)
    _check(P.permute_rows(a, dp), R.permute_rows_vec(m, storage, hp), storage)
    _check(P.permute_cols(a, dp), R.permute_cols_vec(m, storage, hp), storage)
    got = papt.to_host()[3].view(np.uint64)         # the special values are still stored, bit for bit
    for v in (np.float64(-0.0), np.float64(0.0), np.float64(np.inf)):
        assert (got == v.view(np.uint64)).sum() == (m[3].view(np.uint64) == v.view(np.uint64)).sum() > 0
    assert (got == NAN_PAYLOAD).sum() == (m[3].view(np.uint64) == NAN_PAYLOAD).sum() > 0


# ---- 3. tile edges of the copy path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_copy_path_tile_edges(idx, ptr):
    import sprs_amd
    from sprs_amd import permutation as P
    t = int(sprs_amd.get_option("perm_tile"))
    lens = [t - 1, 1, t, t + 1, 2 * t + 3, 0, 0, 1]
    shape, ip, ix, dt = ragged_csr(lens, 2 * t + 40, seed=8, positive=False)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), _special(dt, 8))
    a = _mat(m, CSR, idx, ptr)
    a_csc = _mat(R.transpose(m), CSC, idx, ptr)     # the same arrays: the columns of the transpose
    for p in ([7, 0, 5, 4, 1, 6, 3, 2], [7, 6, 5, 4, 3, 2, 1, 0], [1, 2, 3, 4, 5, 6, 7, 0], [4, 5, 6, 7, 0, 1, 2, 3]):
        _check(P.permute_rows(a, _perm(p, idx)), R.permute_rows_vec(m, CSR, p))
        _check(P.permute_cols(a_csc, _perm(p, idx)), R.permute_cols_vec(R.transpose(m), CSC, p), CSC)
    # more slices in one tile than the tile keeps slice starts for: the starts are searched in memory
    many = 3 * t
    lens = np.ones(many, dtype=np.int64)
    lens[::7] = 0
    lens[5] = t + 5
    shape, ip, ix, dt = ragged_csr(lens, t + 9, seed=9, positive=False)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), dt)
    p = np.random.default_rng(3).permutation(many)
    _check(P.permute_rows(_mat(m, CSR, idx, ptr), _perm(p, idx)), R.permute_rows_vec(m, CSR, p))


# ---- 4. rectangular and degenerate shapes --------------------------------------------------------------------------------------

def _shapes():
    out = []
    for (rows, cols), seed in (((5, 4), 1), ((1, 37), 2), ((37, 1), 3), ((0, 6), 4), ((6, 0), 5), ((23, 90), 6)):
        rng = np.random.default_rng(seed)
        lens = rng.integers(0, min(cols, 70) + 1, rows) if cols else np.zeros(rows, dtype=np.int64)
        shape, ip, ix, dt = ragged_csr(lens, cols, seed=seed, positive=False)
        out.append(((rows, cols), ip.astype(np.int64), ix.astype(np.int64), _special(dt, seed)))
    return out


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_rectangular_shapes(storage):
    from sprs_amd import permutation as P
    for m in _shapes():
        if storage == CSC:
            m = R.transpose(m)
        rows, cols = m[0]
        rng = np.random.default_rng(rows * 100 + cols)
        hp, hq = rng.permutation(rows), rng.permutation(cols)
        a, p, q = _mat(m, storage), _perm(hp), _perm(hq)
        paq = P.transform_mat_paq(a, p, q)
        _check(paq, R.transform_mat_paq_ref(m, storage, hp, hq), storage)
        assert R.same_mat(paq.to_host(), P.permute_rows(P.permute_cols(a, q), p).to_host())
        _check(P.permute_rows(a, p), R.permute_rows_ref(m, storage, hp), storage)
        _check(P.permute_cols(a, q), R.permute_cols_ref(m, storage, hq), storage)
        _check(P.transform_mat_paq(P.transform_mat_paq(a, p, q), p.inv(), q.inv()), m, storage)
        _check(P.transform_mat_paq(a, None, None), m, storage)


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_papt_round_trip_and_inverse(storage):
    from sprs_amd import permutation as P
    n = 150
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 20, n)
    lens[[3, 77]] = [n, 100]
    shape, ip, ix, dt = ragged_csr(lens, n, seed=12, positive=False)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), _special(dt, 12))
    hp = rng.permutation(n)
    a, p = _mat(m, storage), _perm(hp)
    papt = P.transform_mat_papt(a, p)
    _check(papt, R.transform_mat_papt_ref(m, storage, hp), storage)
    _check(P.transform_mat_papt(papt, p.inv()), m, storage)
    pi = p.inv()
    assert np.array_equal(pi.vec(), p.inv_vec()) and np.array_equal(pi.inv_vec(), p.vec())
    pii = pi.inv()
    assert np.array_equal(pii.vec(), hp) and np.array_equal(pii.inv_vec(), R.perm_new(hp)[1])


# ---- 5. permutations themselves ------------------------------------------------------------------------------------------------

def _device_words(arr):
    """a host uint64 array as a device buffer (the words travel unchanged)"""
    from sprs_amd.device import DeviceVec
    return DeviceVec.from_host(np.ascontiguousarray(arr, dtype=np.uint64).view(np.float64))


def test_from_device_validation():
    """dim 100 003 is validated on the device: valid, one duplicate in the last position, one value equal to dim"""
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.permutation import DevicePerm
    n = 100003
    hp = np.random.default_rng(5).permutation(n).astype(np.uint64)
    p = DevicePerm.from_device(_device_words(hp))
    assert p.dim == n and p.index_bytes() == 8 and np.array_equal(p.vec(), hp)
    inv = np.empty(n, dtype=np.uint64)
    inv[hp] = np.arange(n, dtype=np.uint64)
    assert np.array_equal(p.inv_vec(), inv)
    dup = hp.copy()
    dup[-1] = dup[0]
    big = hp.copy()
    big[n // 2] = n
    for bad in (dup, big):
        with pytest.raises(SprsHipError) as e:
            DevicePerm.from_device(_device_words(bad))
        assert e.value.status == _ffi.BAD_STRUCTURE and str(e.value).endswith("invalid permutation")
        with pytest.raises(SprsHipError) as e:      # the upload validates a permutation of this size on the device too
            DevicePerm(bad)
        assert e.value.status == _ffi.BAD_STRUCTURE
    assert np.array_equal(DevicePerm.from_device(_device_words(hp)).inv_vec(), inv)       # a following valid call works
    unchecked = DevicePerm.from_device(_device_words(big), validate=False)                # nothing is written out of range
    assert unchecked.dim == n


def test_is_identity():
    from sprs_amd.permutation import DevicePerm
    for n in (1, 64, 100003):
        assert _perm(np.arange(n)).is_identity() and not _perm(np.arange(n)).is_identity_variant()
        if n > 1:
            swapped = np.arange(n)
            swapped[[n - 2, n - 1]] = [n - 1, n - 2]
            assert not _perm(swapped).is_identity()
    assert DevicePerm.identity(9).is_identity() and _perm(np.zeros(0, dtype=np.uint64)).is_identity()


@pytest.mark.parametrize("dtype", [np.uint64, np.uint32])
def test_perm_mul_vec(dtype):
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.device import DeviceVec
    from sprs_amd.permutation import DevicePerm
    for n in (0, 1, 63, 64, 65, 100003):
        rng = np.random.default_rng(n)
        hp = rng.permutation(n)
        x = _special(rng.standard_normal(n), n)
        p = _perm(hp, dtype)
        dx = DeviceVec.from_host(x)
        y = (p * dx).to_host()
        assert np.array_equal(y.view(np.uint64), x[hp].view(np.uint64))
        back = (p.inv() * DeviceVec.from_host(y)).to_host()
        assert np.array_equal(back.view(np.uint64), x.view(np.uint64))
        assert np.array_equal((DevicePerm.identity(n, dtype) * dx).to_host().view(np.uint64), x.view(np.uint64))
    p = _perm([2, 0, 1, 3], dtype)
    v = DeviceVec.from_host(np.arange(8.0))
    lib = _ffi.lib
    at = lambda k: C.c_void_p(v.ptr + 8 * k)
    for xo, yo in ((0, 0), (0, 3), (3, 0), (1, 2)):  # aliasing refused
        assert lib.sprs_hip_perm_mul_vec_f64(p._h, at(xo), at(yo), 4, None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_perm_mul_vec_f64(p._h, at(0), at(4), 4, None) == _ffi.OK
    assert v.to_host().tolist() == [0.0, 1.0, 2.0, 3.0, 2.0, 0.0, 1.0, 3.0]
    with pytest.raises(SprsHipError) as e:
        p * DeviceVec.from_host(np.arange(5.0))
    assert e.value.status == _ffi.DIM_MISMATCH and str(e.value).endswith("Dimension mismatch")


def test_errors(fx):
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd import permutation as P
    from sprs_amd.permutation import DevicePerm
    rect = as_csr(fx["permute_rows"]["mat"])         # 5 x 4
    sq = as_csr(fx["transform_mat_papt"]["mat"])     # 5 x 5
    for storage in (CSR, CSC):
        a = _mat(rect if storage == CSC else R.to_other(rect, CSC), storage)
        s = _mat(sq, storage)
        p4, p5, i4, i5 = _perm([1, 0, 3, 2]), _perm([1, 0, 3, 2, 4]), DevicePerm.identity(4), DevicePerm.identity(5)
        for f in (lambda: P.permute_rows(a, p4), lambda: P.permute_cols(a, p5), lambda: P.transform_mat_paq(a, p5, p5),
                  lambda: P.transform_mat_paq(a, p4, p4), lambda: P.permute_rows(a, i4), lambda: P.permute_cols(a, i5),
                  lambda: P.transform_mat_papt(a, p5), lambda: P.transform_mat_papt(a, p4), lambda: P.transform_mat_papt(a, i5),
                  lambda: P.transform_mat_papt(s, p4), lambda: P.transform_mat_papt(s, i4)):
            with pytest.raises(SprsHipError) as e:
                f()
            assert e.value.status == _ffi.DIM_MISMATCH and str(e.value).endswith("Dimension mismatch")
        # the declared index width of the permutation must be the matrix's I
        for dt in (np.uint32, np.uint16):
            w5, wi = _perm([1, 0, 3, 2, 4], dt), DevicePerm.identity(5, dt)
            for f in (lambda: P.permute_rows(a, w5), lambda: P.transform_mat_papt(s, w5), lambda: P.transform_mat_paq(s, p5, w5),
                      lambda: P.transform_mat_papt(s, wi), lambda: P.permute_rows(a, wi)):
                with pytest.raises(SprsHipError) as e:
                    f()
                assert e.value.status == _ffi.STORAGE_MISMATCH
        _check(P.permute_rows(a, i5), rect if storage == CSC else R.to_other(rect, CSC), storage)   # the departure: a copy
        _check(P.permute_cols(a, i4), rect if storage == CSC else R.to_other(rect, CSC), storage)


# ---- 6. the operand is const ---------------------------------------------------------------------------------------------------

def test_operand_untouched():
    from sprs_amd import permutation as P
    from sprs_amd.device import DeviceVec
    n = 300
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 30, n)
    lens[10] = 200
    shape, ip, ix, dt = ragged_csr(lens, n, seed=21)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), dt)
    for storage in (CSR, CSC):
        a = _mat(m, storage)
        a * DeviceVec.from_host(np.ones(n))         # the handle now carries an SpMV plan
        before, plan = a.to_host(), a.spmv_plan_info()
        p, q = _perm(rng.permutation(n)), _perm(rng.permutation(n))
        P.transform_mat_papt(a, p), P.transform_mat_paq(a, p, q), P.permute_rows(a, p), P.permute_cols(a, q)
        assert R.same_mat(a.to_host(), before) and R.same_mat(before, m) and a.spmv_plan_info() == plan


# ---- 7. a consumer: (P A P^T)(P x) == P (A x) ----------------------------------------------------------------------------------

def test_consumer_spmv():
    """small integers: every product and every sum is exact, so the two sides agree bitwise whatever order SpMV adds in"""
    from sprs_amd import permutation as P
    from sprs_amd.device import DeviceVec
    n = 2000
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 40, n)
    lens[[5, 900]] = [1500, 70]
    shape, ip, ix, dt = ragged_csr(lens, n, seed=31)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), rng.integers(-8, 9, ix.size).astype(np.float64))
    x = rng.integers(-8, 9, n).astype(np.float64)
    hp = rng.permutation(n)
    p, dx = _perm(hp), DeviceVec.from_host(x)
    for storage in (CSR, CSC):
        a = _mat(m, storage)
        lhs = (P.transform_mat_papt(a, p) * (p * dx)).to_host()
        rhs = (p * (a * dx)).to_host()
        assert np.array_equal(lhs.view(np.uint64), rhs.view(np.uint64)) and np.any(lhs != 0)


# ---- 8. real device only -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def powerlaw():
    """a seeded power-law matrix of 2 * 10^5 rows and about 2 * 10^6 entries: rows ~ n * u^3, columns ~ n * u^2, duplicates folded"""
    n = 200000
    rng = np.random.default_rng(3)
    e = 2_100_000
    key = np.unique((n * rng.random(e) ** 3).astype(np.int64) * n + (n * rng.random(e) ** 2).astype(np.int64))
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ip[1:])
    m = ((n, n), ip, key % n, _special(rng.standard_normal(key.size), 3))
    return m, rng.permutation(n), rng.permutation(n)


@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_powerlaw_200k(powerlaw):
    from sprs_amd import permutation as P
    from sprs_amd.triplet import TriMat
    m, hp, hq = powerlaw
    n = m[0][0]
    assert np.diff(m[1]).max() > 4096 and 1_800_000 < m[2].size < 2_200_000      # the hub class is exercised
    a, p, q = _mat(m, CSR, np.uint32, np.uint64), _perm(hp, np.uint32), _perm(hq, np.uint32)
    papt = P.transform_mat_papt(a, p)
    want = R.transform_mat_papt_vec(m, CSR, hp)
    _check(papt, want)
    _check(P.transform_mat_paq(a, p, q), R.transform_mat_paq_vec(m, CSR, hp, hq))
    _check(P.permute_rows(a, p), R.permute_rows_vec(m, CSR, hp))
    a_csc = _mat(m, CSC, np.uint32, np.uint64)
    _check(P.transform_mat_paq(a_csc, p, q), R.transform_mat_paq_vec(m, CSC, hp, hq), CSC)
    # an independent device route: the relabelled triplets through the triplet assembler
    inv_p = np.argsort(hp)                          # entry (i, j) of A is entry (inv[i], inv[j]) of P A P^T
    row_of = np.repeat(np.arange(n), np.diff(m[1]))
    tri = TriMat((n, n), inv_p[row_of], inv_p[m[2]], m[3]).to_csr(idx_dtype=np.uint32)
    assert R.same_mat(tri.to_host(), want)


@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_non_blocking_stream():
    """operand and permutation are written on a non-blocking torch stream and used there with no host synchronise in between"""
    import torch
    from sprs_amd import permutation as P
    from sprs_amd.device import DeviceCsMat
    from sprs_amd.permutation import DevicePerm
    n = 6000
    rng = np.random.default_rng(51)
    lens = rng.integers(0, 90, n)
    lens[[17, 4000]] = [5000, 4096]
    shape, ip, ix, dt = ragged_csr(lens, n, seed=51, positive=False)
    m = (shape, ip.astype(np.int64), ix.astype(np.int64), dt)
    hp = rng.permutation(n)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        t_ip = torch.zeros(m[1].size, dtype=torch.int64, device=dev)
        t_ix = torch.zeros(m[2].size, dtype=torch.int64, device=dev)
        t_dt = torch.zeros(m[3].size, dtype=torch.float64, device=dev)
        t_p = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda._sleep(20_000_000)                  # keep the stream busy: the copies below land late
        t_ip.copy_(torch.from_numpy(m[1]).to(dev, non_blocking=True))
        t_ix.copy_(torch.from_numpy(m[2]).to(dev, non_blocking=True))
        t_dt.copy_(torch.from_numpy(m[3]).to(dev, non_blocking=True))
        t_p.copy_(torch.from_numpy(hp.astype(np.int64)).to(dev, non_blocking=True))
        a = DeviceCsMat.wrap_torch(m[0], t_ip, t_ix, t_dt)
        p = DevicePerm.from_device(t_p, stream=s)
        assert not p.is_identity(stream=s)
        papt = P.transform_mat_papt(a, p, stream=s)
        rows = P.permute_rows(a, p, stream=s)
    _check(papt, R.transform_mat_papt_vec(m, CSR, hp))
    _check(rows, R.permute_rows_vec(m, CSR, hp))
    assert np.array_equal(p.vec(), hp.astype(np.uint64))
