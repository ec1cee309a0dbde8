"""The Python restatement of the reference's permutations (tests/perm_ref.py) against the reference's own expectations
(sprs/src/sparse/permutation.rs:587-782), its numpy twin against the line-by-line one, and the argument checks of the new
entry points that need no device.  (A matrix handle cannot be made without a device: the dimension, squareness and width
checks of the two matrix entries run in tests/test_perm_gpu.py, which tests/test_perm_emu_cpu.py also runs on the CPU.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import perm_ref as R
from conftest import ROOT, as_csr
from helpers import ragged_csr

CSR, CSC = R.CSR, R.CSC


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "perm_fixtures.json")) as f:
        return json.load(f)


def test_reference_perm_mul_and_validity(fx):
    c = fx["perm_mul"]
    assert R.perm_mul(c["perm"], c["x"]) == c["y"]
    assert R.perm_mul(None, c["x"]) == c["x"]
    for p in fx["perm_validity"]["valid"]:
        assert R.perm_is_valid(p)
        perm, inv = R.perm_new(p)
        assert [perm[inv[i]] for i in range(len(p))] == list(range(len(p)))
    for p in fx["perm_validity"]["invalid"]:
        assert not R.perm_is_valid(p)
        with pytest.raises(AssertionError, match="invalid permutation"):
            R.perm_new(p)
    assert R.is_identity([0, 1, 2]) and R.is_identity(None) and not R.is_identity([0, 2, 1])


@pytest.mark.parametrize("twin", ["ref", "vec"])
def test_reference_expectations_matrices(fx, twin):
    f = lambda name: getattr(R, "%s_%s" % (name, twin))
    c = fx["transform_mat_papt"]
    mat, want = as_csr(c["mat"]), as_csr(c["expected"])
    assert R.same_mat(f("transform_mat_papt")(mat, CSC, c["perm"]), want)
    assert R.same_mat(f("transform_mat_papt")(R.to_other(mat, CSC), CSR, c["perm"]), R.to_other(want, CSC))
    c = fx["transform_mat_paq"]
    mat, want = as_csr(c["mat"]), as_csr(c["expected"])
    assert R.same_mat(f("transform_mat_paq")(mat, CSC, c["row_perm"], c["col_perm"]), want)
    assert R.same_mat(f("transform_mat_paq")(R.to_other(mat, CSC), CSR, c["row_perm"], c["col_perm"]), R.to_other(want, CSC))
    aq = f("permute_cols")(mat, CSC, c["col_perm"])             # "the same result as applying the permutations separately"
    assert R.same_mat(f("permute_rows")(aq, CSC, c["row_perm"]), want)
    c = fx["permute_rows"]
    mat, want = as_csr(c["mat"]), as_csr(c["expected"])
    assert R.same_mat(f("permute_rows")(mat, CSC, c["perm"]), want)
    assert R.same_mat(f("permute_rows")(R.to_other(mat, CSC), CSR, c["perm"]), R.to_other(want, CSC))
    c = fx["permute_cols"]
    mat, want = as_csr(c["mat"]), as_csr(c["expected"])
    # mat.transpose_view() is the CSR matrix with mat's arrays; the result is compared through its transpose
    assert R.same_mat(R.transpose(f("permute_cols")(R.transpose(mat), CSR, c["perm"])), want)
    got = f("permute_cols")(R.transpose(R.to_other(mat, CSC)), CSC, c["perm"])
    assert R.same_mat(R.transpose(got), R.to_other(want, CSC))


def test_shortcuts_and_asserts(fx):
    mat = as_csr(fx["permute_rows"]["mat"])         # 5 x 4
    for twin in ("ref", "vec"):
        paq, papt = getattr(R, "transform_mat_paq_" + twin), getattr(R, "transform_mat_papt_" + twin)
        assert R.same_mat(paq(mat, CSC, None, None), mat)
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            paq(mat, CSC, [0, 1, 2, 3], None)
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            paq(mat, CSC, None, [0, 1, 2, 3, 4])
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            papt(mat, CSC, [0, 1, 2, 3, 4])         # not square
        sq = as_csr(fx["transform_mat_papt"]["mat"])
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            papt(sq, CSC, [0, 1, 2, 3])
        assert R.same_mat(papt(sq, CSC, [0, 1, 2, 3, 4]), sq)         # a FinitePerm equal to the identity: a copy
        empty = ((0, 3), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
        assert R.same_mat(paq(empty, CSC, [], [2, 0, 1]), empty)


def _special(m, seed):
    rng = np.random.default_rng(seed)
    dt = m[3].copy()
    dt[rng.random(dt.size) < 0.05] = -0.0
    dt[rng.random(dt.size) < 0.05] = 0.0
    dt[rng.random(dt.size) < 0.03] = np.inf
    b = dt.view(np.uint64)
    b[rng.random(dt.size) < 0.03] = 0x7FF8000000ABCDEF           # a NaN with a payload
    return m[0], m[1], m[2], dt


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_numpy_twin_equals_line_by_line(seed, storage):
    rng = np.random.default_rng(seed)
    rows, cols = 70, 45
    lens = rng.integers(0, 12, rows)
    lens[rng.choice(rows, 3, replace=False)] = rng.integers(cols // 2, cols, 3)
    m = _special(ragged_csr(lens, cols, seed=seed, positive=False), seed)
    if storage == CSC:
        m = R.transpose(m)                          # the same arrays as a 45 x 70 CSC matrix
    p, q = rng.permutation(m[0][0]), rng.permutation(m[0][1])
    assert R.same_mat(R.transform_mat_paq_vec(m, storage, p, q), R.transform_mat_paq_ref(m, storage, p, q))
    assert R.same_mat(R.permute_rows_vec(m, storage, p), R.permute_rows_ref(m, storage, p))
    assert R.same_mat(R.permute_cols_vec(m, storage, q), R.permute_cols_ref(m, storage, q))
    assert R.same_mat(R.transform_mat_paq_ref(m, storage, p, q),
                      R.permute_rows_ref(R.permute_cols_ref(m, storage, q), storage, p))
    n = 40
    sq = _special(ragged_csr(rng.integers(0, 9, n), n, seed=seed + 9, positive=False), seed + 9)
    s = rng.permutation(n)
    got = R.transform_mat_papt_vec(sq, storage, s)
    assert R.same_mat(got, R.transform_mat_papt_ref(sq, storage, s))
    assert R.same_mat(R.transform_mat_papt_ref(got, storage, R.perm_new(s)[1]), sq)


def test_argument_checks_need_no_device(fx):
    from sprs_amd import _ffi
    lib = _ffi.lib
    h, m = C.c_void_p(), C.c_void_p()
    flag = C.c_int32()
    for call in (lambda: lib.sprs_hip_perm_upload(None, 0, None, 8, 1),
                 lambda: lib.sprs_hip_perm_from_device(None, 0, None, 8, 1, None),
                 lambda: lib.sprs_hip_perm_identity(None, 3, 8),
                 lambda: lib.sprs_hip_perm_info(None, None, None, None),
                 lambda: lib.sprs_hip_perm_is_identity(None, C.byref(flag), None),
                 lambda: lib.sprs_hip_perm_device_ptrs(None, None, None),
                 lambda: lib.sprs_hip_perm_download(None, None, None),
                 lambda: lib.sprs_hip_perm_inv(None, C.byref(h)),
                 lambda: lib.sprs_hip_perm_mul_vec_f64(None, None, None, 0, None),
                 lambda: lib.sprs_hip_csmat_transform_paq(None, None, None, C.byref(m), None),
                 lambda: lib.sprs_hip_csmat_transform_papt(None, None, C.byref(m), None)):
        assert call() == _ffi.INVALID_ARG and b"NULL" in lib.sprs_hip_last_error()
    assert lib.sprs_hip_perm_free(None) == _ffi.OK
    a = np.arange(5, dtype=np.uint64)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    assert lib.sprs_hip_perm_upload(C.byref(h), 5, vp(a), 3, 1) == _ffi.INVALID_ARG and b"2, 4 or 8" in lib.sprs_hip_last_error()
    assert lib.sprs_hip_perm_upload(C.byref(h), 5, None, 8, 1) == _ffi.INVALID_ARG
    assert lib.sprs_hip_perm_from_device(C.byref(h), 5, vp(a), 2, 1, None) == _ffi.INVALID_ARG and b"4 or 8" in lib.sprs_hip_last_error()
    assert lib.sprs_hip_perm_identity(C.byref(h), 5, 1) == _ffi.INVALID_ARG
    # perm_is_valid runs on the host for a small permutation, before any device work (permutation.rs:776-782)
    for bad in fx["perm_validity"]["invalid"]:
        for dt in (np.uint16, np.uint32, np.uint64):
            arr = np.array(bad, dtype=dt)
            st = lib.sprs_hip_perm_upload(C.byref(h), arr.size, vp(arr), arr.dtype.itemsize, 1)
            assert st == _ffi.BAD_STRUCTURE and lib.sprs_hip_last_error() == b"invalid permutation" and not h.value


def test_identity_variant_needs_no_device():
    """Permutation::identity has no arrays: info, is_identity, inv, download, the dimension and aliasing checks of P * x"""
    from sprs_amd import _ffi
    from sprs_amd.permutation import DevicePerm
    lib = _ffi.lib
    for dt in (np.uint16, np.uint32, np.uint64):
        p = DevicePerm.identity(7, dt)
        assert p.dim == 7 and p.index_bytes() == np.dtype(dt).itemsize and p.is_identity_variant() and p.is_identity()
        q = p.inv()
        assert q.is_identity_variant() and q.dim == 7 and q.index_bytes() == np.dtype(dt).itemsize
        assert p.vec().dtype == dt and p.vec().tolist() == list(range(7)) and p.inv_vec().tolist() == list(range(7))
        a, b = C.c_void_p(), C.c_void_p()
        assert lib.sprs_hip_perm_device_ptrs(p._h, C.byref(a), C.byref(b)) == _ffi.OK and not a.value and not b.value
    p = DevicePerm.identity(4)
    x = np.zeros(16)
    at = lambda k: C.c_void_p(x.ctypes.data + 8 * k)
    assert lib.sprs_hip_perm_mul_vec_f64(p._h, at(0), at(8), 5, None) == _ffi.DIM_MISMATCH
    assert lib.sprs_hip_last_error() == b"Dimension mismatch"
    assert lib.sprs_hip_perm_mul_vec_f64(p._h, None, at(8), 4, None) == _ffi.INVALID_ARG
    for xo, yo in ((0, 0), (0, 3), (3, 0), (2, 1)):
        assert lib.sprs_hip_perm_mul_vec_f64(p._h, at(xo), at(yo), 4, None) == _ffi.INVALID_ARG
        assert b"overlap" in lib.sprs_hip_last_error()
    assert DevicePerm.identity(0).vec().size == 0


def test_published_fixed_options():
    import sprs_amd
    for name in ("perm_tile", "perm_cap"):
        t = sprs_amd.get_option(name)
        assert t >= 256 and t % 256 == 0
        for v in (t - 1, t + 1, 0):
            with pytest.raises(sprs_amd.SprsHipError):
                sprs_amd.set_option(name, v)
        sprs_amd.set_option(name, t)
