"""CPU-only checks of the dense <-> sparse boundary: tests/dense_ref.py reproduces sprs' own test vectors
(tests/golden/dense_fixtures.json), its line-by-line functions and its numpy twins agree bit for bit, and the argument checks
of the new entries and of their Python mirrors report what the reference reports, in its order, without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dense_ref as R
from conftest import ROOT

CSR, CSC = R.CSR, R.CSC
FAKE = 0x10000          # a device address that is never dereferenced: every call below fails in its argument checks


ENTRIES = ("sprs_hip_csmat_from_dense_f64", "sprs_hip_csmat_assign_to_dense_f64", "sprs_hip_csmat_to_dense_f64",
           "sprs_hip_csmat_binop_dense_f64", "sprs_hip_csmat_add_dense_f64")


@pytest.fixture(scope="module", autouse=True)
def _the_library_has_the_entries():
    """the restatement below is the yardstick of these entries: without them there is nothing for it to measure"""
    from sprs_amd import _ffi, to_dense  # noqa: F401
    for name in ENTRIES:
        assert hasattr(_ffi.lib, name) and name in _ffi.SIGNATURES, name


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "dense_fixtures.json")) as f:
        return json.load(f)


def fmat(d):
    return R.mat(d["storage"], d["shape"], d["indptr"], d["indices"], d["data"])


def eye(dim, storage=CSR):
    return R.mat(storage, (dim, dim), list(range(dim + 1)), list(range(dim)), [1.0] * dim)


# ---- the reference's own vectors -------------------------------------------------------------------------------------------------

def test_to_dense_fixtures(fx):
    """to_dense.rs:56-92"""
    c = fx["to_dense"]
    for storage in (CSR, CSC):
        deye = np.zeros((c["eye_dim"],) * 2)
        R.assign_to_dense(deye, eye(c["eye_dim"], storage))
        assert R.same_dense(deye, np.eye(c["eye_dim"]))
    assert R.same_dense(R.to_dense(fmat(fx["mat1"])), np.array(c["mat1_expected"]))
    assert R.same_dense(R.to_dense(fmat(fx["mat3"])), np.array(c["mat3_expected"]))
    assert R.same_dense(R.to_dense_vec(fmat(fx["mat3"])), np.array(c["mat3_expected"]))


def test_from_dense_fixtures(fx):
    """csmat.rs:2494-2540, both epsilons"""
    c = fx["from_dense"]
    assert R.same_mat(R.csr_from_dense(np.eye(c["eye_dim"]), c["eye_epsilon"]), eye(c["eye_dim"], CSR))
    assert R.same_mat(R.csc_from_dense(np.eye(c["eye_dim"]), c["eye_epsilon"]), eye(c["eye_dim"], CSC))
    m = np.array(c["m"])
    assert R.same_mat(R.csr_from_dense(m, c["epsilon"]), fmat(c["csr_expected"]))
    assert R.same_mat(R.csc_from_dense(m, c["epsilon"]), fmat(c["csc_expected"]))
    assert R.same_mat(R.from_dense_vec(m, c["epsilon"], CSR), fmat(c["csr_expected"]))
    assert R.same_mat(R.from_dense_vec(m, c["epsilon"], CSC), fmat(c["csc_expected"]))


def test_binop_dense_fixtures(fx):
    """binop.rs:600-690"""
    c = fx["csr_add_dense_rowmaj"]
    n = c["eye_dim"]
    assert R.same_dense(R.add_dense_mat_same_ordering(eye(n), np.full((n, n), c["eye_rhs_fill"]), c["alpha"], c["beta"]), np.eye(n))
    a, b, want = fmat(fx["mat1"]), np.array(fx["mat_dense1"]), np.array(c["mat1_plus_mat_dense1"])
    assert R.same_dense(R.add_dense_mat_same_ordering(a, b, c["alpha"], c["beta"]), want)
    assert R.same_dense(R.add_dense(a, b), want)
    assert R.same_dense(R.add_dense(R.to_other_storage(a), b), want)
    assert R.same_dense(R.add_dense(a, np.asfortranarray(b), "F"), want)
    c = fx["csr_mul_dense_rowmaj"]
    n = c["eye_dim"]
    assert R.same_dense(R.mul_dense_mat_same_ordering(eye(n), np.full((n, n), c["rhs_fill"]), c["alpha"]), np.eye(n))
    c = fx["binop_standard_layouts"]
    for pair in c["pairs"]:
        shape = tuple(c["shape"])
        outer = shape[0] if pair["storage"] == CSR else shape[1]
        zero = R.mat(pair["storage"], shape, [0] * (outer + 1), [], [])
        out = np.full(shape, c["rhs_fill"], order=pair["order"])
        R.csmat_binop_dense_raw(zero, np.full(shape, c["rhs_fill"], order=pair["order"]), lambda x, y: 0.0, out, pair["order"], pair["order"])
        assert R.same_dense(out, np.zeros(shape))


def test_reference_asserts():
    a = eye(3)
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        R.assign_to_dense(np.zeros((3, 4)), a)
    with pytest.raises(AssertionError, match="Dimension mismatch"):     # both wrong: the dimensions are reported
        R.csmat_binop_dense_raw(a, np.zeros((4, 3)), R.closure(R.ADD, 1, 1), np.zeros((4, 3)), "F", "F")
    with pytest.raises(AssertionError, match="Storage mismatch"):
        R.csmat_binop_dense_raw(a, np.zeros((3, 3)), R.closure(R.ADD, 1, 1), np.zeros((3, 3)), "F", "F")
    with pytest.raises(AssertionError, match="Storage mismatch"):
        R.csmat_binop_dense_raw(a, np.zeros((3, 3)), R.closure(R.ADD, 1, 1), np.zeros((3, 3)), "C", "F")


# ---- loop against numpy twin -----------------------------------------------------------------------------------------------------

def special_dense(shape, seed, eps=0.25):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(shape)
    m[rng.random(shape) < 0.5] = 0.0
    for v in (-0.0, np.nan, np.inf, -np.inf, 5e-324, eps, -eps):
        m[rng.random(shape) < 0.04] = v
    return m


@pytest.mark.parametrize("epsilon", [0.0, -1.0, float("nan"), 0.25, float("inf")])
def test_from_dense_loop_equals_twin(epsilon):
    for seed, shape in enumerate([(7, 13), (1, 40), (40, 1), (0, 5), (5, 0)]):
        m = special_dense(shape, seed)
        for storage in (CSR, CSC):
            got, want = R.from_dense_vec(m, epsilon, storage), R.from_dense(m, epsilon, storage)
            assert R.same_mat(got, want)
            assert not np.isnan(want[4]).any() and not (want[4] == 0).any()
            if epsilon == 0.25:
                assert not (np.abs(want[4]) == 0.25).any()


def test_assign_and_binop_loop_equals_twin():
    for seed in range(4):
        rng = np.random.default_rng(seed)
        shape = (9, 6) if seed % 2 else (5, 11)
        lhs = R.from_dense(special_dense(shape, seed + 10) + 0.0, 0.0, seed // 2)
        lhs = (lhs[0], lhs[1], lhs[2], lhs[3], np.where(rng.random(lhs[4].size) < 0.2, -0.0, lhs[4]))
        order = "C" if lhs[0] == CSR else "F"
        sentinel = np.full(shape, 7.5)
        assert R.same_dense(R.assign_to_dense_vec(sentinel.copy(), lhs), R.assign_to_dense(sentinel.copy(), lhs))
        rhs = np.array(special_dense(shape, seed + 20), order=order)
        for alpha, beta in ((1, 1), (-1, 1), (2.5, -0.5), (0, 1), (np.inf, 1)):
            want = R.add_dense_mat_same_ordering(lhs, rhs, alpha, beta, order)
            got = R.binop_dense_vec(lhs, rhs, R.ADD, alpha, beta)
            with np.errstate(invalid="ignore"):
                both_nan = np.isnan(alpha * R.to_dense_vec(lhs)) & np.isnan(rhs)
            assert np.array_equal(R.bits(got)[~both_nan], R.bits(want)[~both_nan]) and np.isnan(got[both_nan]).all()
        for alpha in (1, -1, 0, np.inf):
            want = R.mul_dense_mat_same_ordering(lhs, rhs, alpha, order)
            got = R.binop_dense_vec(lhs, rhs, R.MUL, alpha)
            with np.errstate(invalid="ignore"):
                both_nan = np.isnan(alpha * R.to_dense_vec(lhs)) & np.isnan(rhs)
            assert np.array_equal(R.bits(got)[~both_nan], R.bits(want)[~both_nan]) and np.isnan(got[both_nan]).all()
    # the operation is performed where lhs stores nothing (binop.rs:426)
    z = R.mat(CSR, (1, 2), [0, 0], [], [])
    r = np.array([[-0.0, np.inf]])
    assert R.bits(R.add_dense_mat_same_ordering(z, r, -1.0, 1.0))[0, 0] == 0x8000000000000000
    assert R.bits(R.add_dense_mat_same_ordering(z, r, 1.0, 1.0))[0, 0] == 0
    assert np.isnan(R.mul_dense_mat_same_ordering(z, r, 1.0)[0, 1])


# ---- the argument checks of the library, without a device ------------------------------------------------------------------------

def err():
    from sprs_amd import _ffi
    return _ffi.lib.sprs_hip_last_error().decode()


def test_from_dense_argument_checks():
    from sprs_amd import _ffi
    lib, h, p = _ffi.lib, C.c_void_p(), C.c_void_p(FAKE)
    ok = dict(storage=0, rows=3, cols=5, layout=_ffi.ROW_MAJOR, ld=5, ib=8, xb=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sprs_hip_csmat_from_dense_f64(C.byref(h), a["storage"], p, a["rows"], a["cols"], a["layout"], a["ld"], 0.0, a["ib"], a["xb"], None)

    assert call(ld=4) == _ffi.INVALID_ARG and "leading dimension" in err()
    assert call(layout=_ffi.COL_MAJOR, ld=2) == _ffi.INVALID_ARG and "leading dimension" in err()
    assert call(layout=2) == _ffi.INVALID_ARG and "layout" in err()
    assert call(ib=3) == _ffi.INVALID_ARG and "2, 4 or 8" in err()
    assert call(xb=1) == _ffi.INVALID_ARG and "2, 4 or 8" in err()
    assert call(storage=5) == _ffi.INVALID_ARG and "storage" in err()
    assert lib.sprs_hip_csmat_from_dense_f64(None, 0, p, 3, 5, 0, 5, 0.0, 8, 8, None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csmat_from_dense_f64(C.byref(h), 0, None, 3, 5, 0, 5, 0.0, 8, 8, None) == _ffi.INVALID_ARG and "NULL" in err()
    assert h.value is None


def test_assign_and_binop_argument_checks():
    from sprs_amd import _ffi
    lib, p, q = _ffi.lib, C.c_void_p(FAKE), C.c_void_p(FAKE << 4)
    for f in (lib.sprs_hip_csmat_assign_to_dense_f64, lib.sprs_hip_csmat_to_dense_f64):
        assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 4, None) == _ffi.INVALID_ARG and "leading dimension" in err()
        assert f(None, p, 3, 5, _ffi.COL_MAJOR, 2, None) == _ffi.INVALID_ARG and "leading dimension" in err()
        assert f(None, p, 3, 5, 9, 5, None) == _ffi.INVALID_ARG and "layout" in err()
        assert f(None, None, 3, 5, _ffi.ROW_MAJOR, 5, None) == _ffi.INVALID_ARG and "NULL" in err()
        assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 5, None) == _ffi.INVALID_ARG and "NULL handle" in err()
    f = lib.sprs_hip_csmat_binop_dense_f64
    assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 4, _ffi.BINOP_ADD, 1.0, 1.0, q, 5, None) == _ffi.INVALID_ARG and "leading dimension" in err()
    assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_ADD, 1.0, 1.0, q, 4, None) == _ffi.INVALID_ARG and "leading dimension" in err()
    assert f(None, p, 3, 5, 7, 5, _ffi.BINOP_ADD, 1.0, 1.0, q, 5, None) == _ffi.INVALID_ARG and "layout" in err()
    assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_SUB, 1.0, 1.0, q, 5, None) == _ffi.INVALID_ARG and "op must be" in err()
    assert f(None, p, 3, 5, _ffi.ROW_MAJOR, 5, _ffi.BINOP_MUL, 1.0, 1.0, q, 5, None) == _ffi.INVALID_ARG and "NULL handle" in err()
    f = lib.sprs_hip_csmat_add_dense_f64
    assert f(None, p, 3, 5, _ffi.COL_MAJOR, 2, q, None) == _ffi.INVALID_ARG and "leading dimension" in err()
    assert f(None, p, 3, 5, _ffi.COL_MAJOR, 3, q, None) == _ffi.INVALID_ARG and "NULL handle" in err()


class _Shape:
    """what the Python mirrors look at before they call the library: a handle's shape and storage"""

    def __init__(self, rows, cols, csr):
        self._r, self._c, self._csr, self._h = rows, cols, csr, None

    def rows(self): return self._r
    def cols(self): return self._c
    def shape(self): return (self._r, self._c)
    def is_csr(self): return self._csr
    def is_csc(self): return not self._csr


class _Dense:
    def __init__(self, rows, cols, col_major=False):
        self.rows, self.cols, self.col_major = rows, cols, col_major


def test_mirrors_report_dimensions_before_storage():
    from sprs_amd import _ffi, binop, to_dense
    lhs = _Shape(3, 5, True)
    with pytest.raises(_ffi.SprsHipError) as e:          # both wrong (binop.rs:397-412)
        binop.csmat_binop_dense_raw(lhs, _Dense(5, 3, True), binop.ADD, _Dense(5, 3, True))
    assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    with pytest.raises(_ffi.SprsHipError) as e:
        binop.csmat_binop_dense_raw(lhs, _Dense(3, 5, False), binop.ADD, _Dense(3, 4, False))
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(_ffi.SprsHipError) as e:
        binop.csmat_binop_dense_raw(lhs, _Dense(3, 5, True), binop.MUL, _Dense(3, 5, True))
    assert e.value.status == _ffi.STORAGE_MISMATCH and "Storage mismatch" in str(e.value)
    with pytest.raises(_ffi.SprsHipError) as e:          # rhs and out of different fastest axes
        binop.csmat_binop_dense_raw(lhs, _Dense(3, 5, False), binop.MUL, _Dense(3, 5, True))
    assert e.value.status == _ffi.STORAGE_MISMATCH
    with pytest.raises(_ffi.SprsHipError) as e:
        binop.csmat_binop_dense_raw(_Shape(3, 5, False), _Dense(3, 5, False), binop.ADD, _Dense(3, 5, False))
    assert e.value.status == _ffi.STORAGE_MISMATCH
    for f in (lambda: to_dense.assign_to_dense(_Dense(3, 4), lhs), lambda: to_dense.to_dense(lhs, _Dense(4, 5)),
              lambda: binop.add_dense(lhs, _Dense(5, 3))):
        with pytest.raises(_ffi.SprsHipError) as e:
            f()
        assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)


def test_padded_device_mat_is_an_addition():
    """DeviceMat's ld is optional: without it the matrix is what it was"""
    import inspect
    from sprs_amd import prod
    sig = inspect.signature(prod.DeviceMat.__init__)
    assert list(sig.parameters)[:5] == ["self", "rows", "cols", "vec", "col_major"] and sig.parameters["ld"].default is None
    import sprs_amd
    assert sprs_amd.get_option("dense_tile") == 2048
    with pytest.raises(sprs_amd.SprsHipError):
        sprs_amd.set_option("dense_tile", 1024)
