"""The Python restatement of the reference's sparse binops (tests/binop_ref.py) against the reference's own expectations
(sprs/src/sparse/binop.rs:488-598), its vectorised twin against the line-by-line one, and the argument checks of the new
entry points, which need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from binop_ref import ADD, MUL, SUB, csmat_binop_ref, csmat_binop_vec, csvec_binop_ref, csvec_binop_vec, same_mat, same_vec
from conftest import ROOT, as_csr
from helpers import ragged_csr


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "binop_fixtures.json")) as f:
        return json.load(f)


def _v(d):
    return d["dim"], d["indices"], d["data"]


@pytest.mark.parametrize("ref", [csmat_binop_ref, csmat_binop_vec])
def test_reference_expectations_matrices(golden, fx, ref):
    m1, m2 = as_csr(golden["mat1"]), as_csr(golden["mat2"])
    for name, op in (("mat1_plus_mat2", ADD), ("mat1_minus_mat2", SUB), ("mat1_times_mat2", MUL)):
        assert same_mat(ref(m1, m2, op), as_csr(fx[name])), name
    assert ref(m1, m2, ADD)[1].tolist() == [0, 5, 8, 9, 12, 15]
    assert ref(m1, m2, SUB)[1].tolist() == [0, 4, 7, 8, 11, 14]
    t = ref(m1, m2, MUL)
    assert t[1].tolist() == [0, 1, 2, 2, 2, 2] and t[2].tolist() == [2, 3] and t[3].tolist() == [9.0, 18.0]
    c = fx["differing_row_patterns"]
    assert same_mat(ref(as_csr(c["a"]), as_csr(c["b"]), ADD), as_csr(c["a_plus_b"]))


def test_reference_expectation_smul(golden):
    """&mat1() * 2. == mat1_times_2(): map keeps the structure"""
    m1, want = as_csr(golden["mat1"]), as_csr(golden["mat1_times_2"])
    assert same_mat((m1[0], m1[1], m1[2], m1[3] * 2.0), want)


@pytest.mark.parametrize("ref", [csvec_binop_ref, csvec_binop_vec])
def test_reference_expectations_vectors(fx, ref):
    c = fx["csvec_binops"]
    assert same_vec(ref(_v(c["vec1"]), _v(c["vec2"]), ADD), _v(c["vec1_plus_vec2"]))
    assert same_vec(ref(_v(c["vec1"]), _v(c["vec3"]), ADD), _v(c["vec1_plus_vec3"]))
    z = fx["zero_sized_vector"]
    assert same_vec(ref(_v(z["vector"]), _v(z["zero"]), ADD), _v(z["vector"]))
    assert same_vec(ref(_v(z["zero"]), _v(z["vector"]), ADD), _v(z["vector"]))
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        ref((8, [1], [1.0]), (9, [1], [1.0]), ADD)


def test_signed_zero_facts():
    """what the vector tests pin: numpy and Python floats agree with IEEE 754"""
    for l, r, op, want_sign in ((-0.0, 0.0, ADD, False), (0.0, -0.0, SUB, False), (-0.0, 0.0, SUB, True)):
        for ref in (csvec_binop_ref, csvec_binop_vec):
            d = ref((1, [0], [l]), (1, [0], [r]), op)[2]
            assert d[0] == 0.0 and bool(np.signbit(d[0])) == want_sign
    for ref in (csmat_binop_ref, csmat_binop_vec):
        one = lambda x: ((1, 1), [0, 1], [0], [x])
        none = ((1, 1), [0, 0], [], [])
        assert ref(one(-0.0), none, ADD)[2].size == 0 and ref(one(5.0), one(-5.0), ADD)[2].size == 0
        assert np.isnan(ref(one(float("inf")), none, MUL)[3][0]) and ref(one(-3.0), none, MUL)[2].size == 0


def _ragged(seed, rows, cols, nans=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 25, rows)
    lens[rng.choice(rows, 3, replace=False)] = rng.integers(cols // 2, cols, 3)
    m = ragged_csr(lens, cols, seed=seed, positive=False)
    dt = np.round(m[3] * 2) / 2
    if nans:                                        # (one operand only: which of TWO NaN operands an addition hands on is the compiler's choice)
        dt[rng.random(dt.size) < 0.02] = np.nan
    dt[rng.random(dt.size) < 0.02] = np.inf
    dt[rng.random(dt.size) < 0.05] = -0.0
    return m[0], m[1], m[2], dt


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_vectorised_twin_equals_line_by_line(seed):
    a, b = _ragged(seed, 120, 90), _ragged(seed + 50, 120, 90, nans=False)
    with np.errstate(invalid="ignore"):
        for op in (ADD, SUB, MUL):
            assert same_mat(csmat_binop_vec(a, b, op), csmat_binop_ref(a, b, op))
            r = 7
            v = (90, a[2][a[1][r]:a[1][r + 1]], a[3][a[1][r]:a[1][r + 1]])
            w = (90, b[2][b[1][r]:b[1][r + 1]], b[3][b[1][r]:b[1][r + 1]])
            assert same_vec(csvec_binop_vec(v, w, op), csvec_binop_ref(v, w, op))


def test_argument_checks_need_no_device():
    from sprs_amd import _ffi
    assert (_ffi.BINOP_ADD, _ffi.BINOP_SUB, _ffi.BINOP_MUL) == (0, 1, 2)
    h = C.c_void_p()
    lib = _ffi.lib
    for call in (lambda: lib.sprs_hip_csmat_binop_f64(None, None, _ffi.BINOP_ADD, C.byref(h), None),
                 lambda: lib.sprs_hip_csmat_add_csmat_f64(None, None, C.byref(h), None),
                 lambda: lib.sprs_hip_csmat_sub_csmat_f64(None, None, C.byref(h), None),
                 lambda: lib.sprs_hip_csmat_scale_f64(None, 2.0, C.byref(h), None),
                 lambda: lib.sprs_hip_csvec_binop_f64(None, None, _ffi.BINOP_SUB, C.byref(h), None)):
        assert call() == _ffi.INVALID_ARG and b"NULL" in lib.sprs_hip_last_error()
    for bad in (-1, 3, 99):
        assert lib.sprs_hip_csmat_binop_f64(None, None, bad, C.byref(h), None) == _ffi.INVALID_ARG
        assert b"SPRS_HIP_BINOP_ADD" in lib.sprs_hip_last_error()
        assert lib.sprs_hip_csvec_binop_f64(None, None, bad, C.byref(h), None) == _ffi.INVALID_ARG
        assert b"SPRS_HIP_BINOP_ADD" in lib.sprs_hip_last_error()


def test_tile_is_a_published_fixed_option():
    import sprs_amd
    t = sprs_amd.get_option("binop_tile")
    assert t >= 256 and t % 256 == 0
    for v in (t - 1, t + 1, 0):
        with pytest.raises(sprs_amd.SprsHipError):
            sprs_amd.set_option("binop_tile", v)
    sprs_amd.set_option("binop_tile", t)
