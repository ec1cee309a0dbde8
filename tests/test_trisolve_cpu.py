"""CPU checks of the sparse triangular solves: the Python restatement used by the GPU tests reproduces the reference's own
unit tests (trisolve.rs:368-442) and agrees with scipy on diagonally dominant systems; the entry point is exported and bound,
checks its arguments without a device and never computes without one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import trisolve_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixtures():
    return json.load(open(os.path.join(HERE, "golden", "trisolve_fixtures.json")))["systems"]


def test_restatement_reproduces_the_reference_unit_tests():
    systems = _fixtures()
    assert sorted(s["solve"] for s in systems) == sorted(ref.SOLVES)
    for s in systems:
        n = s["shape"][0]
        assert s["shape"] == [n, n] and s["storage"] == ("CSC" if s["solve"].endswith("csc") else "CSR")
        x = ref.SOLVES[s["solve"]](n, s["indptr"], s["indices"], s["data"], s["b"])
        assert np.array_equal(x, np.array(s["x"], dtype=np.float64)), s["solve"]


def _system(n, seed):
    """non-symmetric, strictly diagonally dominant, full (both triangles present)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=seed, data_rvs=rng.standard_normal).tocsr()
    a = (a + sp.diags(np.abs(a).sum(axis=1).A1 + 1.0 + rng.random(n))).tocsr()
    a.sort_indices()
    return a


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_restatement_agrees_with_scipy(n):
    """to 1e-12 of max |x| (residuals of such systems are ~1e-15: the bound only guards the restatement's logic)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve_triangular
    a = _system(n, 100 + n)
    b = np.random.default_rng(n).standard_normal(n)
    for kind in ref.SOLVES:
        lower = kind[0] == "l"
        m = a.tocsc() if kind.endswith("csc") else a
        m.sort_indices()
        x = ref.SOLVES[kind](n, m.indptr, m.indices, m.data, b)
        want = spsolve_triangular((sp.tril(a) if lower else sp.triu(a)).tocsr(), b, lower=lower)
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max(), kind
        assert 1 <= ref.levels(kind, n, m.indptr, m.indices) <= n
    # the level count does not depend on the storage the triangle comes in
    c = a.tocsc()
    c.sort_indices()
    for uplo in "lu":
        assert ref.levels(uplo + "solve_csr", n, a.indptr, a.indices) == ref.levels(uplo + "solve_csc", n, c.indptr, c.indices)


def test_restatement_singular_returns():
    # | 1     |   row 1 has no diagonal; | 0 . | an explicit zero
    with pytest.raises(ref.Singular) as e:
        ref.lsolve_csr_dense_rhs(2, [0, 1, 2], [0, 0], [1.0, 1.0], [1.0, 1.0])
    assert (e.value.index, e.value.reason) == (1, "diagonal element is 0")
    with pytest.raises(ref.Singular) as e:
        ref.usolve_csr_dense_rhs(2, [0, 1, 2], [0, 1], [-0.0, 1.0], [1.0, 1.0])
    assert (e.value.index, e.value.reason) == (0, "diagonal element is a numeric 0")
    with pytest.raises(ref.Singular) as e:
        ref.lsolve_csc_dense_rhs(2, [0, 1, 2], [1, 1], [1.0, 0.0], [1.0, 1.0])
    assert (e.value.index, e.value.reason) == (0, "diagonal element is a structural 0")
    with pytest.raises(ref.Singular) as e:
        ref.usolve_csc_dense_rhs(2, [0, 1, 2], [1, 1], [1.0, 0.0], [1.0, 1.0])
    assert (e.value.index, e.value.reason) == (1, "diagonal element is a numeric 0")
    assert str(e.value) == "Singular matrix at index 1 (diagonal element is a numeric 0)"


def test_entry_point_is_exported_and_bound():
    import sprs_amd
    from sprs_amd import _ffi, linalg
    assert hasattr(_ffi.lib, "sprs_hip_trisolve_f64") and "sprs_hip_trisolve_f64" in _ffi.SIGNATURES
    assert (_ffi.SINGULAR_MATRIX, _ffi.LOWER, _ffi.UPPER) == (9, 0, 1)
    for name in ("lsolve_csr_dense_rhs", "usolve_csr_dense_rhs", "lsolve_csc_dense_rhs", "usolve_csc_dense_rhs"):
        assert getattr(sprs_amd, name) is getattr(linalg, name)
    header = open(os.path.join(os.path.dirname(HERE), "include", "sprs_hip.h")).read()
    assert "sprs_hip_trisolve_info" in header and "#define SPRS_HIP_SINGULAR_MATRIX 9" in header


def test_argument_checks_need_no_device():
    from sprs_amd import _ffi
    x = np.ones(4)
    st = _ffi.lib.sprs_hip_trisolve_f64(None, _ffi.LOWER, C.c_void_p(x.ctypes.data), 4, None, None)
    assert st == _ffi.INVALID_ARG and b"NULL handle" in _ffi.lib.sprs_hip_last_error()


def test_wrappers_raise_without_a_device():
    """no CPU fallback: on a machine without a GPU there is no DeviceCsMat to solve with"""
    import sprs_amd
    from sprs_amd.device import DeviceCsMat, DeviceVec
    if sprs_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    for fn in (sprs_amd.lsolve_csr_dense_rhs, sprs_amd.usolve_csr_dense_rhs, sprs_amd.lsolve_csc_dense_rhs, sprs_amd.usolve_csc_dense_rhs):
        with pytest.raises(sprs_amd.SprsHipError) as e:
            fn(DeviceCsMat.eye(4), DeviceVec.from_host(np.ones(4)))
        assert e.value.status == sprs_amd._ffi.NO_DEVICE
