"""CPU checks of the yardstick of the matrix extraction: the plain-Python restatement (tests/extract_ref.py) reproduces the
numbers of the reference's own tests (tests/golden/reduce_fixtures.json), carries the last-maximum rule of to_inner_onehot, and
the C entry points refuse bad arguments without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import extract_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(HERE, "golden", "reduce_fixtures.json")))


def _data(a):
    return np.array([NAN if x == "nan" else float(x) for x in a], dtype=np.float64)


def test_diag_fixtures(fx):
    """csmat.rs:2875-2948 diag and diag_rectangular"""
    for name in ("diag", "diag_rectangular"):
        m = fx[name]
        n, oi, od = ref.diag(m["shape"], m["indptr"], m["indices"], _data(m["data"]))
        e = m["expected"]
        assert n == e["dim"] and oi.tolist() == e["indices"] and od.tolist() == e["data"]


def test_nnz_index_fixture(fx):
    """csmat.rs:2622-2637: the identity of order 11 (CSR and, the diagonal being its own transpose, CSC)"""
    q = fx["mat_nnz_index"]
    n = q["eye"]
    ip, ix = np.arange(n + 1), np.arange(n)
    for row, col, want in q["queries"]:
        assert ref.nnz_index(ip, ix, False, row, col) == want == ref.nnz_index(ip, ix, True, row, col)


def test_onehot_fixtures(fx):
    """csmat.rs:2951-2999"""
    assert [m["name"] for m in fx["onehot"]] == ["onehot_zero", "onehot_eye", "onehot_sparse_csc", "onehot_ignores_nan"]
    for m in fx["onehot"]:
        ip, ix, dt = ref.to_inner_onehot(m["indptr"], m["indices"], _data(m["data"]))
        e = m["expected"]
        assert ip.tolist() == e["indptr"] and ix.tolist() == e["indices"] and dt.tolist() == e["data"], m["name"]


def test_onehot_takes_the_last_of_equal_maxima():
    """Iterator::max_by returns the last maximum; -0.0 and +0.0 compare equal; NaNs are skipped, infinities take part"""
    one = lambda idx, dat: ref.to_inner_onehot([0, len(idx)], idx, dat)[1].tolist()
    assert one([2, 5, 7], [3.0, 3.0, 3.0]) == [7] and one([2, 5, 7], [3.0, 1.0, 3.0]) == [7] and one([2, 5, 7], [3.0, 3.0, 1.0]) == [5]
    assert one([1, 4], [0.0, -0.0]) == [4] and one([1, 4], [-0.0, 0.0]) == [4]
    assert one([1, 4], [NAN, NAN]) == [] and one([1, 4, 6], [NAN, -np.inf, NAN]) == [4]
    assert one([1, 4, 6], [-np.inf, -np.inf, NAN]) == [4] and one([0, 3], [np.inf, 1e308]) == [0]
    ip, ix, dt = ref.to_inner_onehot([0, 0, 2, 2, 3], [1, 2, 0], [NAN, NAN, -1.0])
    assert ip.tolist() == [0, 0, 0, 0, 1] and ix.tolist() == [0] and dt.tolist() == [1.0]


def test_outer_view_and_diag_of_the_transpose():
    """the diagonal of the transpose is the diagonal: one walk serves CSR and CSC"""
    rng = np.random.default_rng(5)
    rows, cols = 9, 13
    dense = np.where(rng.random((rows, cols)) < 0.3, rng.standard_normal((rows, cols)), 0.0)
    ip, ix, dt = [0], [], []
    for r in range(rows):
        nz = np.nonzero(dense[r])[0]
        ix += nz.tolist()
        dt += dense[r, nz].tolist()
        ip.append(len(ix))
    n, oi, od = ref.diag((rows, cols), ip, ix, dt)
    want = [i for i in range(min(rows, cols)) if dense[i, i] != 0.0]
    assert n == 9 and oi.tolist() == want and od.tolist() == [dense[i, i] for i in want]
    vi, vd = ref.outer_view(ip, ix, dt, 3)
    assert vi.tolist() == np.nonzero(dense[3])[0].tolist() and ref.outer_view(ip, ix, dt, rows) is None
    for r in range(rows):
        for c in range(cols):
            p = ref.nnz_index(ip, ix, False, r, c)
            assert (p is None) == (dense[r, c] == 0.0) and (p is None or dt[p] == dense[r, c])
    assert ref.nnz_index(ip, ix, False, rows, 0) is None and ref.nnz_index(ip, ix, False, 0, cols) is None


def test_entry_points_check_arguments_without_a_device():
    from sprs_amd import _ffi
    lib = _ffi.lib
    h = C.c_void_p()
    assert lib.sprs_hip_csmat_outer_view(None, 0, C.byref(h), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csmat_diag_f64(None, C.byref(h), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csmat_nnz_index(None, 0, None, None, None, None, None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csmat_to_inner_onehot_f64(None, C.byref(h), None) == _ffi.INVALID_ARG
    assert b"NULL" in lib.sprs_hip_last_error()
