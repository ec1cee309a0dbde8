"""Single precision without a GPU: the numpy restatements of tests/f32_ref.py against the reference's own f32 material (its
mul_csr_vec golden vector, its test_bicgstab_f32 system) and the argument checks of the f32 entry points, which need no
device."""
import ctypes as C

import numpy as np

import f32_ref
from conftest import as_csr


def test_chain_restatement_matches_the_golden_vector(golden):
    fx = golden["mul_csr_vec"]
    shape, ip, ix, dt = as_csr(fx)
    y = f32_ref.mul_vec(shape, ip, ix, dt.astype(np.float32), np.array(fx["x"], dtype=np.float32))
    assert y.dtype == np.float32
    assert np.all(np.abs(y.astype(np.float64) - np.array(fx["expected"])) < fx["epsilon"])
    # accumulate form: the chain starts from y0, empty rows keep its bits
    y0 = np.array([1.0, -0.0, 2.0, 3.0, 4.0], dtype=np.float32)
    ya = f32_ref.mul_acc_mat_vec_csr(shape, ip, ix, dt.astype(np.float32), np.array(fx["x"], dtype=np.float32), y0.copy())
    assert ya[1].tobytes() == y0[1].tobytes()
    assert np.all(np.abs(ya.astype(np.float64) - (y0 + np.array(fx["expected"]))) < 1e-6)


def test_bicgstab_restatement_on_the_reference_f32_system():
    """test_bicgstab_f32 (bicgstab.rs:313-350): Ok, and |1 - b_i / (A x)_i| < 1e-18 in f32"""
    csr = f32_ref.csc_to_csr(*f32_ref.REF_SYSTEM_CSC)
    one = np.ones(4, dtype=np.float32)
    solver, ok = f32_ref.BiCGSTAB.solve(csr, one, one, f32_ref.REF_TOL, f32_ref.REF_MAX_ITER)
    assert ok
    b_recovered = f32_ref.mul_vec(*csr, solver.x)
    for i in range(4):
        assert np.abs(np.float32(1.0) - one[i] / b_recovered[i]) < np.float32(f32_ref.REF_TOL), "Solved output did not match input"
    print("iterations %d soft %d hard %d err %r" % (solver.iteration_count, solver.soft_restart_count, solver.hard_restart_count,
                                                     solver.err))
    assert solver.err.dtype == np.float32 and solver.rho.dtype == np.float32 and solver.x.dtype == np.float32
    assert solver.iteration_count <= f32_ref.REF_MAX_ITER and solver.hard_restart_count >= 1


def test_csc_to_csr_restatement():
    shape, ip, ix, dt = f32_ref.csc_to_csr(*f32_ref.REF_SYSTEM_CSC)
    dense = np.zeros((4, 4), dtype=np.float32)
    cip, cix, cdt = f32_ref.REF_SYSTEM_CSC[1:]
    for c in range(4):
        for k in range(int(cip[c]), int(cip[c + 1])):
            dense[int(cix[k]), c] = cdt[k]
    for r in range(4):
        cols = ix[ip[r]:ip[r + 1]]
        assert np.all(np.diff(cols) > 0)
        assert np.array_equal(dense[r, cols], dt[ip[r]:ip[r + 1]]) and np.count_nonzero(dense[r]) == cols.size


def test_null_handles_are_refused_without_a_device():
    from sprs_amd import _ffi
    lib, bad = _ffi.lib, _ffi.INVALID_ARG
    out = C.c_void_p()
    ip = np.array([0, 1], dtype=np.uint64)
    ix = np.array([0], dtype=np.uint64)
    dt = np.ones(1, dtype=np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.sprs_hip_csmat_f32_upload(None, 0, 1, 1, vp(ip), 8, vp(ix), 8, vp(dt), 1) == bad
    assert lib.sprs_hip_csmat_f32_upload(C.byref(out), 0, 1, 1, None, 8, vp(ix), 8, vp(dt), 1) == bad
    assert lib.sprs_hip_csmat_f32_wrap_device(None, 0, 1, 1, 1, None, 8, None, 8, None) == bad
    assert lib.sprs_hip_csmat_f32_info(None, None, None, None, None, None, None) == bad
    assert lib.sprs_hip_csmat_f32_device_ptrs(None, None, None, None) == bad
    assert lib.sprs_hip_csmat_f32_download(None, None, None, None) == bad
    assert lib.sprs_hip_csmat_f32_transpose_view(None, C.byref(out)) == bad
    assert lib.sprs_hip_csmat_f32_refresh(None) == bad
    assert lib.sprs_hip_csmat_f32_prepare(None, None) == bad
    assert lib.sprs_hip_csmat_f32_to_other_storage(None, C.byref(out)) == bad
    assert lib.sprs_hip_csmat_f32_from_f64(None, C.byref(out), None) == bad
    assert lib.sprs_hip_csmat_f32_to_f64(None, C.byref(out), None) == bad
    assert lib.sprs_hip_spmv_f32(None, None, 0, None, 0, 0, None) == bad
    assert lib.sprs_hip_mul_acc_mat_vec_csc_f32(None, None, 0, None, 0, None) == bad
    assert lib.sprs_hip_csmat_mul_vec_f32(None, None, 0, None, 0, None) == bad
    assert lib.sprs_hip_bicgstab_f32(None, None, None, 0, 1e-6, 1, 0.1, None, None, None) == bad
    assert b"NULL" in lib.sprs_hip_last_error()
    assert lib.sprs_hip_csmat_f32_free(None) == _ffi.OK          # like free(NULL)


def test_upload_argument_checks_need_no_device():
    """the same validate rule and texts as the f64 upload; 2-byte host arrays are refused with a message that says so"""
    from sprs_amd import _ffi
    lib = _ffi.lib
    h = C.c_void_p()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    dt = np.ones(2, dtype=np.float32)
    ip16, ix16 = np.array([0, 1], dtype=np.uint16), np.array([0], dtype=np.uint16)
    for pb, ib in ((2, 2), (2, 4), (4, 2), (8, 2)):
        assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 0, 1, 1, vp(ip16), pb, vp(ix16), ib, vp(dt), 1) == _ffi.INVALID_ARG
        msg = lib.sprs_hip_last_error()
        assert b"4 or 8 bytes" in msg and b"2-byte" in msg
    ip = np.array([0, 2], dtype=np.uint64)
    assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 7, 1, 2, vp(ip), 8, vp(ip), 8, vp(dt), 1) == _ffi.INVALID_ARG
    ix = np.array([1, 0], dtype=np.uint64)
    assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 0, 1, 2, vp(ip), 8, vp(ix), 8, vp(dt), 1) == _ffi.BAD_STRUCTURE
    assert b"not sorted" in lib.sprs_hip_last_error()
    ix = np.array([0, 5], dtype=np.uint32)
    assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 0, 1, 2, vp(ip), 8, vp(ix), 4, vp(dt), 1) == _ffi.BAD_STRUCTURE
    assert b"larger than inner dimension" in lib.sprs_hip_last_error()
    assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 0, 1, 2, vp(ip), 8, None, 8, vp(dt), 1) == _ffi.INVALID_ARG
