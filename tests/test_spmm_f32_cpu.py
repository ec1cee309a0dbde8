"""The parts of the f32 SpMM that need no device: the argument checks of the four C entries that come before any device work, the
TypeErrors of the Python wrappers for operands of mixed precision, and the numpy chain of tests/spmm_f32_ref.py against a
float64 product on exact-integer data."""
import ctypes as C
import os

import numpy as np
import pytest

import spmm_f32_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_bound_and_mirrored():
    from sprs_amd import _ffi
    names = ("sprs_hip_spmm_rowmaj_f32", "sprs_hip_csmat_mulacc_dense_f32", "sprs_hip_csmat_mul_dense_f32", "sprs_hip_dense_dot_csmat_f32")
    header = open(os.path.join(ROOT, "include", "sprs_hip.h")).read()
    hpp = open(os.path.join(ROOT, "include", "sprs_hip.hpp")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "sprs-hip-sys", "src", "lib.rs")).read()
    rs = open(os.path.join(ROOT, "rust", "sprs-hip", "src", "lib.rs")).read()
    for n in names:
        assert hasattr(_ffi.lib, n) and n in _ffi.SIGNATURES and n in header and n in sys_rs
        # the f32 twin has its f64 namesake's signature
        assert _ffi.SIGNATURES[n] == _ffi.SIGNATURES[n[:-3] + "f64"]
    for n in names[1:]:
        assert n in hpp and n in rs


def test_argument_checks_need_no_device():
    from sprs_amd import _ffi
    lib = _ffi.lib
    msg = lambda: lib.sprs_hip_last_error()
    x = np.ones(8, dtype=np.float32)
    p = C.c_void_p(x.ctypes.data)
    lay = C.c_int32(7)
    assert lib.sprs_hip_spmm_rowmaj_f32(None, p, 2, 2, 2, p, 2, 2, 0, None) == _ffi.INVALID_ARG and b"NULL handle" in msg()
    assert lib.sprs_hip_csmat_mulacc_dense_f32(None, p, 2, 2, 0, 2, p, 2, 0, 2, 0, None) == _ffi.INVALID_ARG and b"NULL handle" in msg()
    assert lib.sprs_hip_csmat_mul_dense_f32(None, p, 2, 2, 0, 2, p, C.byref(lay), None) == _ffi.INVALID_ARG and b"NULL" in msg()
    assert lib.sprs_hip_dense_dot_csmat_f32(p, 2, 2, 0, 2, None, p, C.byref(lay), None) == _ffi.INVALID_ARG and b"NULL" in msg()
    assert lay.value == 7                                   # *out_layout is written on success only


def test_option_spmm_f32_pair_is_a_normal_switch():
    import sprs_amd
    assert sprs_amd.get_option("spmm_f32_pair") == 1
    try:
        sprs_amd.set_option("spmm_f32_pair", 0)
        assert sprs_amd.get_option("spmm_f32_pair") == 0
        sprs_amd.set_option("spmm_f32_pair", 2)
        assert sprs_amd.get_option("spmm_f32_pair") == 2
        for bad in (-1, 3):
            with pytest.raises(sprs_amd.SprsHipError):
                sprs_amd.set_option("spmm_f32_pair", bad)
        assert sprs_amd.get_option("spmm_f32_pair") == 2
    finally:
        sprs_amd.set_option("spmm_f32_pair", 1)


def test_mixed_precision_is_a_type_error_before_the_library_is_called():
    """operands built around null pointers: a wrapper that reached the library would fail otherwise (or crash)"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32
    a32, a64 = DeviceCsMatF32(None), DeviceCsMat(None)
    m32 = lambda r, c: prod.DeviceMatF32(r, c, DeviceVecF32(r * c, ptr=0))
    m64 = lambda r, c: prod.DeviceMat(r, c, DeviceVec(r * c, ptr=0))
    for fn in (prod.csr_mulacc_dense_rowmaj, prod.csr_mulacc_dense_colmaj, prod.csc_mulacc_dense_rowmaj, prod.csc_mulacc_dense_colmaj):
        for args in ((a32, m64(3, 2), m32(3, 2)), (a32, m32(3, 2), m64(3, 2)), (a64, m32(3, 2), m64(3, 2)), (a64, m64(3, 2), m32(3, 2))):
            with pytest.raises(TypeError, match="same precision"):
                fn(*args)
    for mat, rhs in ((a32, m64(3, 2)), (a64, m32(3, 2))):
        with pytest.raises(TypeError):
            prod.csmat_mul_dense(mat, rhs)
        with pytest.raises(TypeError):
            mat * rhs
        with pytest.raises(TypeError):
            mat @ rhs
        with pytest.raises(TypeError):
            prod.dense_dot_csmat(rhs, mat)
    with pytest.raises(TypeError):
        prod.DeviceMatF32(2, 2, DeviceVec(4, ptr=0))
    with pytest.raises(TypeError):
        prod.DeviceMat(2, 2, DeviceVecF32(4, ptr=0))
    assert not issubclass(prod.DeviceMatF32, prod.DeviceMat) and not issubclass(prod.DeviceMat, prod.DeviceMatF32)
    assert m32(2, 3).ld == 3 and prod.DeviceMatF32(2, 3, DeviceVecF32(6, ptr=0), col_major=True).ld == 2
    assert prod.DeviceMatF32(2, 3, DeviceVecF32(10, ptr=0), ld=5).layout == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_chain_against_a_float64_product(seed):
    """integers in [-8, 8], rows of at most 300 entries: every partial sum is an integer far below 2^24, so the f32 chain equals
    the float64 product exactly, in the operator and in the accumulate form; empty rows keep their bits"""
    rng = np.random.default_rng(seed)
    rows, cols, k = 40, 320, 5 + seed
    lens = rng.integers(0, 301, size=rows)
    lens[[3, 17]] = 0
    ip = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    ix = np.concatenate([np.sort(rng.choice(cols, size=int(l), replace=False)) for l in lens]).astype(np.uint32)
    dt = (rng.integers(1, 9, size=ix.size) * rng.choice([-1, 1], size=ix.size)).astype(np.float32)
    rhs = rng.integers(-8, 9, size=(cols, k)).astype(np.float32)
    out0 = rng.integers(-8, 9, size=(rows, k)).astype(np.float32)
    out0[3, 0], out0[17, 1] = np.float32(-0.0), np.float32(np.nan)
    dense = np.zeros((rows, cols))
    dense[np.repeat(np.arange(rows), lens), ix.astype(np.int64)] = dt
    want = dense @ rhs.astype(np.float64)
    got = spmm_f32_ref.mul_dense((rows, cols), ip, ix, dt, rhs)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    acc = spmm_f32_ref.csr_mulacc_dense_rowmaj((rows, cols), ip, ix, dt, rhs, out0.copy())
    full = lens > 0
    assert np.array_equal(acc[full].astype(np.float64), want[full] + out0[full])
    assert acc[~full].tobytes() == out0[~full].tobytes()
    # rows above max_len are left alone
    part = spmm_f32_ref.csr_mulacc_dense_rowmaj((rows, cols), ip, ix, dt, rhs, out0.copy(), max_len=100)
    assert part[lens > 100].tobytes() == out0[lens > 100].tobytes() and part[lens <= 100].tobytes() == acc[lens <= 100].tobytes()
    # column by column it is the SpMV chain of f32_ref
    assert spmm_f32_ref.mul_vec_columns((rows, cols), ip, ix, dt, rhs).tobytes() == got.tobytes()


def test_reference_chain_rounds_every_step_to_f32():
    """1 + 2^-24 + 2^-24 left to right in f32 stays 1 (each add is a tie to even); in float64 it is 1 + 2^-23"""
    ip, ix = np.array([0, 3]), np.array([0, 1, 2])
    dt = np.ones(3, dtype=np.float32)
    rhs = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    assert spmm_f32_ref.mul_dense((1, 3), ip, ix, dt, rhs)[0, 0] == np.float32(1.0)
    rhs2 = np.array([[2.0 ** -24], [2.0 ** -24], [1.0]], dtype=np.float32)
    assert spmm_f32_ref.mul_dense((1, 3), ip, ix, dt, rhs2)[0, 0] == np.float32(1.0 + 2.0 ** -23)


def test_result_layout_rule():
    assert [spmm_f32_ref.result_col_major(k) for k in (0, 1, 7, 8, 9, 64)] == [True, True, True, False, False, False]
