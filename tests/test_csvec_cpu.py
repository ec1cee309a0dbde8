"""CPU checks of the sparse-vector products: the Python restatement used by the GPU tests reproduces the reference's own hand
values (prod.rs:461-500), and without a device every new entry point that touches device memory fails with NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from conftest import as_csr
from csvec_ref import csr_mul_csvec_ref, masked_dot_vec

V5 = ([0, 2, 4], [1.0, 1.0, 1.0])


def _transpose(ip, ix, dt, rows, cols):
    ip = np.asarray(ip, dtype=np.int64)
    row_of = np.repeat(np.arange(rows), np.diff(ip))
    order = np.lexsort((row_of, np.asarray(ix, dtype=np.int64)))
    tip = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(ix, dtype=np.int64), minlength=cols))])
    return tip, row_of[order], np.asarray(dt)[order]


def test_restatement_reproduces_the_reference_hand_values(golden):
    shape, ip, ix, dt = as_csr(golden["mat1"])
    # mul_csr_csvec / mul_csc_csvec (prod.rs:461-468, 485-491): CsVec::new(5, [0, 1, 2], [3, 5, 5])
    for structural in (False, True):
        d, i, v = csr_mul_csvec_ref(ip, ix, dt, 5, 5, *V5, structural=structural)
        assert d == 5 and list(i) == [0, 1, 2] and list(v) == [3.0, 5.0, 5.0]
        d, i, v, _ = masked_dot_vec(ip, ix, dt, 5, 5, *V5, structural=structural)
        assert d == 5 and list(i) == [0, 1, 2] and list(v) == [3.0, 5.0, 5.0]
    # mul_csvec_csr / mul_csvec_csc (prod.rs:476-483, 493-500): CsVec::new(5, [2, 3], [8, 11]) — the columns of mat1
    tip, tix, tdt = _transpose(ip, ix, dt, 5, 5)
    d, i, v = csr_mul_csvec_ref(tip, tix, tdt, 5, 5, *V5, structural=True)
    assert d == 5 and list(i) == [2, 3] and list(v) == [8.0, 11.0]
    # mat1_csc holds the same columns
    _, cip, cix, cdt = as_csr(golden["mat1_csc"])
    assert np.array_equal(cip, tip) and np.array_equal(cix, tix) and np.array_equal(cdt, tdt)
    # mul_csr_zero_csvec (prod.rs:470-474): empty of dimension 0
    d, i, v = csr_mul_csvec_ref(ip, ix, dt, 5, 0, [], [])
    assert d == 0 and i.size == 0


def test_restatements_agree_on_order_sensitive_sums():
    rng = np.random.default_rng(0)
    lens = rng.integers(0, 30, 200)
    ip = np.concatenate([[0], np.cumsum(lens)])
    ix = np.concatenate([np.sort(rng.choice(100, int(l), replace=False)) for l in lens])
    dt = rng.choice([1e16, -1e16, 1.0, -1.0, 0.0, -0.0, 3.5], ix.size)
    vidx = np.sort(rng.choice(100, 60, replace=False))
    vval = rng.choice([1.0, -1.0, 0.0, 2.0], 60)
    for structural in (False, True):
        d1, i1, v1 = csr_mul_csvec_ref(ip, ix, dt, 200, 100, vidx, vval, structural)
        d2, i2, v2, _ = masked_dot_vec(ip, ix, dt, 200, 100, vidx, vval, structural)
        assert d1 == d2 and np.array_equal(i1, i2) and np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
    # (1e16 + 1) - 1e16 = 0 in sprs' order: the restatement keeps the order (a sum by pairs would give 1)
    d, i, v = csr_mul_csvec_ref([0, 3], [0, 1, 2], [1e16, 1.0, -1e16], 1, 3, [0, 1, 2], [1.0, 1.0, 1.0])
    assert d == 1 and i.size == 0


def _no_device():
    import sprs_amd
    return sprs_amd.device_count() == 0


def test_new_entry_points_need_a_device():
    """without a device every new entry point that touches device memory reports NO_DEVICE (no CPU fallback); freeing a
    NULL vector is a no-op"""
    from sprs_amd import _ffi
    lib = _ffi.lib
    assert lib.sprs_hip_csvec_free(None) == _ffi.OK
    # argument checks need no device
    h = C.c_void_p()
    idx = np.array([0, 2], dtype=np.uint64)
    val = np.ones(2)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.sprs_hip_csvec_upload(C.byref(h), 4, 2, vp(idx), 3, vp(val), 1) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_upload(C.byref(h), 4, 2, None, 8, vp(val), 1) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csmat_mul_csvec_f64(None, None, C.byref(h), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_mul_csmat_f64(None, None, C.byref(h), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_info(None, None, None, None) == _ffi.INVALID_ARG
    # host-side validation comes before any device work, with the reference's texts (vec.rs:440-491)
    bad = np.array([2, 0], dtype=np.uint64)
    assert lib.sprs_hip_csvec_upload(C.byref(h), 4, 2, vp(bad), 8, vp(val), 1) == _ffi.BAD_STRUCTURE
    assert lib.sprs_hip_last_error() == b"Unsorted indices"
    assert lib.sprs_hip_csvec_upload(C.byref(h), 2, 2, vp(idx), 8, vp(val), 1) == _ffi.BAD_STRUCTURE
    assert lib.sprs_hip_last_error() == b"indices larger than vector size"
    i16 = np.array([0, 2], dtype=np.uint16)
    assert lib.sprs_hip_csvec_upload(C.byref(h), 70000, 2, vp(i16), 2, vp(val), 1) == _ffi.INDEX_OVERFLOW
    assert lib.sprs_hip_last_error() == b"Index size is too small"
    if not _no_device():
        pytest.skip("a GPU is present: the NO_DEVICE half runs on CPU-only machines")
    assert lib.sprs_hip_csvec_upload(C.byref(h), 4, 2, vp(idx), 8, vp(val), 1) == _ffi.NO_DEVICE
    assert lib.sprs_hip_csvec_wrap_device(C.byref(h), 4, 0, None, 8, None) == _ffi.NO_DEVICE


def test_device_csvec_raises_without_a_device():
    import sprs_amd
    from sprs_amd.device import DeviceCsVec
    if not _no_device():
        pytest.skip("a GPU is present")
    with pytest.raises(sprs_amd.SprsHipError) as e:
        DeviceCsVec.from_host(4, np.array([1], dtype=np.uint32), np.ones(1))
    assert e.value.status == sprs_amd._ffi.NO_DEVICE
