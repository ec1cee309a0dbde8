"""Twins of `sprs::sparse::construct` and `sprs::sparse::kronecker` for device operands (sprs/src/sparse/construct.rs,
kronecker.rs): kronecker_product, same_storage_fast_stack, vstack, hstack and bmat keep the reference's names and argument
order and return a new DeviceCsMat whose indptr, indices and value bits are the reference's.  Where the reference panics,
SprsHipError carries the text.  One departure: kronecker_product refuses by SHAPE what the reference refuses by stored index
(INDEX_OVERFLOW when inner(a) * inner(b) - 1 or nnz(a) * nnz(b) does not fit the operands' index types)."""
import ctypes as C

from . import _ffi
from ._ffi import check, lib
from .device import DeviceCsMat, _stream_arg


def kronecker_product(a, b, stream=None):
    """kronecker.rs:50-99: the result has the storage of `a`; nothing is dropped."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_kronecker_f64(a._h, b._h, C.byref(h), _stream_arg(stream)))
    return DeviceCsMat(h.value)


def _handles(mats):
    arr = (C.c_void_p * max(len(mats), 1))()
    for k, m in enumerate(mats):
        arr[k] = None if m is None else m._h.value
    return arr


def _stack(entry, mats, stream):
    mats = list(mats)
    h = C.c_void_p()
    check(entry(_handles(mats), len(mats), C.byref(h), _stream_arg(stream)))
    return DeviceCsMat(h.value)


def same_storage_fast_stack(mats, stream=None):
    """construct.rs:10-45: along the outer axis, in the operands' storage."""
    return _stack(lib.sprs_hip_csmat_same_storage_fast_stack, mats, stream)


def vstack(mats, stream=None):
    """construct.rs:48-63: always CSR."""
    return _stack(lib.sprs_hip_csmat_vstack, mats, stream)


def hstack(mats, stream=None):
    """construct.rs:66-81: always CSC."""
    return _stack(lib.sprs_hip_csmat_hstack, mats, stream)


def bmat(mats, stream=None):
    """construct.rs:94-160: a list of lists of DeviceCsMat or None; the result is CSR.  The ragged list is refused here, where
    the reference asserts it: between "Empty stacking list" and "Empty bmat row"."""
    rows = [list(r) for r in mats]
    if not rows or not rows[0]:
        raise _ffi.SprsHipError(_ffi.INVALID_ARG, "Empty stacking list")
    if any(len(r) != len(rows[0]) for r in rows):
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_bmat(_handles([m for r in rows for m in r]), len(rows), len(rows[0]), C.byref(h), _stream_arg(stream)))
    return DeviceCsMat(h.value)
