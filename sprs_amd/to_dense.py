"""Twin of `sprs::sparse::to_dense` for device operands (sprs/src/sparse/to_dense.rs) and of the dense constructors of CsMat
(csmat.rs:499-549, 1127-1134).  Same names, argument order and failure behaviour: where the reference panics, SprsHipError
carries the panic text.  Values are moved, never computed: every bit of a stored value arrives."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import CSC, CSR, check, lib


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


def _dims(array, spmat):
    """the two asserts of assign_to_dense (to_dense.rs:20-21)"""
    if spmat.cols() != array.cols or spmat.rows() != array.rows:
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")


def assign_to_dense(array, spmat, stream=None):
    """to_dense::assign_to_dense (to_dense.rs:12-30): array[row, col] = value for every stored entry of spmat; `array` (a
    DeviceMat of either layout, padded or not) is not zeroed first, so everything else in it is preserved."""
    _dims(array, spmat)
    check(lib.sprs_hip_csmat_assign_to_dense_f64(spmat._h, C.c_void_p(array.vec.ptr), array.rows, array.cols, array.layout, array.ld,
                                                 _stream_ptr(stream)))
    return array


def to_dense(spmat, out=None, stream=None):
    """CsMat::to_dense (csmat.rs:1127-1134): Array::zeros((rows, cols)) — standard layout — then assign_to_dense.  `out`: a
    DeviceMat to fill instead (its rows x cols elements are zeroed, its padding is not touched)."""
    from .device import DeviceVec
    from .prod import DeviceMat
    if out is None:
        r, c = spmat.shape()
        out = DeviceMat(r, c, DeviceVec(r * c))
    _dims(out, spmat)
    check(lib.sprs_hip_csmat_to_dense_f64(spmat._h, C.c_void_p(out.vec.ptr), out.rows, out.cols, out.layout, out.ld, _stream_ptr(stream)))
    return out


def from_dense(m, epsilon, storage, idx_dtype=np.uint64, ptr_dtype=np.uint64, stream=None):
    """CsMat::csr_from_dense (storage = CSR) / csc_from_dense (CSC) of a DeviceMat (csmat.rs:499-549): the elements with
    |x| > max(epsilon, 0) — a negative or NaN epsilon is 0 — as a new DeviceCsMat with the given index types."""
    from .device import DeviceCsMat
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_from_dense_f64(C.byref(h), storage, C.c_void_p(m.vec.ptr), m.rows, m.cols, m.layout, m.ld, float(epsilon),
                                            np.dtype(ptr_dtype).itemsize, np.dtype(idx_dtype).itemsize, _stream_ptr(stream)))
    return DeviceCsMat(h.value)


def csr_from_dense(m, epsilon, idx_dtype=np.uint64, ptr_dtype=np.uint64, stream=None):
    return from_dense(m, epsilon, CSR, idx_dtype, ptr_dtype, stream)


def csc_from_dense(m, epsilon, idx_dtype=np.uint64, ptr_dtype=np.uint64, stream=None):
    return from_dense(m, epsilon, CSC, idx_dtype, ptr_dtype, stream)
