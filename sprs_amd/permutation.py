"""Twin of `sprs::sparse::permutation` for device operands (sprs/src/sparse/permutation.rs): `DevicePerm` is PermOwned, `p * x`
is `&P * x`, and permute_rows / permute_cols / transform_mat_papt / transform_mat_paq keep the reference's names and argument
order.  Values are moved, never computed: results are the reference's bit for bit.  Where the reference panics, SprsHipError
carries the text.  One departure: permute_rows / permute_cols handed the Identity variant return a copy (the reference reaches
unreachable!() there, permutation.rs:315, 370)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import check, lib
from .device import DeviceCsMat, DeviceVec, _DT, _stream_arg, _vp


class DevicePerm:
    """A permutation behind a `sprs_hip_perm*` handle: the Identity variant, or perm and perm_inv in HBM."""

    def __init__(self, perm, validate=True):
        """PermOwned::new (permutation.rs:52-66) from host indices of 2, 4 or 8 bytes; an invalid permutation (a value out of
        range or twice) is BAD_STRUCTURE "invalid permutation" when validate."""
        self._h = C.c_void_p(0)
        perm = np.ascontiguousarray(perm)
        if perm.size == 0 and perm.dtype.kind == "f":
            perm = perm.astype(np.uint64)
        if perm.dtype.kind not in "iu" or perm.ndim != 1:
            raise TypeError("a one-dimensional integer array expected")
        if perm.dtype.itemsize == 1:
            perm = perm.astype(np.uint16)
        h = C.c_void_p()
        check(lib.sprs_hip_perm_upload(C.byref(h), perm.size, _vp(perm), perm.dtype.itemsize, 1 if validate else 0))
        self._h = h

    @classmethod
    def _wrap(cls, handle):
        p = cls.__new__(cls)
        p._h = C.c_void_p(handle)
        return p

    @classmethod
    def from_device(cls, src, idx_bytes=None, validate=True, stream=None):
        """From indices already on the device — an int32 / int64 torch tensor (an argsort, ...) or a DeviceVec holding 8-byte
        indices; the array is COPIED, the handle owns its arrays."""
        if isinstance(src, DeviceVec):
            ptr, n, width = src.ptr, src.n, idx_bytes or 8
        else:
            assert src.is_cuda and src.is_contiguous() and src.dim() == 1
            ptr, n, width = (src.data_ptr() if src.numel() else 0), src.numel(), idx_bytes or src.element_size()
        h = C.c_void_p()
        check(lib.sprs_hip_perm_from_device(C.byref(h), n, C.c_void_p(ptr), width, 1 if validate else 0, _stream_arg(stream)))
        return cls._wrap(h.value)

    @classmethod
    def identity(cls, dim, idx_dtype=np.uint64):
        """Permutation::identity (permutation.rs:113-118): the Identity variant, no arrays."""
        h = C.c_void_p()
        check(lib.sprs_hip_perm_identity(C.byref(h), int(dim), np.dtype(idx_dtype).itemsize))
        return cls._wrap(h.value)

    def _info(self):
        d, ib, ident = C.c_uint64(), C.c_int32(), C.c_int32()
        check(lib.sprs_hip_perm_info(self._h, C.byref(d), C.byref(ib), C.byref(ident)))
        return d.value, ib.value, bool(ident.value)

    @property
    def dim(self):                                  # permutation.rs:139
        return self._info()[0]

    def index_bytes(self): return self._info()[1]
    def is_identity_variant(self): return self._info()[2]

    def is_identity(self, stream=None):
        """permutation.rs:144-152: the elementwise test — a stored permutation equal to 0..dim counts."""
        flag = C.c_int32()
        check(lib.sprs_hip_perm_is_identity(self._h, C.byref(flag), _stream_arg(stream)))
        return bool(flag.value)

    def inv(self):
        """permutation.rs:120-137, as a new owning handle."""
        h = C.c_void_p()
        check(lib.sprs_hip_perm_inv(self._h, C.byref(h)))
        return DevicePerm._wrap(h.value)

    def _download(self, which):
        dim, ib, _ = self._info()
        out = np.empty(dim, dtype=_DT[ib])
        check(lib.sprs_hip_perm_download(self._h, _vp(out) if which == 0 else None, _vp(out) if which == 1 else None))
        return out

    def vec(self):                                  # permutation.rs:211-217
        return self._download(0)

    def inv_vec(self):                              # permutation.rs:219-226
        return self._download(1)

    def mul_vec(self, x, out=None, stream=None):
        """`&P * x` (permutation.rs:255-278): y[i] = x[p[i]]."""
        out = DeviceVec(x.n) if out is None else out
        check(lib.sprs_hip_perm_mul_vec_f64(self._h, C.c_void_p(x.ptr), C.c_void_p(out.ptr), x.n, _stream_arg(stream)))
        return out

    def __mul__(self, rhs):
        if isinstance(rhs, DeviceVec):
            return self.mul_vec(rhs)
        return NotImplemented

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.sprs_hip_perm_free(h)
            self._h = C.c_void_p(0)


def _h(perm):
    return None if perm is None else perm._h


def transform_mat_paq(mat, row_perm, col_perm, stream=None):
    """permutation.rs:496-581: P * A * Q.  None or the Identity variant on a side leaves that side alone."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_transform_paq(mat._h, _h(row_perm), _h(col_perm), C.byref(h), _stream_arg(stream)))
    return DeviceCsMat(h.value)


def permute_rows(mat, perm, stream=None):
    """permutation.rs:407-420: P * A."""
    return transform_mat_paq(mat, perm, None, stream)


def permute_cols(mat, perm, stream=None):
    """permutation.rs:423-436: A * P."""
    return transform_mat_paq(mat, None, perm, stream)


def transform_mat_papt(mat, perm, stream=None):
    """permutation.rs:439-491: P * A * P^T; the matrix must be square and of the permutation's dimension."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_transform_papt(mat._h, perm._h, C.byref(h), _stream_arg(stream)))
    return DeviceCsMat(h.value)
