"""Device containers: Python twins of the Rust wrapper crate's `DeviceCsMat` /
`DeviceVec` (rust/sprs-hip/src/lib.rs), themselves device twins of sprs'
CsMatBase (sprs/src/sparse.rs:94-122) and of the dense vectors accepted through
DenseVector (sprs/src/dense_vector.rs:10-29)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import CSC, CSR, check, lib

_DT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


class _DeviceVecBase:
    """What DeviceVec and DeviceVecF32 share: a dense vector in HBM of the subclass's element type.  The two are SIBLINGS: an
    isinstance test for one never admits the other, so no entry that reads n doubles is handed n floats."""
    _dtype = None          # numpy element type
    _itemsize = 0

    def __init__(self, n, ptr=None, owner=None):
        self.n = int(n)
        self._owner = owner
        if ptr is None:
            p = C.c_void_p()
            check(lib.sprs_hip_malloc(C.byref(p), self.n * self._itemsize))
            self.ptr = p.value
            self._owned = True
        else:
            self.ptr = int(ptr)
            self._owned = False

    @classmethod
    def from_host(cls, arr):
        """casts to the element type (numpy's astype: round to nearest even)"""
        arr = np.ascontiguousarray(arr, dtype=cls._dtype)
        v = cls(arr.size)
        check(lib.sprs_hip_memcpy_h2d(C.c_void_p(v.ptr), _vp(arr), arr.size * cls._itemsize))
        return v

    @classmethod
    def zeros(cls, n):
        v = cls(n)
        check(lib.sprs_hip_memset(C.c_void_p(v.ptr), 0, v.n * cls._itemsize, None))
        return v

    def to_host(self):
        out = np.empty(self.n, dtype=self._dtype)
        check(lib.sprs_hip_synchronize(None))
        check(lib.sprs_hip_memcpy_d2h(_vp(out), C.c_void_p(self.ptr), self.n * self._itemsize))
        return out

    def dim(self):   # DenseVector::dim, dense_vector.rs:14
        return self.n

    def __len__(self):
        return self.n

    def __del__(self):
        if getattr(self, "_owned", False) and self.ptr:
            lib.sprs_hip_free(C.c_void_p(self.ptr))
            self.ptr = 0


class DeviceVec(_DeviceVecBase):
    """A dense f64 vector in HBM.  Either owns its buffer or borrows one
    (e.g. a torch tensor's `data_ptr()`), like a `&mut [f64]` would."""
    _dtype, _itemsize = np.float64, 8

    @classmethod
    def borrow(cls, tensor):
        """Borrow a contiguous float64 torch CUDA tensor (no copy)."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.element_size() == 8
        return cls(tensor.numel(), ptr=tensor.data_ptr(), owner=tensor)


class DeviceVecF32(_DeviceVecBase):
    """A dense f32 vector in HBM: the operand and result type of the single-precision products (DeviceCsMatF32).  Not a
    DeviceVec: an entry that reads n doubles must never be handed n floats."""
    _dtype, _itemsize = np.float32, 4

    @classmethod
    def borrow(cls, tensor):
        """Borrow a contiguous float32 torch CUDA tensor (no copy); TypeError for any other element type."""
        if tensor.element_size() != 4 or not tensor.is_floating_point():
            raise TypeError("float32 elements expected")
        assert tensor.is_cuda and tensor.is_contiguous()
        return cls(tensor.numel(), ptr=tensor.data_ptr(), owner=tensor)


class _DeviceCsMatBase:
    """The container part DeviceCsMat and DeviceCsMatF32 share: a CSR/CSC matrix whose indptr / indices / data live in HBM
    behind a handle of the subclass's type.  The two are SIBLINGS (see _DeviceVecBase).  Every entry is looked up by the
    class: _c("info") is sprs_hip_csmat_info or sprs_hip_csmat_f32_info, _op("spmv") sprs_hip_spmv_f64 or sprs_hip_spmv_f32."""
    _dtype = None          # numpy type of the values
    _vec_type = None       # the dense vector class of the same precision
    _container, _suffix = None, None

    @classmethod
    def _c(cls, name):
        return getattr(lib, cls._container + name)

    @classmethod
    def _op(cls, name):
        return getattr(lib, "sprs_hip_%s_%s" % (name, cls._suffix))

    def __init__(self, handle, keep=None):
        self._h = C.c_void_p(handle)
        self._keep = keep   # objects the handle borrows from

    @classmethod
    def from_host(cls, shape, indptr, indices, data, storage=CSR, validate=True):
        """CsMat::new / new_csc when validate (csmat.rs:146-166), new_trusted otherwise; data is cast to the class's type."""
        indptr = np.ascontiguousarray(indptr)
        indices = np.ascontiguousarray(indices)
        data = np.ascontiguousarray(data, dtype=cls._dtype)
        if indptr.dtype.kind not in "iu" or indices.dtype.kind not in "iu":
            raise TypeError("integer index arrays expected")
        if indices.size != data.size:
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "indices and data lengths differ")
        outer = shape[0] if storage == CSR else shape[1]
        if indptr.size != outer + 1:
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "Indptr length does not match dimension")
        if validate and int(indptr[-1]) - int(indptr[0]) != indices.size:
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match")
        h = C.c_void_p()
        check(cls._c("upload")(C.byref(h), storage, shape[0], shape[1], _vp(indptr), indptr.dtype.itemsize, _vp(indices),
                               indices.dtype.itemsize, _vp(data), 1 if validate else 0))
        return cls(h.value)

    @classmethod
    def _wrap_torch(cls, shape, indptr_t, indices_t, data_t, storage):
        h = C.c_void_p()
        check(cls._c("wrap_device")(
            C.byref(h), storage, shape[0], shape[1], indices_t.numel(),
            C.c_void_p(indptr_t.data_ptr()), indptr_t.element_size(),
            C.c_void_p(indices_t.data_ptr() if indices_t.numel() else 0), indices_t.element_size(),
            C.c_void_p(data_t.data_ptr() if data_t.numel() else 0)))
        return cls(h.value, keep=(indptr_t, indices_t, data_t))

    # -- accessors ------------------------------------------------------------
    def _info(self):
        r, c, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pb, ib, st = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._c("info")(self._h, C.byref(r), C.byref(c), C.byref(n), C.byref(pb), C.byref(ib), C.byref(st)))
        return r.value, c.value, n.value, pb.value, ib.value, st.value

    def rows(self): return self._info()[0]
    def cols(self): return self._info()[1]
    def shape(self): return self._info()[:2]
    def nnz(self): return self._info()[2]
    def storage(self): return self._info()[5]
    def is_csr(self): return self.storage() == CSR
    def is_csc(self): return self.storage() == CSC
    def index_bytes(self): return self._info()[4]
    def indptr_bytes(self): return self._info()[3]

    def device_ptrs(self):
        """-> (indptr, indices, data) device addresses (into_raw_storage), still owned by the handle"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._c("device_ptrs")(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def to_host(self):
        """-> (shape, indptr, indices, data) numpy arrays (into_raw_storage, csmat.rs:946-954)."""
        r, c, n, pb, ib, st = self._info()
        outer = r if st == CSR else c
        indptr = np.empty(outer + 1, dtype=_DT[pb])
        indices = np.empty(n, dtype=_DT[ib])
        data = np.empty(n, dtype=self._dtype)
        check(self._c("download")(self._h, _vp(indptr), _vp(indices), _vp(data)))
        return (r, c), indptr, indices, data

    def refresh(self):
        """Drop the cached multiply plans and the CSR form after the wrapped device arrays were modified in place."""
        check(self._c("refresh")(self._h))

    def prepare(self, stream=None):
        """Build the full SpMV plan (and `stream`'s scratch) now.  f64: without it the re-laid-out copy plans come with the
        SECOND multiply of the handle — the first one runs on the plain tile index.  f32: needed before an SpMV on a capturing
        stream."""
        check(self._c("prepare")(self._h, _stream_arg(stream)))
        return self

    def transpose_view(self):
        """csmat.rs:982-991: free, shares buffers."""
        h = C.c_void_p()
        check(self._c("transpose_view")(self._h, C.byref(h)))
        return type(self)(h.value, keep=self)

    def to_other_storage(self):
        """csmat.rs:1405-1426."""
        h = C.c_void_p()
        check(self._c("to_other_storage")(self._h, C.byref(h)))
        return type(self)(h.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._c("free")(h)
            self._h = C.c_void_p(0)


class DeviceCsMat(_DeviceCsMatBase):
    """A CSR/CSC matrix whose indptr / indices / data live in HBM behind a
    `sprs_hip_csmat*` handle."""
    _dtype, _container, _suffix = np.float64, "sprs_hip_csmat_", "f64"

    # -- constructors -------------------------------------------------------
    @classmethod
    def new_from_unsorted(cls, shape, indptr, indices, data, storage=CSR, stream=None):
        """CsMat::new_from_unsorted (csmat.rs:374-384): host arrays whose outer slices need not be sorted; they are uploaded as
        they are and sorted and validated on the device."""
        indptr, indices = np.ascontiguousarray(indptr), np.ascontiguousarray(indices)
        if indptr.size != (shape[0] if storage == CSR else shape[1]) + 1:
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "Indptr length does not match dimension",
                                    kind=_ffi.KIND_SIZE_MISMATCH, outer=_ffi.NO_OUTER)
        if int(indptr[-1]) - int(indptr[0]) != indices.size:    # (the upload sizes its copies by the indptr)
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match",
                                    kind=_ffi.KIND_SIZE_MISMATCH, outer=_ffi.NO_OUTER)
        return cls.from_host(shape, indptr, indices, data, storage=storage, validate=False).sort_indices(stream)

    @classmethod
    def new_from_unsorted_csc(cls, shape, indptr, indices, data, stream=None):
        """CsMat::new_from_unsorted_csc (csmat.rs:391-401)."""
        return cls.new_from_unsorted(shape, indptr, indices, data, storage=CSC, stream=stream)

    @classmethod
    def wrap_torch(cls, shape, indptr_t, indices_t, data_t, storage=CSR, validate=False):
        """Borrow torch CUDA tensors as the three CSR arrays (no copy).  validate: run check_structure on the device before
        returning (CsMat::new instead of new_trusted)."""
        m = cls._wrap_torch(shape, indptr_t, indices_t, data_t, storage)
        if validate:
            m.check_structure()
        return m

    @classmethod
    def eye(cls, dim, idx_dtype=np.uint64, ptr_dtype=np.uint64):
        """CsMatI::eye (csmat.rs:416-426)."""
        return cls.from_host((dim, dim), np.arange(dim + 1, dtype=ptr_dtype),
                             np.arange(dim, dtype=idx_dtype), np.ones(dim), validate=False)

    @classmethod
    def csr_from_dense(cls, m, epsilon, idx_dtype=np.uint64, ptr_dtype=np.uint64, stream=None):
        """CsMat::csr_from_dense (csmat.rs:499-539) of a prod.DeviceMat: the elements with |x| > max(epsilon, 0)."""
        from . import to_dense
        return to_dense.csr_from_dense(m, epsilon, idx_dtype, ptr_dtype, stream)

    @classmethod
    def csc_from_dense(cls, m, epsilon, idx_dtype=np.uint64, ptr_dtype=np.uint64, stream=None):
        """CsMat::csc_from_dense (csmat.rs:541-549)."""
        from . import to_dense
        return to_dense.csc_from_dense(m, epsilon, idx_dtype, ptr_dtype, stream)

    def to_dense(self, out=None, stream=None):
        """CsMat::to_dense (csmat.rs:1127-1134) as a prod.DeviceMat in standard layout (or into `out`)."""
        from . import to_dense
        return to_dense.to_dense(self, out, stream)

    def slice_outer_to_host(self, start, end):
        """Rows [start, end) as a host view: indptr NOT rebased (slicing.rs:65-89)."""
        r, c, n, pb, ib, st = self._info()
        cnt = C.c_uint64()
        check(lib.sprs_hip_csmat_download_outer(self._h, start, end, None, None, None, C.byref(cnt)))
        indptr = np.empty(end - start + 1, dtype=_DT[pb])
        indices = np.empty(cnt.value, dtype=_DT[ib])
        data = np.empty(cnt.value, dtype=np.float64)
        check(lib.sprs_hip_csmat_download_outer(self._h, start, end, _vp(indptr), _vp(indices),
                                                _vp(data), None))
        return indptr, indices, data

    def slice_outer(self, start, end):
        """slice_outer (slicing.rs:65-89) + to_proper, materialised on the device."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_slice_outer(self._h, start, end, C.byref(h)))
        return DeviceCsMat(h.value)

    def check_structure(self, stream=None):
        """utils::check_compressed_structure (sparse.rs:300-358) on the device arrays.  Raises SprsHipError (BAD_STRUCTURE, the
        reference's text) carrying `.kind` (_ffi.KIND_*) and `.outer`, the first offending outer slice."""
        info = _ffi.StructureInfo()
        _ffi.check_structure_status(lib.sprs_hip_csmat_check_structure(self._h, C.byref(info), _stream_arg(stream)), info)
        return self

    def sort_indices(self, stream=None):
        """A new handle whose outer slices are sorted by inner index, validated (sprs_hip_csmat_from_unsorted); this one is only
        read.  Errors as check_structure."""
        h, info = C.c_void_p(), _ffi.StructureInfo()
        _ffi.check_structure_status(lib.sprs_hip_csmat_from_unsorted(self._h, C.byref(h), C.byref(info), _stream_arg(stream)), info)
        return DeviceCsMat(h.value)

    def spmv_plan_info(self):
        """-> (kind, plan_bytes): 0 none yet, 1 nnz tiles, 2 XCD-sliced copy, 3 banded copy (hot columns from LDS)."""
        kind, nbytes = C.c_int32(), C.c_uint64()
        check(lib.sprs_hip_csmat_spmv_plan_info(self._h, C.byref(kind), C.byref(nbytes)))
        return kind.value, nbytes.value

    def to_f32(self, stream=None):
        """CsMat::map(|&v| v as f32) (csmat.rs:1289-1305) as a DeviceCsMatF32: the structure copied, the values rounded to
        nearest even (overflow gives inf, NaN stays NaN)."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_f32_from_f64(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsMatF32(h.value)

    def degrees(self, stream=None, out=None):
        """csmat.rs:1205-1216: per outer index the stored entries off the diagonal, as a host uint64 array.  `out`: a
        DeviceVec of outer-dimension words that receives the counts instead (they stay on the device; returns out)."""
        outer = self.rows() if self.is_csr() else self.cols()
        buf = DeviceVec(outer) if out is None else out
        check(lib.sprs_hip_csmat_degrees(self._h, C.c_void_p(buf.ptr), _stream_arg(stream)))
        if out is not None:
            return out
        check(lib.sprs_hip_synchronize(_stream_arg(stream)))
        res = np.empty(outer, dtype=np.uint64)
        check(lib.sprs_hip_memcpy_d2h(_vp(res), C.c_void_p(buf.ptr), outer * 8))
        return res

    def max_outer_nnz(self, stream=None):
        """csmat.rs:1188-1193."""
        v = C.c_uint64()
        check(lib.sprs_hip_csmat_max_outer_nnz(self._h, C.byref(v), _stream_arg(stream)))
        return v.value

    # -- extraction ---------------------------------------------------------------
    def outer_view(self, i, stream=None):
        """csmat.rs:1219-1231: the i-th outer slice as a DeviceCsVec that BORROWS this matrix's arrays (zero-copy; it keeps the
        matrix alive), or None when i >= outer dims."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_outer_view(self._h, int(i), C.byref(h), _stream_arg(stream)))
        return DeviceCsVec(h.value, keep=self) if h.value else None

    def diag(self, stream=None):
        """csmat.rs:1234-1256: the stored diagonal entries (an explicit 0.0 included) as a new DeviceCsVec of dim min(rows, cols)."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_diag_f64(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsVec(h.value)

    def _lookup(self, rows, cols, stream):
        scalar = np.ndim(rows) == 0 and np.ndim(cols) == 0
        r, c = np.broadcast_arrays(np.atleast_1d(np.asarray(rows, dtype=np.uint64)), np.atleast_1d(np.asarray(cols, dtype=np.uint64)))
        nq = r.size
        rb, cb, pb, vb = _u64_to_device(r), _u64_to_device(c), DeviceVec(max(nq, 1)), DeviceVec(max(nq, 1))
        check(lib.sprs_hip_csmat_nnz_index(self._h, nq, C.c_void_p(rb.ptr), C.c_void_p(cb.ptr), C.c_void_p(pb.ptr), C.c_void_p(vb.ptr),
                                           _stream_arg(stream)))
        pos, val = _lookup_results(pb, vb, nq, stream)
        return scalar, pos, val

    def nnz_index(self, rows, cols, stream=None):
        """csmat.rs:1312-1330, batched: the position in indices / data of every (row, col), _ffi.NONE where nothing is stored
        (out-of-range rows and cols included).  Ints give an int or None, arrays a uint64 array."""
        scalar, pos, _ = self._lookup(rows, cols, stream)
        if scalar:
            return None if int(pos[0]) == _ffi.NONE else int(pos[0])
        return pos

    def nnz_index_outer_inner(self, outer, inner, stream=None):
        """csmat.rs:1332-1351: the same by (outer, inner)."""
        return self.nnz_index(outer, inner, stream) if self.is_csr() else self.nnz_index(inner, outer, stream)

    def get(self, rows, cols, stream=None):
        """csmat.rs get: the stored value of every (row, col); an int pair gives a float or None, arrays give (values, found)
        with 0.0 where nothing is stored."""
        scalar, pos, val = self._lookup(rows, cols, stream)
        if scalar:
            return None if int(pos[0]) == _ffi.NONE else float(val[0])
        return val, pos != np.uint64(_ffi.NONE)

    def get_outer_inner(self, outer, inner, stream=None):
        """csmat.rs get_outer_inner."""
        return self.get(outer, inner, stream) if self.is_csr() else self.get(inner, outer, stream)

    def to_inner_onehot(self, stream=None):
        """csmat.rs:1017-1056: per outer slice the last maximal non-NaN entry, with value 1.0, as a new matrix."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_to_inner_onehot_f64(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsMat(h.value)

    # -- operators: `&A * &x`, `&A * &B` ---------------------------------------
    def __mul__(self, rhs):
        from . import prod
        if isinstance(rhs, DeviceVecF32):
            raise TypeError("an f64 matrix times an f32 vector: convert one operand (DeviceCsMat.to_f32)")
        if isinstance(rhs, DeviceCsVec):
            return prod.csmat_mul_csvec(self, rhs)        # vec.rs:1104-1131
        if isinstance(rhs, DeviceVec):
            return prod.csmat_mul_vec(self, rhs)          # csmat.rs:2119-2160
        if isinstance(rhs, DeviceCsMat):
            return prod.csmat_mul_csmat(self, rhs)        # csmat.rs:1866-1949
        if isinstance(rhs, DeviceCsMatF32):
            raise TypeError("an f64 matrix times an f32 matrix: convert one operand (DeviceCsMat.to_f32 / DeviceCsMatF32.to_f64)")
        if isinstance(rhs, prod.DeviceMat):
            return prod.csmat_mul_dense(self, rhs)        # csmat.rs:1989-2048
        if isinstance(rhs, prod.DeviceMatF32):
            raise TypeError("an f64 matrix times an f32 dense matrix: convert one operand (DeviceCsMat.to_f32)")
        if isinstance(rhs, (float, np.floating)):
            from . import binop
            return binop.scale(self, rhs)                 # binop.rs:132-163
        return NotImplemented

    def __matmul__(self, rhs):
        if isinstance(rhs, (float, np.floating)):
            return NotImplemented
        return self.__mul__(rhs)

    def __rmul__(self, lhs):
        """`s * A` for a Python or numpy float: the same map as `&A * s` (x * s and s * x are one IEEE product)"""
        if isinstance(lhs, (float, np.floating)):
            from . import binop
            return binop.scale(self, lhs)
        return NotImplemented

    def __add__(self, rhs):
        if isinstance(rhs, DeviceCsMat):
            from . import binop
            return binop.add_mat(self, rhs)               # binop.rs:52-64
        from . import prod
        if isinstance(rhs, prod.DeviceMat):
            from . import binop
            return binop.add_dense(self, rhs)             # csmat.rs:1951-1987
        return NotImplemented

    def __sub__(self, rhs):
        if isinstance(rhs, DeviceCsMat):
            from . import binop
            return binop.sub_mat(self, rhs)               # binop.rs:99-111
        return NotImplemented

class DeviceCsMatF32(_DeviceCsMatBase):
    """A CSR/CSC matrix of f32 values in HBM behind a `sprs_hip_csmat_f32*` handle: CsMat<f32>.  Built for it: the container,
    `&A * &x` and the two mul_acc forms with DeviceVecF32, `&A * &B` and the four mulacc_dense forms with prod.DeviceMatF32,
    prod.dense_dot_csmat (prod.py), `&A * &B` with another DeviceCsMatF32 and the smmp functions (smmp.py), BiCGSTAB
    (linalg.py); `to_f64()` reaches every other
    operation.  The SpMV runs on the nnz-tile plan or on the banded plan (`spmv_plan_info()`, option spmv_f32_band_tile).  Index arrays are 4 or 8 bytes wide (no 2-byte ones)."""
    _dtype, _container, _suffix = np.float32, "sprs_hip_csmat_f32_", "f32"

    @classmethod
    def wrap_torch(cls, shape, indptr_t, indices_t, data_t, storage=CSR):
        """Borrow torch CUDA tensors (int32 / int64 index arrays, float32 data) as the three arrays (no copy)."""
        if data_t.element_size() != 4 or not data_t.is_floating_point():
            raise TypeError("float32 data expected")
        return cls._wrap_torch(shape, indptr_t, indices_t, data_t, storage)

    def spmv_plan_info(self):
        """-> (kind, plan_bytes): 0 none yet, 1 nnz tiles, 3 banded copy (hot columns from LDS, float throughout); a CSC handle
        reports the plan of its cached CSR form."""
        kind, nbytes = C.c_int32(), C.c_uint64()
        check(lib.sprs_hip_csmat_f32_spmv_plan_info(self._h, C.byref(kind), C.byref(nbytes)))
        return kind.value, nbytes.value

    def to_f64(self, stream=None):
        """CsMat::map(|&v| v as f64): exact."""
        h = C.c_void_p()
        check(lib.sprs_hip_csmat_f32_to_f64(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsMat(h.value)

    def __mul__(self, rhs):
        from . import prod
        if isinstance(rhs, DeviceVecF32):
            return prod.csmat_mul_vec(self, rhs)
        if isinstance(rhs, DeviceVec):
            raise TypeError("an f32 matrix times an f64 vector: convert one operand (DeviceCsMatF32.to_f64)")
        if isinstance(rhs, prod.DeviceMatF32):
            return prod.csmat_mul_dense(self, rhs)        # csmat.rs:1989-2048
        if isinstance(rhs, prod.DeviceMat):
            raise TypeError("an f32 matrix times an f64 dense matrix: convert one operand (DeviceCsMatF32.to_f64)")
        if isinstance(rhs, DeviceCsMatF32):
            return prod.csmat_mul_csmat(self, rhs)        # csmat.rs:1866-1949, N = f32
        if isinstance(rhs, DeviceCsMat):
            raise TypeError("an f32 matrix times an f64 matrix: convert one operand (DeviceCsMatF32.to_f64 / DeviceCsMat.to_f32)")
        return NotImplemented

    __matmul__ = __mul__


DeviceCsMat._vec_type, DeviceCsMatF32._vec_type = DeviceVec, DeviceVecF32


def _stream_arg(stream):
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


def _u64_to_device(arr):
    """a host array as uint64 words in a DeviceVec (complete when this returns)"""
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    buf = DeviceVec(max(arr.size, 1))
    if arr.size:
        check(lib.sprs_hip_memcpy_h2d(C.c_void_p(buf.ptr), _vp(arr), arr.size * 8))
    return buf


def _lookup_results(pos_buf, val_buf, nq, stream):
    """(pos, val) host arrays of a batched nnz_index / get once `stream` has finished them"""
    check(lib.sprs_hip_synchronize(_stream_arg(stream)))
    pos, val = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.float64)
    if nq:
        check(lib.sprs_hip_memcpy_d2h(_vp(pos), C.c_void_p(pos_buf.ptr), nq * 8))
        check(lib.sprs_hip_memcpy_d2h(_vp(val), C.c_void_p(val_buf.ptr), nq * 8))
    return pos, val


class DeviceCsVec:
    """A sparse vector whose indices / data live in HBM behind a `sprs_hip_csvec*` handle: twin of CsVecBase
    (sprs/src/sparse.rs:165-173).  `mat * vec` and `vec * mat` with a DeviceCsMat are the products of vec.rs:1084-1131."""

    def __init__(self, handle, keep=None):
        self._h = C.c_void_p(handle)
        self._keep = keep   # objects the handle borrows from

    @classmethod
    def from_host(cls, dim, indices, data, validate=True):
        """CsVec::new (vec.rs:430-434) when validate, new_trusted otherwise; indices of 2, 4 or 8 bytes."""
        indices = np.ascontiguousarray(indices)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if indices.dtype.kind not in "iu":
            raise TypeError("integer index array expected")
        if indices.size != data.size:    # vec.rs:452-459
            raise _ffi.SprsHipError(_ffi.BAD_STRUCTURE, "indices and data do not have compatible lengths")
        h = C.c_void_p()
        check(lib.sprs_hip_csvec_upload(C.byref(h), int(dim), indices.size, _vp(indices), indices.dtype.itemsize, _vp(data),
                                        1 if validate else 0))
        return cls(h.value)

    @classmethod
    def new_from_unsorted(cls, dim, indices, data, stream=None):
        """CsVec::new_from_unsorted (vec.rs:536-557): uploaded as it is, checked, sorted when unsorted and checked again on the
        device."""
        return cls.from_host(dim, indices, data, validate=False).sort_indices(stream)

    def check_structure(self, stream=None):
        """The invariants of CsVec::try_new (vec.rs:440-491) on the device arrays; raises SprsHipError carrying `.kind`."""
        info = _ffi.StructureInfo()
        _ffi.check_structure_status(lib.sprs_hip_csvec_check_structure(self._h, C.byref(info), _stream_arg(stream)), info)
        return self

    def sort_indices(self, stream=None):
        """A new sorted, validated vector (sprs_hip_csvec_from_unsorted); this one is only read."""
        h, info = C.c_void_p(), _ffi.StructureInfo()
        _ffi.check_structure_status(lib.sprs_hip_csvec_from_unsorted(self._h, C.byref(h), C.byref(info), _stream_arg(stream)), info)
        return DeviceCsVec(h.value)

    @classmethod
    def borrow(cls, dim, indices_t, data_t, validate=False):
        """Borrow two contiguous torch CUDA tensors (int32 / int64 indices, float64 data) without a copy (new_trusted, or
        CsVec::new with validate: the check runs on the device)."""
        assert indices_t.is_cuda and data_t.is_cuda and indices_t.is_contiguous() and data_t.is_contiguous()
        assert data_t.element_size() == 8 and indices_t.numel() == data_t.numel()
        h = C.c_void_p()
        check(lib.sprs_hip_csvec_wrap_device(C.byref(h), int(dim), indices_t.numel(),
                                             C.c_void_p(indices_t.data_ptr() if indices_t.numel() else 0),
                                             indices_t.element_size(), C.c_void_p(data_t.data_ptr() if data_t.numel() else 0)))
        v = cls(h.value, keep=(indices_t, data_t))
        if validate:
            v.check_structure()
        return v

    def _info(self):
        d, n, ib = C.c_uint64(), C.c_uint64(), C.c_int32()
        check(lib.sprs_hip_csvec_info(self._h, C.byref(d), C.byref(n), C.byref(ib)))
        return d.value, n.value, ib.value

    def dim(self): return self._info()[0]          # vec.rs:681
    def nnz(self): return self._info()[1]          # vec.rs:686
    def index_bytes(self): return self._info()[2]

    def to_host(self):
        """-> (dim, indices, data) numpy arrays (into_raw_storage, vec.rs:675)."""
        dim, n, ib = self._info()
        indices = np.empty(n, dtype=_DT[ib])
        data = np.empty(n, dtype=np.float64)
        check(lib.sprs_hip_synchronize(None))
        check(lib.sprs_hip_csvec_download(self._h, _vp(indices), _vp(data)))
        return dim, indices, data

    def scatter(self, out, stream=None):
        """CsVec::scatter (vec.rs:965) into a DeviceVec of length dim: zeros, then the stored values."""
        check(lib.sprs_hip_csvec_scatter_f64(self._h, C.c_void_p(out.ptr), out.n, _stream_arg(stream)))
        return out

    def to_dense(self, stream=None):
        """CsVec::to_dense (vec.rs:621) as a DeviceVec."""
        return self.scatter(DeviceVec(self.dim()), stream)

    # -- reductions: every sum is the reference's left-to-right chain, bit for bit ---------------------------------
    def dot(self, rhs, stream=None):
        """CsVec::dot (vec.rs:828-881) with a DeviceCsVec, a DeviceVec or a contiguous float64 torch CUDA tensor."""
        out = C.c_double()
        if isinstance(rhs, DeviceCsVec):
            check(lib.sprs_hip_csvec_dot_f64(self._h, rhs._h, C.byref(out), _stream_arg(stream)))
            return out.value
        return self.dot_dense(rhs, stream)

    def dot_dense(self, rhs, stream=None):
        """CsVec::dot_dense (vec.rs:894-904)."""
        if not isinstance(rhs, DeviceVec):
            rhs = DeviceVec.borrow(rhs)
        out = C.c_double()
        check(lib.sprs_hip_csvec_dot_dense_f64(self._h, C.c_void_p(rhs.ptr), rhs.n, C.byref(out), _stream_arg(stream)))
        return out.value

    def _norm(self, kind, p, stream):
        out = C.c_double()
        check(lib.sprs_hip_csvec_norm_f64(self._h, kind, float(p), C.byref(out), _stream_arg(stream)))
        return out.value

    def squared_l2_norm(self, stream=None):    # vec.rs:907-913
        return self._norm(_ffi.NORM_SQUARED_L2, 0.0, stream)

    def l2_norm(self, stream=None):            # vec.rs:916-922
        return self._norm(_ffi.NORM_L2, 0.0, stream)

    def l1_norm(self, stream=None):            # vec.rs:925-930
        return self._norm(_ffi.NORM_L1, 0.0, stream)

    def norm(self, p, stream=None):            # vec.rs:939-958
        return self._norm(_ffi.NORM_P, p, stream)

    def unit_normalize(self, stream=None):
        """unit_normalize (vec.rs:1051-1061) as a NEW vector: handles are immutable snapshots, this one is only read."""
        h = C.c_void_p()
        check(lib.sprs_hip_csvec_unit_normalize_f64(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsVec(h.value)

    def _lookup(self, index, stream):
        q = np.atleast_1d(np.asarray(index, dtype=np.uint64))
        nq = q.size
        qb, pb, vb = _u64_to_device(q), DeviceVec(max(nq, 1)), DeviceVec(max(nq, 1))
        check(lib.sprs_hip_csvec_nnz_index(self._h, nq, C.c_void_p(qb.ptr), C.c_void_p(pb.ptr), C.c_void_p(vb.ptr), _stream_arg(stream)))
        return _lookup_results(pb, vb, nq, stream)

    def nnz_index(self, index, stream=None):
        """vec.rs:800-805, batched: the position of every index in the stored arrays, _ffi.NONE where it is not stored.  An int
        gives an int or None, an array a uint64 array."""
        pos, _ = self._lookup(index, stream)
        if np.ndim(index) == 0:
            return None if int(pos[0]) == _ffi.NONE else int(pos[0])
        return pos

    def get(self, index, stream=None):
        """vec.rs:787-792: an int gives the stored value or None; an array gives (values, found), 0.0 where nothing is stored."""
        pos, val = self._lookup(index, stream)
        if np.ndim(index) == 0:
            return None if int(pos[0]) == _ffi.NONE else float(val[0])
        return val, pos != np.uint64(_ffi.NONE)

    def __mul__(self, rhs):
        from . import prod
        if isinstance(rhs, DeviceCsMat):
            return prod.csvec_mul_csmat(self, rhs)        # vec.rs:1084-1102
        return NotImplemented

    __matmul__ = __mul__

    def __add__(self, rhs):
        if isinstance(rhs, DeviceCsVec):
            from . import binop
            return binop.csvec_binop(self, rhs, _ffi.BINOP_ADD)   # vec.rs:1133-1179
        return NotImplemented

    def __sub__(self, rhs):
        if isinstance(rhs, DeviceCsVec):
            from . import binop
            return binop.csvec_binop(self, rhs, _ffi.BINOP_SUB)   # vec.rs:1181-1226
        return NotImplemented

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.sprs_hip_csvec_free(h)
            self._h = C.c_void_p(0)
