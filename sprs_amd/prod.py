"""Twin of `sprs::prod` for device operands (sprs/src/sparse/prod.rs) plus the
operator dispatch of csmat.rs.  Same names, argument order and failure
behaviour: where the reference panics, SprsHipError carries the panic text."""
import ctypes as C

from . import _ffi
from ._ffi import CSC, CSR, check, lib
from .device import DeviceCsMat, DeviceCsVec, DeviceVec


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


def _is_f32(mat, *vecs):
    """True for a DeviceCsMatF32 with DeviceVecF32 operands, False for the f64 classes; a mix raises TypeError (the reference's
    N is one type per call: the entries of one precision must never read the buffers of the other)"""
    from .device import DeviceCsMatF32, DeviceVecF32
    f32 = isinstance(mat, DeviceCsMatF32)
    for v in vecs:
        if isinstance(v, DeviceVecF32) != f32:
            raise TypeError("matrix and vectors must have the same precision: %s with %s" % (type(mat).__name__, type(v).__name__))
    return f32


def mul_acc_mat_vec_csr(mat, in_vec, res_vec, stream=None):
    """prod::mul_acc_mat_vec_csr (prod.rs:103-127): res_vec += mat * in_vec.  A DeviceCsMatF32 with DeviceVecF32 operands runs
    the f32 entry."""
    _is_f32(mat, in_vec, res_vec)
    check(mat._op("spmv")(mat._h, C.c_void_p(in_vec.ptr), in_vec.n, C.c_void_p(res_vec.ptr), res_vec.n, 1, _stream_ptr(stream)))


def mul_acc_mat_vec_csc(mat, in_vec, res_vec, stream=None):
    """prod::mul_acc_mat_vec_csc (prod.rs:74-99): res_vec += mat * in_vec for a CSC matrix (sprs_hip_mul_acc_mat_vec_csc_f64:
    the matrix is converted once to CSR on the device, the copy is cached in the HANDLE, the CSR kernel runs — every result
    element still receives its products by ascending column).  A DeviceCsMatF32 with DeviceVecF32 operands runs the f32 entry."""
    _is_f32(mat, in_vec, res_vec)
    check(mat._op("mul_acc_mat_vec_csc")(mat._h, C.c_void_p(in_vec.ptr), in_vec.n, C.c_void_p(res_vec.ptr), res_vec.n, _stream_ptr(stream)))


class _DenseMat:
    """What DeviceMat and DeviceMatF32 share: a dense matrix in HBM in one of ndarray's two contiguous layouts.  The two are
    SIBLINGS, not parent and child: an isinstance test for one never admits the other."""
    _np_dtype = None

    @staticmethod
    def _vec_type():
        raise NotImplementedError

    def __init__(self, rows, cols, vec=None, col_major=False, ld=None):
        """ld: the leading dimension in elements (None: contiguous) — the lines of the matrix are ld apart in `vec`, which then
        holds lines * ld elements (the last line's padding included).  Only the dense <-> sparse entries take a padded matrix."""
        self.rows, self.cols, self.col_major = int(rows), int(cols), bool(col_major)
        self._ld = None if ld is None else int(ld)
        lines = self.cols if self.col_major else self.rows
        want = self.rows * self.cols if self._ld is None else lines * self._ld
        self.vec = vec if vec is not None else self._vec_type().zeros(want)
        if not isinstance(self.vec, self._vec_type()):
            raise TypeError("%s holds a %s, not a %s" % (type(self).__name__, self._vec_type().__name__, type(self.vec).__name__))
        assert self.vec.n == want

    @classmethod
    def from_host(cls, arr, col_major=False, ld=None, fill=0.0):
        """ld: pad every line to ld elements; the padding holds `fill` (a float, or an array of lines x (ld - width))"""
        import numpy as np
        arr = np.asarray(arr, dtype=cls._np_dtype)
        if ld is not None:
            lines = arr.T if col_major else arr
            if int(ld) < lines.shape[1]:
                raise _ffi.SprsHipError(_ffi.INVALID_ARG, "leading dimension smaller than the extent it strides over")
            buf = np.empty((lines.shape[0], int(ld)), dtype=cls._np_dtype)
            buf[:, lines.shape[1]:] = fill
            buf[:, :lines.shape[1]] = lines
            return cls(arr.shape[0], arr.shape[1], cls._vec_type().from_host(buf.reshape(-1)), col_major, ld)
        flat = np.asfortranarray(arr).reshape(-1, order="F") if col_major else np.ascontiguousarray(arr).reshape(-1)
        return cls(arr.shape[0], arr.shape[1], cls._vec_type().from_host(np.ascontiguousarray(flat)), col_major)

    def to_host(self):
        flat = self.vec.to_host()
        if self._ld is not None:
            lines, width = (self.cols, self.rows) if self.col_major else (self.rows, self.cols)
            body = flat.reshape(lines, self._ld)[:, :width]
            return body.T if self.col_major else body
        return flat.reshape(self.cols, self.rows).T if self.col_major else flat.reshape(self.rows, self.cols)

    @property
    def layout(self):
        return _ffi.COL_MAJOR if self.col_major else _ffi.ROW_MAJOR

    @property
    def ld(self):
        if self._ld is not None:
            return self._ld
        return self.rows if self.col_major else self.cols


class DeviceMat(_DenseMat):
    """Dense f64 matrix in HBM in one of ndarray's two contiguous layouts: `Array2` in standard (row-major) order, or
    `Array::zeros(shape.f())` (column-major) — what `&CsMat * &Array2` returns for fewer than 8 columns (csmat.rs:2017-2024)."""
    _np_dtype = "float64"

    @staticmethod
    def _vec_type():
        return DeviceVec


class DeviceMatF32(_DenseMat):
    """Dense f32 matrix in HBM over a DeviceVecF32: the operand and result type of the dense products of a DeviceCsMatF32.
    Constructor, from_host (casts to float32), to_host, layout, ld, padding and fill as DeviceMat."""
    _np_dtype = "float32"

    @staticmethod
    def _vec_type():
        from .device import DeviceVecF32
        return DeviceVecF32


def _is_f32_dense(mat, *dense):
    """True for a DeviceCsMatF32 with DeviceMatF32 operands, False for the f64 classes; any mix raises TypeError before the
    library is called (as _is_f32 for the vectors)"""
    from .device import DeviceCsMatF32
    f32 = isinstance(mat, DeviceCsMatF32)
    for d in dense:
        if isinstance(d, DeviceMatF32) != f32:
            raise TypeError("matrix and dense operands must have the same precision: %s with %s" % (type(mat).__name__, type(d).__name__))
    return f32


def _dims(lhs, rhs, out):
    """the three dimension asserts of the four dense kernels come FIRST, the storage assert last (prod.rs:199-202, 228-231,
    256-259, 284-288): with both wrong every mirror reports the dimensions"""
    _is_f32_dense(lhs, rhs, out)       # a mix of precisions is a TypeError, whatever the shapes are
    if rhs.cols != out.cols or lhs.cols() != rhs.rows or lhs.rows() != out.rows:
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")


def _mulacc_dense(lhs, rhs, out, stream):
    _is_f32_dense(lhs, rhs, out)
    check(lhs._op("csmat_mulacc_dense")(lhs._h, C.c_void_p(rhs.vec.ptr), rhs.rows, rhs.cols, rhs.layout, rhs.ld,
                                        C.c_void_p(out.vec.ptr), out.rows, out.layout, out.ld, 1, _stream_ptr(stream)))


def _storage(lhs, want_csr):
    if lhs.is_csc() == want_csr:
        raise _ffi.SprsHipError(_ffi.STORAGE_MISMATCH, "Storage mismatch")       # prod.rs:202, 231, 258, 288


def csr_mulacc_dense_rowmaj(lhs, rhs, out, stream=None):
    """prod::csr_mulacc_dense_rowmaj (prod.rs:189-214): out += lhs * rhs."""
    _dims(lhs, rhs, out)
    _storage(lhs, True)
    _mulacc_dense(lhs, rhs, out, stream)


def csr_mulacc_dense_colmaj(lhs, rhs, out, stream=None):
    """prod::csr_mulacc_dense_colmaj (prod.rs:274-298): out += lhs * rhs (the reference walks the rhs column by column; the
    device entry is told by the operands' layouts how to address them).  rhs / out: DeviceMat, or two equally long lists of
    column vectors (out[:, j] += lhs * rhs[:, j])."""
    if isinstance(rhs, (list, tuple)):
        if len(rhs) != len(out) or any(lhs.cols() != r.n or lhs.rows() != o.n for r, o in zip(rhs, out)):
            raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
        _storage(lhs, True)
        for r, o in zip(rhs, out):
            mul_acc_mat_vec_csr(lhs, r, o, stream)
        return
    _dims(lhs, rhs, out)
    _storage(lhs, True)
    _mulacc_dense(lhs, rhs, out, stream)


def csc_mulacc_dense_rowmaj(lhs, rhs, out, stream=None):
    """prod::csc_mulacc_dense_rowmaj (prod.rs:219-241): out += lhs * rhs for a CSC lhs.  The reference walks the columns of
    lhs in order and adds `lval * rhs[col, :]` into out[row, :], so every out[i, j] receives its products by ascending column —
    the order the CSR kernel uses on the converted matrix (cached in the handle, below the C ABI)."""
    _dims(lhs, rhs, out)
    _storage(lhs, False)
    _mulacc_dense(lhs, rhs, out, stream)


def csc_mulacc_dense_colmaj(lhs, rhs, out, stream=None):
    """prod::csc_mulacc_dense_colmaj (prod.rs:246-270); rhs / out as in csr_mulacc_dense_colmaj."""
    if isinstance(rhs, (list, tuple)):
        if len(rhs) != len(out) or any(lhs.cols() != r.n or lhs.rows() != o.n for r, o in zip(rhs, out)):
            raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")      # prod.rs:256-257
        _storage(lhs, False)
        for r, o in zip(rhs, out):
            mul_acc_mat_vec_csc(lhs, r, o, stream)
        return
    _dims(lhs, rhs, out)
    _storage(lhs, False)
    _mulacc_dense(lhs, rhs, out, stream)


def csmat_mul_dense(mat, rhs, stream=None):
    """`&CsMat * &Array2` (csmat.rs:1989-2048), ONE call below the C ABI (sprs_hip_csmat_mul_dense_f64): the four arms
    (CSR | CSC) x (>= 8 columns | fewer); the result comes back row-major for >= 8 columns and column-major (`.f()`) below,
    like the reference's."""
    _is_f32_dense(mat, rhs)
    out = type(rhs)(mat.rows(), rhs.cols, rhs._vec_type()(mat.rows() * rhs.cols))
    lay = C.c_int32(0)
    check(mat._op("csmat_mul_dense")(mat._h, C.c_void_p(rhs.vec.ptr), rhs.rows, rhs.cols, rhs.layout, rhs.ld,
                                     C.c_void_p(out.vec.ptr), C.byref(lay), _stream_ptr(stream)))
    out.col_major = lay.value == _ffi.COL_MAJOR
    return out


def dense_dot_csmat(lhs, mat, stream=None):
    """`Array2::dot(&CsMat)` (csmat.rs:2050-2117): dense . sparse through the transposes of the reference, below the C ABI."""
    _is_f32_dense(mat, lhs)
    out = type(lhs)(lhs.rows, mat.cols(), lhs._vec_type()(lhs.rows * mat.cols()))
    lay = C.c_int32(0)
    check(mat._op("dense_dot_csmat")(C.c_void_p(lhs.vec.ptr), lhs.rows, lhs.cols, lhs.layout, lhs.ld, mat._h,
                                     C.c_void_p(out.vec.ptr), C.byref(lay), _stream_ptr(stream)))
    out.col_major = lay.value == _ffi.COL_MAJOR
    return out


def csmat_mul_vec(mat, vec, out=None, stream=None):
    """`&CsMat * &Array1` (csmat.rs:2119-2160): fresh zero result; CSR goes through csr_mulacc_dense_colmaj with one column,
    CSC through csc_mulacc_dense_colmaj (csmat.rs:2140-2156) — dispatched below the C ABI (sprs_hip_csmat_mul_vec_f64)."""
    _is_f32(mat, vec, *([] if out is None else [out]))
    if out is None:
        out = mat._vec_type(mat.rows())
    check(mat._op("csmat_mul_vec")(mat._h, C.c_void_p(vec.ptr), vec.n, C.c_void_p(out.ptr), out.n, _stream_ptr(stream)))
    return out


def csmat_mul_csmat(lhs, rhs):
    """csmat_mul_csmat (csmat.rs:1895-1949): storage dispatch around smmp::mul_csr_csr, done below the C ABI
    (sprs_hip_csmat_mul_csmat / _f32); the result has the lhs' storage order and the operands' class.  TypeError when the
    operands differ in precision."""
    from .smmp import _same_precision
    cls = _same_precision(lhs, rhs)
    h = C.c_void_p()
    check(getattr(lib, "sprs_hip_csmat_mul_csmat" + ("_f32" if cls._suffix == "f32" else ""))(lhs._h, rhs._h, C.byref(h)))
    return cls(h.value)


def csr_mul_csvec(mat, vec, stream=None):
    """prod::csr_mul_csvec (prod.rs:161-184): CSR x sparse vector; an entry is kept only where its value is != 0.  A vector of
    dimension 0 gives an empty vector of dimension 0.  A CSC matrix raises "Storage mismatch" (the reference takes a CSR view)."""
    if mat.is_csc():
        raise _ffi.SprsHipError(_ffi.STORAGE_MISMATCH, "Storage mismatch")
    return csmat_mul_csvec(mat, vec, stream)


def csmat_mul_csvec(mat, vec, stream=None):
    """`&CsMat * &CsVec` (vec.rs:1104-1131): csr_mul_csvec for CSR, `mat * vec.col_view()` (structural) for CSC — one call below
    the C ABI (sprs_hip_csmat_mul_csvec_f64), which returns once the result is complete on `stream`."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_mul_csvec_f64(mat._h, vec._h, C.byref(h), _stream_ptr(stream)))
    return DeviceCsVec(h.value)


def csvec_mul_csmat(vec, mat, stream=None):
    """`&CsVec * &CsMat` (vec.rs:1084-1102): `(vec.row_view() * mat).outer_view(0)`, structural, below the C ABI
    (sprs_hip_csvec_mul_csmat_f64)."""
    h = C.c_void_p()
    check(lib.sprs_hip_csvec_mul_csmat_f64(vec._h, mat._h, C.byref(h), _stream_ptr(stream)))
    return DeviceCsVec(h.value)


def csvec_dot_by_binary_search(vec1, vec2, stream=None):
    """prod::csvec_dot_by_binary_search (prod.rs:14-70): the entries of the shorter vector looked up in the other by binary search,
    the matched products added by ascending index — on the device the same function as CsVec::dot (sprs_hip_csvec_dot_f64)."""
    return vec1.dot(vec2, stream)
