"""Twin of `sprs::binop` for device operands (sprs/src/sparse/binop.rs) plus the operators built on it: `&A + &B`, `&A - &B`,
`&A * s`, `&v + &w`, `&v - &w`.  Same names, argument order and failure behaviour: where the reference panics, SprsHipError
carries the panic text.  Every result entry is one IEEE operation, so results are the reference's bit for bit."""
import ctypes as C

from . import _ffi
from ._ffi import BINOP_ADD, BINOP_MUL, BINOP_SUB, check, lib
from .device import DeviceCsMat, DeviceCsVec

ADD, SUB, MUL = BINOP_ADD, BINOP_SUB, BINOP_MUL
_OPS = {"add": ADD, "+": ADD, "sub": SUB, "-": SUB, "mul": MUL, "*": MUL}


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


def _op(op):
    return _OPS[op] if isinstance(op, str) else int(op)


def csmat_binop(lhs, rhs, op, stream=None):
    """binop::csmat_binop (binop.rs:178-223) with op = ADD | SUB | MUL (or "add" / "sub" / "mul"): the merge of every outer
    slice pair; an index on one side only meets +0.0; entries with val == 0.0 are dropped (NaN kept).  Equal shapes
    ("Dimension mismatch") and equal storages ("Storage mismatch") are required."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_binop_f64(lhs._h, rhs._h, _op(op), C.byref(h), _stream_ptr(stream)))
    return DeviceCsMat(h.value)


def mul_mat_same_storage(lhs, rhs, stream=None):
    """binop::mul_mat_same_storage (binop.rs:115-130): the elementwise product."""
    return csmat_binop(lhs, rhs, MUL, stream)


def add_mat(lhs, rhs, stream=None):
    """`&lhs + &rhs` (binop.rs:52-64): rhs.to_other_storage() first when the storages differ; the result has lhs' storage."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_add_csmat_f64(lhs._h, rhs._h, C.byref(h), _stream_ptr(stream)))
    return DeviceCsMat(h.value)


def sub_mat(lhs, rhs, stream=None):
    """`&lhs - &rhs` (binop.rs:99-111)."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_sub_csmat_f64(lhs._h, rhs._h, C.byref(h), _stream_ptr(stream)))
    return DeviceCsMat(h.value)


def scale(mat, alpha, stream=None):
    """`&mat * alpha` (binop.rs:132-163) = mat.map(|x| x * alpha): same structure, nothing dropped."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_scale_f64(mat._h, float(alpha), C.byref(h), _stream_ptr(stream)))
    return DeviceCsMat(h.value)


def _dense_out(rhs):
    """Array::zeros(shape) / Array::zeros(shape.f()) by rhs' fastest axis (binop.rs:309-315): contiguous, rhs' layout"""
    from .device import DeviceVec
    from .prod import DeviceMat
    return DeviceMat(rhs.rows, rhs.cols, DeviceVec(rhs.rows * rhs.cols), rhs.col_major)


def csmat_binop_dense_raw(lhs, rhs, op, out, alpha=1.0, beta=1.0, stream=None):
    """binop::csmat_binop_dense_raw (binop.rs:384-433) with one of the two closures the reference ships: op = ADD writes
    (alpha * l) + (beta * r), op = MUL (alpha * l) * r, into EVERY element of `out` (l = +0.0 where lhs stores nothing; the
    operation is performed there too).  rhs / out: DeviceMat of one layout, padded or not.  The reference's checks in its
    order: "Dimension mismatch", then "Storage mismatch" unless CSR meets row-major / CSC column-major."""
    if lhs.cols() != rhs.cols or lhs.cols() != out.cols or lhs.rows() != rhs.rows or lhs.rows() != out.rows:
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")                 # binop.rs:397-403
    if rhs.col_major != out.col_major or lhs.is_csr() == rhs.col_major:
        raise _ffi.SprsHipError(_ffi.STORAGE_MISMATCH, "Storage mismatch")               # binop.rs:404-412
    check(lib.sprs_hip_csmat_binop_dense_f64(lhs._h, C.c_void_p(rhs.vec.ptr), rhs.rows, rhs.cols, rhs.layout, rhs.ld, _op(op), float(alpha),
                                             float(beta), C.c_void_p(out.vec.ptr), out.ld, _stream_ptr(stream)))
    return out


def add_dense_mat_same_ordering(lhs, rhs, alpha, beta, stream=None):
    """binop::add_dense_mat_same_ordering (binop.rs:279-323): alpha * lhs + beta * rhs as a new DeviceMat in rhs' layout."""
    return csmat_binop_dense_raw(lhs, rhs, ADD, _dense_out(rhs), alpha, beta, stream)


def mul_dense_mat_same_ordering(lhs, rhs, alpha, stream=None):
    """binop::mul_dense_mat_same_ordering (binop.rs:331-371): the coefficient-wise alpha * lhs * rhs in rhs' layout."""
    return csmat_binop_dense_raw(lhs, rhs, MUL, _dense_out(rhs), alpha, 1.0, stream)


def add_dense(lhs, rhs, stream=None):
    """`&lhs + &rhs` for a dense rhs (csmat.rs:1951-1987): lhs.to_other_storage() first when its storage does not match rhs'
    layout (below the C ABI); the result has rhs' layout."""
    if lhs.cols() != rhs.cols or lhs.rows() != rhs.rows:
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
    out = _dense_out(rhs)
    check(lib.sprs_hip_csmat_add_dense_f64(lhs._h, C.c_void_p(rhs.vec.ptr), rhs.rows, rhs.cols, rhs.layout, rhs.ld, C.c_void_p(out.vec.ptr),
                                           _stream_ptr(stream)))
    return out


def csvec_binop(lhs, rhs, op, stream=None):
    """binop::csvec_binop (binop.rs:442-467): the same merge on two sparse vectors; every merged index is kept, zeros
    included.  A vector of dimension 0 takes the other's dimension (csvec_fix_zeros)."""
    h = C.c_void_p()
    check(lib.sprs_hip_csvec_binop_f64(lhs._h, rhs._h, _op(op), C.byref(h), _stream_ptr(stream)))
    return DeviceCsVec(h.value)
