"""Twin of `sprs::smmp` for device operands (sprs/src/sparse/smmp.rs).  Every function takes two DeviceCsMat (f64) or two
DeviceCsMatF32 and returns the operands' class; operands of different precision raise TypeError."""
import ctypes as C

from ._ffi import check, lib
from .device import DeviceCsMat, DeviceCsMatF32


def _same_precision(*mats):
    """the class of the operands; TypeError naming the conversion when they differ"""
    cls = type(mats[0])
    if cls not in (DeviceCsMat, DeviceCsMatF32):
        raise TypeError("DeviceCsMat or DeviceCsMatF32 operands expected, got %s" % cls.__name__)
    for m in mats[1:]:
        if type(m) is not cls:
            raise TypeError("operands differ in precision (%s and %s): convert with DeviceCsMat.to_f32 or DeviceCsMatF32.to_f64"
                            % (cls.__name__, type(m).__name__))
    return cls


def _entry(cls, f64_name, stem):
    """the f64 entry keeps its historical name; its f32 twin is sprs_hip_<stem>_f32"""
    return getattr(lib, "sprs_hip_%s_f32" % stem if cls is DeviceCsMatF32 else f64_name)


def mul_csr_csr(lhs, rhs):
    """smmp::mul_csr_csr (smmp.rs:196-416): C = lhs * rhs, all CSR, rows
    sorted, structural zeros kept.  Returns a new DeviceCsMat (DeviceCsMatF32 for f32 operands: every product and every
    partial sum rounded to f32, in the reference's order)."""
    cls = _same_precision(lhs, rhs)
    h = C.c_void_p()
    check(_entry(cls, "sprs_hip_spgemm_f64", "spgemm")(lhs._h, rhs._h, C.byref(h)))
    return cls(h.value)


def symbolic(a, b):
    """smmp::symbolic (smmp.rs:81-131): the structure of a * b — indptr and sorted indices, structural zeros
    kept — as a matrix of the operands' class whose values are 0.0."""
    cls = _same_precision(a, b)
    h = C.c_void_p()
    check(_entry(cls, "sprs_hip_spgemm_symbolic", "spgemm_symbolic")(a._h, b._h, C.byref(h)))
    return cls(h.value)


def numeric(a, b, c):
    """smmp::numeric (smmp.rs:151-189): the values of a * b into c, which must have the product's structure
    (as `symbolic` returns it); BAD_STRUCTURE otherwise."""
    cls = _same_precision(a, b, c)
    check(_entry(cls, "sprs_hip_spgemm_numeric", "spgemm_numeric")(a._h, b._h, c._h))
    return c


class SpgemmPlan:
    """The symbolic phase of a * b, kept (sprs_hip_spgemm_plan_*): what a caller of the reference keeps between
    smmp::symbolic and smmp::numeric (smmp.rs:81-131, 151-189) — here the cut of the work too, so that `numeric`
    launches the value kernels only.  a and b must stay alive and keep their structure; their values may change.
    The plan holds structure only: `serving(a2, b2)` gives a plan object over the SAME device plan for operands of either
    precision that wrap the same indptr / indices device arrays."""

    def __init__(self, a, b):
        self._cls = _same_precision(a, b)
        self.a, self.b = a, b
        self._owner = None
        h = C.c_void_p()
        check(_entry(self._cls, "sprs_hip_spgemm_plan_create", "spgemm_plan_create")(a._h, b._h, C.byref(h)))
        self._h = h

    def serving(self, a, b):
        """this plan for other handles over the same structure arrays (f64 or f32); the library checks that they match"""
        other = object.__new__(SpgemmPlan)
        other._cls = _same_precision(a, b)
        other.a, other.b, other._h, other._owner = a, b, self._h, self       # (the owner frees the device plan)
        return other

    def nnz(self):
        n = C.c_uint64()
        check(lib.sprs_hip_spgemm_plan_nnz(self._h, C.byref(n)))
        return n.value

    def structure(self):
        """C with indptr and sorted indices, values 0.0 (smmp::symbolic's result)"""
        h = C.c_void_p()
        check(_entry(self._cls, "sprs_hip_spgemm_plan_structure", "spgemm_plan_structure")(self._h, self.a._h, self.b._h, C.byref(h)))
        return self._cls(h.value)

    def product(self):
        """C = a * b complete"""
        h = C.c_void_p()
        check(_entry(self._cls, "sprs_hip_spgemm_plan_product", "spgemm_plan_product")(self._h, self.a._h, self.b._h, C.byref(h)))
        return self._cls(h.value)

    def numeric(self, c):
        """the values of a * b into c (structure as returned by structure() / product()); value kernels only"""
        _same_precision(self.a, c)
        check(_entry(self._cls, "sprs_hip_spgemm_plan_numeric", "spgemm_plan_numeric")(self._h, self.a._h, self.b._h, c._h))
        return c

    def __del__(self):
        if getattr(self, "_owner", None) is not None:
            return
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:       # (lib is None while the interpreter shuts down)
            lib.sprs_hip_spgemm_plan_free(h)
            self._h = C.c_void_p(0)
