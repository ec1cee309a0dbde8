"""Twin of the `sprs-ldl` crate (sprs-ldl/src/lib.rs) for device operands, under the reference's names: the `Ldl` builder,
`LdlSymbolic`, `LdlNumeric`, `ldl_lsolve`, `ldl_ltsolve` (and `linalg.diag_solve`).

The matrix, the permutation, the factors and the vectors stay in HBM.  l_colptr, the elimination tree, l_indices and every bit of
l_data, d and the solution are the reference's: the numeric pass walks each row's pattern in the order the reference's stack leaves
it in.  f64 only.  Where the reference panics or returns Err, SprsHipError carries the text; SINGULAR_MATRIX has `.index` and
`.reason` like the triangular solves of `linalg`."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import check, lib
from .device import DeviceCsMat, DeviceVec, _stream_arg
from .linalg import _SINGULAR_REASONS, _TriInfo
from .ordering import reverse_cuthill_mckee
from .permutation import DevicePerm


class SymmetryCheck:
    """sprs::SymmetryCheck"""
    CheckSymmetry = True
    DontCheckSymmetry = False


class PermutationCheck:
    """sprs::PermutationCheck: kept for the builder's signature; the native path never reads it (lib.rs:125-130)"""
    CheckPerm = True
    DontCheckPerm = False


class FillInReduction:
    """sprs::FillInReduction"""
    NoReduction = "NoReduction"
    ReverseCuthillMcKee = "ReverseCuthillMcKee"
    CAMDSuiteSparse = "CAMDSuiteSparse"


def _raise_singular(status, info):
    err = _ffi.SprsHipError(status, lib.sprs_hip_last_error().decode("utf-8", "replace"))
    err.index = int(info.singular_index)
    err.reason = _SINGULAR_REASONS[int(info.singular_reason)]
    raise err


class LdlSymbolic:
    """lib.rs:94-100, 228-324: the symbolic decomposition behind a `sprs_hip_ldl_sym*` handle."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        n, nnz, stats = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 4)()
        check(lib.sprs_hip_ldl_symbolic_info(self._h, C.byref(n), C.byref(nnz), stats))
        self._n, self._nnz = n.value, nnz.value
        self.stats = dict(zip(("etree_launches", "launches", "readbacks"), (int(x) for x in stats)))

    @classmethod
    def new(cls, mat, stream=None):
        """LdlSymbolic::new (lib.rs:234-241): the identity permutation, symmetry checked"""
        return cls.new_perm(mat, None, SymmetryCheck.CheckSymmetry, stream)

    @classmethod
    def new_perm(cls, mat, perm, check_symmetry=SymmetryCheck.CheckSymmetry, stream=None):
        """LdlSymbolic::new_perm (lib.rs:252-284); perm a DevicePerm or None"""
        h = C.c_void_p()
        check(lib.sprs_hip_ldl_symbolic(mat._h, None if perm is None else perm._h, 1 if check_symmetry else 0, C.byref(h),
                                        _stream_arg(stream)))
        return cls(h.value)

    def problem_size(self):                             # lib.rs:288
        return self._n

    def nnz(self):                                      # lib.rs:294
        return self._nnz

    def colptr(self):
        """l_colptr as host uint64"""
        out = np.zeros(self._n + 1, dtype=np.uint64)
        check(lib.sprs_hip_ldl_symbolic_colptr(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def parents(self):
        """the elimination tree as a host list, None for a root"""
        out = np.zeros(max(self._n, 1), dtype=np.uint64)
        check(lib.sprs_hip_ldl_symbolic_parents(self._h, C.c_void_p(out.ctypes.data)))
        return [None if int(p) == 2**64 - 1 else int(p) for p in out[:self._n]]

    def perm(self):
        h = C.c_void_p()
        check(lib.sprs_hip_ldl_symbolic_perm(self._h, C.byref(h)))
        return DevicePerm._wrap(h.value)

    def factor(self, mat, stream=None):
        """LdlSymbolic::factor (lib.rs:300-323).  The reference consumes self; here the handle stays usable."""
        h, info = C.c_void_p(), _TriInfo()
        status = lib.sprs_hip_ldl_factor_f64(self._h, mat._h, C.byref(h), C.byref(info), _stream_arg(stream))
        if status == _ffi.SINGULAR_MATRIX:
            _raise_singular(status, info)
        check(status)
        return LdlNumeric(h.value, self._n, self._nnz)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.sprs_hip_ldl_symbolic_free(h)
            self._h = C.c_void_p(0)


class LdlNumeric:
    """lib.rs:102-111, 326-442: the numeric decomposition behind a `sprs_hip_ldl_num*` handle."""

    def __init__(self, handle, n, nnz):
        self._h = C.c_void_p(handle)
        self._n, self._nnz = n, nnz

    @classmethod
    def new(cls, mat, stream=None):
        """LdlNumeric::new (lib.rs:332-338)"""
        return LdlSymbolic.new(mat, stream).factor(mat, stream)

    @classmethod
    def new_perm(cls, mat, perm, check_symmetry=SymmetryCheck.CheckSymmetry, stream=None):
        """LdlNumeric::new_perm (lib.rs:349-359)"""
        return LdlSymbolic.new_perm(mat, perm, check_symmetry, stream).factor(mat, stream)

    def update(self, mat, stream=None):
        """LdlNumeric::update (lib.rs:364-381): new values on the pattern that was analysed"""
        info = _TriInfo()
        status = lib.sprs_hip_ldl_update_f64(self._h, mat._h, C.byref(info), _stream_arg(stream))
        if status == _ffi.SINGULAR_MATRIX:
            _raise_singular(status, info)
        check(status)

    def solve(self, rhs, out=None, stream=None):
        """LdlNumeric::solve (lib.rs:388-410): rhs a DeviceVec (or a contiguous float64 torch CUDA tensor); a new vector"""
        if not isinstance(rhs, DeviceVec):
            rhs = DeviceVec.borrow(rhs)
        out = DeviceVec(rhs.n) if out is None else out
        check(lib.sprs_hip_ldl_solve_f64(self._h, C.c_void_p(rhs.ptr), C.c_void_p(out.ptr), rhs.n, _stream_arg(stream)))
        return out

    def d(self, stream=None):
        """lib.rs:413: the diagonal factor as a new DeviceVec"""
        out = DeviceVec(self._n)
        check(lib.sprs_hip_ldl_d(self._h, C.c_void_p(out.ptr), self._n, _stream_arg(stream)))
        check(lib.sprs_hip_synchronize(_stream_arg(stream)))
        return out

    def l(self, stream=None):
        """lib.rs:418-429: L as a new CSC DeviceCsMat without its unit diagonal"""
        h = C.c_void_p()
        check(lib.sprs_hip_ldl_l(self._h, C.byref(h), _stream_arg(stream)))
        return DeviceCsMat(h.value)

    def problem_size(self):                             # lib.rs:433
        return self._n

    def nnz(self):                                      # lib.rs:439
        return self._nnz

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.sprs_hip_ldl_numeric_free(h)
            self._h = C.c_void_p(0)


class Ldl:
    """The builder (lib.rs:74-226).  Defaults: CheckSymmetry, ReverseCuthillMcKee, CheckPerm."""

    def __init__(self, check_symmetry=SymmetryCheck.CheckSymmetry, check_perm=PermutationCheck.CheckPerm,
                 fill_red_method=FillInReduction.ReverseCuthillMcKee):
        self._sym, self._perm, self._fill = check_symmetry, check_perm, fill_red_method

    @classmethod
    def new(cls):
        return cls()

    def check_symmetry(self, check):
        return Ldl(check, self._perm, self._fill)

    def check_perm(self, check):
        return Ldl(self._sym, check, self._fill)

    def fill_in_reduction(self, method):
        return Ldl(self._sym, self._perm, method)

    def perm(self, mat, stream=None):
        """lib.rs:139-162: None stands for PermOwnedI::identity"""
        if self._fill == FillInReduction.NoReduction:
            return None
        if self._fill == FillInReduction.ReverseCuthillMcKee:
            return reverse_cuthill_mckee(mat, stream=stream).perm
        if self._fill == FillInReduction.CAMDSuiteSparse:
            raise RuntimeError("Unavailable without the `sprs_suitesparse_camd` feature")       # lib.rs:150-152
        raise RuntimeError("Unhandled method, report a bug at https://github.com/vbarrielle/sprs/issues/199")

    def symbolic(self, mat, stream=None):               # lib.rs:164-170
        return LdlSymbolic.new_perm(mat, self.perm(mat, stream), self._sym, stream)

    def numeric(self, mat, stream=None):                # lib.rs:190-201
        return self.symbolic(mat, stream).factor(mat, stream)


def _tri(fn, l, x, stream):
    check(fn(l._h, C.c_void_p(x.ptr), x.n, _stream_arg(stream)))
    return x


def ldl_lsolve(l, x, stream=None):
    """lib.rs:597-609, in place on the DeviceVec x: l a CSC DeviceCsMat, strictly lower, unit diagonal implied"""
    return _tri(lib.sprs_hip_ldl_lsolve_f64, l, x, stream)


def ldl_ltsolve(l, x, stream=None):
    """lib.rs:613-626"""
    return _tri(lib.sprs_hip_ldl_ltsolve_f64, l, x, stream)
