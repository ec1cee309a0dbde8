"""Host mirror of the reference's two callers that loop on the SpMV, over the device path:
sprs::linalg::bicgstab (sprs/src/sparse/linalg/bicgstab.rs) behind `sprs_hip_bicgstab_f64` (every vector resident
in HBM: two SpMVs, four fused element-wise kernels and three dot launches per iteration) and the Gauss-Seidel
solver of the heat example (sprs/examples/heat.rs:103-139) behind `sprs_hip_gauss_seidel_f64`; and of the four dense-rhs
triangular solves of sprs::linalg::trisolve (sprs/src/sparse/linalg/trisolve.rs) behind `sprs_hip_trisolve_f64`, and of its
sparse-rhs solve behind `sprs_hip_lsolve_csc_sparse_rhs_f64`.  BiCGSTAB, Gauss-Seidel, the dense-rhs triangular solves and
diag_solve dispatch on the operand class: a DeviceCsMatF32 with DeviceVecF32 vectors runs the `_f32` entry."""
import ctypes as C

from . import _ffi
from ._ffi import check, lib
from .device import DeviceVec


class _Info(C.Structure):
    _fields_ = [("iteration_count", C.c_uint64), ("soft_restart_count", C.c_uint64),
                ("hard_restart_count", C.c_uint64), ("err", C.c_double), ("rho", C.c_double),
                ("converged", C.c_int32)]


class BiCGSTAB:
    """Result of a solve, with the reference's accessors (bicgstab.rs:236-300).  The reference returns
    `Ok(solver)` / `Err(solver)` (iteration limit reached, results still inside); here `converged`
    tells the two apart and `solve` raises nothing for the latter, as `Err` is not a panic."""

    def __init__(self, a, x, b, info, soft_restart_threshold):
        self._a, self._x, self._b, self._i, self._thr = a, x, b, info, soft_restart_threshold

    @classmethod
    def solve(cls, a, x0, b, tol, max_iter, soft_restart_threshold=0.1, stream=None):
        """BiCGSTAB::solve(a, x0, b, tol, max_iter) (bicgstab.rs:148-171).  a: square DeviceCsMat (CSR or
        CSC), x0 / b: DeviceVec.  Dimension mismatch raises like the reference's panics.  A DeviceCsMatF32 with DeviceVecF32
        vectors runs BiCGSTAB::<f32> (sprs_hip_bicgstab_f32): tol and the threshold are rounded to f32 first."""
        from .device import DeviceCsMatF32, DeviceVecF32
        n = x0.n
        if b.n != n:
            raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
        f32 = isinstance(a, DeviceCsMatF32)
        if isinstance(x0, DeviceVecF32) != f32 or isinstance(b, DeviceVecF32) != f32:
            raise TypeError("matrix and vectors must have the same precision")
        x = a._vec_type(n)
        info = _Info()
        # tol and the threshold travel as doubles: rounded to the matrix's precision first (the identity for f64)
        check(a._op("bicgstab")(a._h, C.c_void_p(x0.ptr), C.c_void_p(b.ptr), n, float(a._dtype(tol)), int(max_iter),
                                float(a._dtype(soft_restart_threshold)), C.c_void_p(x.ptr), C.byref(info),
                                C.c_void_p(int(stream) if stream else 0)))
        return cls(a, x, b, info, soft_restart_threshold)

    @property
    def converged(self):
        return bool(self._i.converged)

    def iteration_count(self):
        return int(self._i.iteration_count)

    def soft_restart_count(self):
        return int(self._i.soft_restart_count)

    def hard_restart_count(self):
        return int(self._i.hard_restart_count)

    def soft_restart_threshold(self):
        return self._thr

    def err(self):
        return float(self._i.err)

    def rho(self):
        return float(self._i.rho)

    def a(self):
        return self._a

    def x(self):
        return self._x

    def b(self):
        return self._b


class _GsInfo(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("error", C.c_double), ("converged", C.c_int32), ("levels", C.c_uint64)]


class GaussSeidelResult:
    """What `gauss_seidel` of the heat example returns (heat.rs:103-139): `Ok((iterations, error))` when
    `converged`, `Err(error)` otherwise (then `iterations == max_iter`).  `levels` is the length of the
    longest chain of rows that have to be swept one after the other (device-side information)."""

    def __init__(self, info):
        self.converged = bool(info.converged)
        self.iterations = int(info.iterations)
        self.error = float(info.error)
        self.levels = int(info.levels)

    def __repr__(self):
        return ("Ok((%d, %r))" % (self.iterations, self.error)) if self.converged else "Err(%r)" % self.error


def _same_precision(mat, *vecs):
    """The vectors of an operation on `mat` are of its precision: DeviceVecF32 with a DeviceCsMatF32 and with no other matrix."""
    from .device import DeviceCsMatF32, DeviceVecF32
    f32 = isinstance(mat, DeviceCsMatF32)
    if any(isinstance(v, DeviceVecF32) != f32 for v in vecs):
        raise TypeError("matrix and vectors must have the same precision")


def gauss_seidel(mat, x, rhs, max_iter, eps, stream=None):
    """gauss_seidel(mat, x, rhs, max_iter, eps) (heat.rs:103-139): mat a square CSR DeviceCsMat, x (start vector,
    overwritten with the result like the reference's `mut x`) and rhs DeviceVecs.  Dimension mismatch and a row
    without a diagonal entry raise, like the reference's asserts / `diag.unwrap()`.  A DeviceCsMatF32 with DeviceVecF32
    vectors runs gauss_seidel::<f32> (sprs_hip_gauss_seidel_f32): eps is rounded to f32 first, `error` is the f32 value."""
    _same_precision(mat, x, rhs)
    if x.n != rhs.n:
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
    info = _GsInfo()
    check(mat._op("gauss_seidel")(mat._h, C.c_void_p(x.ptr), C.c_void_p(rhs.ptr), x.n, int(max_iter), float(mat._dtype(eps)),
                                  C.byref(info), C.c_void_p(int(stream) if stream else 0)))
    return GaussSeidelResult(info)


class _TriInfo(C.Structure):
    _fields_ = [("levels", C.c_uint64), ("singular_index", C.c_uint64), ("singular_reason", C.c_int32)]


class TriSolveResult:
    """`Ok(())` of a triangular solve.  `levels` is the length of the longest chain of unknowns that have to be solved one
    after the other (device-side information)."""

    def __init__(self, info):
        self.levels = int(info.levels)

    def __repr__(self):
        return "Ok(())"


_SINGULAR_REASONS = {1: "numeric", 2: "structural"}


def _trisolve(mat, rhs, storage, uplo, stream):
    _same_precision(mat, rhs)
    if mat.storage() != storage:                    # assert!(mat.is_csr() / is_csc(), "Storage mismatch"): trisolve.rs:42, 98, 174, 232
        raise _ffi.SprsHipError(_ffi.STORAGE_MISMATCH, "Storage mismatch")
    info = _TriInfo()
    status = mat._op("trisolve")(mat._h, uplo, C.c_void_p(rhs.ptr), rhs.n, C.byref(info),
                                 C.c_void_p(int(stream) if stream else 0))
    if status == _ffi.SINGULAR_MATRIX:              # Err(LinalgError::SingularMatrix(SingularMatrixInfo { index, reason }))
        err = _ffi.SprsHipError(status, lib.sprs_hip_last_error().decode("utf-8", "replace"))
        err.index = int(info.singular_index)
        err.reason = _SINGULAR_REASONS[int(info.singular_reason)]
        raise err
    check(status)
    return TriSolveResult(info)


def lsolve_csr_dense_rhs(mat, rhs, stream=None):
    """lsolve_csr_dense_rhs(lower_tri_mat, rhs) (trisolve.rs:30-73): mat a square CSR DeviceCsMat (its upper triangle is
    ignored), rhs a DeviceVec solved in place.  Raises SprsHipError: DIM_MISMATCH / STORAGE_MISMATCH like the reference's
    asserts, SINGULAR_MATRIX (with `.index` and `.reason`, "numeric" or "structural") where it returns Err.  All four solves take
    a DeviceCsMatF32 with a DeviceVecF32 as well (sprs_hip_trisolve_f32: the reference's f32 bits); a vector of the other
    precision raises TypeError."""
    return _trisolve(mat, rhs, _ffi.CSR, _ffi.LOWER, stream)


def usolve_csr_dense_rhs(mat, rhs, stream=None):
    """usolve_csr_dense_rhs(upper_tri_mat, rhs) (trisolve.rs:219-262): as lsolve_csr_dense_rhs, with the upper triangle."""
    return _trisolve(mat, rhs, _ffi.CSR, _ffi.UPPER, stream)


def lsolve_csc_dense_rhs(mat, rhs, stream=None):
    """lsolve_csc_dense_rhs(lower_tri_mat, rhs) (trisolve.rs:85-149): mat a square CSC DeviceCsMat; a diagonal that is not
    stored is reported as "structural", a stored zero as "numeric"."""
    return _trisolve(mat, rhs, _ffi.CSC, _ffi.LOWER, stream)


def usolve_csc_dense_rhs(mat, rhs, stream=None):
    """usolve_csc_dense_rhs(upper_tri_mat, rhs) (trisolve.rs:161-210): every unknown receives its subtractions by DESCENDING
    column, so the bits differ from usolve_csr_dense_rhs on the same matrix, as they do in the reference."""
    return _trisolve(mat, rhs, _ffi.CSC, _ffi.UPPER, stream)


class _SpTriInfo(C.Structure):
    _fields_ = [("reach", C.c_uint64), ("reach_levels", C.c_uint64), ("reach_launches", C.c_uint64), ("solve_levels", C.c_uint64),
                ("singular_index", C.c_uint64), ("singular_reason", C.c_int32)]


def lsolve_csc_sparse_rhs(mat, rhs, stream=None):
    """lsolve_csc_sparse_rhs(lower_tri_mat, rhs, ..) (trisolve.rs:286-358): mat a square CSC DeviceCsMat, rhs a DeviceCsVec.
    Returns the solution as a new DeviceCsVec whose pattern is the reach of rhs in ascending order (numeric zeros kept), where
    the reference leaves an unsorted stack and a dense workspace; `.reach`, `.reach_levels`, `.reach_launches` and
    `.solve_levels` of the result are device-side information.  Fill-in unknowns start from +0.0.  Raises SprsHipError:
    INVALID_ARG for a CSR matrix ("Storage mismatch"), DIM_MISMATCH, and SINGULAR_MATRIX (with `.index`, the smallest singular
    index of the reach, and `.reason`) — a singular column outside the reach is not an error."""
    from .device import DeviceCsVec
    info, h = _SpTriInfo(), C.c_void_p()
    status = lib.sprs_hip_lsolve_csc_sparse_rhs_f64(mat._h, rhs._h, C.byref(h), C.byref(info), C.c_void_p(int(stream) if stream else 0))
    if status == _ffi.SINGULAR_MATRIX:              # Err(LinalgError::SingularMatrix(SingularMatrixInfo { index, reason }))
        err = _ffi.SprsHipError(status, lib.sprs_hip_last_error().decode("utf-8", "replace"))
        err.index = int(info.singular_index)
        err.reason = _SINGULAR_REASONS[int(info.singular_reason)]
        raise err
    check(status)
    out = DeviceCsVec(h.value)
    out.reach, out.reach_levels = int(info.reach), int(info.reach_levels)
    out.reach_launches, out.solve_levels = int(info.reach_launches), int(info.solve_levels)
    return out


def diag_solve(diag, x, stream=None):
    """linalg::diag_solve (sprs/src/sparse/linalg.rs:17-29): x[i] /= diag[i], in place on the DeviceVec x; two DeviceVecF32
    run diag_solve::<f32>."""
    from .device import DeviceVecF32
    if isinstance(diag, DeviceVecF32) != isinstance(x, DeviceVecF32):
        raise TypeError("diag and x must have the same precision")
    if diag.n != x.n:                               # assert_eq!(diag.len(), x.len())
        raise _ffi.SprsHipError(_ffi.DIM_MISMATCH, "Dimension mismatch")
    entry = lib.sprs_hip_diag_solve_f32 if isinstance(x, DeviceVecF32) else lib.sprs_hip_diag_solve_f64
    check(entry(C.c_void_p(diag.ptr), C.c_void_p(x.ptr), x.n, C.c_void_p(int(getattr(stream, "cuda_stream", stream)) if stream else 0)))
    return x
