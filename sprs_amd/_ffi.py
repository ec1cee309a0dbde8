"""ctypes binding of libsprs_hip.so (include/sprs_hip.h).

This is the Python stand-in for the `sprs-hip-sys` crate: raw declarations
only.  There is NO CPU fallback: if the shared library is missing the import
fails loudly, and if no gfx950 device is usable every compute entry point
returns SPRS_HIP_NO_DEVICE, surfaced as SprsHipError.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPRS_HIP_LIBRARY: explicit path of the shared library to bind (deployments that keep it elsewhere; the
# kernel-logic tests point it at the emulator build of the same sources, tests/emu).  No fallback either way.
LIB_PATH = os.environ.get("SPRS_HIP_LIBRARY") or os.path.join(_HERE, "libsprs_hip.so")

OK, DIM_MISMATCH, STORAGE_MISMATCH, INDEX_OVERFLOW, BAD_STRUCTURE, INVALID_ARG, \
    OUT_OF_MEMORY, HIP_ERROR, NO_DEVICE, SINGULAR_MATRIX = range(10)
CSR, CSC = 0, 1
LOWER, UPPER = 0, 1
ROW_MAJOR, COL_MAJOR = 0, 1
ROUTE_RCCL, ROUTE_PEER = 0, 1
BINOP_ADD, BINOP_SUB, BINOP_MUL = 0, 1, 2
NORM_SQUARED_L2, NORM_L2, NORM_L1, NORM_P = 0, 1, 2, 3
NONE = (1 << 64) - 1           # a position of the batched nnz_index: nothing is stored there (the reference's None)
START_NEXT, START_MINIMUM_DEGREE, START_PSEUDO_PERIPHERAL = 0, 1, 2
KIND_OK, KIND_UNSORTED, KIND_SIZE_MISMATCH, KIND_OUT_OF_RANGE = 0, 1, 2, 3     # StructureErrorKind (errors.rs)
NO_OUTER = (1 << 64) - 1       # StructureInfo.outer of a finding about the dimensions or the indptr

STATUS_NAMES = {
    OK: "OK", DIM_MISMATCH: "DIM_MISMATCH", STORAGE_MISMATCH: "STORAGE_MISMATCH",
    INDEX_OVERFLOW: "INDEX_OVERFLOW", BAD_STRUCTURE: "BAD_STRUCTURE", INVALID_ARG: "INVALID_ARG",
    OUT_OF_MEMORY: "OUT_OF_MEMORY", HIP_ERROR: "HIP_ERROR", NO_DEVICE: "NO_DEVICE",
    SINGULAR_MATRIX: "SINGULAR_MATRIX",
}

u64, i32, i64, vp = C.c_uint64, C.c_int32, C.c_int64, C.c_void_p
P = C.POINTER

# name -> (restype, argtypes); must list every symbol include/sprs_hip.h declares
SIGNATURES = {
    "sprs_hip_last_error": (C.c_char_p, []),
    "sprs_hip_last_hip_code": (i32, []),
    "sprs_hip_version": (C.c_char_p, []),
    "sprs_hip_device_count": (i32, [P(i32)]),
    "sprs_hip_set_device": (i32, [i32]),
    "sprs_hip_malloc": (i32, [P(vp), u64]),
    "sprs_hip_free": (i32, [vp]),
    "sprs_hip_memcpy_h2d": (i32, [vp, vp, u64]),
    "sprs_hip_memcpy_d2h": (i32, [vp, vp, u64]),
    "sprs_hip_memcpy_d2d": (i32, [vp, vp, u64, vp]),
    "sprs_hip_memset": (i32, [vp, i32, u64, vp]),
    "sprs_hip_synchronize": (i32, [vp]),
    "sprs_hip_pool_trim": (i32, [P(u64)]),
    "sprs_hip_mul_acc_mat_vec_csc_f64": (i32, [vp, vp, u64, vp, u64, vp]),
    "sprs_hip_csmat_mul_vec_f64": (i32, [vp, vp, u64, vp, u64, vp]),
    "sprs_hip_csmat_mulacc_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, vp, u64, i32, u64, i32, vp]),
    "sprs_hip_csmat_mul_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, vp, P(i32), vp]),
    "sprs_hip_dense_dot_csmat_f64": (i32, [vp, u64, u64, i32, u64, vp, vp, P(i32), vp]),
    "sprs_hip_dist_comm_count": (i32, [vp, P(i32)]),
    "sprs_hip_spgemm_symbolic": (i32, [vp, vp, P(vp)]),
    "sprs_hip_spgemm_numeric": (i32, [vp, vp, vp]),
    "sprs_hip_spgemm_plan_create": (i32, [vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_nnz": (i32, [vp, P(u64)]),
    "sprs_hip_spgemm_plan_structure": (i32, [vp, vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_product": (i32, [vp, vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_numeric": (i32, [vp, vp, vp, vp]),
    "sprs_hip_spgemm_plan_free": (i32, [vp]),
    "sprs_hip_bicgstab_f64": (i32, [vp, vp, vp, u64, C.c_double, u64, C.c_double, vp, vp, vp]),
    "sprs_hip_gauss_seidel_f64": (i32, [vp, vp, vp, u64, u64, C.c_double, vp, vp]),
    "sprs_hip_trisolve_f64": (i32, [vp, i32, vp, u64, vp, vp]),
    "sprs_hip_lsolve_csc_sparse_rhs_f64": (i32, [vp, vp, P(vp), vp, vp]),
    "sprs_hip_csmat_upload": (i32, [P(vp), i32, u64, u64, vp, i32, vp, i32, vp, i32]),
    "sprs_hip_csmat_wrap_device": (i32, [P(vp), i32, u64, u64, u64, vp, i32, vp, i32, vp]),
    "sprs_hip_csmat_info": (i32, [vp, P(u64), P(u64), P(u64), P(i32), P(i32), P(i32)]),
    "sprs_hip_csmat_device_ptrs": (i32, [vp, P(vp), P(vp), P(vp)]),
    "sprs_hip_csmat_download": (i32, [vp, vp, vp, vp]),
    "sprs_hip_csmat_download_outer": (i32, [vp, u64, u64, vp, vp, vp, P(u64)]),
    "sprs_hip_csmat_slice_outer": (i32, [vp, u64, u64, P(vp)]),
    "sprs_hip_csmat_refresh": (i32, [vp]),
    "sprs_hip_csmat_prepare": (i32, [vp, vp]),
    "sprs_hip_csmat_spmv_plan_info": (i32, [vp, P(i32), P(u64)]),
    "sprs_hip_csmat_transpose_view": (i32, [vp, P(vp)]),
    "sprs_hip_csmat_free": (i32, [vp]),
    "sprs_hip_spmv_f64": (i32, [vp, vp, u64, vp, u64, i32, vp]),
    "sprs_hip_spmv_f64_host": (i32, [u64, u64, vp, i32, vp, i32, vp, vp, u64, vp, u64, i32]),
    "sprs_hip_spmm_rowmaj_f64": (i32, [vp, vp, u64, u64, u64, vp, u64, u64, i32, vp]),
    "sprs_hip_spgemm_f64": (i32, [vp, vp, P(vp)]),
    "sprs_hip_csmat_to_other_storage": (i32, [vp, P(vp)]),
    "sprs_hip_dist_unique_id": (i32, [vp]),
    "sprs_hip_dist_create": (i32, [P(vp), vp, i32, i32, u64, u64, P(u64), vp, i32]),
    "sprs_hip_dist_spmv_f64": (i32, [vp, vp, u64, vp, u64, vp]),
    "sprs_hip_dist_peer_handle": (i32, [vp, vp]),
    "sprs_hip_dist_peer_connect": (i32, [vp, vp, i32]),
    "sprs_hip_dist_set_route": (i32, [vp, i32]),
    "sprs_hip_dist_route": (i32, [vp, P(i32)]),
    "sprs_hip_dist_free": (i32, [vp]),
    "sprs_hip_csmat_mul_csmat": (i32, [vp, vp, P(vp)]),
    "sprs_hip_triplets_to_cs": (i32, [u64, u64, u64, vp, vp, i32, vp, i32, i32, i32, P(vp)]),
    "sprs_hip_csvec_upload": (i32, [P(vp), u64, u64, vp, i32, vp, i32]),
    "sprs_hip_csvec_wrap_device": (i32, [P(vp), u64, u64, vp, i32, vp]),
    "sprs_hip_csvec_info": (i32, [vp, P(u64), P(u64), P(i32)]),
    "sprs_hip_csvec_device_ptrs": (i32, [vp, P(vp), P(vp)]),
    "sprs_hip_csvec_download": (i32, [vp, vp, vp]),
    "sprs_hip_csvec_free": (i32, [vp]),
    "sprs_hip_csvec_scatter_f64": (i32, [vp, vp, u64, vp]),
    "sprs_hip_csmat_mul_csvec_f64": (i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csvec_mul_csmat_f64": (i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csmat_binop_f64": (i32, [vp, vp, i32, P(vp), vp]),
    "sprs_hip_csmat_add_csmat_f64": (i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csmat_sub_csmat_f64": (i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csmat_scale_f64": (i32, [vp, C.c_double, P(vp), vp]),
    "sprs_hip_csvec_binop_f64": (i32, [vp, vp, i32, P(vp), vp]),
    "sprs_hip_csvec_dot_f64": (i32, [vp, vp, P(C.c_double), vp]),
    "sprs_hip_csvec_dot_dense_f64": (i32, [vp, vp, u64, P(C.c_double), vp]),
    "sprs_hip_csvec_norm_f64": (i32, [vp, i32, C.c_double, P(C.c_double), vp]),
    "sprs_hip_csvec_unit_normalize_f64": (i32, [vp, P(vp), vp]),
    "sprs_hip_csvec_nnz_index": (i32, [vp, u64, vp, vp, vp, vp]),
    "sprs_hip_csmat_outer_view": (i32, [vp, u64, P(vp), vp]),
    "sprs_hip_csmat_diag_f64": (i32, [vp, P(vp), vp]),
    "sprs_hip_csmat_nnz_index": (i32, [vp, u64, vp, vp, vp, vp, vp]),
    "sprs_hip_csmat_to_inner_onehot_f64": (i32, [vp, P(vp), vp]),
    "sprs_hip_perm_upload": (i32, [P(vp), u64, vp, i32, i32]),
    "sprs_hip_perm_from_device": (i32, [P(vp), u64, vp, i32, i32, vp]),
    "sprs_hip_perm_identity": (i32, [P(vp), u64, i32]),
    "sprs_hip_perm_info": (i32, [vp, P(u64), P(i32), P(i32)]),
    "sprs_hip_perm_is_identity": (i32, [vp, P(i32), vp]),
    "sprs_hip_perm_device_ptrs": (i32, [vp, P(vp), P(vp)]),
    "sprs_hip_perm_download": (i32, [vp, vp, vp]),
    "sprs_hip_perm_inv": (i32, [vp, P(vp)]),
    "sprs_hip_perm_free": (i32, [vp]),
    "sprs_hip_perm_mul_vec_f64": (i32, [vp, vp, vp, u64, vp]),
    "sprs_hip_csmat_transform_paq": (i32, [vp, vp, vp, P(vp), vp]),
    "sprs_hip_csmat_transform_papt": (i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csmat_check_structure": (i32, [vp, vp, vp]),
    "sprs_hip_csvec_check_structure": (i32, [vp, vp, vp]),
    "sprs_hip_csmat_from_unsorted": (i32, [vp, P(vp), vp, vp]),
    "sprs_hip_csvec_from_unsorted": (i32, [vp, P(vp), vp, vp]),
    "sprs_hip_csmat_is_symmetric": (i32, [vp, P(i32), vp]),
    "sprs_hip_csmat_degrees": (i32, [vp, vp, vp]),
    "sprs_hip_csmat_max_outer_nnz": (i32, [vp, P(u64), vp]),
    "sprs_hip_csmat_cuthill_mckee": (i32, [vp, i32, i32, i32, P(vp), vp]),
    "sprs_hip_ordering_info": (i32, [vp, P(u64), P(u64), P(u64)]),
    "sprs_hip_ordering_perm": (i32, [vp, P(vp)]),
    "sprs_hip_ordering_parts": (i32, [vp, vp]),
    "sprs_hip_ordering_free": (i32, [vp]),
    "sprs_hip_ldl_symbolic": (i32, [vp, vp, i32, P(vp), vp]),
    "sprs_hip_ldl_symbolic_info": (i32, [vp, P(u64), P(u64), P(u64)]),
    "sprs_hip_ldl_symbolic_colptr": (i32, [vp, vp]),
    "sprs_hip_ldl_symbolic_parents": (i32, [vp, vp]),
    "sprs_hip_ldl_symbolic_perm": (i32, [vp, P(vp)]),
    "sprs_hip_ldl_symbolic_free": (i32, [vp]),
    "sprs_hip_ldl_factor_f64": (i32, [vp, vp, P(vp), vp, vp]),
    "sprs_hip_ldl_update_f64": (i32, [vp, vp, vp, vp]),
    "sprs_hip_ldl_solve_f64": (i32, [vp, vp, vp, u64, vp]),
    "sprs_hip_ldl_d": (i32, [vp, vp, u64, vp]),
    "sprs_hip_ldl_l": (i32, [vp, P(vp), vp]),
    "sprs_hip_ldl_numeric_free": (i32, [vp]),
    "sprs_hip_ldl_lsolve_f64": (i32, [vp, vp, u64, vp]),
    "sprs_hip_ldl_ltsolve_f64": (i32, [vp, vp, u64, vp]),
    "sprs_hip_diag_solve_f64": (i32, [vp, vp, u64, vp]),
    "sprs_hip_csmat_kronecker_f64":(i32, [vp, vp, P(vp), vp]),
    "sprs_hip_csmat_same_storage_fast_stack": (i32, [P(vp), u64, P(vp), vp]),
    "sprs_hip_csmat_vstack": (i32, [P(vp), u64, P(vp), vp]),
    "sprs_hip_csmat_hstack": (i32, [P(vp), u64, P(vp), vp]),
    "sprs_hip_csmat_bmat": (i32, [P(vp), u64, u64, P(vp), vp]),
    "sprs_hip_csmat_from_dense_f64": (i32, [P(vp), i32, vp, u64, u64, i32, u64, C.c_double, i32, i32, vp]),
    "sprs_hip_csmat_assign_to_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, vp]),
    "sprs_hip_csmat_to_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, vp]),
    "sprs_hip_csmat_binop_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, i32, C.c_double, C.c_double, vp, u64, vp]),
    "sprs_hip_csmat_add_dense_f64": (i32, [vp, vp, u64, u64, i32, u64, vp, vp]),
    "sprs_hip_csmat_f32_upload": (i32, [P(vp), i32, u64, u64, vp, i32, vp, i32, vp, i32]),
    "sprs_hip_csmat_f32_wrap_device": (i32, [P(vp), i32, u64, u64, u64, vp, i32, vp, i32, vp]),
    "sprs_hip_csmat_f32_info": (i32, [vp, P(u64), P(u64), P(u64), P(i32), P(i32), P(i32)]),
    "sprs_hip_csmat_f32_device_ptrs": (i32, [vp, P(vp), P(vp), P(vp)]),
    "sprs_hip_csmat_f32_download": (i32, [vp, vp, vp, vp]),
    "sprs_hip_csmat_f32_transpose_view": (i32, [vp, P(vp)]),
    "sprs_hip_csmat_f32_refresh": (i32, [vp]),
    "sprs_hip_csmat_f32_prepare": (i32, [vp, vp]),
    "sprs_hip_csmat_f32_spmv_plan_info": (i32, [vp, P(i32), P(u64)]),
    "sprs_hip_csmat_f32_free": (i32, [vp]),
    "sprs_hip_csmat_f32_to_other_storage": (i32, [vp, P(vp)]),
    "sprs_hip_csmat_f32_from_f64": (i32, [vp, P(vp), vp]),
    "sprs_hip_csmat_f32_to_f64": (i32, [vp, P(vp), vp]),
    "sprs_hip_spmv_f32": (i32, [vp, vp, u64, vp, u64, i32, vp]),
    "sprs_hip_mul_acc_mat_vec_csc_f32": (i32, [vp, vp, u64, vp, u64, vp]),
    "sprs_hip_csmat_mul_vec_f32": (i32, [vp, vp, u64, vp, u64, vp]),
    "sprs_hip_bicgstab_f32": (i32, [vp, vp, vp, u64, C.c_double, u64, C.c_double, vp, vp, vp]),
    "sprs_hip_trisolve_f32": (i32, [vp, i32, vp, u64, vp, vp]),
    "sprs_hip_gauss_seidel_f32": (i32, [vp, vp, vp, u64, u64, C.c_double, vp, vp]),
    "sprs_hip_diag_solve_f32": (i32, [vp, vp, u64, vp]),
    "sprs_hip_spmm_rowmaj_f32": (i32, [vp, vp, u64, u64, u64, vp, u64, u64, i32, vp]),
    "sprs_hip_csmat_mulacc_dense_f32": (i32, [vp, vp, u64, u64, i32, u64, vp, u64, i32, u64, i32, vp]),
    "sprs_hip_csmat_mul_dense_f32": (i32, [vp, vp, u64, u64, i32, u64, vp, P(i32), vp]),
    "sprs_hip_dense_dot_csmat_f32": (i32, [vp, u64, u64, i32, u64, vp, vp, P(i32), vp]),
    "sprs_hip_spgemm_f32": (i32, [vp, vp, P(vp)]),
    "sprs_hip_spgemm_symbolic_f32": (i32, [vp, vp, P(vp)]),
    "sprs_hip_spgemm_numeric_f32": (i32, [vp, vp, vp]),
    "sprs_hip_spgemm_plan_create_f32": (i32, [vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_structure_f32": (i32, [vp, vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_product_f32": (i32, [vp, vp, vp, P(vp)]),
    "sprs_hip_spgemm_plan_numeric_f32": (i32, [vp, vp, vp, vp]),
    "sprs_hip_csmat_mul_csmat_f32": (i32, [vp, vp, P(vp)]),
    "sprs_hip_set_option": (i32, [C.c_char_p, i64]),
    "sprs_hip_get_option": (i32, [C.c_char_p, P(i64)]),
}


class SprsHipError(RuntimeError):
    """A non-OK status from libsprs_hip.so.  The message of the contract
    violations is the reference's own panic text ("Dimension mismatch",
    "Storage mismatch", "Index type is not large enough to hold ...")."""

    def __init__(self, status, message, hip_code=0, kind=None, outer=None):
        self.status = status
        self.hip_code = hip_code
        self.kind = kind       # structure checks: the StructureErrorKind (KIND_*) ...
        self.outer = outer     # ... and the first offending outer slice (NO_OUTER: the dimensions or the indptr)
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "sprs_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C sprs_amd/csrc`.  There is no CPU fallback." % LIB_PATH)



def _preload_shared_hip_runtime():
    """One process must use ONE libamdhip64: PyTorch wheels bundle their own
    copy (same SONAME as /opt/rocm's).  If torch is installed, load its copy
    first so that libsprs_hip.so and torch share a single HIP runtime whatever
    the import order (bench.py and the multi-GPU path hand torch-owned device
    buffers to this library).  torch itself is NOT imported here."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:   # fall back to the system ROCm runtime (RUNPATH of the .so)
        pass


_preload_shared_hip_runtime()
lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(lib, _name)   # AttributeError here == the .so does not match the header
    _f.restype = _res
    _f.argtypes = _args


class StructureInfo(C.Structure):
    """sprs_hip_structure_info"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("outer", C.c_uint64)]


def check_structure_status(status, info):
    """check() for the four structure entry points: the error carries the info struct's kind and outer slice"""
    if status != OK:
        raise SprsHipError(status, lib.sprs_hip_last_error().decode("utf-8", "replace"), lib.sprs_hip_last_hip_code(),
                           kind=info.kind, outer=info.outer)


def check(status):
    if status != OK:
        raise SprsHipError(status, lib.sprs_hip_last_error().decode("utf-8", "replace"),
                           lib.sprs_hip_last_hip_code())
