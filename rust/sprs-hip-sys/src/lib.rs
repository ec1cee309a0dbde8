//! Raw declarations of `include/sprs_hip.h` (NOT COMPILED in the build
//! environment of this repository: no rustc there).  One item per C entry point.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const SPRS_HIP_OK: i32 = 0;
pub const SPRS_HIP_DIM_MISMATCH: i32 = 1;
pub const SPRS_HIP_STORAGE_MISMATCH: i32 = 2;
pub const SPRS_HIP_INDEX_OVERFLOW: i32 = 3;
pub const SPRS_HIP_BAD_STRUCTURE: i32 = 4;
pub const SPRS_HIP_INVALID_ARG: i32 = 5;
pub const SPRS_HIP_OUT_OF_MEMORY: i32 = 6;
pub const SPRS_HIP_HIP_ERROR: i32 = 7;
pub const SPRS_HIP_NO_DEVICE: i32 = 8;
pub const SPRS_HIP_SINGULAR_MATRIX: i32 = 9;
pub const SPRS_HIP_LOWER: i32 = 0;
pub const SPRS_HIP_UPPER: i32 = 1;
pub const SPRS_HIP_CSR: i32 = 0;
pub const SPRS_HIP_CSC: i32 = 1;
pub const SPRS_HIP_ROW_MAJOR: i32 = 0;
pub const SPRS_HIP_COL_MAJOR: i32 = 1;
pub const SPRS_HIP_ROUTE_RCCL: i32 = 0;
pub const SPRS_HIP_ROUTE_PEER: i32 = 1;
pub const SPRS_HIP_BINOP_ADD: i32 = 0;
pub const SPRS_HIP_BINOP_SUB: i32 = 1;
pub const SPRS_HIP_BINOP_MUL: i32 = 2;
pub const SPRS_HIP_NORM_SQUARED_L2: i32 = 0;
pub const SPRS_HIP_NORM_L2: i32 = 1;
pub const SPRS_HIP_NORM_L1: i32 = 2;
pub const SPRS_HIP_NORM_P: i32 = 3;
pub const SPRS_HIP_START_NEXT: i32 = 0;
pub const SPRS_HIP_START_MINIMUM_DEGREE: i32 = 1;
pub const SPRS_HIP_START_PSEUDO_PERIPHERAL: i32 = 2;

#[repr(C)]
pub struct sprs_hip_spgemm_plan {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_dist {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_csmat {
    _private: [u8; 0],
}

/// `CsMat<f32>`: a handle type of its own, so that no `f64` entry can be handed `f32` buffers.
#[repr(C)]
pub struct sprs_hip_csmat_f32 {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_csvec {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_perm {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_ordering {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_ldl_sym {
    _private: [u8; 0],
}

#[repr(C)]
pub struct sprs_hip_ldl_num {
    _private: [u8; 0],
}

/// counters of BiCGSTAB::solve (include/sprs_hip.h)
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sprs_hip_bicgstab_info {
    pub iteration_count: u64,
    pub soft_restart_count: u64,
    pub hard_restart_count: u64,
    pub err: f64,
    pub rho: f64,
    pub converged: i32,
}

/// result of gauss_seidel (include/sprs_hip.h; the reference's examples/heat.rs:103-139)
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sprs_hip_gauss_seidel_info {
    pub iterations: u64,
    pub error: f64,
    pub converged: i32,
    pub levels: u64,
}

/// result of sprs_hip_trisolve_f64 (include/sprs_hip.h; the reference's sparse/linalg/trisolve.rs).  Filled in by the
/// library before any use: singular_index = u64::MAX and singular_reason = 0 unless the matrix is singular
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sprs_hip_trisolve_info {
    pub levels: u64,
    pub singular_index: u64,
    pub singular_reason: i32,
}

/// result of sprs_hip_lsolve_csc_sparse_rhs_f64 (include/sprs_hip.h; trisolve.rs:286-358): the size of the reach, the levels
/// and launches of the search that found it, the levels of the handle's lower level plan; the singular report as above
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sprs_hip_sptrisolve_info {
    pub reach: u64,
    pub reach_levels: u64,
    pub reach_launches: u64,
    pub solve_levels: u64,
    pub singular_index: u64,
    pub singular_reason: i32,
}

/// result of the structure checks and of new_from_unsorted (include/sprs_hip.h): kind = StructureErrorKind (0 ok, 1 Unsorted,
/// 2 SizeMismatch, 3 OutOfRange), outer = the first offending outer slice (u64::MAX for the dimensions or the indptr)
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct sprs_hip_structure_info {
    pub kind: i32,
    pub reserved: i32,
    pub outer: u64,
}

extern "C" {
    pub fn sprs_hip_last_error() -> *const c_char;
    pub fn sprs_hip_last_hip_code() -> i32;
    pub fn sprs_hip_version() -> *const c_char;
    pub fn sprs_hip_device_count(count: *mut i32) -> i32;
    pub fn sprs_hip_set_device(device: i32) -> i32;
    pub fn sprs_hip_malloc(dev_ptr: *mut *mut c_void, bytes: u64) -> i32;
    pub fn sprs_hip_free(dev_ptr: *mut c_void) -> i32;
    pub fn sprs_hip_memcpy_h2d(dev_dst: *mut c_void, host_src: *const c_void, bytes: u64) -> i32;
    pub fn sprs_hip_memcpy_d2h(host_dst: *mut c_void, dev_src: *const c_void, bytes: u64) -> i32;
    pub fn sprs_hip_memcpy_d2d(dev_dst: *mut c_void, dev_src: *const c_void, bytes: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_memset(dev_dst: *mut c_void, byte_value: i32, bytes: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_synchronize(stream: *mut c_void) -> i32;
    pub fn sprs_hip_pool_trim(freed_bytes: *mut u64) -> i32;
    pub fn sprs_hip_bicgstab_f64(a: *mut sprs_hip_csmat, x0_dev: *const f64, b_dev: *const f64, n: u64, tol: f64,
                                 max_iter: u64, soft_restart_threshold: f64, x_dev: *mut f64,
                                 info: *mut sprs_hip_bicgstab_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_gauss_seidel_f64(a: *mut sprs_hip_csmat, x_dev: *mut f64, rhs_dev: *const f64, n: u64, max_iter: u64,
                                     eps: f64, info: *mut sprs_hip_gauss_seidel_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_trisolve_f64(a: *mut sprs_hip_csmat, uplo: i32, x_dev: *mut f64, n: u64,
                                 info: *mut sprs_hip_trisolve_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_lsolve_csc_sparse_rhs_f64(l: *mut sprs_hip_csmat, rhs: *const sprs_hip_csvec, out: *mut *mut sprs_hip_csvec,
                                              info: *mut sprs_hip_sptrisolve_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_upload(
        out: *mut *mut sprs_hip_csmat, storage: i32, rows: u64, cols: u64,
        indptr: *const c_void, iptr_bytes: i32, indices: *const c_void, idx_bytes: i32,
        data: *const f64, validate: i32,
    ) -> i32;
    pub fn sprs_hip_csmat_wrap_device(
        out: *mut *mut sprs_hip_csmat, storage: i32, rows: u64, cols: u64, nnz: u64,
        dev_indptr: *const c_void, iptr_bytes: i32, dev_indices: *const c_void, idx_bytes: i32,
        dev_data: *const f64,
    ) -> i32;
    pub fn sprs_hip_csmat_info(
        m: *const sprs_hip_csmat, rows: *mut u64, cols: *mut u64, nnz: *mut u64,
        iptr_bytes: *mut i32, idx_bytes: *mut i32, storage: *mut i32,
    ) -> i32;
    pub fn sprs_hip_csmat_device_ptrs(
        m: *const sprs_hip_csmat, indptr: *mut *const c_void, indices: *mut *const c_void,
        data: *mut *const f64,
    ) -> i32;
    pub fn sprs_hip_csmat_download(m: *const sprs_hip_csmat, indptr: *mut c_void, indices: *mut c_void, data: *mut f64) -> i32;
    pub fn sprs_hip_csmat_download_outer(
        m: *const sprs_hip_csmat, start: u64, end: u64, indptr_out: *mut c_void,
        indices_out: *mut c_void, data_out: *mut f64, nnz_out: *mut u64,
    ) -> i32;
    pub fn sprs_hip_csmat_slice_outer(m: *const sprs_hip_csmat, start: u64, end: u64, out: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_csmat_refresh(m: *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_csmat_prepare(m: *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_spmv_plan_info(m: *const sprs_hip_csmat, kind: *mut i32, plan_bytes: *mut u64) -> i32;
    pub fn sprs_hip_csmat_transpose_view(m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_csmat_free(m: *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spmv_f64(
        a: *const sprs_hip_csmat, x_dev: *const f64, x_len: u64, y_dev: *mut f64, y_len: u64,
        accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_spmv_f64_host(
        rows: u64, cols: u64, indptr: *const c_void, iptr_bytes: i32, indices: *const c_void,
        idx_bytes: i32, data: *const f64, x: *const f64, x_len: u64, y: *mut f64, y_len: u64,
        accumulate: i32,
    ) -> i32;
    pub fn sprs_hip_spmm_rowmaj_f64(
        a: *const sprs_hip_csmat, rhs_dev: *const f64, rhs_rows: u64, k: u64, ld_rhs: u64,
        out_dev: *mut f64, out_rows: u64, ld_out: u64, accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_mul_acc_mat_vec_csc_f64(
        a: *const sprs_hip_csmat, x_dev: *const f64, x_len: u64, y_dev: *mut f64, y_len: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mul_vec_f64(
        a: *const sprs_hip_csmat, x_dev: *const f64, x_len: u64, y_dev: *mut f64, y_len: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mulacc_dense_f64(
        lhs: *const sprs_hip_csmat, rhs_dev: *const f64, rhs_rows: u64, k: u64, rhs_layout: i32, ld_rhs: u64,
        out_dev: *mut f64, out_rows: u64, out_layout: i32, ld_out: u64, accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mul_dense_f64(
        lhs: *const sprs_hip_csmat, rhs_dev: *const f64, rhs_rows: u64, k: u64, rhs_layout: i32, ld_rhs: u64,
        out_dev: *mut f64, out_layout: *mut i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_dense_dot_csmat_f64(
        lhs_dev: *const f64, lhs_rows: u64, lhs_cols: u64, lhs_layout: i32, ld_lhs: u64, rhs: *const sprs_hip_csmat,
        out_dev: *mut f64, out_layout: *mut i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_spgemm_f64(a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_symbolic(a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c_structure: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_numeric(a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c: *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_plan_create(a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, plan: *mut *mut sprs_hip_spgemm_plan) -> i32;
    pub fn sprs_hip_spgemm_plan_nnz(plan: *const sprs_hip_spgemm_plan, nnz: *mut u64) -> i32;
    pub fn sprs_hip_spgemm_plan_structure(plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c_structure: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_plan_product(plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_plan_numeric(plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, c: *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_spgemm_plan_free(plan: *mut sprs_hip_spgemm_plan) -> i32;
    pub fn sprs_hip_csmat_to_other_storage(m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_dist_unique_id(id_128_bytes: *mut c_void) -> i32;
    pub fn sprs_hip_dist_create(
        d: *mut *mut sprs_hip_dist, id_128_bytes: *const c_void, world: i32, rank: i32, rows: u64, cols: u64,
        row_starts: *const u64, local_block: *const sprs_hip_csmat, nsub: i32,
    ) -> i32;
    pub fn sprs_hip_dist_spmv_f64(d: *mut sprs_hip_dist, x_dev: *const f64, x_len: u64, y_dev: *mut f64, y_len: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_dist_comm_count(d: *const sprs_hip_dist, ranks: *mut i32) -> i32;
    pub fn sprs_hip_dist_peer_handle(d: *mut sprs_hip_dist, handle_64_bytes: *mut c_void) -> i32;
    pub fn sprs_hip_dist_peer_connect(d: *mut sprs_hip_dist, handles: *const c_void, world: i32) -> i32;
    pub fn sprs_hip_dist_set_route(d: *mut sprs_hip_dist, route: i32) -> i32;
    pub fn sprs_hip_dist_route(d: *const sprs_hip_dist, route: *mut i32) -> i32;
    pub fn sprs_hip_dist_free(d: *mut sprs_hip_dist) -> i32;
    pub fn sprs_hip_csmat_mul_csmat(lhs: *const sprs_hip_csmat, rhs: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat) -> i32;
    pub fn sprs_hip_csvec_upload(
        out: *mut *mut sprs_hip_csvec, dim: u64, nnz: u64, indices: *const c_void, idx_bytes: i32, data: *const f64, validate: i32,
    ) -> i32;
    pub fn sprs_hip_csvec_wrap_device(
        out: *mut *mut sprs_hip_csvec, dim: u64, nnz: u64, dev_indices: *const c_void, idx_bytes: i32, dev_data: *const f64,
    ) -> i32;
    pub fn sprs_hip_csvec_info(v: *const sprs_hip_csvec, dim: *mut u64, nnz: *mut u64, idx_bytes: *mut i32) -> i32;
    pub fn sprs_hip_csvec_device_ptrs(v: *const sprs_hip_csvec, indices: *mut *const c_void, data: *mut *const f64) -> i32;
    pub fn sprs_hip_csvec_download(v: *const sprs_hip_csvec, indices: *mut c_void, data: *mut f64) -> i32;
    pub fn sprs_hip_csvec_free(v: *mut sprs_hip_csvec) -> i32;
    pub fn sprs_hip_csvec_scatter_f64(v: *const sprs_hip_csvec, out_dev: *mut f64, out_len: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_mul_csvec_f64(
        a: *const sprs_hip_csmat, v: *const sprs_hip_csvec, out: *mut *mut sprs_hip_csvec, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csvec_mul_csmat_f64(
        v: *const sprs_hip_csvec, b: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csvec, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_binop_f64(
        lhs: *const sprs_hip_csmat, rhs: *const sprs_hip_csmat, op: i32, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_add_csmat_f64(
        lhs: *const sprs_hip_csmat, rhs: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_sub_csmat_f64(
        lhs: *const sprs_hip_csmat, rhs: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_scale_f64(m: *const sprs_hip_csmat, alpha: f64, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_binop_f64(
        lhs: *const sprs_hip_csvec, rhs: *const sprs_hip_csvec, op: i32, out: *mut *mut sprs_hip_csvec, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csvec_dot_f64(v: *const sprs_hip_csvec, w: *const sprs_hip_csvec, out_host: *mut f64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_dot_dense_f64(v: *const sprs_hip_csvec, x_dev: *const f64, x_len: u64, out_host: *mut f64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_norm_f64(v: *const sprs_hip_csvec, kind: i32, p: f64, out_host: *mut f64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_unit_normalize_f64(v: *const sprs_hip_csvec, out: *mut *mut sprs_hip_csvec, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_nnz_index(
        v: *const sprs_hip_csvec, nq: u64, q_dev: *const u64, pos_dev: *mut u64, val_dev: *mut f64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_outer_view(m: *const sprs_hip_csmat, i: u64, out: *mut *mut sprs_hip_csvec, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_diag_f64(m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csvec, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_nnz_index(
        m: *const sprs_hip_csmat, nq: u64, rows_dev: *const u64, cols_dev: *const u64, pos_dev: *mut u64, val_dev: *mut f64,
        stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_to_inner_onehot_f64(m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_perm_upload(out: *mut *mut sprs_hip_perm, dim: u64, perm: *const c_void, idx_bytes: i32, validate: i32) -> i32;
    pub fn sprs_hip_perm_from_device(
        out: *mut *mut sprs_hip_perm, dim: u64, dev_perm: *const c_void, idx_bytes: i32, validate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_perm_identity(out: *mut *mut sprs_hip_perm, dim: u64, idx_bytes: i32) -> i32;
    pub fn sprs_hip_perm_info(p: *const sprs_hip_perm, dim: *mut u64, idx_bytes: *mut i32, identity_variant: *mut i32) -> i32;
    pub fn sprs_hip_perm_is_identity(p: *const sprs_hip_perm, flag: *mut i32, stream: *mut c_void) -> i32;
    pub fn sprs_hip_perm_device_ptrs(p: *const sprs_hip_perm, perm: *mut *const c_void, perm_inv: *mut *const c_void) -> i32;
    pub fn sprs_hip_perm_download(p: *const sprs_hip_perm, perm: *mut c_void, perm_inv: *mut c_void) -> i32;
    pub fn sprs_hip_perm_inv(p: *const sprs_hip_perm, out: *mut *mut sprs_hip_perm) -> i32;
    pub fn sprs_hip_perm_free(p: *mut sprs_hip_perm) -> i32;
    pub fn sprs_hip_perm_mul_vec_f64(p: *const sprs_hip_perm, x_dev: *const f64, y_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_transform_paq(
        m: *const sprs_hip_csmat, row_perm: *const sprs_hip_perm, col_perm: *const sprs_hip_perm, out: *mut *mut sprs_hip_csmat,
        stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_transform_papt(
        m: *const sprs_hip_csmat, p: *const sprs_hip_perm, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_check_structure(m: *const sprs_hip_csmat, info: *mut sprs_hip_structure_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csvec_check_structure(v: *const sprs_hip_csvec, info: *mut sprs_hip_structure_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_from_unsorted(
        m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat, info: *mut sprs_hip_structure_info, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csvec_from_unsorted(
        v: *const sprs_hip_csvec, out: *mut *mut sprs_hip_csvec, info: *mut sprs_hip_structure_info, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_is_symmetric(m: *const sprs_hip_csmat, flag: *mut i32, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_degrees(m: *const sprs_hip_csmat, out_dev: *mut u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_max_outer_nnz(m: *const sprs_hip_csmat, out: *mut u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_cuthill_mckee(
        m: *const sprs_hip_csmat, start: i32, reversed: i32, check_symmetric: i32, out: *mut *mut sprs_hip_ordering, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_ordering_info(o: *const sprs_hip_ordering, dim: *mut u64, n_parts: *mut u64, stats: *mut u64) -> i32;
    pub fn sprs_hip_ordering_perm(o: *const sprs_hip_ordering, out: *mut *mut sprs_hip_perm) -> i32;
    pub fn sprs_hip_ordering_parts(o: *const sprs_hip_ordering, parts: *mut u64) -> i32;
    pub fn sprs_hip_ordering_free(o: *mut sprs_hip_ordering) -> i32;
    pub fn sprs_hip_ldl_symbolic(
        m: *const sprs_hip_csmat, perm: *const sprs_hip_perm, check_symmetry: i32, out: *mut *mut sprs_hip_ldl_sym, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_ldl_symbolic_info(s: *const sprs_hip_ldl_sym, n: *mut u64, nnz: *mut u64, stats: *mut u64) -> i32;
    pub fn sprs_hip_ldl_symbolic_colptr(s: *const sprs_hip_ldl_sym, colptr: *mut u64) -> i32;
    pub fn sprs_hip_ldl_symbolic_parents(s: *const sprs_hip_ldl_sym, parents: *mut u64) -> i32;
    pub fn sprs_hip_ldl_symbolic_perm(s: *const sprs_hip_ldl_sym, out: *mut *mut sprs_hip_perm) -> i32;
    pub fn sprs_hip_ldl_symbolic_free(s: *mut sprs_hip_ldl_sym) -> i32;
    pub fn sprs_hip_ldl_factor_f64(
        s: *const sprs_hip_ldl_sym, m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_ldl_num, info: *mut sprs_hip_trisolve_info,
        stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_ldl_update_f64(f: *mut sprs_hip_ldl_num, m: *const sprs_hip_csmat, info: *mut sprs_hip_trisolve_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_ldl_solve_f64(f: *mut sprs_hip_ldl_num, b_dev: *const f64, x_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_ldl_d(f: *const sprs_hip_ldl_num, d_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_ldl_l(f: *const sprs_hip_ldl_num, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_ldl_numeric_free(f: *mut sprs_hip_ldl_num) -> i32;
    pub fn sprs_hip_ldl_lsolve_f64(l: *mut sprs_hip_csmat, x_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_ldl_ltsolve_f64(l: *mut sprs_hip_csmat, x_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_diag_solve_f64(d_dev: *const f64, x_dev: *mut f64, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_kronecker_f64(
        a: *const sprs_hip_csmat, b: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_same_storage_fast_stack(
        mats: *mut *const sprs_hip_csmat, n: u64, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_vstack(mats: *mut *const sprs_hip_csmat, n: u64, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_hstack(mats: *mut *const sprs_hip_csmat, n: u64, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_bmat(
        blocks: *mut *const sprs_hip_csmat, super_rows: u64, super_cols: u64, out: *mut *mut sprs_hip_csmat, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_from_dense_f64(
        out: *mut *mut sprs_hip_csmat, storage: i32, m_dev: *const f64, rows: u64, cols: u64, layout: i32, ld: u64, epsilon: f64,
        iptr_bytes: i32, idx_bytes: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_assign_to_dense_f64(
        m: *const sprs_hip_csmat, out_dev: *mut f64, rows: u64, cols: u64, layout: i32, ld: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_to_dense_f64(
        m: *const sprs_hip_csmat, out_dev: *mut f64, rows: u64, cols: u64, layout: i32, ld: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_binop_dense_f64(
        lhs: *const sprs_hip_csmat, rhs_dev: *const f64, rows: u64, cols: u64, layout: i32, ld: u64, op: i32, alpha: f64, beta: f64,
        out_dev: *mut f64, out_ld: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_add_dense_f64(
        lhs: *const sprs_hip_csmat, rhs_dev: *const f64, rows: u64, cols: u64, layout: i32, ld: u64, out_dev: *mut f64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_triplets_to_cs(
        rows: u64, cols: u64, n: u64, row_inds_dev: *const c_void, col_inds_dev: *const c_void, in_idx_bytes: i32,
        data_dev: *const f64, storage: i32, out_idx_bytes: i32, out_iptr_bytes: i32, out: *mut *mut sprs_hip_csmat,
    ) -> i32;
    // single precision: the f32 container, SpMV in both storages, BiCGSTAB, the casts to and from the f64 handle
    pub fn sprs_hip_csmat_f32_upload(
        out: *mut *mut sprs_hip_csmat_f32, storage: i32, rows: u64, cols: u64, indptr: *const c_void, iptr_bytes: i32,
        indices: *const c_void, idx_bytes: i32, data: *const f32, validate: i32,
    ) -> i32;
    pub fn sprs_hip_csmat_f32_wrap_device(
        out: *mut *mut sprs_hip_csmat_f32, storage: i32, rows: u64, cols: u64, nnz: u64, dev_indptr: *const c_void, iptr_bytes: i32,
        dev_indices: *const c_void, idx_bytes: i32, dev_data: *const f32,
    ) -> i32;
    pub fn sprs_hip_csmat_f32_info(
        m: *const sprs_hip_csmat_f32, rows: *mut u64, cols: *mut u64, nnz: *mut u64, iptr_bytes: *mut i32, idx_bytes: *mut i32,
        storage: *mut i32,
    ) -> i32;
    pub fn sprs_hip_csmat_f32_device_ptrs(
        m: *const sprs_hip_csmat_f32, indptr: *mut *const c_void, indices: *mut *const c_void, data: *mut *const f32,
    ) -> i32;
    pub fn sprs_hip_csmat_f32_download(m: *const sprs_hip_csmat_f32, indptr: *mut c_void, indices: *mut c_void, data: *mut f32) -> i32;
    pub fn sprs_hip_csmat_f32_transpose_view(m: *const sprs_hip_csmat_f32, out: *mut *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_csmat_f32_refresh(m: *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_csmat_f32_prepare(m: *mut sprs_hip_csmat_f32, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_f32_spmv_plan_info(m: *const sprs_hip_csmat_f32, kind: *mut i32, plan_bytes: *mut u64) -> i32;
    pub fn sprs_hip_csmat_f32_free(m: *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_csmat_f32_to_other_storage(m: *const sprs_hip_csmat_f32, out: *mut *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_csmat_f32_from_f64(m: *const sprs_hip_csmat, out: *mut *mut sprs_hip_csmat_f32, stream: *mut c_void) -> i32;
    pub fn sprs_hip_csmat_f32_to_f64(m: *const sprs_hip_csmat_f32, out: *mut *mut sprs_hip_csmat, stream: *mut c_void) -> i32;
    pub fn sprs_hip_spmv_f32(
        a: *const sprs_hip_csmat_f32, x_dev: *const f32, x_len: u64, y_dev: *mut f32, y_len: u64, accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_mul_acc_mat_vec_csc_f32(
        a: *const sprs_hip_csmat_f32, x_dev: *const f32, x_len: u64, y_dev: *mut f32, y_len: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mul_vec_f32(
        a: *const sprs_hip_csmat_f32, x_dev: *const f32, x_len: u64, y_dev: *mut f32, y_len: u64, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_bicgstab_f32(
        a: *mut sprs_hip_csmat_f32, x0_dev: *const f32, b_dev: *const f32, n: u64, tol: f64, max_iter: u64, soft_restart_threshold: f64,
        x_dev: *mut f32, info: *mut sprs_hip_bicgstab_info, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_trisolve_f32(a: *mut sprs_hip_csmat_f32, uplo: i32, x_dev: *mut f32, n: u64,
                                 info: *mut sprs_hip_trisolve_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_gauss_seidel_f32(a: *mut sprs_hip_csmat_f32, x_dev: *mut f32, rhs_dev: *const f32, n: u64, max_iter: u64,
                                     eps: f64, info: *mut sprs_hip_gauss_seidel_info, stream: *mut c_void) -> i32;
    pub fn sprs_hip_diag_solve_f32(d_dev: *const f32, x_dev: *mut f32, n: u64, stream: *mut c_void) -> i32;
    pub fn sprs_hip_spmm_rowmaj_f32(
        a: *const sprs_hip_csmat_f32, rhs_dev: *const f32, rhs_rows: u64, k: u64, ld_rhs: u64,
        out_dev: *mut f32, out_rows: u64, ld_out: u64, accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mulacc_dense_f32(
        lhs: *const sprs_hip_csmat_f32, rhs_dev: *const f32, rhs_rows: u64, k: u64, rhs_layout: i32, ld_rhs: u64,
        out_dev: *mut f32, out_rows: u64, out_layout: i32, ld_out: u64, accumulate: i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_csmat_mul_dense_f32(
        lhs: *const sprs_hip_csmat_f32, rhs_dev: *const f32, rhs_rows: u64, k: u64, rhs_layout: i32, ld_rhs: u64,
        out_dev: *mut f32, out_layout: *mut i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_dense_dot_csmat_f32(
        lhs_dev: *const f32, lhs_rows: u64, lhs_cols: u64, lhs_layout: i32, ld_lhs: u64, rhs: *const sprs_hip_csmat_f32,
        out_dev: *mut f32, out_layout: *mut i32, stream: *mut c_void,
    ) -> i32;
    pub fn sprs_hip_spgemm_f32(a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c: *mut *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_spgemm_symbolic_f32(a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c_structure: *mut *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_spgemm_numeric_f32(a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c: *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_spgemm_plan_create_f32(a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, plan: *mut *mut sprs_hip_spgemm_plan) -> i32;
    pub fn sprs_hip_spgemm_plan_structure_f32(
        plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c_structure: *mut *mut sprs_hip_csmat_f32,
    ) -> i32;
    pub fn sprs_hip_spgemm_plan_product_f32(
        plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c: *mut *mut sprs_hip_csmat_f32,
    ) -> i32;
    pub fn sprs_hip_spgemm_plan_numeric_f32(
        plan: *mut sprs_hip_spgemm_plan, a: *const sprs_hip_csmat_f32, b: *const sprs_hip_csmat_f32, c: *mut sprs_hip_csmat_f32,
    ) -> i32;
    pub fn sprs_hip_csmat_mul_csmat_f32(lhs: *const sprs_hip_csmat_f32, rhs: *const sprs_hip_csmat_f32, out: *mut *mut sprs_hip_csmat_f32) -> i32;
    pub fn sprs_hip_set_option(name: *const c_char, value: i64) -> i32;
    pub fn sprs_hip_get_option(name: *const c_char, value: *mut i64) -> i32;
}
