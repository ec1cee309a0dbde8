/*
 * sprs_hip.h — C ABI of libsprs_hip.so, the MI355X (gfx950) backend for the
 * sprs CSR SpMV / SpGEMM hot path.
 *
 * This is the boundary a `sprs-hip-sys` Rust crate binds (rust/sprs-hip-sys,
 * following the reference's own *_sys + safe-wrapper split,
 * suitesparse_bindings/suitesparse_ldl_sys/src/lib.rs:10-80 and
 * sprs_suitesparse_ldl/src/lib.rs:53-129).  Conventions, all taken from how
 * the reference already crosses a C ABI:
 *   - CSR is passed as (rows, cols, indptr*, indices*, data*) raw pointers
 *     (sprs-benches/src/main.rs:28-41  <->  sprs-benches/src/eigen.cpp:6-29);
 *   - index widths are given in bytes: 8 = usize/u64/i64/isize (sprs default,
 *     sprs/src/sparse.rs:111-122), 4 = u32/i32 (sprs/src/indexing.rs:124-130);
 *   - matrices are opaque handles freed by an explicit call, owned on the
 *     Rust side by a struct with Drop (sprs_suitesparse_umfpack/src/lib.rs:30-46);
 *   - every entry point returns a status; nothing unwinds across the boundary.
 *     Status codes map 1:1 onto the reference's panics / errors so the wrapper
 *     can re-raise them with the same text (see each code).
 *
 * All citations are relative to the sprs repository root.
 * No torch / C++ types appear here: plain pointers and sizes only.
 */
#ifndef SPRS_HIP_H
#define SPRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ----------------------------------------------------------- */

#define SPRS_HIP_OK 0
/* assert "Dimension mismatch": prod.rs:114-117, prod.rs:283-285; assert_eq!(lhs.cols(), rhs.rows()) smmp.rs:207 */
#define SPRS_HIP_DIM_MISMATCH 1
/* assert "Storage mismatch": prod.rs:118, prod.rs:286 */
#define SPRS_HIP_STORAGE_MISMATCH 2
/* panic "Index type is not large enough to hold ...": csmat.rs:1794-1797; I::from_usize / Iptr::from_usize smmp.rs:116,121 */
#define SPRS_HIP_INDEX_OVERFLOW 3
/* StructureError::{Unsorted,SizeMismatch,OutOfRange}: errors.rs:4-8, sparse.rs:300-358 */
#define SPRS_HIP_BAD_STRUCTURE 4
/* null pointer / unsupported width / misaligned device buffer */
#define SPRS_HIP_INVALID_ARG 5
/* hipMalloc failed */
#define SPRS_HIP_OUT_OF_MEMORY 6
/* any other HIP runtime error -> LinalgError::ThirdPartyError(code, msg), errors.rs:70,94-96 */
#define SPRS_HIP_HIP_ERROR 7
/* no usable gfx950 device: the product path never falls back to the CPU */
#define SPRS_HIP_NO_DEVICE 8
/* LinalgError::SingularMatrix(SingularMatrixInfo { index, reason }), errors.rs:59-92: the triangular solves.
 * sprs_hip_last_error() carries the reference's text, "Singular matrix at index {} ({reason})" */
#define SPRS_HIP_SINGULAR_MATRIX 9

/* CompressedStorage, sprs/src/sparse.rs:30-40 */
#define SPRS_HIP_CSR 0
#define SPRS_HIP_CSC 1
/* which triangle sprs_hip_trisolve_f64 solves with: lsolve_* or usolve_* (sprs/src/sparse/linalg/trisolve.rs) */
#define SPRS_HIP_LOWER 0
#define SPRS_HIP_UPPER 1
/* dense operands: C order (ndarray's standard layout) or Fortran order (`.f()`), with a leading dimension */
#define SPRS_HIP_ROW_MAJOR 0
#define SPRS_HIP_COL_MAJOR 1

/* Thread-local text of the last failure on the calling thread ("" if none),
 * and the raw hipError_t behind a SPRS_HIP_HIP_ERROR (0 otherwise). */
const char *sprs_hip_last_error(void);
int32_t sprs_hip_last_hip_code(void);
/* "sprs_hip <version> gfx950 ..." */
const char *sprs_hip_version(void);

/* ---- device / raw buffers (DeviceVec plumbing) ------------------------- */

int32_t sprs_hip_device_count(int32_t *count);
int32_t sprs_hip_set_device(int32_t device);
int32_t sprs_hip_malloc(void **dev_ptr, uint64_t bytes);
int32_t sprs_hip_free(void *dev_ptr);
int32_t sprs_hip_memcpy_h2d(void *dev_dst, const void *host_src, uint64_t bytes);
int32_t sprs_hip_memcpy_d2h(void *host_dst, const void *dev_src, uint64_t bytes);
int32_t sprs_hip_memcpy_d2d(void *dev_dst, const void *dev_src, uint64_t bytes, void *stream);
int32_t sprs_hip_memset(void *dev_dst, int32_t byte_value, uint64_t bytes, void *stream);
int32_t sprs_hip_synchronize(void *stream); /* NULL = whole device */
/* Result matrices (sprs_hip_spgemm_f64, sprs_hip_csmat_to_other_storage, uploads) take their index/value
 * blocks from a pool of previously released ones and return them there on sprs_hip_csmat_free (options
 * "pool" = 1, "pool_max_bytes"): the driver needs seconds to re-issue tens of GB that were just freed.
 * sprs_hip_pool_trim hands everything cached back to the driver (Rust analogue: dropping the CsMat really
 * frees — call this where that matters, e.g. before another library needs the memory). */
int32_t sprs_hip_pool_trim(uint64_t *freed_bytes /* may be NULL */);

/* ---- device CSR/CSC container: twin of CsMatBase (sparse.rs:94-122) ---- */

typedef struct sprs_hip_csmat sprs_hip_csmat;

/* Copies a host matrix into device buffers OWNED by the handle (the host
 * arrays stay the caller's).  `indptr` has outer+1 entries and may be
 * non-zero-based, as slice_outer views are (indptr.rs:118-124, 216-219):
 * `indices`/`data` then point at the element addressed by indptr[0], and the
 * device copy is rebased (to_proper, indptr.rs:206-214).
 * validate != 0 runs check_compressed_structure (sparse.rs:300-358) first and
 * returns SPRS_HIP_BAD_STRUCTURE where CsMat::new would panic; validate == 0
 * is new_trusted / new_unchecked (csmat.rs:265-301). */
/* Index widths: 4 or 8 bytes on the device.  Host arrays may also be 2 bytes wide (sprs' u16 / i16, indexing.rs:124-130):
 * they are widened to 4 bytes on upload, sprs_hip_csmat_info keeps reporting 2, downloads narrow again, and every
 * result derived from such a matrix is checked against the 2-byte range where the reference's I::from_usize /
 * Iptr::from_usize would panic (SPRS_HIP_INDEX_OVERFLOW; sprs/tests/gh374.rs is reproduced literally). */
int32_t sprs_hip_csmat_upload(sprs_hip_csmat **out, int32_t storage, uint64_t rows, uint64_t cols,
                              const void *indptr, int32_t iptr_bytes, const void *indices,
                              int32_t idx_bytes, const double *data, int32_t validate);

/* Wraps buffers that already live on the current device (NOT owned, must
 * outlive the handle; zero-based indptr; 16-byte aligned). */
int32_t sprs_hip_csmat_wrap_device(sprs_hip_csmat **out, int32_t storage, uint64_t rows,
                                   uint64_t cols, uint64_t nnz, const void *dev_indptr,
                                   int32_t iptr_bytes, const void *dev_indices, int32_t idx_bytes,
                                   const double *dev_data);

/* shape / nnz / widths / storage; any out pointer may be NULL */
int32_t sprs_hip_csmat_info(const sprs_hip_csmat *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz,
                            int32_t *iptr_bytes, int32_t *idx_bytes, int32_t *storage);
/* raw device pointers (into_raw_storage, csmat.rs:946-954), still owned by the handle */
int32_t sprs_hip_csmat_device_ptrs(const sprs_hip_csmat *m, const void **indptr,
                                   const void **indices, const double **data);
/* whole matrix to host buffers of outer+1 / nnz / nnz entries */
int32_t sprs_hip_csmat_download(const sprs_hip_csmat *m, void *indptr, void *indices, double *data);
/* outer slices [start, end) only — slice_outer (slicing.rs:65-89).  indptr_out
 * gets end-start+1 NON-rebased entries (as the reference's view does);
 * indices_out/data_out get indptr[end]-indptr[start] entries.  Either may be
 * NULL to query sizes through *nnz_out. */
int32_t sprs_hip_csmat_download_outer(const sprs_hip_csmat *m, uint64_t start, uint64_t end,
                                      void *indptr_out, void *indices_out, double *data_out,
                                      uint64_t *nnz_out);
/* slice_outer (slicing.rs:65-89) as a NEW owning handle: outer slices [start, end), indptr
 * rebased (to_proper, indptr.rs:206-214).  The reference's view is zero-copy; the device twin
 * materialises the slice (one D2D copy) so that it is a self-contained, 16-byte aligned matrix —
 * this is how the multi-GPU path cuts row blocks. */
int32_t sprs_hip_csmat_slice_outer(const sprs_hip_csmat *m, uint64_t start, uint64_t end,
                                   sprs_hip_csmat **out);
/* Handles are immutable snapshots, like a `&CsMat`: the multiply plans cached inside a handle
 * (tile index, XCD-sliced copy, SpMM chunks) are derived from its arrays on first use.  After
 * modifying the arrays of a WRAPPED handle in place (sprs_hip_csmat_wrap_device), call this to drop
 * the cached plans; they are rebuilt by the next multiply. */
int32_t sprs_hip_csmat_refresh(sprs_hip_csmat *m);
/* PLAN POLICY.  A handle's FIRST SpMV runs on the plain tile index over its own arrays (built in microseconds); the plans
 * that re-lay the matrix out — the banded copy with the hot columns served from LDS, the XCD-sliced copy: ~0.1 s to build
 * for a 3e8-entry matrix, i.e. about 80 SpMVs, and 0.7 x the matrix in extra HBM — are built by the SECOND SpMV of the
 * handle, so a handle that multiplies once (`&a * &x` on a temporary) never pays for them.  A caller that knows it will
 * iterate (a solver) calls this once after the upload: the full plan is built now, on `stream`, and the first SpMV already
 * runs at the steady-state rate.  Idempotent; option spmv_plan_defer = 0 brings back "build at the first multiply".
 * What a caller that does NOT prepare must know: (i) multiply #1 and multiply #2 of one handle run on different plans and so
 * add the products of a row in different (each deterministic) orders — both within 1e-10 of the reference, but not
 * bit-identical to each other; from multiply #2 on every result has the same bits.  A solver whose first iteration must
 * reproduce later ones prepares the handle.  (ii) Multiply #2 allocates, builds and synchronises (the plan build): it must
 * not sit inside a timed or a CAPTURED region — an SpMV on a stream that is being captured into a hipGraph fails with
 * SPRS_HIP_INVALID_ARG unless the handle's final plan already exists.  The flag and the multiply count belong to the handle the
 * caller holds: a CSC handle hands them to its cached CSR copy, also to the one rebuilt after sprs_hip_csmat_refresh.
 * No counterpart in the reference (its CsMat has no derived state). */
int32_t sprs_hip_csmat_prepare(sprs_hip_csmat *m, void *stream);
/* What the SpMV plan cached in the handle looks like (after the first multiply; kind 0 before):
 * kind 1 = nnz tiles over the handle's own arrays, 2 = XCD-sliced copy (spmv.hip), 3 = banded copy
 * with the hot columns served from LDS (spmv_band.hip); plan_bytes = HBM the plan holds besides the
 * handle's arrays.  No counterpart in the reference (its CsMat has no derived state). */
int32_t sprs_hip_csmat_spmv_plan_info(const sprs_hip_csmat *m, int32_t *kind, uint64_t *plan_bytes);
/* transpose_view (csmat.rs:982-991): free, shares the buffers, flips storage + shape */
int32_t sprs_hip_csmat_transpose_view(const sprs_hip_csmat *m, sprs_hip_csmat **out);
int32_t sprs_hip_csmat_free(sprs_hip_csmat *m);

/* ---- SpMV --------------------------------------------------------------- */

/* Twin of prod::mul_acc_mat_vec_csr (prod.rs:103-127) when accumulate != 0:
 *     y[i] += sum_k A[i,k] * x[k]      (y keeps its previous content),
 * and of `&A * &x` (csmat.rs:2119-2160 -> prod::csr_mulacc_dense_colmaj,
 * prod.rs:274-298) when accumulate == 0:  y[i] = sum_k A[i,k] * x[k].
 * x_dev / y_dev are device pointers of x_len / y_len doubles.
 * SPRS_HIP_DIM_MISMATCH unless A.cols == x_len && A.rows == y_len;
 * SPRS_HIP_STORAGE_MISMATCH unless A is CSR.  Asynchronous on `stream`
 * (hipStream_t; NULL = default stream).  Products are formed with a separately
 * rounded multiply and add like MulAcc (mul_acc.rs:28-30); only the summation
 * ORDER inside a row differs from the reference (tree instead of left-to-right),
 * and it is run-to-run deterministic. */
int32_t sprs_hip_spmv_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len,
                          double *y_dev, uint64_t y_len, int32_t accumulate, void *stream);

/* One-shot host form (upload, multiply, download, synchronous): what a plain
 * `prod::mul_acc_mat_vec_csr(mat.view(), &x[..], &mut y[..])` call maps to.  The handle lives for one multiply, so it
 * runs on the plain nnz-tiled plan: no re-laid-out copy of the matrix is built (the banded plan of a kept handle takes
 * ~0.1 s to build on a 3e8-entry matrix for a 1 ms SpMV). */
int32_t sprs_hip_spmv_f64_host(uint64_t rows, uint64_t cols, const void *indptr,
                               int32_t iptr_bytes, const void *indices, int32_t idx_bytes,
                               const double *data, const double *x, uint64_t x_len, double *y,
                               uint64_t y_len, int32_t accumulate);

/* ---- SpMM: CSR x dense row-major ------------------------------------------ */

/* Twin of prod::csr_mulacc_dense_rowmaj (prod.rs:189-214), the kernel `&CsMat * &Array2` uses for
 * a rhs of >= 8 columns (csmat.rs:2002-2016):  out[i, :] += A[i, c] * rhs[c, :]  over the stored
 * entries of row i (accumulate != 0), or the same on a zeroed `out` (accumulate == 0).
 * rhs_dev: rhs_rows x k doubles, row-major, leading dimension ld_rhs (>= k); out_dev: out_rows x k,
 * leading dimension ld_out.  SPRS_HIP_DIM_MISMATCH unless A.cols == rhs_rows && A.rows == out_rows;
 * SPRS_HIP_STORAGE_MISMATCH unless A is CSR.  Asynchronous on `stream`; deterministic. */
int32_t sprs_hip_spmm_rowmaj_f64(const sprs_hip_csmat *a, const double *rhs_dev, uint64_t rhs_rows,
                                 uint64_t k, uint64_t ld_rhs, double *out_dev, uint64_t out_rows,
                                 uint64_t ld_out, int32_t accumulate, void *stream);

/* ---- products with dense operands: the operator dispatch below the ABI --------------------------- */

/* Twin of prod::mul_acc_mat_vec_csc (prod.rs:74-99): y += A x for a CSC matrix.  SPRS_HIP_DIM_MISMATCH unless
 * A.cols == x_len && A.rows == y_len, then SPRS_HIP_STORAGE_MISMATCH unless A is CSC (prod.rs:88-92).  The reference scatters
 * column by column; here the matrix is converted ONCE to CSR on the device (to_other_storage, csmat.rs:1405-1426), the copy is
 * cached in the handle (dropped by sprs_hip_csmat_refresh / _free) and the CSR kernels run on it: every y[i] still receives
 * its products by ascending column. */
int32_t sprs_hip_mul_acc_mat_vec_csc_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len, double *y_dev,
                                         uint64_t y_len, void *stream);

/* Twin of `&CsMat * &Array1` and its Dot (csmat.rs:2119-2178): y = A x on a zeroed result for EITHER storage —
 * CSR -> csr_mulacc_dense_colmaj, CSC -> csc_mulacc_dense_colmaj with one column (csmat.rs:2140-2156), the latter on the cached
 * CSR form.  SPRS_HIP_DIM_MISMATCH as the kernels' asserts (prod.rs:257-259, 284-289). */
int32_t sprs_hip_csmat_mul_vec_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len, double *y_dev,
                                   uint64_t y_len, void *stream);

/* The four dense kernels of prod.rs in one entry: csr_mulacc_dense_rowmaj / _colmaj (prod.rs:189-214, 274-298) and
 * csc_mulacc_dense_rowmaj / _colmaj (prod.rs:219-270):  out += lhs * rhs  (accumulate != 0) or  out = lhs * rhs  on a zeroed
 * out (accumulate == 0), lhs in either storage (CSC through the cached CSR form), rhs (rhs_rows x k) and out (out_rows x k)
 * each in the layout its tag names with leading dimension ld (row-major: >= k, column-major: >= rows).  The reference's four
 * functions differ in the loop order only (every out[i, j] receives its products by ascending column index in all of them);
 * the layouts tell this entry how to address the operands.  Column-major x column-major with k < 8 — what `&CsMat * &Array2`
 * makes for fewer than 8 columns — runs column by column through the SpMV.  SPRS_HIP_DIM_MISMATCH unless lhs.cols == rhs_rows
 * && lhs.rows == out_rows (prod.rs:199-201, 228-230, 257-259, 284-289). */
int32_t sprs_hip_csmat_mulacc_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                        int32_t rhs_layout, uint64_t ld_rhs, double *out_dev, uint64_t out_rows,
                                        int32_t out_layout, uint64_t ld_out, int32_t accumulate, void *stream);

/* Twin of `&CsMat * &Array2` / `CsMat::dot(&Array2)` (csmat.rs:1989-2048, 2119-2137): the four arms (CSR | CSC) x (>= 8 columns |
 * fewer).  out_dev: lhs.rows x k doubles, contiguous; written in the layout the reference allocates — row-major for k >= 8,
 * column-major (`.f()`) below — which *out_layout reports. */
int32_t sprs_hip_csmat_mul_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                     int32_t rhs_layout, uint64_t ld_rhs, double *out_dev, int32_t *out_layout, void *stream);

/* Twin of `Array2::dot(&CsMat)` (csmat.rs:2050-2117): lhs (lhs_rows x lhs_cols, dense) . rhs (sparse) as (rhs^T lhs^T)^T with
 * the reference's free transposes (transpose_view, .t(), reversed_axes).  out_dev: lhs_rows x rhs.cols doubles, contiguous, in
 * the layout *out_layout reports (the reversed axes of what the transposed product allocates).  Synchronous (the transposed
 * operand is a temporary view).  A CSR rhs is converted once to CSC (cached in the handle). */
int32_t sprs_hip_dense_dot_csmat_f64(const double *lhs_dev, uint64_t lhs_rows, uint64_t lhs_cols, int32_t lhs_layout,
                                     uint64_t ld_lhs, const sprs_hip_csmat *rhs, double *out_dev, int32_t *out_layout,
                                     void *stream);

/* ---- BiCGSTAB: a caller that loops on the SpMV -------------- */

/* Counters and scalars of sprs::linalg::bicgstab::BiCGSTAB after solve()
 * (iteration_count / soft_restart_count / hard_restart_count / err / rho,
 * bicgstab.rs:236-262); converged = solve() returned Ok rather than Err. */
typedef struct sprs_hip_bicgstab_info {
    uint64_t iteration_count;
    uint64_t soft_restart_count;
    uint64_t hard_restart_count;
    double err;
    double rho;
    int32_t converged;
} sprs_hip_bicgstab_info;

/* Twin of BiCGSTAB::solve(a, x0, b, tol, max_iter) (bicgstab.rs:148-171) with device-resident dense
 * vectors: solves A x = b from the start vector x0, unpreconditioned, with the reference's soft restart
 * (|rho| / err^2 < soft_restart_threshold; the reference's default is 0.1, with_restart_threshold) and
 * hard restart (true residual recomputed before convergence is claimed).  A: square CSR or CSC handle
 * (a CSC operand is converted once on the device).  x0_dev, b_dev, x_dev: n doubles each; x_dev may not
 * alias x0_dev / b_dev.  Like the reference, running out of iterations is not an error: the status is
 * SPRS_HIP_OK, info->converged is 0 and x_dev holds the last iterate.  SPRS_HIP_DIM_MISMATCH unless
 * A.rows == A.cols == n.  Blocks until done (the restart decisions need the scalars on the host).
 * Element-wise arithmetic is bit-identical to the reference's; dot products are serial (== reference)
 * for n <= 2048 — the reference's own 4 x 4 test system reproduces bit for bit — and a fixed two-level
 * tree above; the SpMVs are sprs_hip_spmv_f64.  Deterministic run to run. */
int32_t sprs_hip_bicgstab_f64(sprs_hip_csmat *a, const double *x0_dev, const double *b_dev, uint64_t n,
                              double tol, uint64_t max_iter, double soft_restart_threshold, double *x_dev,
                              sprs_hip_bicgstab_info *info, void *stream);

/* ---- Gauss-Seidel: the other caller that loops on the SpMV -- */

/* What gauss_seidel() of the reference's heat example returns (sprs/examples/heat.rs:103-139):
 * Ok((it, error)) -> converged = 1, iterations = it (index of the sweep after which error < eps);
 * Err(error)      -> converged = 0, iterations = max_iter.  levels = length of the longest chain of
 * rows that must be swept one after the other (what bounds a sweep on the device). */
typedef struct sprs_hip_gauss_seidel_info {
    uint64_t iterations;
    double error;
    int32_t converged;
    uint64_t levels;
} sprs_hip_gauss_seidel_info;

/* Twin of gauss_seidel(mat, x, rhs, max_iter, eps) (heat.rs:103-139) with device-resident vectors:
 * up to max_iter sweeps  x[row] = (rhs[row] - sum_{col != row} val * x[col]) / diag  over the rows in
 * order, x updated IN PLACE (x_dev is the start vector and the result), each followed by the
 * reference's convergence test  error = sqrt(sum_i ((A x)_i - rhs_i)) < eps  (the SIGNED sum of the
 * residual, as the reference has it: a negative sum gives NaN and the sweeps go on).  A sweep is a
 * recurrence over the rows; on the device the rows run in dependency-level order (computed once per
 * handle) and a row reads this sweep's value of an earlier row as soon as that row has published
 * it, so every x[row] is computed from the same operands in the same order as on the CPU: the
 * iterates are bit-identical to the reference's.  `error` is A x by sprs_hip_spmv_f64 and a fixed
 * tree sum (ndarray's eight-accumulator sum rounds differently: equal to ~1e-13 of sum |r_i|).
 * A: square CSR handle with fewer than 2^32 rows (SPRS_HIP_STORAGE_MISMATCH for CSC: the reference's
 * outer_iterator would sweep the transpose); x_dev, rhs_dev: n doubles, not aliased.
 * SPRS_HIP_DIM_MISMATCH unless A.rows == A.cols == n (heat.rs:109-110); SPRS_HIP_BAD_STRUCTURE for a
 * row without a stored diagonal entry when a sweep would reach it (`diag.unwrap()`, heat.rs:127).
 * Running out of sweeps is not an error (Err(error) in the reference): status OK, converged = 0.
 * Blocks until done (the convergence test needs `error` on the host).  Deterministic. */
int32_t sprs_hip_gauss_seidel_f64(sprs_hip_csmat *a, double *x_dev, const double *rhs_dev, uint64_t n,
                                  uint64_t max_iter, double eps, sprs_hip_gauss_seidel_info *info,
                                  void *stream);

/* ---- sparse triangular solves (sprs::linalg::trisolve) --------------------- */

/* levels = length of the longest chain of unknowns that must be solved one after the other (what bounds a solve on
 * the device).  After SPRS_HIP_SINGULAR_MATRIX: singular_index = the index the reference reports, singular_reason =
 * 1 "a numeric 0" (a stored diagonal == 0; also a CSR diagonal that is not stored, which the CSR functions do not
 * tell apart) or 2 "a structural 0" (CSC only: the diagonal is not stored).  Otherwise UINT64_MAX and 0. */
typedef struct sprs_hip_trisolve_info {
    uint64_t levels;
    uint64_t singular_index;
    int32_t singular_reason;
} sprs_hip_trisolve_info;

/* Twins of the four dense-rhs solves of sprs/src/sparse/linalg/trisolve.rs, in place on the n doubles of x_dev (the
 * right-hand side on entry, the solution on return).  The handle's storage selects the CSR or the CSC function, uplo
 * lsolve (SPRS_HIP_LOWER) or usolve (SPRS_HIP_UPPER):
 *
 *   solve        order of unknowns   subtractions into unknown r, in this order          singular when
 *   lsolve_csr   0 .. n-1            stored entries of row r with c < r, stored order    diagonal not stored or == 0
 *                (trisolve.rs:30-73)                                                      ("diagonal element is 0")
 *   usolve_csr   n-1 .. 0            stored entries of row r with c > r, stored order    the same ("diagonal element is a
 *                (trisolve.rs:219-262)                                                    numeric 0")
 *   lsolve_csc   0 .. n-1            entries (r, c) with c < r, ascending c              not stored: "a structural 0";
 *                (trisolve.rs:85-149)                                                     stored and == 0: "a numeric 0"
 *   usolve_csc   n-1 .. 0            entries (r, c) with c > r, DESCENDING c             as lsolve_csc
 *                (trisolve.rs:161-210)
 *
 * The matrix need not be triangular: the other triangle is skipped.  Every update is x -= val * x[c] with a rounded
 * multiply and a rounded subtract, the last step one IEEE division by the diagonal: the solution is bit-identical to
 * the reference's (usolve_csr and usolve_csc differ in bits from each other, as they do there).  -0.0 on the diagonal
 * counts as zero, NaN does not.  On the device the unknowns run in dependency-level order (computed once per handle
 * and triangle; the lower order is the Gauss-Seidel one) and a row reads an earlier unknown as soon as it has been
 * published.  A CSC handle is solved on its cached CSR form; a transpose view of a CSR factor L is a CSC handle, so
 * L^T x = b needs no copy of the caller's making.
 * Indices must be sorted inside each outer slice, as every validated handle has them: an unvalidated unsorted handle
 * gets no promise about the result.
 * SPRS_HIP_DIM_MISMATCH unless A.rows == A.cols ("Non square matrix passed to solver") == n ("Dimension mismatch")
 * (check_solver_dimensions, trisolve.rs:10-21); SPRS_HIP_INVALID_ARG for a NULL handle or vector, another uplo, or
 * n >= 2^32; n == 0 is OK with no work.
 * SPRS_HIP_SINGULAR_MATRIX where the reference returns Err(SingularMatrix): the index is the first singular one in
 * the reference's processing order (the smallest for SPRS_HIP_LOWER, the largest for SPRS_HIP_UPPER); the contents of
 * x_dev are unspecified then.
 * Blocks until done (the singular report needs a read-back); runs its work on `stream`.  Deterministic. */
int32_t sprs_hip_trisolve_f64(sprs_hip_csmat *a, int32_t uplo, double *x_dev, uint64_t n,
                              sprs_hip_trisolve_info *info, void *stream);

/* ---- SpGEMM ------------------------------------------------------------- */

/* Twin of smmp::mul_csr_csr (smmp.rs:196-416): C = A * B, all CSR, same index
 * types as the operands (smmp.rs:196-199).  Returns a NEW owning handle:
 * shape (A.rows, B.cols), zero-based indptr, every row strictly increasing
 * (sort_unstable, smmp.rs:126), structural zeros kept (no value test,
 * smmp.rs:109-119).  SPRS_HIP_DIM_MISMATCH unless A.cols == B.rows;
 * SPRS_HIP_STORAGE_MISMATCH unless both are CSR and share index widths;
 * SPRS_HIP_INDEX_OVERFLOW if nnz(C) does not fit Iptr.  Synchronous. */
int32_t sprs_hip_spgemm_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **c);

/* The two halves of smmp::mul_csr_csr as the reference exposes them:
 * sprs_hip_spgemm_symbolic — twin of smmp::symbolic (smmp.rs:81-131): the STRUCTURE of C = A * B (indptr and
 *   the sorted indices of every row, structural zeros kept) as a new handle whose values are 0.0;
 * sprs_hip_spgemm_numeric  — twin of smmp::numeric (smmp.rs:151-189): the VALUES of the product into `c`,
 *   which must have the product's structure (what _symbolic returned, for these or any operands with the same
 *   patterns — the re-use the reference's split exists for).  Unlike the reference, a `c` with another
 *   structure is detected: SPRS_HIP_BAD_STRUCTURE (nnz or indptr differ).  Same contract checks and
 *   status codes as sprs_hip_spgemm_f64; c's shape / storage / index types are checked like numeric()'s asserts
 *   (smmp.rs:161-166).  Both block until done. */
int32_t sprs_hip_spgemm_symbolic(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **c_structure);
int32_t sprs_hip_spgemm_numeric(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat *c);

/* The same split with the symbolic work KEPT, as the reference's callers keep (indptr, indices) between symbolic and
 * numeric (smmp.rs:81-131 -> 151-189; sprs-benches/src/main.rs:211-260 re-multiplies the same operands):
 *   sprs_hip_spgemm_plan_create     the symbolic phase for (a, b): per-row product counts, how the rows are cut into
 *                                   tasks, the exact output counts, their prefix sum = C.indptr, nnz(C)
 *   sprs_hip_spgemm_plan_nnz        nnz of the product
 *   sprs_hip_spgemm_plan_structure  C with indptr + sorted indices, values 0.0            (what smmp::symbolic returns)
 *   sprs_hip_spgemm_plan_product    C complete: structure and values in one numeric pass  (== sprs_hip_spgemm_f64)
 *   sprs_hip_spgemm_plan_numeric    the VALUES into a c of the product's structure (shape, nnz, indptr checked ->
 *                                   SPRS_HIP_BAD_STRUCTURE; c's indices are not touched): only the value kernels run
 * a and b must be the handles (same structure buffers) the plan was made for, else SPRS_HIP_INVALID_ARG; their VALUES
 * may have changed in place in between.  All of these block until done. */
typedef struct sprs_hip_spgemm_plan sprs_hip_spgemm_plan;
int32_t sprs_hip_spgemm_plan_create(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_spgemm_plan **plan);
int32_t sprs_hip_spgemm_plan_nnz(const sprs_hip_spgemm_plan *plan, uint64_t *nnz);
int32_t sprs_hip_spgemm_plan_structure(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                       sprs_hip_csmat **c_structure);
int32_t sprs_hip_spgemm_plan_product(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                     sprs_hip_csmat **c);
int32_t sprs_hip_spgemm_plan_numeric(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                     sprs_hip_csmat *c);
int32_t sprs_hip_spgemm_plan_free(sprs_hip_spgemm_plan *plan);

/* Storage conversion raw::convert_mat_storage / to_other_storage
 * (csmat.rs:1405-1426, 1782-1829): new owning handle with the other storage
 * order.  SPRS_HIP_INDEX_OVERFLOW where the reference panics (csmat.rs:1794). */
int32_t sprs_hip_csmat_to_other_storage(const sprs_hip_csmat *m, sprs_hip_csmat **out);

/* `&lhs * &rhs` for two sparse matrices: csmat_mul_csmat (csmat.rs:1895-1949), the storage dispatch around
 * smmp::mul_csr_csr — (CSR,CSR) multiplies directly, (CSR,CSC) converts the rhs, (CSC,*) multiplies the transpose
 * views the other way round and transposes back; the result has the storage of the lhs.  This is what the `Mul` impls
 * of the host mirrors call.  Status codes as sprs_hip_spgemm_f64 and sprs_hip_csmat_to_other_storage. */
int32_t sprs_hip_csmat_mul_csmat(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out);

/* ---- device sparse vector: twin of CsVecBase (sparse.rs:165-173) and its products with sparse matrices ---- */

typedef struct sprs_hip_csvec sprs_hip_csvec;

/* Copies a host sparse vector (dim, nnz sorted indices of idx_bytes = 2, 4 or 8 each, nnz values) into device buffers OWNED
 * by the handle.  validate != 0 checks the invariants of CsVec::try_new (vec.rs:440-491, sorted_indices sparse.rs:360-369) —
 * on the host for small vectors, on the device for large ones — in the reference's order:
 *   dim does not fit the index width        SPRS_HIP_INDEX_OVERFLOW  "Index size is too small"
 *   indices not strictly increasing         SPRS_HIP_BAD_STRUCTURE   "Unsorted indices"
 *   last index >= dim                       SPRS_HIP_BAD_STRUCTURE   "indices larger than vector size"
 * (indices and data of unequal lengths — "indices and data do not have compatible lengths" — cannot reach this entry: it takes
 * one nnz.)  validate == 0 is new_trusted.  2-byte indices are widened to 4 on the device and narrowed on download. */
int32_t sprs_hip_csvec_upload(sprs_hip_csvec **out, uint64_t dim, uint64_t nnz, const void *indices, int32_t idx_bytes,
                              const double *data, int32_t validate);
/* Borrows device buffers (torch tensors, ...): NOT owned, must outlive the handle; idx_bytes 4 or 8; not validated
 * (new_trusted); the products never write outside their own tables whatever the indices hold. */
int32_t sprs_hip_csvec_wrap_device(sprs_hip_csvec **out, uint64_t dim, uint64_t nnz, const void *dev_indices, int32_t idx_bytes,
                                   const double *dev_data);
/* dim (vec.rs:681), nnz (vec.rs:686) and the declared index width; any out pointer may be NULL */
int32_t sprs_hip_csvec_info(const sprs_hip_csvec *v, uint64_t *dim, uint64_t *nnz, int32_t *idx_bytes);
/* raw device pointers (into_raw_storage, vec.rs:675), still owned by the handle */
int32_t sprs_hip_csvec_device_ptrs(const sprs_hip_csvec *v, const void **indices, const double **data);
/* indices (nnz entries of the declared width) and data (nnz doubles) to host buffers; either may be NULL */
int32_t sprs_hip_csvec_download(const sprs_hip_csvec *v, void *indices, double *data);
int32_t sprs_hip_csvec_free(sprs_hip_csvec *v);
/* CsVec::scatter / to_dense (vec.rs:621, 965): out_dev[i] = v[i] for stored i, 0.0 elsewhere.  out_len must equal dim
 * (SPRS_HIP_DIM_MISMATCH).  Asynchronous on `stream`. */
int32_t sprs_hip_csvec_scatter_f64(const sprs_hip_csvec *v, double *out_dev, uint64_t out_len, void *stream);

/* `&CsMat * &CsVec` (vec.rs:1104-1131): NEW owning vector of dimension a.rows (index width: a's declared one).
 *   CSR a: prod::csr_mul_csvec (prod.rs:161-184) — entry o = the ordered dot of row o with v (dot_acc merge, vec.rs:846-880),
 *          kept only where val != 0 (both signed zeros dropped, NaN kept); v.dim == 0 gives an empty vector of dimension 0
 *          whatever a.cols is (prod.rs:171-174);
 *   CSC a: a * v.col_view() (csmat_mul_csmat, csmat.rs:1944-1947) — the same sums, STRUCTURAL: every o with a matched index,
 *          explicit zeros kept.
 * Every sum starts from +0.0 and adds unfused products by ascending inner index: bit-identical to the reference.
 * SPRS_HIP_DIM_MISMATCH "Dimension mismatch" unless a.cols == v.dim (prod.rs:175); SPRS_HIP_INDEX_OVERFLOW when a result index
 * does not fit the declared width.  Runs on `stream` and blocks until the result is complete there. */
int32_t sprs_hip_csmat_mul_csvec_f64(const sprs_hip_csmat *a, const sprs_hip_csvec *v, sprs_hip_csvec **out, void *stream);
/* `&CsVec * &CsMat` (vec.rs:1084-1102): (v.row_view() * b).outer_view(0) — NEW owning vector of dimension b.cols, entry o =
 * sum over i ascending of v[i] * b[i, o] (mul_csr_csr, smmp.rs), structural.  SPRS_HIP_DIM_MISMATCH unless v.dim == b.rows.
 * Index width, stream and blocking as sprs_hip_csmat_mul_csvec_f64. */
int32_t sprs_hip_csvec_mul_csmat_f64(const sprs_hip_csvec *v, const sprs_hip_csmat *b, sprs_hip_csvec **out, void *stream);

/* ---- sparse +, -, elementwise * and scale (sprs/src/sparse/binop.rs) ----------------------------------------------------
 * One merge of the two sorted index lists of every outer slice (nnz_or_zip): an index only in lhs gives op(l, +0.0), only in
 * rhs op(+0.0, r), in both op(l, r) — the operation is performed, never a copy.  Every result entry is ONE IEEE operation:
 * indptr, indices and value bits are the reference's (NaN results too wherever the reference's own bits are defined: x - NaN
 * hands the NaN on with its sign, as subsd / fsub do; with NaNs on BOTH sides of + or * a host compiler may hand on either).
 * All five return a NEW owning handle, run on `stream` and block until the result is complete there; the operands are const
 * (no plan, no cached other-storage copy is touched). */
#define SPRS_HIP_BINOP_ADD 0
#define SPRS_HIP_BINOP_SUB 1
#define SPRS_HIP_BINOP_MUL 2
/* csmat_binop (binop.rs:178-271) with op = ADD | SUB | MUL (MUL: binop::mul_mat_same_storage, binop.rs:115-130).  An entry is
 * kept iff !(val == 0.0): +0.0 and -0.0 are dropped — explicit zeros of an operand and exact cancellations vanish, an index on
 * one side only vanishes under MUL — and NaN is kept (inf * 0.0).  Result: lhs' shape, storage and index types, proper indptr.
 * SPRS_HIP_INVALID_ARG for another op; SPRS_HIP_DIM_MISMATCH "Dimension mismatch" unless the shapes are equal;
 * SPRS_HIP_STORAGE_MISMATCH "Storage mismatch" unless the storages are, and when the declared index types differ (the
 * reference's generics force one I and one Iptr); SPRS_HIP_INDEX_OVERFLOW when the result's nnz does not fit Iptr. */
int32_t sprs_hip_csmat_binop_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, int32_t op, sprs_hip_csmat **out,
                                 void *stream);
/* `&lhs + &rhs` and `&lhs - &rhs` (binop.rs:52-64, 99-111): csmat_binop after rhs.to_other_storage() when the storages
 * differ (done below this boundary; the copy lives for the call).  The result has lhs' storage. */
int32_t sprs_hip_csmat_add_csmat_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out, void *stream);
int32_t sprs_hip_csmat_sub_csmat_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out, void *stream);
/* `&m * alpha` (binop.rs:132-163) = m.map(|x| x * alpha): the structure is copied unchanged and nothing is dropped — a stored
 * 0.0 stays stored, x * 0.0 is stored as +-0.0. */
int32_t sprs_hip_csmat_scale_f64(const sprs_hip_csmat *m, double alpha, sprs_hip_csmat **out, void *stream);
/* csvec_binop (binop.rs:442-479): the same merge, but EVERY merged index is appended, zeros included (-0.0 + 0.0 = +0.0 is
 * stored).  csvec_fix_zeros: an operand of dimension 0 takes the other's dimension; afterwards unequal dimensions are
 * SPRS_HIP_DIM_MISMATCH "Dimension mismatch".  Unequal declared index widths: SPRS_HIP_STORAGE_MISMATCH. */
int32_t sprs_hip_csvec_binop_f64(const sprs_hip_csvec *lhs, const sprs_hip_csvec *rhs, int32_t op, sprs_hip_csvec **out,
                                 void *stream);

/* ---- permutations (sprs/src/sparse/permutation.rs) -------------------------------------------------------------------------
 * sprs_hip_perm is the device twin of PermOwned: the Identity variant (a dimension, no arrays) or the arrays perm and perm_inv,
 * perm_inv[perm[i]] = i, both owned by the handle.  The matrix functions are ONE algorithm (permutation.rs:296-591): result
 * outer slice r' is outer slice o[r'] of the operand, every inner index j becomes g[j], each slice is sorted by the new index:
 *                                   CSR: o, g                 CSC: o, g
 *   permute_rows(A, p)              p.perm, identity          identity, p.perm_inv
 *   permute_cols(A, q)              identity, q.perm_inv      q.perm, identity
 *   transform_mat_paq(A, p, q)      p.perm, q.perm_inv        q.perm, p.perm_inv
 *   transform_mat_papt(A, p)        p.perm, p.perm_inv        the same (permutation.rs:453-454)
 * Values are moved, never computed: indptr, indices and value bits are the reference's, no tolerance anywhere. */
typedef struct sprs_hip_perm sprs_hip_perm;

/* PermOwned::new (permutation.rs:52-66) from a host array of dim indices of idx_bytes = 2, 4 or 8 each (2-byte indices are
 * widened to 4 on the device and narrowed on download).  validate != 0 runs perm_is_valid (permutation.rs:39-49: every value
 * in [0, dim), none twice) — on the host for small dim, on the device for large — and fails with SPRS_HIP_BAD_STRUCTURE
 * "invalid permutation".  The inverse is built on the device. */
int32_t sprs_hip_perm_upload(sprs_hip_perm **out, uint64_t dim, const void *perm, int32_t idx_bytes, int32_t validate);
/* The same from a DEVICE array (idx_bytes 4 or 8; a torch argsort, ...), which is COPIED on `stream`: the handle owns both of
 * its arrays.  Validation runs on the device (range test, scatter inv[p[i]] = i of the values in range, test inv[p[i]] == i: of
 * two equal values one always loses); nothing is written out of range whatever the array holds. */
int32_t sprs_hip_perm_from_device(sprs_hip_perm **out, uint64_t dim, const void *dev_perm, int32_t idx_bytes, int32_t validate,
                                  void *stream);
/* Permutation::identity (permutation.rs:113-118): the Identity variant, no arrays, no device needed; idx_bytes 2, 4 or 8 */
int32_t sprs_hip_perm_identity(sprs_hip_perm **out, uint64_t dim, int32_t idx_bytes);
/* dim, the declared index width, and whether the handle is the Identity VARIANT; any out pointer may be NULL */
int32_t sprs_hip_perm_info(const sprs_hip_perm *p, uint64_t *dim, int32_t *idx_bytes, int32_t *identity_variant);
/* PermOwned::is_identity (permutation.rs:144-152), the ELEMENTWISE test: 1 for the Identity variant and for stored arrays
 * equal to 0..dim.  Runs on `stream` and blocks until the answer is there. */
int32_t sprs_hip_perm_is_identity(const sprs_hip_perm *p, int32_t *flag, void *stream);
/* raw device pointers, still owned by the handle; NULLs for the Identity variant */
int32_t sprs_hip_perm_device_ptrs(const sprs_hip_perm *p, const void **perm, const void **perm_inv);
/* vec() / inv_vec() (permutation.rs:211-226) to host buffers of dim entries of the declared width; either may be NULL; the
 * Identity variant gives 0..dim */
int32_t sprs_hip_perm_download(const sprs_hip_perm *p, void *perm, void *perm_inv);
/* inv() (permutation.rs:120-137): a NEW owning handle with the two arrays swapped (Identity gives Identity) */
int32_t sprs_hip_perm_inv(const sprs_hip_perm *p, sprs_hip_perm **out);
int32_t sprs_hip_perm_free(sprs_hip_perm *p);
/* `&P * x` (permutation.rs:255-278): y_dev[i] = x_dev[p[i]], Identity copies.  Asynchronous on `stream`.  n != dim is
 * SPRS_HIP_DIM_MISMATCH "Dimension mismatch", overlapping x_dev / y_dev SPRS_HIP_INVALID_ARG. */
int32_t sprs_hip_perm_mul_vec_f64(const sprs_hip_perm *p, const double *x_dev, double *y_dev, uint64_t n, void *stream);
/* transform_mat_paq (permutation.rs:496-591); with one side NULL or the Identity variant it is permute_rows / permute_cols
 * (permutation.rs:296-436), with both a plain copy — as it is when rows == 0 or cols == 0.  (Departure: the reference's
 * permute_rows / permute_cols reach unreachable!() when handed the Identity variant directly; here they copy.)
 * NEW owning handle with m's shape, storage and declared index widths; every step runs on `stream` and the call blocks until
 * the result is complete there; m is const (no plan, no cached other-storage copy is touched).  Before any device work:
 *   NULL m / out                                            SPRS_HIP_INVALID_ARG
 *   row_perm.dim != rows or col_perm.dim != cols             SPRS_HIP_DIM_MISMATCH     "Dimension mismatch"
 *   a permutation's declared index width != m's              SPRS_HIP_STORAGE_MISMATCH (the reference's generics force one I)
 * m's slices must be sorted, as in every validated handle; an unvalidated handle with unsorted, duplicated or out-of-range
 * indices gets an unspecified result but never an access outside the arrays. */
int32_t sprs_hip_csmat_transform_paq(const sprs_hip_csmat *m, const sprs_hip_perm *row_perm, const sprs_hip_perm *col_perm,
                                     sprs_hip_csmat **out, void *stream);
/* transform_mat_papt (permutation.rs:439-491): P A P^T.  SPRS_HIP_DIM_MISMATCH unless m is square and rows == p.dim; a plain
 * copy when p.is_identity() — the elementwise test, so a stored permutation equal to 0..dim counts.  Otherwise as above. */
int32_t sprs_hip_csmat_transform_papt(const sprs_hip_csmat *m, const sprs_hip_perm *p, sprs_hip_csmat **out, void *stream);

/* ---- structure checks and unsorted input (sprs/src/sparse.rs:300-358, csmat.rs:311-401, vec.rs:536-557) ---------------------
 * For arrays that were assembled on the device (sprs_hip_csmat_wrap_device, sprs_hip_csvec_wrap_device, `validate = 0` uploads):
 * the check and the sort run there, nothing but the verdict travels to the host.  All four block until the answer (and the
 * result) is complete on `stream` and return SPRS_HIP_OK or SPRS_HIP_BAD_STRUCTURE with the reference's text in
 * sprs_hip_last_error().  `info` may be NULL. */
typedef struct sprs_hip_structure_info {
    int32_t kind;      /* StructureErrorKind (errors.rs): 0 ok, 1 Unsorted, 2 SizeMismatch, 3 OutOfRange */
    int32_t reserved;
    uint64_t outer;    /* the first offending outer slice; ~0 for a finding about the dimensions or the indptr; 0 for a vector */
} sprs_hip_structure_info;
/* utils::check_compressed_structure in the reference's order:
 *   1. the dimensions against the declared index widths: "Index type not large enough for this matrix", "Iptr type not large
 *      enough for this matrix" (OutOfRange);
 *   2. the indptr, in a pass of its own: "Unsorted indptr" (Unsorted), "An indptr value is larger than allowed" (OutOfRange),
 *      "Indices length and inpdtr's nnz do not match" (SizeMismatch); an indptr that does not start at 0 is SPRS_HIP_INVALID_ARG
 *      (device handles are zero based).  `indices` is not read unless this pass found nothing;
 *   3. the outer slices: "Indices are not sorted" (Unsorted: an index <= its predecessor), "Indice is larger than inner
 *      dimension" (OutOfRange: the last index of a slice >= inner).  The lowest offending slice is reported; Unsorted wins
 *      inside one slice.
 * Index arrays are read as unsigned at the handle's width: a negative value of a signed array is a large index (OutOfRange).  The
 * reference would report such a value ("Indices value out of range of usize") ahead of any Unsorted slice; this check reports in
 * slice order. */
int32_t sprs_hip_csmat_check_structure(const sprs_hip_csmat *m, sprs_hip_structure_info *info, void *stream);
/* CsVec::try_new's invariants (vec.rs:440-491): "Index size is too small" (OutOfRange), "Unsorted indices" (Unsorted), "indices
 * larger than vector size" (SizeMismatch, as in the reference). */
int32_t sprs_hip_csvec_check_structure(const sprs_hip_csvec *v, sprs_hip_structure_info *info, void *stream);
/* CsMat::new_from_unsorted / new_from_unsorted_csc: a NEW owning handle in m's storage and index widths whose outer slices are
 * sorted by inner index, validated as above.  m is only read (the reference sorts in place because it takes ownership).  Values
 * travel as 64-bit words.  Slices that are already sorted are copied; a valid m costs the check and a copy.  The indptr pass
 * (2.) runs first, where the reference would index out of bounds and panic (csmat.rs:337-340).  Two equal indices in a slice are
 * Unsorted; a slice that holds both a duplicate and an index >= inner is Unsorted, as in the reference.  On any finding *out
 * stays NULL and `info` names the kind and the first offending slice.  An inner dimension above 2^40 is not supported. */
int32_t sprs_hip_csmat_from_unsorted(const sprs_hip_csmat *m, sprs_hip_csmat **out, sprs_hip_structure_info *info, void *stream);
/* CsVec::new_from_unsorted: check, sort only on Unsorted, check again ("Unsorted indices" for a duplicate, "indices larger than
 * vector size" for a last index >= dim). */
int32_t sprs_hip_csvec_from_unsorted(const sprs_hip_csvec *v, sprs_hip_csvec **out, sprs_hip_structure_info *info, void *stream);

/* ---- orderings (sprs/src/sparse/linalg/ordering.rs, symmetric.rs, csmat.rs:1188-1216) --------------------------------------
 * Everything here walks the OUTER dimension as the reference does: a CSC handle is read as the CSR arrays of its transpose.
 * `stream` comes last: the kernels run there, host results are complete on return.
 *
 * is_symmetric (symmetric.rs:7-34): *flag = 1 when the matrix is square and every stored entry (o, i, v) has a stored entry
 * (i, o) whose value is not `!=` v — a NaN anywhere (the diagonal included) gives 0, -0.0 equals 0.0.  A non-square matrix gives
 * 0 without a launch. */
int32_t sprs_hip_csmat_is_symmetric(const sprs_hip_csmat *m, int32_t *flag, void *stream);
/* CsMat::degrees (csmat.rs:1205-1216): out_dev[o] = stored entries of outer slice o whose index is not o, for a DEVICE array of
 * outer-dimension uint64_t.  Asynchronous on `stream`.  The slices must be sorted and free of duplicates (a validated handle). */
int32_t sprs_hip_csmat_degrees(const sprs_hip_csmat *m, uint64_t *out_dev, void *stream);
/* CsMat::max_outer_nnz (csmat.rs:1188-1193): the longest outer slice, 0 for an empty matrix */
int32_t sprs_hip_csmat_max_outer_nnz(const sprs_hip_csmat *m, uint64_t *out, void *stream);

/* cuthill_mckee_custom (ordering.rs:440-526).  `start` is the strategy that picks the first vertex of every connected
 * component (ordering.rs:14-267), reversed != 0 is order::Reversed (position n - 1 - k instead of k, delimiters mirrored),
 * reverse_cuthill_mckee (ordering.rs:546-559) is (SPRS_HIP_START_PSEUDO_PERIPHERAL, 1).  The result is the reference's own
 * permutation with ties between vertices of equal degree broken by vertex id — the stable outcome of its
 * sort_unstable_by_key —, so it is one deterministic permutation whatever the device does first.  Diagonal entries are no
 * neighbours and count in no degree.  Before any device work:
 *   NULL m / out, a start other than the three below          SPRS_HIP_INVALID_ARG
 *   rows != cols                                              SPRS_HIP_DIM_MISMATCH  the text of the reference's assert_eq!
 *   rows - 1 does not fit m's declared index width             SPRS_HIP_INDEX_OVERFLOW
 * check_symmetric != 0 runs is_symmetric first (the reference's debug_assert!): SPRS_HIP_BAD_STRUCTURE "matrix is not
 * symmetric".  Without it a non-symmetric pattern is ordered as the reference's loop orders it: along the stored direction —
 * its one panic there included: the pseudo-peripheral search can return a vertex of an earlier component, SPRS_HIP_BAD_STRUCTURE
 * "Vertex returned by starting strategy should always be unvisited" (ordering.rs:488-491).
 * A 0 x 0 matrix gives an empty permutation and connected_parts == [0].  2^31 or more vertices: SPRS_HIP_INVALID_ARG. */
#define SPRS_HIP_START_NEXT 0
#define SPRS_HIP_START_MINIMUM_DEGREE 1
#define SPRS_HIP_START_PSEUDO_PERIPHERAL 2
typedef struct sprs_hip_ordering sprs_hip_ordering;
int32_t sprs_hip_csmat_cuthill_mckee(const sprs_hip_csmat *m, int32_t start, int32_t reversed, int32_t check_symmetric,
                                     sprs_hip_ordering **out, void *stream);
/* dim, the number of entries of connected_parts (components + 1), and — stats may be NULL — four counters of the call that
 * made the ordering: components, levels of the ordering pass, launches (a sort or a scan counts as one), host read-backs */
int32_t sprs_hip_ordering_info(const sprs_hip_ordering *o, uint64_t *dim, uint64_t *n_parts, uint64_t *stats /* 4 */);
/* Ordering::perm: a NEW owning permutation handle (perm and perm_inv) with the matrix's declared index width, as PermOwnedI<I> */
int32_t sprs_hip_ordering_perm(const sprs_hip_ordering *o, sprs_hip_perm **out);
/* Ordering::connected_parts to a host array of n_parts uint64_t */
int32_t sprs_hip_ordering_parts(const sprs_hip_ordering *o, uint64_t *parts);
int32_t sprs_hip_ordering_free(sprs_hip_ordering *o);

/* ---- LDL^T factorization (sprs-ldl/src/lib.rs, sprs/src/sparse/linalg.rs:17-29) --------------------------------------------
 * P A P^T = L D L^T for a symmetric matrix, f64.  Everything walks the OUTER dimension of the handle as the reference does
 * (outer_iterator_papt, csmat.rs:1170-1185), so a CSR and a CSC handle of a symmetric matrix give the same factors; only for a
 * non-symmetric matrix with the check off do they differ, as they do in the reference.  colptr, parents, l_indices and every bit
 * of l_data and d are the reference's: the numeric pass walks the pattern of each row in the order the reference's stack leaves
 * it in.  `stream` comes last: the kernels run there, handles and host results are complete on return.
 *
 * ldl_symbolic (lib.rs:445-496; LdlSymbolic::new_perm, lib.rs:252-284): perm = NULL is the identity.  Before any device work:
 *   NULL m / out                                              SPRS_HIP_INVALID_ARG
 *   rows != cols ("matrix should be square"), perm.dim != rows  SPRS_HIP_DIM_MISMATCH
 *   perm's declared index width differs from m's               SPRS_HIP_STORAGE_MISMATCH
 * check_symmetry != 0 runs is_symmetric first: SPRS_HIP_BAD_STRUCTURE "Matrix is not symmetric" (lib.rs:461-463).
 * SPRS_HIP_INDEX_OVERFLOW when nnz(L) does not fit m's declared index width.  n = 0 and n = 1 are accepted (factor is not). */
typedef struct sprs_hip_ldl_sym sprs_hip_ldl_sym;
typedef struct sprs_hip_ldl_num sprs_hip_ldl_num;
int32_t sprs_hip_ldl_symbolic(const sprs_hip_csmat *m, const sprs_hip_perm *perm, int32_t check_symmetry, sprs_hip_ldl_sym **out,
                              void *stream);
/* problem_size (lib.rs:288), nnz (lib.rs:294) and — stats may be NULL — four counters of the call that made the handle: launches
 * of the elimination-tree pass, all launches (a sort or a scan counts as one), host read-backs, 0 */
int32_t sprs_hip_ldl_symbolic_info(const sprs_hip_ldl_sym *s, uint64_t *n, uint64_t *nnz, uint64_t *stats /* 4 */);
/* l_colptr to a host array of n + 1 uint64_t */
int32_t sprs_hip_ldl_symbolic_colptr(const sprs_hip_ldl_sym *s, uint64_t *colptr);
/* the elimination tree to a host array of n uint64_t: parents[i], UINT64_MAX for a root (etree.rs: None) */
int32_t sprs_hip_ldl_symbolic_parents(const sprs_hip_ldl_sym *s, uint64_t *parents);
/* the permutation the analysis was made with: a NEW handle (the Identity variant when none was given) */
int32_t sprs_hip_ldl_symbolic_perm(const sprs_hip_ldl_sym *s, sprs_hip_perm **out);
int32_t sprs_hip_ldl_symbolic_free(sprs_hip_ldl_sym *s);
/* LdlSymbolic::factor (lib.rs:300-323): a numeric handle that shares s's analysis and keeps it alive (s may be freed, or
 * factored again).  m: square, of s's dimension (SPRS_HIP_DIM_MISMATCH) and index type (SPRS_HIP_STORAGE_MISMATCH), with the
 * pattern that was analysed (a stored entry outside it: SPRS_HIP_HIP_ERROR, nothing is written out of range).
 *   n < 2        SPRS_HIP_INVALID_ARG  "assertion failed: n > 1 (DStack::with_capacity, sprs/src/stack.rs:39)" (lib.rs:313)
 *   d[k] == 0    SPRS_HIP_SINGULAR_MATRIX "Singular matrix at index k (diagonal element is a numeric 0)" (lib.rs:585-590) with the
 *                smallest such k; info (may be NULL) then holds singular_index = k, singular_reason = 1, as after
 *                sprs_hip_trisolve_f64; no handle is returned
 * Nothing else is checked, as in the reference.  A polling loop that times out is SPRS_HIP_HIP_ERROR, never a hang. */
int32_t sprs_hip_ldl_factor_f64(const sprs_hip_ldl_sym *s, const sprs_hip_csmat *m, sprs_hip_ldl_num **out,
                                sprs_hip_trisolve_info *info, void *stream);
/* LdlNumeric::update (lib.rs:364-381): the same with new values into the handle's arrays; after an error its factors are
 * unspecified */
int32_t sprs_hip_ldl_update_f64(sprs_hip_ldl_num *f, const sprs_hip_csmat *m, sprs_hip_trisolve_info *info, void *stream);
/* LdlNumeric::solve (lib.rs:388-410): x = P^-1 ltsolve(diag_solve(lsolve(P b))) for DEVICE arrays of n doubles (x may be b) */
int32_t sprs_hip_ldl_solve_f64(sprs_hip_ldl_num *f, const double *b_dev, double *x_dev, uint64_t n, void *stream);
/* LdlNumeric::d (lib.rs:413): the n pivots into a DEVICE array.  Asynchronous on `stream`. */
int32_t sprs_hip_ldl_d(const sprs_hip_ldl_num *f, double *d_dev, uint64_t n, void *stream);
/* LdlNumeric::l (lib.rs:418-429): a NEW owning CSC handle, n x n, strictly lower, no diagonal stored; indptr and indices both in
 * the index type of the matrix that was analysed */
int32_t sprs_hip_ldl_l(const sprs_hip_ldl_num *f, sprs_hip_csmat **out, void *stream);
int32_t sprs_hip_ldl_numeric_free(sprs_hip_ldl_num *f);
/* ldl_lsolve (lib.rs:597-609) and ldl_ltsolve (lib.rs:613-626), in place on the n doubles of x_dev, for a CSC handle that is
 * STRICTLY lower triangular with an implied unit diagonal (what sprs_hip_ldl_l returns; entries on or above the diagonal are not
 * read).  lsolve: columns 0 .. n-1 scatter, so x[r] receives its products by ascending column; ltsolve: columns n-1 .. 0, each
 * subtracting in stored order.  SPRS_HIP_STORAGE_MISMATCH for a CSR handle, SPRS_HIP_DIM_MISMATCH as sprs_hip_trisolve_f64. */
int32_t sprs_hip_ldl_lsolve_f64(sprs_hip_csmat *l, double *x_dev, uint64_t n, void *stream);
int32_t sprs_hip_ldl_ltsolve_f64(sprs_hip_csmat *l, double *x_dev, uint64_t n, void *stream);
/* linalg::diag_solve (linalg.rs:17-29): x[i] /= d[i] on DEVICE arrays.  Asynchronous on `stream`. */
int32_t sprs_hip_diag_solve_f64(const double *d_dev, double *x_dev, uint64_t n, void *stream);

/* ---- sparse-rhs triangular solve (sprs/src/sparse/linalg/trisolve.rs:286-358) ---------------------------------------------- */

/* reach = unknowns of the solution's pattern; reach_levels = breadth-first levels of the search that found them;
 * reach_launches = launches of its frontier kernels, each followed by one read-back of its state (the one-workgroup kernel
 * runs up to `sptrisolve_budget` narrow levels per launch, a wide level is a launch of its own); solve_levels = levels of the
 * handle's lower level plan, from which the solve order is drawn (an upper bound on the chain inside the reach).
 * singular_index / singular_reason as in sprs_hip_trisolve_info. */
typedef struct sprs_hip_sptrisolve_info {
    uint64_t reach, reach_levels, reach_launches, solve_levels;
    uint64_t singular_index;    /* UINT64_MAX */
    int32_t singular_reason;    /* 0 / 1 numeric / 2 structural */
} sprs_hip_sptrisolve_info;

/* Twin of lsolve_csc_sparse_rhs (sprs/src/sparse/linalg/trisolve.rs:286-358): L x = rhs with a sparse rhs, at a cost that
 * follows the REACH of rhs — every column a search over the columns of L gets to from a stored index of rhs (stored zeros
 * are roots too; every stored entry of a column is followed, the diagonal and entries above it included) — instead of n.
 * *out = a NEW owning CsVec handle: dimension n, L's declared index width, the reach in ASCENDING order with every index of
 * it stored (numeric zeros kept), x there.  Differences from the reference, all three deliberate:
 *   (a) the reference leaves the pattern as an unsorted stack beside a dense workspace and processes its columns in the
 *       reverse post-order of its depth-first search; here unknown r receives its products by ascending column (each
 *       product rounded, then each subtraction, then one division).  Exact arithmetic gives identical bits; general values
 *       can differ in the last bits where a row receives two or more products;
 *   (b) a fill-in unknown (in the reach, not stored in rhs) starts from +0.0, not from the previous contents of a workspace;
 *   (c) of several singular columns in the reach the SMALLEST index is reported (the reference: the first in its search
 *       order), "a structural 0" for a diagonal that is not stored, "a numeric 0" for a stored 0.0 or -0.0 (NaN is not
 *       zero).  A singular column outside the reach is not an error, and an inf or NaN stored under a column outside the
 *       reach never reaches x.
 * l must be a CSC handle (a transpose view of a CSR matrix is one) with sorted columns; the solve runs on its cached CSR
 * form, whose level plan and scratch are kept in the handle: after the first solve, a solve makes no pass over n or
 * nnz(L).
 * SPRS_HIP_INVALID_ARG for a NULL handle, vector or out, a CSR handle ("Storage mismatch") or n >= 2^32;
 * SPRS_HIP_DIM_MISMATCH unless L is square and rhs.dim == n; SPRS_HIP_INDEX_OVERFLOW when n does not fit L's declared
 * index width; SPRS_HIP_SINGULAR_MATRIX ("Singular matrix at index i (reason)") with *out == NULL; n == 0 or an rhs without
 * stored entries give an empty vector.  Blocks until done; runs its work on `stream`. */
int32_t sprs_hip_lsolve_csc_sparse_rhs_f64(sprs_hip_csmat *l, const sprs_hip_csvec *rhs, sprs_hip_csvec **out,
                                           sprs_hip_sptrisolve_info *info, void *stream);

/* ---- construction (sprs/src/sparse/kronecker.rs, construct.rs) -----------------------------------------------------------
 * New owning handles assembled on the device; indptr, indices and value bits are the reference's.  All operands of one call
 * must declare the same index and indptr widths (the reference's one I / Iptr): SPRS_HIP_STORAGE_MISMATCH otherwise.  The
 * result takes them.  `stream` as for the binops: the kernels run there and the result is complete on return; an operand
 * that has to change its storage first goes through sprs_hip_csmat_to_other_storage (null stream, after a wait for `stream`).
 * *out is written on success only.
 *
 * kronecker_product (kronecker.rs:50-99): the result has a's storage (b is converted when it has the other one); outer slice
 * ia * outer(b) + ib holds the products of the stored entries of slice ia of a and slice ib of b in stored order, index
 * ai * inner(b) + bi, value av * bv — one multiply, nothing dropped.  SPRS_HIP_INDEX_OVERFLOW, decided by SHAPE before
 * anything is allocated: a shape product that overflows 64 bits, inner(a) * inner(b) - 1 that does not fit the index width,
 * nnz(a) * nnz(b) that does not fit the indptr width.  (The reference panics only when a STORED index does not fit.) */
int32_t sprs_hip_csmat_kronecker_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **out, void *stream);
/* same_storage_fast_stack (construct.rs:10-45): the n matrices one after the other along their outer axis, in their storage.
 * `mats` is a host array of n handles.  In the reference's order: n == 0 SPRS_HIP_INVALID_ARG "Empty stacking list", unequal
 * inner dimensions SPRS_HIP_DIM_MISMATCH "Dimension mismatch", unequal storages SPRS_HIP_STORAGE_MISMATCH "Storage mismatch". */
int32_t sprs_hip_csmat_same_storage_fast_stack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream);
/* vstack / hstack (construct.rs:48-81): the fast stack of the CSR / CSC forms of the operands; the result is always CSR for
 * vstack and CSC for hstack.  Errors as above (unequal column / row counts are "Dimension mismatch"). */
int32_t sprs_hip_csmat_vstack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream);
int32_t sprs_hip_csmat_hstack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream);
/* bmat (construct.rs:94-160): `blocks` is a host array of super_rows * super_cols handles, row-major, NULL = None (a zero block
 * of the super-row's largest row count by the super-column's largest column count).  The result is CSR.  In the reference's
 * order: no super-row or no super-column SPRS_HIP_INVALID_ARG "Empty stacking list", a super-row of NULLs "Empty bmat row", a
 * super-column of NULLs "Empty bmat col" (both SPRS_HIP_INVALID_ARG), then SPRS_HIP_DIM_MISMATCH "Dimension mismatch" as the
 * reference's hstack of every super-row and vstack of the results find it: the present blocks of a super-row must have equal
 * row counts, and the super-rows equal TOTAL column counts — a block's column offset is the sum of the ACTUAL column counts to
 * its left in its own super-row (a NULL counts the super-column's maximum), so [2 | 3] over [3 | 2] columns is accepted. */
int32_t sprs_hip_csmat_bmat(const sprs_hip_csmat **blocks, uint64_t super_rows, uint64_t super_cols, sprs_hip_csmat **out, void *stream);

/* ---- dense <-> sparse (sprs/src/sparse/csmat.rs:499-549, to_dense.rs, binop.rs:273-433) -----------------------------------
 * A dense operand is f64 in DEVICE memory, SPRS_HIP_ROW_MAJOR or SPRS_HIP_COL_MAJOR, with a leading dimension ld in elements:
 * ld >= cols for row-major, ld >= rows for column-major, SPRS_HIP_INVALID_ARG otherwise (also for a bad layout tag or a NULL
 * array that has elements).  The unit inner stride is the only one: ndarray's general strides (binop.rs' mul_dense_strided
 * walks s![..;2, ..;2]) are out of scope.  Elements in the padding between the extent and ld are never read into a result and
 * never written.  `stream` comes last: the kernels run there.  Every result element is one or two IEEE operations without a
 * reduction, unfused (multiply, then add): results are the reference's bit for bit; a NaN made out of no NaN carries the sign
 * bit, as on the x86 the reference runs on.
 *
 * csr_from_dense / csc_from_dense (csmat.rs:499-549; storage = SPRS_HIP_CSR / SPRS_HIP_CSC): a new owning handle of the elements
 * with fabs(x) > eps, eps = epsilon > 0 ? epsilon : 0 (a negative or NaN epsilon is 0).  NaN, both zeros and |x| == eps are
 * dropped, infinities and denormals above eps kept; a kept value's bits are stored unchanged, inner indices ascend, indptr is
 * proper.  Any layout with any storage (the reference reverses the axes of the view).  iptr_bytes / idx_bytes: 2, 4 or 8, as
 * sprs_hip_csmat_upload.  SPRS_HIP_INDEX_OVERFLOW where I::from_usize / Iptr::from_usize panic: a KEPT inner index above the
 * index type's maximum (a wide matrix whose kept entries all fit is fine), a total nnz above the indptr type's.  The result is
 * complete on return; *out is written on success only. */
int32_t sprs_hip_csmat_from_dense_f64(sprs_hip_csmat **out, int32_t storage, const double *m_dev, uint64_t rows, uint64_t cols,
                                      int32_t layout, uint64_t ld, double epsilon, int32_t iptr_bytes, int32_t idx_bytes, void *stream);
/* assign_to_dense (to_dense.rs:12-30): out[row, col] = value for every stored entry; every other element of out, padding
 * included, is untouched.  SPRS_HIP_DIM_MISMATCH "Dimension mismatch" unless m is rows x cols (the reference's two asserts).  Any
 * storage with any layout.  An inner index at or above the inner dimension (an unchecked handle) is skipped — never a store
 * outside the rows x cols elements; of duplicated indices one survives, unspecified which.  Asynchronous on `stream`. */
int32_t sprs_hip_csmat_assign_to_dense_f64(const sprs_hip_csmat *m, double *out_dev, uint64_t rows, uint64_t cols, int32_t layout,
                                           uint64_t ld, void *stream);
/* CsMat::to_dense (csmat.rs:1127-1134): the rows x cols elements set to +0.0 (not the padding), then assign_to_dense. */
int32_t sprs_hip_csmat_to_dense_f64(const sprs_hip_csmat *m, double *out_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                    void *stream);
/* csmat_binop_dense_raw (binop.rs:384-433) with the two closures the reference ships: op = SPRS_HIP_BINOP_ADD writes
 * (alpha * l) + (beta * r) — add_dense_mat_same_ordering, binop.rs:279-323 —, SPRS_HIP_BINOP_MUL (alpha * l) * r, beta ignored —
 * mul_dense_mat_same_ordering, binop.rs:331-371 — into EVERY element of out; l is +0.0 where lhs stores nothing and the
 * operation is performed there too (alpha = -1, r = -0.0 gives -0.0; (alpha * 0) * inf is NaN).  out has the layout of rhs and
 * the leading dimension out_ld.  Checks in the reference's order (binop.rs:397-412) after the argument checks: lhs is rows x cols
 * or SPRS_HIP_DIM_MISMATCH "Dimension mismatch"; CSR with row-major / CSC with column-major or SPRS_HIP_STORAGE_MISMATCH "Storage
 * mismatch".  out overlapping rhs is SPRS_HIP_INVALID_ARG (the reference cannot alias them either).  Asynchronous on `stream`. */
int32_t sprs_hip_csmat_binop_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rows, uint64_t cols, int32_t layout,
                                       uint64_t ld, int32_t op, double alpha, double beta, double *out_dev, uint64_t out_ld, void *stream);
/* `&CsMat + &Array2` (csmat.rs:1951-1987): the binop above with ADD and alpha = beta = 1 into a contiguous out of rhs' layout
 * (out_ld = cols / rows); a lhs whose storage does not match the layout goes through to_other_storage first (null stream, after a
 * wait for `stream`; the copy lives for the call, which then returns when the result is complete). */
int32_t sprs_hip_csmat_add_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rows, uint64_t cols, int32_t layout,
                                     uint64_t ld, double *out_dev, void *stream);

/* ---- reductions and extraction: the small questions asked of a vector or matrix that already sits on the device ----------------
 * THE ORDERED SUM.  Every scalar below is the reference's left-to-right chain (dot_acc from Acc::zero(), vec.rs:856-880; the
 * others through Iterator::sum) of unfused terms, bit for bit at every size: a grid forms the terms in entry order, ONE wave adds
 * them in that order.  No float atomics: the same bits from run to run.  The serial chain's rate bounds these calls on very long
 * vectors; that is the price of the reference's bits.  The one documented difference: every chain starts from +0.0 (dot_acc does
 * too; the neutral element of Iterator::sum for f64 has not been the same in every Rust toolchain), so the SIGN of a zero
 * result of dot_dense and of the norms may differ from a given build of the reference.
 * All of them run on `stream`; an entry that returns a scalar or a new handle blocks until the result is complete there.
 * Temporaries are sized by nnz or by the number of queries, never by dim. */

/* CsVec::dot with a sparse rhs (vec.rs:828-881) and prod::csvec_dot_by_binary_search (prod.rs:14-70), one device function: each
 * entry of the vector with fewer entries (v on equal counts, prod.rs:25) binary-searches the other's indices; the products
 * v[i] * w[i] of the matched indices are added by ascending index — matched zeros and NaNs like any other term.  The index widths
 * may differ (the reference compares usize).  SPRS_HIP_DIM_MISMATCH "Dimension mismatch" unless v.dim == w.dim (vec.rs:855).  The
 * search stays inside [0, nnz) whatever a borrowed, unchecked vector holds. */
int32_t sprs_hip_csvec_dot_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, double *out_host, void *stream);
/* CsVec::dot_dense and dot with a dense rhs (vec.rs:857-860, 894-904): the chain over data[i] * x[indices[i]] in storage order.
 * x_len must equal v.dim (SPRS_HIP_DIM_MISMATCH).  An index >= x_len of a borrowed vector contributes no term and is never read. */
int32_t sprs_hip_csvec_dot_dense_f64(const sprs_hip_csvec *v, const double *x_dev, uint64_t x_len, double *out_host, void *stream);
/* squared_l2_norm (vec.rs:907-913: terms x * x), l2_norm (916-922: its sqrt, taken on the HOST from the scalar that came back —
 * the reference's libm, the reference's bits), l1_norm (925-930: terms |x|) and norm(p) (939-958), kind = SPRS_HIP_NORM_P:
 *   p = +inf  fold(-inf, max) of |x|: 0.0 for an empty vector, -inf for one of NaNs only (f64::max ignores NaN);
 *   p = -inf  fold(+inf, min) of |x|: 0.0 for an empty vector;
 *   p = 0     the count of entries with !(|x| == 0), NaN counted, as a double;
 *   else      the chain over pow(|x|, p) formed on the device, then pow(sum, 1 / p) on the host.  The device's pow is not the
 *             host's: this is the one result that is close to, not bit-equal with, the reference (DESIGN.md has the measure).
 * The first three are order-free (exact) and run as an ordinary parallel reduction.  p is ignored for the other kinds. */
#define SPRS_HIP_NORM_SQUARED_L2 0
#define SPRS_HIP_NORM_L2 1
#define SPRS_HIP_NORM_L1 2
#define SPRS_HIP_NORM_P 3
int32_t sprs_hip_csvec_norm_f64(const sprs_hip_csvec *v, int32_t kind, double p, double *out_host, void *stream);
/* unit_normalize (vec.rs:1051-1061): the squared norm by the chain; when it is > 0 every value is divided by its sqrt (taken on
 * the host; a plain IEEE divide on the device).  Handles are immutable snapshots, so — like sprs_hip_csmat_scale_f64 — this
 * returns a NEW owning vector with the same indices, width and dim and leaves v alone; a zero vector comes back as a copy. */
int32_t sprs_hip_csvec_unit_normalize_f64(const sprs_hip_csvec *v, sprs_hip_csvec **out, void *stream);
/* nnz_index / get (vec.rs:787-805), batched: for the nq indices q_dev[q] (device, uint64_t) pos_dev[q] = the position in the stored
 * arrays or UINT64_MAX (None) and, when val_dev is not NULL, val_dev[q] = the stored value or 0.0.  An index >= dim is None.
 * nq = 0 and nnz = 0 launch no kernel.  Asynchronous on `stream`. */
int32_t sprs_hip_csvec_nnz_index(const sprs_hip_csvec *v, uint64_t nq, const uint64_t *q_dev, uint64_t *pos_dev, double *val_dev,
                                 void *stream);
/* outer_view (csmat.rs:1219-1231): zero-copy, as transpose_view is — a BORROWING vector over indices + indptr[i] and
 * data + indptr[i], of dim = the inner dimension and m's index widths (device and declared); the two indptr values are read back
 * on `stream`.  i >= outer dims: SPRS_HIP_OK with *out = NULL (the reference's None).  The view is valid until m is freed. */
int32_t sprs_hip_csmat_outer_view(const sprs_hip_csmat *m, uint64_t i, sprs_hip_csvec **out, void *stream);
/* diag (csmat.rs:1234-1256): NEW owning vector of dim min(rows, cols) in m's index width; entry i is stored iff (i, i) is —
 * structural: an explicit 0.0 on the diagonal is kept.  The same for CSR and CSC. */
int32_t sprs_hip_csmat_diag_f64(const sprs_hip_csmat *m, sprs_hip_csvec **out, void *stream);
/* nnz_index / get (csmat.rs:1312-1351), batched: for the nq pairs (rows_dev[q], cols_dev[q]) (device, uint64_t) pos_dev[q] = the
 * global position in indices / data or UINT64_MAX (None), val_dev (may be NULL) as above.  For a CSC handle (outer, inner) =
 * (col, row).  An outer index >= outer dims or an inner index that is not stored is None, not an error.  Asynchronous on `stream`. */
int32_t sprs_hip_csmat_nnz_index(const sprs_hip_csmat *m, uint64_t nq, const uint64_t *rows_dev, const uint64_t *cols_dev,
                                 uint64_t *pos_dev, double *val_dev, void *stream);
/* to_inner_onehot (csmat.rs:1017-1056): NEW owning matrix of m's shape, storage and index types with a proper indptr: outer slice
 * o is populated iff it has a non-NaN entry; its one index is the inner index of the maximum — the LAST of equal maxima
 * (Iterator::max_by; -0.0 == +0.0), NaNs skipped, +-inf taking part — and its value 1.0. */
int32_t sprs_hip_csmat_to_inner_onehot_f64(const sprs_hip_csmat *m, sprs_hip_csmat **out, void *stream);

/* ---- row-sharded SpMV over the GPUs of one node (one process per GPU, RCCL over xGMI) ----
 * The reference has no distributed code; the shard is its slice_outer (slicing.rs:65-89) with a rebased indptr
 * (indptr.rs:206-214): rank g owns rows [row_starts[g], row_starts[g+1]) and a full replica of x; one exchange, an
 * all-gather-v of y, issued as ONE group of direct sends / receives with every peer (xGMI is a point-to-point mesh).
 *   sprs_hip_dist_unique_id  128 bytes from ncclGetUniqueId: call on ONE rank and hand them to the others (MPI, a
 *                            torch.distributed broadcast, a file ...), like every NCCL / RCCL program does
 *   sprs_hip_dist_create     collective.  local_block = this rank's rows as a CSR handle with all `cols` columns and a
 *                            zero-based indptr (sprs_hip_csmat_slice_outer makes one).  It is cut into nsub sub-blocks of
 *                            equal cost; the exchange of a finished sub-block overlaps the multiply of the next
 *                            (nsub = 1: multiply, then exchange).  Every rank passes the same world, row_starts, nsub.
 *   sprs_hip_dist_spmv_f64   collective.  y (length rows, on this rank's device) = A * x (x: length cols, replicated).
 *                            Asynchronous on `stream`; y is complete for work queued on `stream` afterwards.
 * RCCL is loaded at run time (dlopen); world = 1 needs none.  SPRS_HIP_HIP_ERROR carries RCCL's message.
 * id_128_bytes = NULL with world > 1: no communicator is made, the handle exchanges over the peer route only (below). */
typedef struct sprs_hip_dist sprs_hip_dist;
int32_t sprs_hip_dist_unique_id(void *id_128_bytes);
int32_t sprs_hip_dist_create(sprs_hip_dist **d, const void *id_128_bytes, int32_t world, int32_t rank, uint64_t rows,
                             uint64_t cols, const uint64_t *row_starts /* world + 1 */, const sprs_hip_csmat *local_block,
                             int32_t nsub);
int32_t sprs_hip_dist_spmv_f64(sprs_hip_dist *d, const double *x_dev, uint64_t x_len, double *y_dev, uint64_t y_len,
                               void *stream);
/* the rank count the RCCL communicator itself reports (ncclCommCount); a world of one has no communicator and reports 1 */
int32_t sprs_hip_dist_comm_count(const sprs_hip_dist *d, int32_t *ranks);
/* THE SECOND EXCHANGE ROUTE: stores into the peers' receive windows over xGMI instead of ncclSend / ncclRecv (both
 * routes, to be compared by the first multi-GPU run).  Every rank exports its window (sprs_hip_dist_peer_handle: 64 bytes, a
 * HIP IPC handle), the host program hands all of them to every rank in rank order — like the RCCL id — and
 * sprs_hip_dist_peer_connect maps them; sprs_hip_dist_set_route(d, SPRS_HIP_ROUTE_PEER) then makes sprs_hip_dist_spmv_f64
 * push every finished sub-block into all peers' windows with one kernel (all links at once), publish an epoch word, wait for
 * the peers' epoch words and copy their rows into y.  Same result as the RCCL route, bit for bit (the multiply is the same
 * kernel).  A handle made with id_128_bytes = NULL and world > 1 has no RCCL communicator and can ONLY use this route (ranks
 * that share a device; hosts without RCCL).  All three calls are collective in the sense that every rank must make them; a
 * peer that does not arrive within 2 s turns the NEXT call into SPRS_HIP_HIP_ERROR instead of hanging the device.
 * sprs_hip_dist_free must not run while a peer may still store into this rank's window (synchronise the ranks first). */
#define SPRS_HIP_ROUTE_RCCL 0
#define SPRS_HIP_ROUTE_PEER 1
int32_t sprs_hip_dist_peer_handle(sprs_hip_dist *d, void *handle_64_bytes);
int32_t sprs_hip_dist_peer_connect(sprs_hip_dist *d, const void *handles /* world x 64 bytes, rank order */, int32_t world);
int32_t sprs_hip_dist_set_route(sprs_hip_dist *d, int32_t route);
int32_t sprs_hip_dist_route(const sprs_hip_dist *d, int32_t *route);
int32_t sprs_hip_dist_free(sprs_hip_dist *d);

/* Triplet (COO) assembly: twin of TriMatBase::to_csr / to_csc (triplet.rs:262-276) = TriMatIter::into_cs
 * (triplet_iter.rs:127-224): the n triplets (row_inds[p], col_inds[p], data[p]) — arrays in DEVICE memory, indices of
 * in_idx_bytes (4 or 8) each — are sorted by (outer, inner) with a stable device radix sort, duplicates are summed in
 * triplet order (`slot = slot + next`, triplet_iter.rs:168-171; the reference's unstable sort leaves that order
 * open), explicit zeros stay stored, empty outer slices get their indptr entries.  New owning handle with `storage`,
 * indices of out_idx_bytes and indptr of out_iptr_bytes.  SPRS_HIP_INVALID_ARG for an index out of bounds (add_triplet
 * asserts it, triplet.rs:171-172) or more than 2^32 rows / columns; SPRS_HIP_INDEX_OVERFLOW as CsMat construction. */
int32_t sprs_hip_triplets_to_cs(uint64_t rows, uint64_t cols, uint64_t n, const void *row_inds_dev, const void *col_inds_dev,
                                int32_t in_idx_bytes, const double *data_dev, int32_t storage, int32_t out_idx_bytes,
                                int32_t out_iptr_bytes, sprs_hip_csmat **out);

/* ---- tuning knobs (A/B runs; never needed for correctness) -------------- */

/* name = "spmv_kernel":    0 auto, 1 nnz-tiled streaming kernel, 2 wave-per-row (A/B only);
 * name = "spmv_xcs":       XCD-sliced plan for long rows: 0 auto, 1 force on, 2 off;
 * name = "spmv_xcs_split": rows with at least this many entries go to the sliced part (default 32);
 * name = "spmv_xcs_idx32": 1 (default): the sliced plan's own copies hold 32-bit column ids when cols < 2^32;
 * name = "spmv_sort_tiles": 1: tiles of the sliced plan's copies are stored sorted by column (default 0: measured slower);
 * name = "spmv_tile":      nnz per workgroup tile: 0 auto (default), 2048 or 4096;
 * name = "spmv_band*":     the banded plan (hot columns from LDS): spmv_band 0 auto / 1 on / 2 off, spmv_band_hot (slices, default
 *                          128), spmv_band_tile (labels per slice: 16384 or 8192; f32 handles read spmv_f32_band_tile: 8192, 16384 or 32768), spmv_band_split (row length from which a row
 *                          is cut into pieces, default 24), spmv_band_rounds, spmv_band_hot_run, spmv_band_cold_tiles,
 *                          spmv_band_overlap, spmv_band_split_permute, spmv_band_phases, spmv_band_hot_cut, spmv_band_pack (2: the hot
 *                          slices keep 10 bytes per entry instead of the lossless 8.5-byte records);
 * name = "spgemm_ordered":  1 (default): SpGEMM adds the products of an entry in the reference's order (values bit-identical
 *                          to sprs', deterministic); 0: unordered atomic adds in the large-row kernel (same products, rounding-
 *                          level differences, not reproducible run to run; since round 4 no faster: the order costs nothing
 *                          once a wave instruction's products go out as ONE ds_add_f64, option spgemm_lane_order);
 * name = "gauss_seidel_blocks": workgroups of the Gauss-Seidel sweep kernel (0 = default: one per CU), "gauss_seidel_naps";
 * name = "ordering_narrow_cap": Cuthill-McKee: widest frontier (vertices, default and maximum 1024) the one-workgroup kernel
 *                          keeps in LDS; wider levels run as a grid; 0: every level does; "ordering_key_bits" (INTEGRATION.md);
 * name = "ldl_lds_cap":    LDL^T numeric pass: longest row of L (entries, default and maximum 1024) whose work vector stays in
 *                          LDS; longer rows use a slice of a device array.  Same bits either way;
 * name = "sptrisolve_budget": sparse-rhs triangular solve: narrow levels of the reach per launch of its one-workgroup kernel
 *                          (default 4096, 1 ... 2^20); same result whatever the value;
 * name = "spgemm_*", "spmm_long_row", "spmm_stream", "pool", "pool_max_bytes": INTEGRATION.md, "Options".
 * The whole table (name, default, range) is SPRS_HIP_OPTIONS in sprs_amd/csrc/common.hpp.  Developer switches — timing
 * experiments with WRONG results (spgemm_debug, spmv_xmask, spmv_band_debug) and the profiling printout spgemm_prof — exist
 * only in libraries built with -DSPRS_HIP_DEVTOOLS; this one rejects them.  get_option("devtools") tells which build it is.
 * get_option("spgemm_f32_lds_add") (read-only) reports the library's probe of the f32 LDS add on the current device: bit 0 the
 * lanes of one add instruction that hit one address are applied in ascending lane order, bit 1 f32 subnormals are kept.
 * Process-wide.  Unknown names / bad values return SPRS_HIP_INVALID_ARG. */
/* Contract: every option has a closed range (the table in sprs_amd/csrc/common.hpp); a value outside it — including a value
 * other than 0 / 1 for an on / off switch — and an unknown or retired name return SPRS_HIP_INVALID_ARG and change nothing
 * (sprs_hip_last_error() names the option and its range).  Nothing is coerced. */
int32_t sprs_hip_set_option(const char *name, int64_t value);
int32_t sprs_hip_get_option(const char *name, int64_t *value);

/* ---- single precision: CsMat<f32>, its SpMV and BiCGSTAB -------------------------------------------------------------
 * The reference is generic over its scalar N and instantiates its solver for f64 and f32 (bicgstab.rs:304-305); its MulAcc
 * products (mul_acc.rs:17-31) are scalar-generic.  An f32 matrix lives behind a handle type OF ITS OWN: no entry that reads
 * the `double` values of a sprs_hip_csmat can be handed one.  Built for f32: the container, SpMV in both storages, BiCGSTAB,
 * and the value casts to and from the f64 handle, through which every other operation of the library stays reachable without
 * leaving the device.  Index widths: 4 or 8 bytes for indptr and indices, in all four pairs, on the host as on the device;
 * 2-byte host arrays are NOT accepted for f32 handles (SPRS_HIP_INVALID_ARG). */

typedef struct sprs_hip_csmat_f32 sprs_hip_csmat_f32;

/* The contracts of their f64 namesakes (sprs_hip_csmat_upload ... sprs_hip_csmat_free above) with float values: the same
 * structure validation, the same SPRS_HIP_BAD_STRUCTURE / SPRS_HIP_DIM_MISMATCH statuses and texts, a possibly non-zero-based
 * host indptr rebased on the way in, wrapped device buffers 16-byte aligned and not owned. */
int32_t sprs_hip_csmat_f32_upload(sprs_hip_csmat_f32 **out, int32_t storage, uint64_t rows, uint64_t cols,
                                  const void *indptr, int32_t iptr_bytes, const void *indices,
                                  int32_t idx_bytes, const float *data, int32_t validate);
int32_t sprs_hip_csmat_f32_wrap_device(sprs_hip_csmat_f32 **out, int32_t storage, uint64_t rows,
                                       uint64_t cols, uint64_t nnz, const void *dev_indptr,
                                       int32_t iptr_bytes, const void *dev_indices, int32_t idx_bytes,
                                       const float *dev_data);
int32_t sprs_hip_csmat_f32_info(const sprs_hip_csmat_f32 *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz,
                                int32_t *iptr_bytes, int32_t *idx_bytes, int32_t *storage);
int32_t sprs_hip_csmat_f32_device_ptrs(const sprs_hip_csmat_f32 *m, const void **indptr,
                                       const void **indices, const float **data);
int32_t sprs_hip_csmat_f32_download(const sprs_hip_csmat_f32 *m, void *indptr, void *indices, float *data);
int32_t sprs_hip_csmat_f32_transpose_view(const sprs_hip_csmat_f32 *m, sprs_hip_csmat_f32 **out);
/* drops the SpMV plan and the cached CSR form of a CSC handle after the wrapped arrays were modified in place */
int32_t sprs_hip_csmat_f32_refresh(sprs_hip_csmat_f32 *m);
/* Builds the SpMV plan now, with the per-stream arrays of `stream` (a CSC handle: of its CSR form, made and cached here): the
 * banded plan where it applies (see sprs_hip_spmv_f32), else the tile index over the handle's arrays and `stream`'s carry array.
 * An unprepared handle takes its FIRST multiply on the tile plan and builds the banded plan at the second, so on a matrix that
 * takes the banded plan call 1 and call 2 may differ in bits (within the f32 bound below), as for the f64 handle; a prepared
 * handle multiplies on one plan from the first call on.  On a matrix that stays on the tile plan preparing changes no bits.
 * Preparing is also what lets an SpMV run on a stream that is being captured into a hipGraph: there the plan and THAT
 * stream's arrays must exist already (the build allocates and synchronises), else SPRS_HIP_INVALID_ARG. */
int32_t sprs_hip_csmat_f32_prepare(sprs_hip_csmat_f32 *m, void *stream);
/* Which plan the handle's SpMV runs on (a CSC handle: its cached CSR form's): *kind = 0 none yet (no multiply, no prepare),
 * 1 the nnz-tile index, 3 the banded copy (hot columns of x from LDS); there is no kind 2 (XCD-sliced) for f32.  *plan_bytes:
 * device memory the plan holds, without per-stream scratch.  Either pointer may be NULL. */
int32_t sprs_hip_csmat_f32_spmv_plan_info(const sprs_hip_csmat_f32 *m, int32_t *kind, uint64_t *plan_bytes);
int32_t sprs_hip_csmat_f32_free(sprs_hip_csmat_f32 *m);
/* Twin of to_other_storage (csmat.rs:1405-1426) for N = f32: every output row strictly increasing, the values travel with
 * their index (bit for bit).  Complete at return. */
int32_t sprs_hip_csmat_f32_to_other_storage(const sprs_hip_csmat_f32 *m, sprs_hip_csmat_f32 **out);
/* CsMat::map (csmat.rs:1289-1305) with |&v| v as f32 / |&v| v as f64: the structure is copied, the values converted by a plain
 * cast — narrowing rounds to nearest even, overflow becomes +-inf, NaN stays NaN; widening is exact.  The result carries the
 * operand's DEVICE index widths (an f64 matrix uploaded from 2-byte host arrays gives 4-byte ones).  Complete at return. */
int32_t sprs_hip_csmat_f32_from_f64(const sprs_hip_csmat *m, sprs_hip_csmat_f32 **out, void *stream);
int32_t sprs_hip_csmat_f32_to_f64(const sprs_hip_csmat_f32 *m, sprs_hip_csmat **out, void *stream);

/* Twin of prod::mul_acc_mat_vec_csr (prod.rs:103-127; accumulate != 0) and of `&A * &x` on a zeroed result (accumulate == 0)
 * for N = f32.  x_dev / y_dev: x_len / y_len floats.  SPRS_HIP_DIM_MISMATCH unless A.cols == x_len && A.rows == y_len, then
 * SPRS_HIP_STORAGE_MISMATCH unless A is CSR.  Asynchronous on `stream`.  Every product is rounded to f32, then added in f32;
 * no float atomics: deterministic run to run on either plan.  Empty rows: the accumulate form leaves y[r] untouched, the other
 * writes +0.0f.
 * TILE plan (option spmv_tile): a row (or the part of a row inside one 2048- / 4096-entry tile of the nnz axis) of fewer than 64
 * entries is summed left to right from 0.0f — the reference's chain, bit for bit, when the row lies inside one tile; a longer
 * one by a wave (tree); a row that spans tiles adds its parts in tile order.  Only SHORT ROWS ON THE TILE PLAN keep the reference
 * chain's bits.
 * BANDED plan (the f64 SpMV's, with float values, x, partial sums and carries; hot slices of 8192, 16384 or 32768 labels: option
 * spmv_f32_band_tile; the other spmv_band* options apply as for f64, spmv_band_pack is ignored): the sums of a row are formed
 * in the plan's fixed order — entry order in a lane, lanes, tiles, ranges, pieces — and agree with the chain to the forward
 * bound gamma_m * sum |a x| of m - 1 f32 additions, not bit for bit.  Taken when spmv_band = 1, or under spmv_band = 0 from the
 * handle's second multiply (or sprs_hip_csmat_f32_prepare) on, for matrices with cols * 4 >= 4 MiB, nnz >= 2^22 and at least half
 * the entries in long rows; dropped silently under auto when the memory for it is not there.  spmv_band = 2: tile plan only.
 * So call 1 and call 2 of an unprepared handle may differ in bits on a matrix that takes the banded plan, as for f64.
 * There is no XCD-sliced plan for f32. */
int32_t sprs_hip_spmv_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len,
                          float *y_dev, uint64_t y_len, int32_t accumulate, void *stream);
/* the CSC accumulate form (prod.rs:74-99) and the either-storage operator `&A * &x`: a CSC handle multiplies through its CSR
 * form, converted once and cached in the handle (dropped by _refresh / _free) */
int32_t sprs_hip_mul_acc_mat_vec_csc_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len, float *y_dev,
                                         uint64_t y_len, void *stream);
int32_t sprs_hip_csmat_mul_vec_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len, float *y_dev,
                                   uint64_t y_len, void *stream);

/* Twin of BiCGSTAB::<f32>::solve (bicgstab.rs:148-171, instantiated at :305): sprs_hip_bicgstab_f64 with every vector, dot
 * product and host scalar (alpha, omega, beta, rho, err; sqrt) in f32, in the reference's expression order.  x0_dev, b_dev,
 * x_dev: n floats.  tol and soft_restart_threshold are f32 values that TRAVEL AS double (every f32 is exactly a double) and
 * are narrowed by a plain cast on entry.  Serial dots for n <= 2048 — with the SpMV's short-row chain the reference's own
 * test_bicgstab_f32 system reproduces bit for bit — the fixed two-level tree above.  info->err / info->rho hold the f32
 * values widened exactly. */
int32_t sprs_hip_bicgstab_f32(sprs_hip_csmat_f32 *a, const float *x0_dev, const float *b_dev, uint64_t n,
                              double tol, uint64_t max_iter, double soft_restart_threshold, float *x_dev,
                              sprs_hip_bicgstab_info *info, void *stream);

/* ---- f32 SpMM: the dense products of an f32 matrix ----------------------------------------------------------------------
 * The reference's dense kernels are generic over the scalar (prod.rs:189-298 over MulAcc, mul_acc.rs:17-31; dispatch at
 * csmat.rs:1989-2117).  The four entries below are the f32 twins of sprs_hip_spmm_rowmaj_f64, sprs_hip_csmat_mulacc_dense_f64,
 * sprs_hip_csmat_mul_dense_f64 and sprs_hip_dense_dot_csmat_f64: the same argument order, checks, statuses and texts, with
 * `float *` operands (leading dimensions in ELEMENTS).  Every product is rounded to f32 and added in f32, multiply and add
 * unfused; no atomics, the same bits from call to call.  The summation order is the entry-stream kernel's (runs of
 * consecutive entries in entry order, joined in run and tile order) — not the reference's single chain, unless option
 * spmm_long_row = L > 0 asks for that chain for rows of <= L entries.  Options spmm_stream, spmm_long_row and spmm_relayout
 * act as documented for f64; option spmm_f32_pair picks the lane form of the f32 stream kernel: paired lanes (two adjacent
 * columns per lane, one 8-byte gather) are ELIGIBLE where the rhs the kernel reads has unit column stride, an even row pitch
 * and an 8-byte aligned base — always so for the re-laid-out copy — and scalar lanes run elsewhere; 1 (default) takes the
 * paired form where it is eligible and was measured faster (column groups of 32 / 64, matrices of >= 8 entries per row), 2
 * wherever it is eligible, 0 never. */

/* Twin of prod::csr_mulacc_dense_rowmaj (prod.rs:189-214) for N = f32: out[i, :] += A[i, c] * rhs[c, :] (accumulate != 0) or
 * the same on a zeroed `out`.  rhs_dev: rhs_rows x k floats, row-major, leading dimension ld_rhs (>= k); out_dev: out_rows x k,
 * leading dimension ld_out.  SPRS_HIP_DIM_MISMATCH unless A.cols == rhs_rows && A.rows == out_rows, then
 * SPRS_HIP_STORAGE_MISMATCH unless A is CSR (prod.rs:199-202).  Asynchronous on `stream`; deterministic. */
int32_t sprs_hip_spmm_rowmaj_f32(const sprs_hip_csmat_f32 *a, const float *rhs_dev, uint64_t rhs_rows,
                                 uint64_t k, uint64_t ld_rhs, float *out_dev, uint64_t out_rows,
                                 uint64_t ld_out, int32_t accumulate, void *stream);

/* The four dense kernels of prod.rs in one entry for N = f32: csr_mulacc_dense_rowmaj / _colmaj (prod.rs:189-214, 274-298) and
 * csc_mulacc_dense_rowmaj / _colmaj (prod.rs:219-270).  lhs in either storage (CSC through the cached CSR form), rhs
 * (rhs_rows x k) and out (out_rows x k) each in the layout its tag names with leading dimension ld in floats (row-major: >= k,
 * column-major: >= rows).  Column-major x column-major with k < 8 runs column by column through sprs_hip_spmv_f32's kernel.
 * SPRS_HIP_DIM_MISMATCH unless lhs.cols == rhs_rows && lhs.rows == out_rows (prod.rs:199-201, 228-230, 257-259, 284-289);
 * SPRS_HIP_INVALID_ARG for a bad layout tag, a leading dimension smaller than the extent it strides over, a NULL matrix, or an
 * `out` that shares an element with `rhs` (two views of one buffer with the same layout and pitch whose lines fall into each
 * other's gaps are accepted). */
int32_t sprs_hip_csmat_mulacc_dense_f32(const sprs_hip_csmat_f32 *lhs, const float *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                        int32_t rhs_layout, uint64_t ld_rhs, float *out_dev, uint64_t out_rows,
                                        int32_t out_layout, uint64_t ld_out, int32_t accumulate, void *stream);

/* Twin of `&CsMat * &Array2` / `CsMat::dot(&Array2)` (csmat.rs:1989-2048, 2119-2137) for N = f32.  out_dev: lhs.rows x k floats,
 * contiguous; written in the layout the reference allocates — row-major for k >= 8 (csmat.rs:2002-2016), column-major (`.f()`,
 * csmat.rs:2017-2045) below — which *out_layout reports. */
int32_t sprs_hip_csmat_mul_dense_f32(const sprs_hip_csmat_f32 *lhs, const float *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                     int32_t rhs_layout, uint64_t ld_rhs, float *out_dev, int32_t *out_layout, void *stream);

/* Twin of `Array2::dot(&CsMat)` (csmat.rs:2050-2117) for N = f32: lhs (lhs_rows x lhs_cols, dense) . rhs (sparse) as
 * (rhs^T lhs^T)^T with the reference's free transposes.  out_dev: lhs_rows x rhs.cols floats, contiguous, in the layout
 * *out_layout reports.  A CSR rhs is converted once to CSC (cached in the handle); the transpose view and its plans stay in the
 * rhs handle until _refresh / _free. */
int32_t sprs_hip_dense_dot_csmat_f32(const float *lhs_dev, uint64_t lhs_rows, uint64_t lhs_cols, int32_t lhs_layout,
                                     uint64_t ld_lhs, const sprs_hip_csmat_f32 *rhs, float *out_dev, int32_t *out_layout,
                                     void *stream);

/* ---- f32 SpGEMM: CsMat<f32> times CsMat<f32> ----------------------------------------------------------------------------
 * smmp::mul_csr_csr is generic over the scalar (smmp.rs:196-416).  The eight entries below are the f32 twins of
 * sprs_hip_spgemm_f64, sprs_hip_spgemm_symbolic / _numeric, the five plan entries that read a matrix, and
 * sprs_hip_csmat_mul_csmat: the same argument order, checks, statuses and texts, on sprs_hip_csmat_f32 handles.
 * Structure: indptr and indices equal the reference's (every reachable column, structural zeros kept, rows sorted).
 * Values: every C(i,j) starts at +0.0f; each product a*b is rounded to f32 and added, unfused, one at a time in ascending
 * position of k in A's row — the reference's f32 chain, bit for bit (an f64 product rounded once at the end is NOT that).
 * Subnormals are kept.  Deterministic; option spgemm_ordered = 0 frees the order of the adds in the large-row kernel exactly
 * as for f64.  The value walks read one 8-byte {column, float} record of B per product (f64: 16 bytes).
 * A sprs_hip_spgemm_plan holds STRUCTURE only (task lists, counts, offsets, the column-bucket table of B; the records of B are
 * packed per call): sprs_hip_spgemm_plan_nnz and _plan_free serve both precisions, and a plan made by either _plan_create
 * serves handles of the OTHER precision wrapped over the same indptr / indices device arrays (the plan matches operands by
 * shape, index widths and those two pointers per operand).  Mixing precisions in one call is impossible by type. */
int32_t sprs_hip_spgemm_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 **c);
/* structure only: an f32 matrix whose values are 0.0f */
int32_t sprs_hip_spgemm_symbolic_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b,
                                     sprs_hip_csmat_f32 **c_structure);
int32_t sprs_hip_spgemm_numeric_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 *c);
int32_t sprs_hip_spgemm_plan_create_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b,
                                        sprs_hip_spgemm_plan **plan);
int32_t sprs_hip_spgemm_plan_structure_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a,
                                           const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 **c_structure);
int32_t sprs_hip_spgemm_plan_product_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a,
                                         const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 **c);
int32_t sprs_hip_spgemm_plan_numeric_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a,
                                         const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 *c);
/* `&lhs * &rhs` in any pair of storages (csmat.rs:1895-1949) through sprs_hip_csmat_f32_to_other_storage and the free
 * transpose views; the result has the storage of the lhs */
int32_t sprs_hip_csmat_mul_csmat_f32(const sprs_hip_csmat_f32 *lhs, const sprs_hip_csmat_f32 *rhs,
                                     sprs_hip_csmat_f32 **out);

/* ---- f32 triangular solves, Gauss-Seidel and diag_solve -----------------------------------------------------------------
 * The recurrences of the reference are generic over the scalar (trisolve.rs:30-262 over N: Num; the heat example's
 * gauss_seidel and linalg::diag_solve alike).  The three entries below are the f32 twins of sprs_hip_trisolve_f64,
 * sprs_hip_gauss_seidel_f64 and sprs_hip_diag_solve_f64: the same argument order, checks, statuses, texts and info structs,
 * on a sprs_hip_csmat_f32 handle and arrays of n floats.  Every product, every subtraction / addition and the division are
 * rounded to f32 (multiply and add unfused, IEEE division, subnormals kept), in the reference's entry order: the solutions
 * and the iterates are the reference's f32 bits — an f64 solve rounded at the end is NOT that.  The level plans are the f64
 * ones (they read structure only), kept in the f32 handle and dropped by _refresh / _free; a CSC handle is solved on its
 * cached CSR form.  On the device a value is handed from row to row as one 4-byte word that is both value and "ready".
 * Singular: a stored diagonal == 0.0f (-0.0f counts, NaN does not) or one that is not stored, reported as for f64.
 * Gauss-Seidel: eps is an f32 value that TRAVELS AS double and is narrowed by a plain cast; the convergence scalar is
 * sqrt(sum_i ((A x)_i - rhs_i)) in f32 — A x by sprs_hip_spmv_f32 on the handle's own plan, then a fixed tree sum — and
 * info->error holds it widened exactly.  Option gauss_seidel_chain > 1 (the band schedule) is f64-only: an f32 sweep with it
 * set returns SPRS_HIP_INVALID_ARG.  There is no f32 LDL^T and no f32 sparse-rhs solve. */
int32_t sprs_hip_trisolve_f32(sprs_hip_csmat_f32 *a, int32_t uplo, float *x_dev, uint64_t n,
                              sprs_hip_trisolve_info *info, void *stream);
int32_t sprs_hip_gauss_seidel_f32(sprs_hip_csmat_f32 *a, float *x_dev, const float *rhs_dev, uint64_t n,
                                  uint64_t max_iter, double eps, sprs_hip_gauss_seidel_info *info,
                                  void *stream);
int32_t sprs_hip_diag_solve_f32(const float *d_dev, float *x_dev, uint64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPRS_HIP_H */
