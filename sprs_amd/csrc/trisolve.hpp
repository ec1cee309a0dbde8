// Device sparse triangular solves with a dense right-hand side — twins of sprs::linalg::trisolve
//   lsolve_csr_dense_rhs   sprs/src/sparse/linalg/trisolve.rs:30-73
//   lsolve_csc_dense_rhs   trisolve.rs:85-149
//   usolve_csc_dense_rhs   trisolve.rs:161-210
//   usolve_csr_dense_rhs   trisolve.rs:219-262
// Included by gauss_seidel.hip, inside namespace sprs_hip and after its helpers (one translation unit of the library and of the
// emulator build, tests/emu): a Gauss-Seidel sweep is a lower triangular solve with extra terms from the previous iterate, and
// this is that sweep without them.  Shared with it: the level plan (gs_plan_build; lower = the sweep's own order, upper = its
// mirror), gs_peek / gs_draw / gs_spin_guard, the batch of GS_B operands requested together, the data-tagged hand-off (GsWord<T>:
// 8-byte granules for f64, 4-byte granules for f32).
//
// ONE ROW-ORIENTED KERNEL FOR THE FOUR SOLVES.  Every solve gives unknown r the chain
//     x_r = (b_r - v_1 x_c1 - v_2 x_c2 - ...) / diag_r        (each product rounded, then each subtraction: trisolve.rs:62, 140)
// and the reference fixes the order of the c_k (the other triangle is skipped: trisolve.rs:59-61, 137-139, 196-198, 248-250):
//   lsolve_csr: the stored entries of row r with c < r, in stored order                          -> lower, forward walk of row r
//   usolve_csr: the stored entries of row r with c > r, in stored order                          -> upper, forward walk
//   lsolve_csc: columns are processed 0 .. n-1 and scatter into the rows, so row r receives its
//               products by ASCENDING c: the forward walk of row r of the CSR form                -> lower, forward walk
//   usolve_csc: columns n-1 .. 0 (trisolve.rs:184): row r receives them by DESCENDING c           -> upper, BACKWARD walk
// (usolve_csr and usolve_csc therefore differ in bits on the same matrix; the walk direction is part of the contract.)
// A CSC handle is solved on its cached CSR form (as_other), where the plans then live.  Column indices are assumed sorted
// inside each row, as every validated handle has them (the walk stops at the diagonal where the direction allows it).
//
// Values travel through a work vector of n granules that the host fills with GS_PENDING: a lane owns a row, requests the
// operands of a batch together with 8-byte agent-scope loads, subtracts the products in entry order once the whole batch has
// arrived, divides by the diagonal and publishes the result with ONE 8-byte agent-scope store (value and "ready" are the same
// granule).  b_r is read from x by the lane that owns row r and by nobody else, so the same lane also stores the result there.
//
// Singular rows (diagonal not stored, or == 0; -0.0 counts, NaN does not: trisolve.rs:64, 127, 186, 253): the reference
// returns at the first one in ITS order — the smallest index for the lower solves, the largest for the upper ones.  Here such a
// row records (index << 1 | structural) with atomicMin (lower) / atomicMax (upper), publishes a quiet NaN so that its
// dependents finish, and the host turns the word into SPRS_HIP_SINGULAR_MATRIX; x is unspecified then.
#pragma once

namespace {

constexpr unsigned int TS_SINGULAR = 4u;                      // status bit beside GS_NO_DIAG / GS_TIMEOUT
constexpr unsigned long long TS_ABSENT = GsWord<double>::ABSENT;      // SPARSE: "this unknown is not part of the solve" (a second NaN no arithmetic yields)

// UNIT: the diagonal is 1 and not stored (the factor L of ldl.hpp: ldl_lsolve / ldl_ltsolve, sprs-ldl/src/lib.rs:595-626); a row
// is then its chain of subtractions, never divided and never singular.
// SPARSE: `order` holds a SUBSET of the unknowns (the reach of a sparse right-hand side, sptrisolve.hpp) and the work vector
// tells three states apart: GS_PENDING (in the subset, not solved yet), a value, and TS_ABSENT (not in the subset: the unknown
// is exactly zero).  An absent operand counts as arrived and its product is SKIPPED — not multiplied by 0.0, which would turn
// a stored inf or NaN of that column into a NaN.  Off, the kernel compiles to what it was.
// T = the scalar of the values, of x and of the arithmetic: every product, every subtraction and the division are rounded to T.
// `work` is declared as the f64 code always had it (its symbols must not move); what it addresses is one GsWord<T>::word per
// unknown: 8-byte words for double, 4-byte words for float.  UNIT and SPARSE are instantiated for double only.
template <typename IDX, typename PTR, bool UPPER, bool BACKWARD, bool UNIT = false, bool SPARSE = false, typename T = double>
__global__ __launch_bounds__(GS_BLOCK) void tri_solve_kernel(const PTR *__restrict__ indptr, const IDX *__restrict__ indices,
                                                             const T *__restrict__ data, const uint32_t *__restrict__ order,
                                                             T *x, unsigned long long *work, uint64_t n,
                                                             unsigned int *next_chunk, unsigned int *status,
                                                             unsigned long long *singular, uint32_t structural) {
    // sorted rows: the wanted triangle ends at the first entry on or past the diagonal in walk direction
    constexpr bool STOP_AT_DIAG = UPPER == BACKWARD;
    using W = GsWord<T>;
    typename W::word *const granule = (typename W::word *)work;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = gs_draw(next_chunk, lane); base < n; base = gs_draw(next_chunk, lane)) {
        const uint64_t pos = base + lane;
        bool done = pos >= n;
        uint32_t row = 0;
        uint64_t p = 0, end = 0;                               // entries not walked yet: [p, end), taken from the front (BACKWARD: from the back)
        T acc = T(0);
        if (!done) {
            row = order[pos];
            p = (uint64_t)indptr[row];
            end = (uint64_t)indptr[row + 1];
            acc = x[row];                                      // b_r (trisolve.rs:53, 133, 192, 242)
        }
        T diag = T(0);
        bool has_diag = false, last = false;
        uint32_t col[GS_B];
        T val[GS_B], xv[GS_B];
        uint32_t nb = 0, pend = 0, spins = 0, absent = 0;
        bool loaded = false, more = true;
        while (more) {
            bool moved = false;
            if (!done) {
                if (!loaded) {                                 // the next (up to) eight entries of my row, in walk order
                    nb = end - p < (uint64_t)GS_B ? (uint32_t)(end - p) : (uint32_t)GS_B;
#pragma unroll
                    for (int u = 0; u < GS_B; ++u)
                        if ((uint32_t)u < nb) {
                            const uint64_t at = BACKWARD ? end - 1 - (uint64_t)u : p + (uint64_t)u;
                            col[u] = (uint32_t)indices[at];
                            val[u] = data[at];
                        }
                    if (BACKWARD) end -= nb;
                    else p += nb;
                    uint32_t touch = 0;                        // (the column ids are needed now: see gs_sweep_kernel)
#pragma unroll
                    for (int u = 0; u < GS_B; ++u)
                        if ((uint32_t)u < nb) touch |= col[u];
                    GS_TOUCH(touch);
                    pend = 0;
                    absent = 0;
#pragma unroll
                    for (int u = 0; u < GS_B; ++u)
                        if ((uint32_t)u < nb && (UPPER ? col[u] > row : col[u] < row)) pend |= 1u << u;
                    loaded = true;
                    moved = true;
                }
                // the poll: the operands of the batch that have not arrived yet, all requested together
                typename W::word bits[GS_B];
#pragma unroll
                for (int u = 0; u < GS_B; ++u)
                    if ((pend >> u) & 1u) bits[u] = gs_peek(granule + col[u]);
#pragma unroll
                for (int u = 0; u < GS_B; ++u)
                    if (((pend >> u) & 1u) && bits[u] != W::PENDING) {
                        xv[u] = W::value(bits[u]);
                        if (SPARSE && bits[u] == W::ABSENT) absent |= 1u << u;
                        pend &= ~(1u << u);
                        moved = true;
                    }
                if (pend == 0u) {                              // every operand of the batch is here: subtract in entry order
#pragma unroll
                    for (int u = 0; u < GS_B; ++u)
                        if ((uint32_t)u < nb) {
                            const uint32_t c = col[u];
                            if (c == row) {
                                diag = val[u];
                                has_diag = true;
                            } else if ((UPPER ? c > row : c < row) && !(SPARSE && ((absent >> u) & 1u))) {
                                const T prod = val[u] * xv[u];
                                acc = acc - prod;
                            }
                            if (STOP_AT_DIAG && (UPPER ? c <= row : c >= row)) last = true;
                        }
                    loaded = false;
                    moved = true;
                    if (last || p == end) {
                        const T xr = UNIT ? acc : acc / diag;   // trisolve.rs:70, 134, 193, 259
                        typename W::word out = W::bits(xr);
                        if (!UNIT && (!has_diag || diag == T(0))) {
                            const unsigned long long word = ((unsigned long long)row << 1) | (has_diag ? 0ull : (unsigned long long)structural);
                            if (UPPER) atomicMax(singular, word);
                            else atomicMin(singular, word);
                            atomicOr(status, TS_SINGULAR);
                            out = W::QNAN;
                        } else {
                            x[row] = xr;
                        }
                        if (out == W::PENDING || (SPARSE && out == W::ABSENT)) out = W::QNAN;   // (a NaN payload handed through from b: still a NaN, but not "pending")
                        __hip_atomic_store(granule + row, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        done = true;
                    }
                }
            }
            more = __ballot(!done) != 0ull;
            if (more && gs_spin_guard(moved, spins, status, 1u)) return;
        }
    }
}

// one solve over arrays in CSR form, rows taken in `order`: the launch and the read-back of the status words into hw
// ([0] chunks drawn, [1] status, [2..3] the singular word)
// (T is deduced from the values; the unit-diagonal form is LDL^T's and exists for double only)
template <typename IDX, typename PTR, typename T>
int32_t tri_run(const void *indptr, const void *indices, const T *data, const uint32_t *order, bool upper, bool csc, bool unit,
                T *x, uint64_t n, unsigned int *hw, hipStream_t stream) {
    DevBuf work, words;
    StreamDrain drain{stream};
    SPRS_TRY_HIP(work.alloc(n * sizeof(T)));
    SPRS_TRY_HIP(words.alloc(64));
    SPRS_TRY_HIP(hipMemsetAsync(work.p, 0xFF, n * sizeof(T), stream));      // every unknown "pending"
    SPRS_TRY_HIP(hipMemsetAsync(words.p, 0, 64, stream));
    if (!upper) SPRS_TRY_HIP(hipMemsetAsync(words.as<unsigned int>() + 2, 0xFF, 8, stream));   // atomicMin starts from the top
    unsigned int *w = words.as<unsigned int>();

    int ncu = 0, dev = 0;
    SPRS_TRY_HIP(hipGetDevice(&dev));
    SPRS_TRY_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    // one workgroup per CU, capped by need: waves beyond the front of the level order only add polls (see gs_impl)
    const uint64_t need = (n + GS_BLOCK - 1) / GS_BLOCK;
    uint64_t grid = (uint64_t)(ncu > 0 ? ncu : 1);
    if (grid > need) grid = need;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(GS_BLOCK), 0, stream, (const PTR *)indptr, (const IDX *)indices, data, order, x,
                           (unsigned long long *)work.p, n, w, w + 1, (unsigned long long *)(w + 2), csc ? 1u : 0u);
    };
    if (unit) {
        if constexpr (std::is_same<T, double>::value) {
            if (!upper) launch(tri_solve_kernel<IDX, PTR, false, false, true>);
            else launch(tri_solve_kernel<IDX, PTR, true, false, true>);
        } else {
            SPRS_FAIL(SPRS_HIP_INVALID_ARG, "triangular solve: the unit-diagonal form is built for f64 only");
        }
    } else if (!upper) launch(tri_solve_kernel<IDX, PTR, false, false, false, false, T>);
    else if (csc) launch(tri_solve_kernel<IDX, PTR, true, true, false, false, T>);
    else launch(tri_solve_kernel<IDX, PTR, true, false, false, false, T>);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(copy_to_host(hw, words.p, 4 * sizeof(unsigned int), stream));
    return SPRS_HIP_OK;
}

template <typename IDX, typename PTR, typename H>
int32_t trisolve_impl(H *a, bool upper, bool csc, typename H::value_type *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    // held from the look-up of the row order to the end of the (blocking) solve, the way gs_impl holds it
    std::lock_guard<std::recursive_mutex> lock(a->mu);
    GsPlan &pl = upper ? a->tri_upper : a->gs;                 // lower: exactly the Gauss-Seidel order
    if (!pl.built) SPRS_TRY(upper ? (gs_plan_build<IDX, PTR, true>(a, pl)) : (gs_plan_build<IDX, PTR, false>(a, pl)));
    if (info) info->levels = pl.nlevels;

    unsigned int hw[4] = {0, 0, 0, 0};
    SPRS_TRY((tri_run<IDX, PTR>(a->indptr, a->indices, (const typename H::value_type *)a->data, pl.order, upper, csc, false, x, n, hw, stream)));
    if ((uint64_t)hw[0] * 64u < n)
        SPRS_FAIL(SPRS_HIP_HIP_ERROR, "triangular solve: only %llu of %llu rows were solved", (unsigned long long)hw[0] * 64ull, (unsigned long long)n);
    if (hw[1] & GS_TIMEOUT)
        SPRS_FAIL(SPRS_HIP_HIP_ERROR, "triangular solve: a row waited for a value that was never published (level order broken)");
    if (hw[1] & TS_SINGULAR) {
        unsigned long long word = 0;
        memcpy(&word, hw + 2, 8);
        const uint64_t index = word >> 1;
        const bool structural = (word & 1ull) != 0ull;
        if (info) {
            info->singular_index = index;
            info->singular_reason = structural ? 2 : 1;
        }
        // the reasons as the four functions spell them: trisolve.rs:67, 130, 145, 189, 204, 256
        const char *reason = structural ? "diagonal element is a structural 0"
                             : (csc || upper) ? "diagonal element is a numeric 0"
                                              : "diagonal element is 0";
        SPRS_FAIL(SPRS_HIP_SINGULAR_MATRIX, "Singular matrix at index %llu (%s)", (unsigned long long)index, reason);   // errors.rs:87-92
    }
    return SPRS_HIP_OK;
}

template <typename H>
int32_t trisolve_entry(H *csr, bool upper, bool csc, typename H::value_type *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return dispatch_widths(csr->idx_bytes, csr->iptr_bytes, [&](auto i, auto p) {
        return trisolve_impl<typename decltype(i)::type, typename decltype(p)::type>(csr, upper, csc, x, n, info, stream);
    });
}

}  // namespace

int32_t trisolve_f64(sprs_hip_csmat *csr, bool upper, bool csc, double *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return trisolve_entry(csr, upper, csc, x, n, info, stream);
}
int32_t trisolve_f32(sprs_hip_csmat_f32 *csr, bool upper, bool csc, float *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return trisolve_entry(csr, upper, csc, x, n, info, stream);
}
