// Device sparse triangular solve with a SPARSE right-hand side — twin of sprs::linalg::trisolve::lsolve_csc_sparse_rhs
//   lsolve_csc_sparse_rhs      sprs/src/sparse/linalg/trisolve.rs:286-358
//   lspsolve_csc_process_col   trisolve.rs:114-149
// Included by gauss_seidel.hip, inside namespace sprs_hip and after trisolve.hpp (one translation unit of the library and of the
// emulator build, tests/emu): the solve is tri_solve_kernel over a subset of the unknowns.
//
// The reference (a) finds the REACH of the right-hand side — every column that a depth-first search over the columns of L gets to
// from a stored index of rhs (stored zeros are roots too; every stored entry of a column is followed, the diagonal and entries
// above it included) — and leaves its post-order in a stack, then (b) scatters rhs into a dense workspace and runs
// lspsolve_csc_process_col over the stack: x_c = x_c / diag_c, then x_r -= val * x_c for the stored rows r > c.
// The cost follows the reach, not n.  So does this one: after the first solve on a handle no step makes a pass over n or nnz(L).
//
// WHERE THE DEVICE TWIN DIFFERS
//  (a) Order and bits.  The reverse post-order of a lexicographic DFS cannot be computed in parallel; the reach is the same SET,
//      so the pattern comes back sorted ascending, in a new CsVec handle (a valid CsVec; the reference leaves an unsorted stack
//      and a dense workspace).  Unknown r receives its products by ASCENDING column: the reference's arithmetic — each product
//      rounded, then each subtraction, then one division — with its columns processed in ascending order.  Whenever that
//      arithmetic is exact the result is bit-identical to the reference's; on general values it can differ in the last bits
//      where a row receives two or more products.
//  (b) Workspace.  The reference only scatters rhs: a fill-in unknown (in the reach, not stored in rhs) starts from whatever
//      x_workspace held.  Here it starts from +0.0, the solve the documentation describes.
//  (c) Singular report.  The reference returns at the first singular column in its DFS order; here the SMALLEST singular index
//      of the reach is reported, with that column's reason ("a structural 0" / "a numeric 0"; -0.0 counts as zero, NaN does
//      not).  A singular column OUTSIDE the reach is not an error: that is where this solve differs from the dense one.
//  Columns outside the reach contribute nothing: an inf or NaN stored at (r, c), r in the reach and c not, never meets x_r (the
//  reader skips the product; a published 0.0 would make inf * 0 = NaN of it).
//
// 1. REACH: a breadth-first closure over the handle's own CSC arrays.  A bitmap of ceil(n / 32) words; atomicOr claims a vertex
//    and the lane that flips the bit appends it to ONE queue, whose tail q[fb, fe) is the frontier of a level.  The set is
//    deterministic, the order of the queue is not, and nothing depends on it.  sp_reach_narrow_kernel is one workgroup that runs
//    level after level out of LDS (workgroup barriers only) until a frontier has more than SP_NARROW_MAX vertices or
//    SP_NARROW_ENTRIES stored entries, or `sptrisolve_budget` levels are done; a wide level runs as a grid tiled on the ENTRIES
//    of the frontier's columns (lengths -> scan -> sp_expand_kernel), so a hub column is shared among waves.  No kernel waits
//    for another workgroup.  A chain of depth d costs ceil(d / budget) launches and read-backs.
// 2. PATTERN: two radix sorts of the queue — by index (the result's pattern) and by position in the handle's lower level plan
//    (pos[v], the inverse of GsPlan::order, made once per handle): the level order restricted to the reach is a level order.
// 3. SOLVE: tri_solve_kernel<.., SPARSE> (lower, forward walk, CSR form) over the restricted order; the work vector says
//    "pending" for the reach and "absent" everywhere else.  b_r is the rhs value, +0.0 for fill-in.
// 4. RESULT: x gathered over the sorted pattern into a new owning CsVec of L's declared index width, numeric zeros kept; the
//    same kernel puts the words and granules of the pattern back to "clean".
#pragma once

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_NARROW_MAX = 1024;                 // frontier vertices the narrow kernel keeps in LDS
constexpr int SP_NARROW_PER = SP_NARROW_MAX / SP_BLOCK;
constexpr int SP_NARROW_ENTRIES = 4096;             // stored entries of a frontier's columns the narrow kernel takes
constexpr int SP_EXPAND = 4;                        // entries a lane of the narrow kernel has in flight together
constexpr int SP_TILE = 2048;                       // entries per workgroup of the wide expansion
constexpr int SP_ITEMS = SP_TILE / SP_BLOCK;

enum : uint64_t { SP_WHY_BUDGET = 0, SP_WHY_WIDE = 1, SP_WHY_DONE = 2 };

// The state of the reach.  It lives in device memory between launches; the host reads it back after every launch of the narrow
// kernel and writes it after every wide level.  cnt: the claims of a wide level (0 outside one).
struct SpState {                                    // (no initialisers: a copy of it lives in LDS)
    uint64_t fb, fe;                                // the frontier is queue[fb, fe)
    uint64_t levels, why, cnt;
};

// the stored entries of column v, inside [0, nnz) whatever the arrays hold
template <typename P>
__device__ __forceinline__ uint64_t sp_slice(const P *ip, uint64_t v, uint64_t n, uint64_t nnz, uint64_t *len) {
    *len = 0;
    if (v >= n) return 0;
    uint64_t s = (uint64_t)ip[v], e = (uint64_t)ip[v + 1];
    if (e > nnz) e = nnz;
    if (s > e) s = e;
    *len = e - s;
    return s;
}

// the lanes of a wave with `claim` set take consecutive places from *cnt: one atomic per wave
__device__ __forceinline__ uint64_t sp_wave_append(bool claim, unsigned long long *cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask = __ballot(claim);
    unsigned long long first = 0;
    if (lane == 0 && mask) first = atomicAdd(cnt, (unsigned long long)__popcll(mask));
    first = __shfl(first, 0, 64);
    return first + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// the roots: every stored index of rhs (a stored 0.0 too, trisolve.rs:322), its value scattered into b
template <typename VI>
__global__ void __launch_bounds__(SP_BLOCK) sp_roots_kernel(const VI *vidx, const double *vdata, uint64_t nnz, uint64_t n, uint32_t *bits,
                                                            uint32_t *queue, double *b, SpState *state) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    bool claim = false;
    uint64_t k = 0;
    if (i < nnz) {
        k = (uint64_t)vidx[i];
        if (k < n) {                                 // (checked at upload; keeps a borrowed, unchecked vector inside the arrays)
            b[k] = vdata[i];
            const uint32_t bit = 1u << (k & 31u);
            claim = (atomicOr(&bits[k >> 5], bit) & bit) == 0u;
        }
    }
    const uint64_t at = sp_wave_append(claim, (unsigned long long *)&state->fe);
    if (claim && at < n) queue[at] = (uint32_t)k;
}

template <typename P, typename I>
__global__ void __launch_bounds__(SP_BLOCK) sp_reach_narrow_kernel(const P *ip, const I *ix, uint64_t n, uint64_t nnz, uint32_t *bits, uint32_t *queue,
                                                                   SpState *state, uint64_t budget) {
    __shared__ SpState st;
    __shared__ uint32_t s_front[2][SP_NARROW_MAX];  // the frontier, and the one being claimed
    __shared__ uint32_t s_off[SP_NARROW_MAX + 1];   // exclusive scan of its columns' lengths
    __shared__ uint64_t s_start[SP_NARROW_MAX];     // where each of its columns starts in ix
    __shared__ uint32_t s_wt[16];
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        st = *state;
        st.why = SP_WHY_BUDGET;
    }
    __syncthreads();
    uint32_t cur = 0;
    bool front_lds = false;                         // s_front[cur] holds queue[fb, fe)
    for (uint64_t step = 0; step < budget; ++step) {
        const uint64_t fb = st.fb, fe = st.fe, F = fe - fb;
        __syncthreads();
        if (F == 0 || F > (uint64_t)SP_NARROW_MAX) {
            if (tid == 0) st.why = F == 0 ? SP_WHY_DONE : SP_WHY_WIDE;
            break;
        }
        if (!front_lds)                              // written by an earlier launch (the roots, a wide level)
            for (uint64_t s = tid; s < F; s += SP_BLOCK) s_front[cur][s] = queue[fb + s];
        __syncthreads();
        uint32_t len[SP_NARROW_PER], sum = 0;
#pragma unroll
        for (int i = 0; i < SP_NARROW_PER; ++i) {
            const uint64_t s = (uint64_t)tid * SP_NARROW_PER + i;
            uint64_t l = 0, s0 = 0;
            if (s < F) s0 = sp_slice(ip, (uint64_t)s_front[cur][s], n, nnz, &l);
            s_start[tid * SP_NARROW_PER + i] = s0;
            len[i] = (uint32_t)(l < (uint64_t)SP_NARROW_ENTRIES + 1 ? l : (uint64_t)SP_NARROW_ENTRIES + 1);
            sum += len[i];
        }
        uint32_t E;
        uint32_t base = block_excl_scan_u32(sum, s_wt, &E);
#pragma unroll
        for (int i = 0; i < SP_NARROW_PER; ++i) {
            s_off[tid * SP_NARROW_PER + i] = base;
            base += len[i];
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        if (E > (uint32_t)SP_NARROW_ENTRIES) {
            if (tid == 0) st.why = SP_WHY_WIDE;
            break;
        }
        // expand: SP_EXPAND entries of the frontier's columns per lane and round, their index loads in flight together and
        // then their claims (one entry at a time a level was a chain of E / 256 x 3 dependent round trips: 14 us a level on
        // the grid Laplacian).  No length was clamped here (E <= SP_NARROW_ENTRIES), so every e < E is a stored entry.
        for (uint32_t e0 = tid; e0 < E; e0 += SP_BLOCK * SP_EXPAND) {
            uint64_t j[SP_EXPAND];
            uint32_t old[SP_EXPAND];
            bool ok[SP_EXPAND];
#pragma unroll
            for (int u = 0; u < SP_EXPAND; ++u) {
                const uint32_t e = e0 + (uint32_t)u * SP_BLOCK;
                ok[u] = e < E;
                j[u] = 0;
                if (ok[u]) {
                    uint32_t lo = 0, top = (uint32_t)F - 1;      // the last column that starts at or before entry e
                    while (lo < top) {
                        const uint32_t mid = (lo + top + 1) >> 1;
                        if (s_off[mid] <= e) lo = mid;
                        else top = mid - 1;
                    }
                    j[u] = (uint64_t)ix[s_start[lo] + (e - s_off[lo])];
                }
            }
#pragma unroll
            for (int u = 0; u < SP_EXPAND; ++u) {
                ok[u] = ok[u] && j[u] < n;
                old[u] = ~0u;
                if (ok[u]) old[u] = atomicOr(&bits[j[u] >> 5], 1u << (j[u] & 31u));
            }
#pragma unroll
            for (int u = 0; u < SP_EXPAND; ++u) {
                if (!ok[u] || ((old[u] >> (j[u] & 31u)) & 1u)) continue;
                const uint32_t at = atomicAdd(&s_cnt, 1u);
                if (fe + at < n) queue[fe + at] = (uint32_t)j[u];
                if (at < (uint32_t)SP_NARROW_MAX) s_front[cur ^ 1u][at] = (uint32_t)j[u];
            }
        }
        __syncthreads();
        const uint32_t C = s_cnt;
        front_lds = true;                            // (more than SP_NARROW_MAX claims: the next round hands over before it reads them)
        cur ^= 1u;
        if (tid == 0) {
            st.fb = fe;
            st.fe = fe + C;
            st.levels += 1;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) *state = st;
}

// ---- one wide level ---------------------------------------------------------------------------------------------------------------
template <typename P>
__global__ void __launch_bounds__(SP_BLOCK) sp_front_len_kernel(const P *ip, const uint32_t *front, uint64_t F, uint64_t n, uint64_t nnz, uint64_t *lens) {
    const uint64_t s = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (s >= F) return;
    uint64_t len;
    (void)sp_slice(ip, (uint64_t)front[s], n, nnz, &len);
    lens[s] = len;
}

// a tile of SP_TILE entries of the frontier's columns (offs = exclusive scan of their lengths, E entries in all); the claims go
// behind the frontier, queue[fe ...]
template <typename P, typename I>
__global__ void __launch_bounds__(SP_BLOCK) sp_expand_kernel(const P *ip, const I *ix, const uint32_t *front, uint64_t F, const uint64_t *offs, uint64_t E,
                                                             uint64_t n, uint64_t nnz, uint64_t fe, uint32_t *bits, uint32_t *queue, SpState *state) {
    const uint64_t k0 = (uint64_t)blockIdx.x * SP_TILE;
    for (int it = 0; it < SP_ITEMS; ++it) {
        const uint64_t e = k0 + (uint64_t)(it * SP_BLOCK) + threadIdx.x;
        bool claim = false;
        uint64_t j = 0;
        if (e < E) {
            uint64_t lo = 0, top = F - 1;            // the last column that starts at or before entry e
            while (lo < top) {
                const uint64_t mid = (lo + top + 1) >> 1;
                if (offs[mid] <= e) lo = mid;
                else top = mid - 1;
            }
            uint64_t len;
            const uint64_t s = sp_slice(ip, (uint64_t)front[lo], n, nnz, &len);
            if (e - offs[lo] < len) {
                j = (uint64_t)ix[s + (e - offs[lo])];
                if (j < n) {
                    const uint32_t bit = 1u << (j & 31u);
                    claim = (atomicOr(&bits[j >> 5], bit) & bit) == 0u;
                }
            }
        }
        const uint64_t at = fe + sp_wave_append(claim, (unsigned long long *)&state->cnt);
        if (claim && at < n) queue[at] = (uint32_t)j;
    }
}

// ---- pattern, order, result ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_BLOCK) sp_pos_kernel(const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ pos) {
    const uint64_t q = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (q < n) pos[order[q]] = (uint32_t)q;
}

__global__ void __launch_bounds__(SP_BLOCK) sp_fill_kernel(unsigned long long *work, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i < n) work[i] = TS_ABSENT;
}

// by_idx = (v, v), by_pos = (pos[v], v) for every v of the reach; its granule of the work vector becomes "pending"
__global__ void __launch_bounds__(SP_BLOCK) sp_keys_kernel(const uint32_t *__restrict__ queue, uint64_t R, const uint32_t *__restrict__ pos,
                                                           uint64_t *__restrict__ by_idx, uint64_t *__restrict__ by_pos, unsigned long long *work) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= R) return;
    const uint64_t v = queue[i];
    by_idx[i] = v;
    by_idx[R + i] = v;
    by_pos[i] = pos[v];
    by_pos[R + i] = v;
    work[v] = GS_PENDING;
}

__global__ void __launch_bounds__(SP_BLOCK) sp_order_kernel(const uint64_t *__restrict__ vals, uint64_t R, uint32_t *__restrict__ order) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i < R) order[i] = (uint32_t)vals[i];
}

// the result over the sorted pattern; the pattern's words and granules go back to "clean" (several lanes may store the same zero
// word: every set bit of it belongs to the pattern)
template <typename OI>
__global__ void __launch_bounds__(SP_BLOCK) sp_gather_kernel(const uint64_t *__restrict__ sorted, uint64_t R, double *b, unsigned long long *work,
                                                             uint32_t *bits, OI *oidx, double *oval) {
    const uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= R) return;
    const uint64_t v = sorted[i];
    oidx[i] = (OI)v;
    oval[i] = b[v];
    b[v] = 0.0;
    work[v] = TS_ABSENT;
    bits[v >> 5] = 0u;
}

inline unsigned sp_blocks(uint64_t n) { return n ? (unsigned)((n + SP_BLOCK - 1) / SP_BLOCK) : 1u; }

inline int sp_bits_for(uint64_t n) {                // bits needed for values < n
    int b = 1;
    while (b < 63 && (1ull << b) < n) ++b;
    return b;
}

// the scratch of the handle, made by its first sparse-rhs solve and kept until refresh / free
int32_t sp_scratch(sprs_hip_csmat *csr, uint64_t n) {
    SpTriScratch &s = csr->sp;
    if (s.bits && s.n == n) return SPRS_HIP_OK;
    s = SpTriScratch();
    SpTriScratch t;                // complete before the handle takes it
    t.n = n;
    hipError_t e = alloc_block(t.blocks, t.bits, (n + 31) / 32 * 4);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.queue, n * 4);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.work, n * 8);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.b, n * 8);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.keys, 4 * n * 8);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.words, 128);
    if (e != hipSuccess) return fail_hip(e, "sparse-rhs triangular solve scratch");
    s = std::move(t);
    return SPRS_HIP_OK;
}

// step 1: the reach of rhs over the columns of l into s.queue[0, S.fe); launches = launches of the narrow kernel + wide levels
template <typename IDX, typename PTR>
int32_t sp_reach(const sprs_hip_csmat *l, SpTriScratch &s, const sprs_hip_csvec *rhs, SpState &S, uint64_t &launches, hipStream_t st) {
    const uint64_t n = l->rows, nnz = l->nnz;
    const PTR *ip = (const PTR *)l->indptr;
    const IDX *ix = (const IDX *)l->indices;
    SpState *state = (SpState *)s.words;
    S = SpState{0, 0, 0, SP_WHY_BUDGET, 0};
    SPRS_TRY_HIP(hipMemsetAsync(state, 0, sizeof(SpState), st));
    dispatch_width(rhs->idx_bytes, [&](auto i) {
        using VI = typename decltype(i)::type;
        hipLaunchKernelGGL(sp_roots_kernel<VI>, dim3(sp_blocks(rhs->nnz)), dim3(SP_BLOCK), 0, st, (const VI *)rhs->indices, (const double *)rhs->data,
                           rhs->nnz, n, s.bits, s.queue, s.b, state);
    });
    SPRS_TRY_HIP(hipGetLastError());
    const uint64_t budget = (uint64_t)options().sptrisolve_budget;
    bool known = false;                              // S is the device's state
    for (;;) {
        if (known && S.fe == S.fb) break;
        if (!(known && S.fe - S.fb > (uint64_t)SP_NARROW_MAX)) {   // (a frontier the narrow kernel would hand straight back is not offered to it)
            hipLaunchKernelGGL((sp_reach_narrow_kernel<PTR, IDX>), dim3(1), dim3(SP_BLOCK), 0, st, ip, ix, n, nnz, s.bits, s.queue, state, budget);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY_HIP(copy_to_host(&S, state, sizeof S, st));
            known = true;
            launches += 1;
            if (S.why != SP_WHY_WIDE) continue;
        }
        // ---- one level run wide ----
        const uint64_t fb = S.fb, fe = S.fe, F = fe - fb;
        if (!s.lens) SPRS_TRY_HIP(alloc_block(s.blocks, s.lens, (2 * n + 1) * 8));
        uint64_t *lens = s.lens, *offs = s.lens + n;
        hipLaunchKernelGGL(sp_front_len_kernel<PTR>, dim3(sp_blocks(F)), dim3(SP_BLOCK), 0, st, ip, (const uint32_t *)s.queue + fb, F, n, nnz, lens);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(exclusive_scan_u64(lens, offs, F, st));
        uint64_t E = 0, C = 0;
        SPRS_TRY_HIP(copy_to_host(&E, offs + F, 8, st));
        if (E / SP_TILE > 0x7FFFFFFEull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "sparse-rhs triangular solve: a level with more than 2^42 entries is not supported");
        if (E) {
            hipLaunchKernelGGL((sp_expand_kernel<PTR, IDX>), dim3((unsigned)((E + SP_TILE - 1) / SP_TILE)), dim3(SP_BLOCK), 0, st, ip, ix,
                               (const uint32_t *)s.queue + fb, F, (const uint64_t *)offs, E, n, nnz, fe, s.bits, s.queue, state);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY_HIP(copy_to_host(&C, &state->cnt, 8, st));
        }
        if (C > n - fe) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "sparse-rhs triangular solve: inconsistent reach");
        S.fb = fe;
        S.fe = fe + C;
        S.levels += 1;
        S.cnt = 0;
        SPRS_TRY_HIP(copy_to_device(state, &S, sizeof S, st));
        launches += 1;
    }
    if (S.fe > n) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "sparse-rhs triangular solve: inconsistent reach");
    return SPRS_HIP_OK;
}

// steps 2 and 3 on the CSR form: the restricted level order, the solve; hw = [0] chunks drawn, [1] status, [2..3] the singular word
template <typename IDX, typename PTR>
int32_t sp_solve(sprs_hip_csmat *csr, SpTriScratch &s, uint64_t R, unsigned int *hw, hipStream_t st) {
    const uint64_t n = csr->rows;
    GsPlan &pl = csr->gs;
    if (!pl.built) SPRS_TRY((gs_plan_build<IDX, PTR, false>(csr, pl)));
    if (!pl.pos) {                                   // once per handle
        SPRS_TRY_HIP(pl.pos_block.alloc(n * sizeof(uint32_t)));
        hipLaunchKernelGGL(sp_pos_kernel, dim3(sp_blocks(n)), dim3(SP_BLOCK), 0, st, (const uint32_t *)pl.order, n, pl.pos_block.as<uint32_t>());
        SPRS_TRY_HIP(hipGetLastError());
        pl.pos = pl.pos_block.as<uint32_t>();
    }
    uint64_t *by_idx = s.keys, *by_pos = s.keys + 2 * R;
    hipLaunchKernelGGL(sp_keys_kernel, dim3(sp_blocks(R)), dim3(SP_BLOCK), 0, st, (const uint32_t *)s.queue, R, (const uint32_t *)pl.pos, by_idx, by_pos, s.work);
    SPRS_TRY_HIP(hipGetLastError());
    const int bits = sp_bits_for(n);
    SPRS_TRY(radix_sort_pairs(by_idx, by_idx + R, R, {{0, bits}}, st));
    SPRS_TRY(radix_sort_pairs(by_pos, by_pos + R, R, {{0, bits}}, st));
    hipLaunchKernelGGL(sp_order_kernel, dim3(sp_blocks(R)), dim3(SP_BLOCK), 0, st, (const uint64_t *)by_pos + R, R, s.queue);   // (the queue is spent)
    SPRS_TRY_HIP(hipGetLastError());

    unsigned int *w = (unsigned int *)(s.words + 8);
    SPRS_TRY_HIP(hipMemsetAsync(w, 0, 64, st));
    SPRS_TRY_HIP(hipMemsetAsync(w + 2, 0xFF, 8, st));                     // atomicMin starts from the top
    int ncu = 0, dev = 0;
    SPRS_TRY_HIP(hipGetDevice(&dev));
    SPRS_TRY_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t need = (R + GS_BLOCK - 1) / GS_BLOCK;                   // the grid cap of tri_run
    uint64_t grid = (uint64_t)(ncu > 0 ? ncu : 1);
    if (grid > need) grid = need;
    hipLaunchKernelGGL((tri_solve_kernel<IDX, PTR, false, false, false, true>), dim3((unsigned)grid), dim3(GS_BLOCK), 0, st, (const PTR *)csr->indptr,
                       (const IDX *)csr->indices, (const double *)csr->data, (const uint32_t *)s.queue, s.b, s.work, R, w, w + 1,
                       (unsigned long long *)(w + 2), 1u);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(copy_to_host(hw, w, 4 * sizeof(unsigned int), st));
    return SPRS_HIP_OK;
}

}  // namespace

int32_t sptrisolve_f64(sprs_hip_csmat *l, sprs_hip_csmat *csr, const sprs_hip_csvec *rhs, OwnedCsvec &out, sprs_hip_sptrisolve_info *info,
                       hipStream_t stream) {
    // held from the look-up of the scratch and of the row order to the end of the (blocking) solve, like trisolve_impl
    std::lock_guard<std::recursive_mutex> lock(csr->mu);
    const uint64_t n = l->rows;
    StreamDrain drain{stream};                       // an early return leaves nothing in flight on the scratch
    SPRS_TRY(sp_scratch(csr, n));
    SpTriScratch &s = csr->sp;
    if (!s.clean) {                                  // the first solve, or the one after an error: the only passes over n
        SPRS_TRY_HIP(hipMemsetAsync(s.bits, 0, (n + 31) / 32 * 4, stream));
        SPRS_TRY_HIP(hipMemsetAsync(s.b, 0, n * 8, stream));
        hipLaunchKernelGGL(sp_fill_kernel, dim3(sp_blocks(n)), dim3(SP_BLOCK), 0, stream, s.work, n);
        SPRS_TRY_HIP(hipGetLastError());
    }
    s.clean = false;                                 // until the pattern has been put back

    SpState S;
    uint64_t launches = 0;
    SPRS_TRY(dispatch_widths(l->idx_bytes, l->iptr_bytes, [&](auto i, auto p) {
        return sp_reach<typename decltype(i)::type, typename decltype(p)::type>(l, s, rhs, S, launches, stream);
    }));
    const uint64_t R = S.fe;
    if (info) {
        info->reach = R;
        info->reach_levels = S.levels;
        info->reach_launches = launches;
    }
    unsigned int hw[4] = {0, 0, 0, 0};
    if (R)
        SPRS_TRY(dispatch_widths(csr->idx_bytes, csr->iptr_bytes, [&](auto i, auto p) {
            return sp_solve<typename decltype(i)::type, typename decltype(p)::type>(csr, s, R, hw, stream);
        }));
    if (info) info->solve_levels = csr->gs.nlevels;
    if (R) {
        if ((uint64_t)hw[0] * 64u < R)
            SPRS_FAIL(SPRS_HIP_HIP_ERROR, "sparse-rhs triangular solve: only %llu of %llu unknowns were solved", (unsigned long long)hw[0] * 64ull,
                      (unsigned long long)R);
        if (hw[1] & GS_TIMEOUT)
            SPRS_FAIL(SPRS_HIP_HIP_ERROR, "sparse-rhs triangular solve: an unknown waited for a value that was never published (level order broken)");
        if (hw[1] & TS_SINGULAR) {
            unsigned long long word = 0;
            memcpy(&word, hw + 2, 8);
            const uint64_t index = word >> 1;
            const bool structural = (word & 1ull) != 0ull;
            if (info) {
                info->singular_index = index;
                info->singular_reason = structural ? 2 : 1;
            }
            SPRS_FAIL(SPRS_HIP_SINGULAR_MATRIX, "Singular matrix at index %llu (%s)", (unsigned long long)index,
                      structural ? "diagonal element is a structural 0" : "diagonal element is a numeric 0");   // trisolve.rs:130, 145
        }
    }
    OwnedCsvec res;
    SPRS_TRY(make_csvec(res, n, R, l->idx_bytes, l->user_idx_bytes()));
    if (R) {
        dispatch_width(l->idx_bytes, [&](auto i) {
            using OI = typename decltype(i)::type;
            hipLaunchKernelGGL(sp_gather_kernel<OI>, dim3(sp_blocks(R)), dim3(SP_BLOCK), 0, stream, (const uint64_t *)s.keys, R, s.b, s.work, s.bits,
                               (OI *)res->indices, res->data);
        });
        SPRS_TRY_HIP(hipGetLastError());
    }
    SPRS_TRY_HIP(hipStreamSynchronize(stream));
    s.clean = true;
    out = std::move(res);
    return SPRS_HIP_OK;
}
