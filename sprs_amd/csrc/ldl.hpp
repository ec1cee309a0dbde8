// Device LDL^T factorization — twins of sprs-ldl (sprs-ldl/src/lib.rs):
//   ldl_symbolic   lib.rs:445-496        ldl_numeric   lib.rs:502-593        LdlNumeric::solve   lib.rs:388-410
//   ldl_lsolve     lib.rs:597-609        ldl_ltsolve   lib.rs:613-626        linalg::diag_solve  sprs/src/sparse/linalg.rs:17-29
// Included by gauss_seidel.hip, inside namespace sprs_hip and after trisolve.hpp (one translation unit of the library and of the
// emulator build, tests/emu).  Shared with the sweeps and the triangular solves: gs_draw / gs_peek / gs_spin_guard, the data-tagged
// 8-byte hand-off (GS_PENDING), the level plans (gs_plan_build) and tri_solve_kernel, whose UNIT flag is L's implicit diagonal.
//
// THE ORDER IS THE CONTRACT.  Row k of L is a sparse triangular solve over the row's pattern, and the reference walks the pattern
// in the order its stack (sprs/src/stack.rs) leaves it in: every stored entry (rank t in stored order, permuted index i <= k) pushes
// the unvisited part of the path i, parent(i), ... IN FRONT of what was pushed before.  With t(i) = the first stored entry whose
// climb reaches i, the pattern is therefore walked by (t descending, i ascending) — a closed form (tests/ldl_ref.py holds both
// formulations).  Every value of the row depends on that order, so the symbolic pass computes it and the numeric kernel follows it.
//
// SYMBOLIC, no host round trip per row:
//   1. ldl_etree_kernel: ONE workgroup walks k = 0 .. n-1 (Liu's algorithm is sequential in k), a budget of rows per launch.  Its
//      lanes take the stored entries of outer perm[k]; a lane climbs from i = perm_inv[j] < k through `ancestor` (the parents with
//      path compression: every node passed now points at k), and gives the root it reaches the parent k.  Lanes that meet write
//      the same values, so the tree — the reference's, which climbs through the parents themselves — does not depend on who wins.
//      The climbs are short; the counts of L, which cost one step per entry of L along chains, are left to step 2.
//   2. ldl_pattern_kernel, twice: given the final parents the rows are independent, so a WAVE takes a row (its own array of n
//      flag words, rows ascending).  Lanes claim the nodes of their paths with a 64-bit atomicMax of (k + 1) << 32 | ~t, so a word
//      left by an earlier row loses and the smallest t wins; a climber that does not improve the word stops.  Then each lane
//      climbs again while the word is its own: the first run counts (row k, and column i with one atomic per entry), two scans
//      give l_colptr and the row pointers — l_colptr[n] is the ONE read-back — and the second run emits (i, k, ~t) into row k's
//      slice.
//   3. three stable radix sorts: by (i, k) = the reference's l_indices (CSC, rows ascending in a column); by (k, ~t) = each row's walk
//      order (ties are one path: i ascending, kept by stability); by k = L by rows, columns ascending (what lsolve reads, and where
//      the numeric kernel finds y[j]: a binary search in the row's columns).
//
// NUMERIC (factor and update), ldl_factor_kernel: one wave per row, rows drawn in ascending k.  Row k reads only columns' entries
// of rows j < k, which were drawn before it, so the lowest unfinished row can always finish: no level plan.  y lives in LDS for
// rows of at most ldl_lds_cap entries, else in the row's slice of a device array.  For each i in walk order: yi is read by all
// lanes, the lanes stride over column i's slots before (k, i), poll l_data (agent-scope loads; the host fills l_data and d with
// GS_PENDING first) and subtract into distinct y slots; then l_ki = yi / d[i], d[k] -= l_ki * yi, and ONE tagged 8-byte store
// publishes L[k, i].  Each product is rounded, then each subtraction (-ffp-contract=off).  d[k] == 0 records k with atomicMin and
// still publishes, so dependents finish; the host reports the smallest such k, the reference's (lib.rs:585-590).
#pragma once

namespace {

constexpr int LDL_BLOCK = 256;
constexpr uint64_t LDL_BUDGET = 2048;                          // rows per launch of the one-workgroup kernels
constexpr uint32_t LDL_CAP_MAX = 1024;                         // option ldl_lds_cap: doubles of y per wave in LDS
constexpr uint32_t LDL_NONE = 0xFFFFFFFFu;
constexpr unsigned int LDL_SINGULAR = 4u, LDL_BROKEN = 8u;     // status bits beside GS_TIMEOUT

// writes of this wave's lanes (y, in LDS or in device memory) become visible to its other lanes
__device__ __forceinline__ void ldl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// position of j in the ascending array cols[0 .. len), or len when absent
__device__ __forceinline__ uint32_t ldl_find(const uint32_t *__restrict__ cols, uint32_t len, uint32_t j) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cols[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && cols[lo] == j ? lo : len;
}

// rows [k0, k1) of ldl_symbolic's loop (lib.rs:471-488), parents only.  ancestor[i] = parents[i] or a later ancestor of i
template <typename IDX, typename PTR>
__global__ __launch_bounds__(LDL_BLOCK) void ldl_etree_kernel(const PTR *__restrict__ indptr, const IDX *__restrict__ indices,
                                                              const IDX *__restrict__ perm, const IDX *__restrict__ pinv, uint64_t n,
                                                              uint64_t k0, uint64_t k1, uint32_t *ancestor, uint32_t *parents) {
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t outer = perm ? (uint64_t)perm[k] : k;
        const uint64_t start = (uint64_t)indptr[outer], end = (uint64_t)indptr[outer + 1];
        for (uint64_t p = start + threadIdx.x; p < end; p += LDL_BLOCK) {
            const uint64_t j = (uint64_t)indices[p];
            uint64_t i = pinv ? (uint64_t)pinv[j] : j;
            while (i < k) {
                const uint32_t next = atomicExch(ancestor + i, (uint32_t)k);
                if (next == LDL_NONE) {                         // a root: uproot(i, k)
                    __hip_atomic_store(parents + i, (uint32_t)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                i = next;                                       // (k itself when another lane of this row came by: the climb ends)
            }
        }
        __syncthreads();                                        // row k + 1 sees row k's links
    }
}

// The pattern of the rows given the final parents, a wave per row: row = first + wave number, + nwaves, ...  EMIT = false counts
// (rowcnt[k], colcnt[i]); EMIT = true writes one (i, k, ~t) triple per entry of L into row k's slice [rowptr[k], rowptr[k + 1])
template <typename IDX, typename PTR, bool EMIT>
__global__ __launch_bounds__(LDL_BLOCK) void ldl_pattern_kernel(const PTR *__restrict__ indptr, const IDX *__restrict__ indices,
                                                                const IDX *__restrict__ perm, const IDX *__restrict__ pinv, uint64_t n,
                                                                const uint32_t *__restrict__ parents, unsigned long long *words,
                                                                unsigned long long *colcnt, unsigned long long *rowcnt,
                                                                const uint64_t *__restrict__ rowptr, uint64_t *__restrict__ keys,
                                                                uint64_t *__restrict__ vals) {
    __shared__ unsigned int cursor[LDL_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t me = (uint64_t)blockIdx.x * (LDL_BLOCK / 64) + wave, nwaves = (uint64_t)gridDim.x * (LDL_BLOCK / 64);
    unsigned long long *word = words + me * n;
    for (uint64_t k = me; k < n; k += nwaves) {
        const uint64_t outer = perm ? (uint64_t)perm[k] : k;
        const uint64_t start = (uint64_t)indptr[outer], end = (uint64_t)indptr[outer + 1];
        if (lane == 0) cursor[wave] = 0u;
        for (uint64_t p = start + lane; p < end; p += 64u) {
            const uint64_t j = (uint64_t)indices[p];
            uint64_t i = pinv ? (uint64_t)pinv[j] : j;
            const unsigned long long w = ((unsigned long long)(k + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(p - start));
            while (i < k) {
                if (atomicMax(word + i, w) >= w) break;         // an earlier entry of this row owns the node and all above it
                i = parents[i];                                 // (LDL_NONE ends the climb: it is not < k)
            }
        }
        ldl_wave_sync();
        const uint64_t base = EMIT ? rowptr[k] : 0, room = EMIT ? rowptr[k + 1] - base : 0;
        for (uint64_t p = start + lane; p < end; p += 64u) {
            const uint64_t j = (uint64_t)indices[p];
            uint64_t i = pinv ? (uint64_t)pinv[j] : j;
            const unsigned long long w = ((unsigned long long)(k + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(p - start));
            while (i < k && __hip_atomic_load(word + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == w) {
                const uint64_t c = (uint64_t)atomicAdd(&cursor[wave], 1u);
                if (EMIT) {
                    if (c < room) {
                        keys[base + c] = (i << 32) | k;
                        vals[base + c] = w;
                    }
                } else {
                    atomicAdd(colcnt + i, 1ull);
                }
                i = parents[i];
            }
        }
        ldl_wave_sync();
        if (!EMIT && lane == 0) rowcnt[k] = cursor[wave];
        ldl_wave_sync();                                        // (the next row clears the cursor)
    }
}

// after the sort by (i, k): slot s of the column form
__global__ void ldl_csc_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals, uint64_t lnz, uint32_t *__restrict__ l_indices,
                               uint32_t *__restrict__ col_of_slot, uint64_t *__restrict__ wkeys, uint64_t *__restrict__ wvals,
                               uint64_t *__restrict__ rkeys, uint64_t *__restrict__ rvals) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= lnz) return;
    const uint64_t key = keys[s];
    l_indices[s] = (uint32_t)key;
    col_of_slot[s] = (uint32_t)(key >> 32);
    wkeys[s] = vals[s] - (1ull << 32);                          // (k, ~t): the walk order
    wvals[s] = s;
    rkeys[s] = key & 0xFFFFFFFFull;                             // k: the row form (stable: columns stay ascending)
    rvals[s] = s;
}

__global__ void ldl_rows_kernel(const uint64_t *__restrict__ row_slot, uint64_t lnz, uint64_t n, const uint32_t *__restrict__ l_indices,
                                const uint32_t *__restrict__ col_of_slot, const uint64_t *__restrict__ rowptr, uint32_t *__restrict__ row_cols,
                                uint32_t *__restrict__ pos_of_slot) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= lnz) return;
    const uint64_t s = row_slot[q];
    row_cols[q] = col_of_slot[s];
    pos_of_slot[s] = l_indices[s] < n ? (uint32_t)(q - rowptr[l_indices[s]]) : 0xFFFFFFFFu;
}

__global__ void ldl_walk_kernel(const uint64_t *__restrict__ walk_slot, uint64_t lnz, const uint32_t *__restrict__ pos_of_slot,
                                uint32_t *__restrict__ walk_pos) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < lnz) walk_pos[q] = pos_of_slot[walk_slot[q]];
}

__global__ void ldl_gather_kernel(const uint64_t *__restrict__ row_slot, uint64_t lnz, const double *__restrict__ l_data, double *__restrict__ row_vals) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < lnz) row_vals[q] = l_data[row_slot[q]];
}

template <typename FROM, typename TO>
__global__ void ldl_narrow_kernel(const FROM *__restrict__ in, uint64_t count, TO *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = (TO)in[i];
}

__global__ void ldl_diag_kernel(const double *__restrict__ d, double *__restrict__ x, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] / d[i];                              // linalg.rs:26
}
__global__ void ldl_diag_kernel(const float *__restrict__ d, float *__restrict__ x, uint64_t n) {      // diag_solve::<f32>
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] / d[i];
}

// ldl_numeric (lib.rs:502-593), one wave per row
template <typename IDX, typename PTR>
__global__ __launch_bounds__(LDL_BLOCK) void ldl_factor_kernel(const PTR *__restrict__ indptr, const IDX *__restrict__ indices,
                                                               const double *__restrict__ data, const IDX *__restrict__ perm,
                                                               const IDX *__restrict__ pinv, uint64_t n, const uint64_t *__restrict__ colptr,
                                                               const uint32_t *__restrict__ l_indices, const uint32_t *__restrict__ col_of_slot,
                                                               const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ row_cols,
                                                               const uint64_t *__restrict__ walk_slot, const uint32_t *__restrict__ walk_pos,
                                                               unsigned long long *l_data, unsigned long long *d, double *scratch, uint32_t cap,
                                                               unsigned int *next_row, unsigned int *status, unsigned long long *singular) {
    __shared__ double y_lds[(LDL_BLOCK / 64) * LDL_CAP_MAX];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t spins = 0;
    for (uint64_t k = gs_draw(next_row, lane) >> 6; k < n; k = gs_draw(next_row, lane) >> 6) {
        const uint64_t base = rowptr[k];
        const uint32_t len = (uint32_t)(rowptr[k + 1] - base);
        const uint32_t *rc = row_cols + base;
        double *y = len <= cap ? y_lds + wave * LDL_CAP_MAX : scratch + base;
        for (uint32_t q = lane; q < len; q += 64u) y[q] = 0.0;
        ldl_wave_sync();
        // y[i] = 0 + val for the stored entries with i <= k (lib.rs:532-535); y[k] is kept in a register as dk
        const uint64_t outer = perm ? (uint64_t)perm[k] : k;
        const uint64_t start = (uint64_t)indptr[outer], end = (uint64_t)indptr[outer + 1];
        double dk_lane = 0.0;
        bool have = false;
        for (uint64_t p = start + lane; p < end; p += 64u) {
            const uint64_t j = (uint64_t)indices[p];
            const uint64_t i = pinv ? (uint64_t)pinv[j] : j;
            if (i > k) continue;
            const double v = 0.0 + data[p];
            if (i == k) {
                dk_lane = v;
                have = true;
            } else {
                const uint32_t pos = ldl_find(rc, len, (uint32_t)i);
                if (pos < len) y[pos] = v;
                else atomicOr(status, LDL_BROKEN);
            }
        }
        const unsigned long long who = __ballot(have);
        double dk = __shfl(dk_lane, who ? __ffsll((long long)who) - 1 : 0, 64);   // (no stored diagonal: y[k] stays 0)
        ldl_wave_sync();
        for (uint32_t q = 0; q < len; ++q) {
            const uint64_t s = walk_slot[base + q];
            const uint32_t i = col_of_slot[s];
            if (i >= k || s < colptr[i] || s >= colptr[i + 1] || walk_pos[base + q] >= len) {   // (never: the symbolic pass filled every slot)
                if (lane == 0) atomicOr(status, LDL_BROKEN);
                continue;
            }
            const double yi = y[walk_pos[base + q]];
            const uint64_t c0 = colptr[i], cnt = s - c0;        // column i's entries of the rows before k
            for (uint64_t e0 = 0; e0 < cnt; e0 += 64u) {
                const uint64_t e = e0 + lane;
                const bool act = e < cnt;
                unsigned long long bits = GS_PENDING;
                for (;;) {
                    bool moved = false;
                    if (act && bits == GS_PENDING) {
                        bits = gs_peek(l_data + c0 + e);
                        moved = bits != GS_PENDING;
                    }
                    if (__ballot(act && bits == GS_PENDING) == 0ull) break;
                    if (gs_spin_guard(moved, spins, status, 1u)) return;
                }
                if (act) {
                    const uint32_t pos = ldl_find(rc, len, l_indices[c0 + e]);
                    if (pos < len) {
                        const double prod = __longlong_as_double((long long)bits) * yi;      // lib.rs:572
                        y[pos] = y[pos] - prod;
                    } else {
                        atomicOr(status, LDL_BROKEN);
                    }
                }
            }
            unsigned long long dbits = GS_PENDING;
            for (;;) {
                dbits = gs_peek(d + i);
                if (__ballot(dbits == GS_PENDING) == 0ull) break;
                if (gs_spin_guard(false, spins, status, 1u)) return;
            }
            const double l_ki = yi / __longlong_as_double((long long)dbits);                 // lib.rs:579-580
            const double prod = l_ki * yi;
            dk = dk - prod;
            unsigned long long out = (unsigned long long)__double_as_longlong(l_ki);
            if (out == GS_PENDING) out = GS_QNAN;               // (a NaN whose bits are the tag: still a NaN, but not "pending")
            if (lane == 0) __hip_atomic_store(l_data + s, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ldl_wave_sync();                                    // the next yi may be one of the slots just updated
        }
        if (lane == 0) {
            if (dk == 0.0) {                                    // lib.rs:585
                atomicMin(singular, (unsigned long long)k);
                atomicOr(status, LDL_SINGULAR);
            }
            unsigned long long out = (unsigned long long)__double_as_longlong(dk);
            if (out == GS_PENDING) out = GS_QNAN;
            __hip_atomic_store(d + k, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

inline int ldl_bits(uint64_t n) {                              // bits that hold every value below n (at least one)
    int b = 1;
    while (b < 32 && (n >> b) != 0u) ++b;
    return b;
}

inline unsigned ldl_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }

template <typename IDX, typename PTR>
int32_t ldl_symbolic_impl(const sprs_hip_csmat *m, LdlSym &s, hipStream_t stream) {
    const uint64_t n = s.n;
    const IDX *perm = s.perm->identity ? nullptr : (const IDX *)s.perm->perm;
    const IDX *pinv = s.perm->identity ? nullptr : (const IDX *)s.perm->perm_inv;
    DevBuf ancestor, words, colcnt, rowcnt;
    StreamDrain drain{stream};
    SPRS_TRY_HIP(alloc_block(s.blocks, s.parents, (n ? n : 1) * sizeof(uint32_t)));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.colptr, (n + 1) * 8));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.rowptr, (n + 1) * 8));
    // the waves of the pattern pass: one array of n flag words each, 1 GiB of them at the most, never more than rows
    int ncu = 0, dev = 0;
    SPRS_TRY_HIP(hipGetDevice(&dev));
    SPRS_TRY_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    uint64_t pgrid = (uint64_t)(ncu > 0 ? ncu : 1) * 2;
    const uint64_t fit = (1ull << 30) / ((n ? n : 1) * 8 * (LDL_BLOCK / 64)), need = (n + LDL_BLOCK / 64 - 1) / (LDL_BLOCK / 64);
    if (pgrid > fit) pgrid = fit ? fit : 1;
    if (pgrid > need) pgrid = need ? need : 1;
    const uint64_t word_bytes = pgrid * (LDL_BLOCK / 64) * (n ? n : 1) * 8;
    SPRS_TRY_HIP(ancestor.alloc(n * sizeof(uint32_t)));
    SPRS_TRY_HIP(words.alloc(word_bytes));
    SPRS_TRY_HIP(colcnt.alloc((n + 1) * 8));
    SPRS_TRY_HIP(rowcnt.alloc((n + 1) * 8));
    SPRS_TRY_HIP(hipMemsetAsync(s.parents, 0xFF, (n ? n : 1) * sizeof(uint32_t), stream));     // every node a root
    SPRS_TRY_HIP(hipMemsetAsync(ancestor.p, 0xFF, n * sizeof(uint32_t), stream));
    SPRS_TRY_HIP(hipMemsetAsync(words.p, 0, word_bytes, stream));
    SPRS_TRY_HIP(hipMemsetAsync(colcnt.p, 0, (n + 1) * 8, stream));
    SPRS_TRY_HIP(hipMemsetAsync(rowcnt.p, 0, (n + 1) * 8, stream));
    for (uint64_t k0 = 0; k0 < n; k0 += LDL_BUDGET) {
        const uint64_t k1 = k0 + LDL_BUDGET < n ? k0 + LDL_BUDGET : n;
        hipLaunchKernelGGL((ldl_etree_kernel<IDX, PTR>), dim3(1), dim3(LDL_BLOCK), 0, stream, (const PTR *)m->indptr, (const IDX *)m->indices, perm,
                           pinv, n, k0, k1, ancestor.as<uint32_t>(), s.parents);
        SPRS_TRY_HIP(hipGetLastError());
        ++s.stats[0];
        ++s.stats[1];
    }
    if (n) {
        hipLaunchKernelGGL((ldl_pattern_kernel<IDX, PTR, false>), dim3((unsigned)pgrid), dim3(LDL_BLOCK), 0, stream, (const PTR *)m->indptr,
                           (const IDX *)m->indices, perm, pinv, n, (const uint32_t *)s.parents, words.as<unsigned long long>(),
                           colcnt.as<unsigned long long>(), rowcnt.as<unsigned long long>(), (const uint64_t *)nullptr, (uint64_t *)nullptr,
                           (uint64_t *)nullptr);
        SPRS_TRY_HIP(hipGetLastError());
    }
    SPRS_TRY(exclusive_scan_u64(colcnt.u64(), s.colptr, n, stream));          // lib.rs:490-495; writes n + 1 entries, the total last
    SPRS_TRY(exclusive_scan_u64(rowcnt.u64(), s.rowptr, n, stream));
    s.stats[1] += 3;
    SPRS_TRY_HIP(copy_to_host(&s.lnz, s.colptr + n, 8, stream));
    ++s.stats[2];
    const uint64_t lnz = s.lnz;
    SPRS_TRY_HIP(alloc_block(s.blocks, s.l_indices, lnz * sizeof(uint32_t)));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.col_of_slot, lnz * sizeof(uint32_t)));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.row_cols, lnz * sizeof(uint32_t)));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.row_slot, lnz * 8));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.walk_slot, lnz * 8));
    SPRS_TRY_HIP(alloc_block(s.blocks, s.walk_pos, lnz * sizeof(uint32_t)));
    if (!lnz) return SPRS_HIP_OK;
    DevBuf keys, vals, wkeys, rkeys, pos_of_slot;
    SPRS_TRY_HIP(keys.alloc(lnz * 8));
    SPRS_TRY_HIP(vals.alloc(lnz * 8));
    SPRS_TRY_HIP(wkeys.alloc(lnz * 8));
    SPRS_TRY_HIP(rkeys.alloc(lnz * 8));
    SPRS_TRY_HIP(pos_of_slot.alloc(lnz * sizeof(uint32_t)));
    // a slot the pattern pass does not fill (it always fills every one) would sort to the end as column 2^32 - 1 and fail the
    // numeric pass's look-ups instead of indexing out of range
    SPRS_TRY_HIP(hipMemsetAsync(keys.p, 0xFF, lnz * 8, stream));
    SPRS_TRY_HIP(hipMemsetAsync(vals.p, 0xFF, lnz * 8, stream));
    SPRS_TRY_HIP(hipMemsetAsync(words.p, 0, word_bytes, stream));             // the counting run's claims
    hipLaunchKernelGGL((ldl_pattern_kernel<IDX, PTR, true>), dim3((unsigned)pgrid), dim3(LDL_BLOCK), 0, stream, (const PTR *)m->indptr,
                       (const IDX *)m->indices, perm, pinv, n, (const uint32_t *)s.parents, words.as<unsigned long long>(),
                       (unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint64_t *)s.rowptr, keys.u64(), vals.u64());
    SPRS_TRY_HIP(hipGetLastError());
    ++s.stats[1];
    const int nb = ldl_bits(n);
    SPRS_TRY(radix_sort_pairs(keys.u64(), vals.u64(), lnz, {{0, nb}, {32, nb}}, stream));
    hipLaunchKernelGGL(ldl_csc_kernel, dim3(ldl_grid(lnz)), dim3(256), 0, stream, (const uint64_t *)keys.u64(), (const uint64_t *)vals.u64(), lnz,
                       s.l_indices, s.col_of_slot, wkeys.u64(), s.walk_slot, rkeys.u64(), s.row_slot);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(radix_sort_pairs(wkeys.u64(), s.walk_slot, lnz, {{0, 32}, {32, nb}}, stream));
    SPRS_TRY(radix_sort_pairs(rkeys.u64(), s.row_slot, lnz, {{0, nb}}, stream));
    hipLaunchKernelGGL(ldl_rows_kernel, dim3(ldl_grid(lnz)), dim3(256), 0, stream, (const uint64_t *)s.row_slot, lnz, n,
                       (const uint32_t *)s.l_indices, (const uint32_t *)s.col_of_slot, (const uint64_t *)s.rowptr, s.row_cols, pos_of_slot.as<uint32_t>());
    SPRS_TRY_HIP(hipGetLastError());
    hipLaunchKernelGGL(ldl_walk_kernel, dim3(ldl_grid(lnz)), dim3(256), 0, stream, (const uint64_t *)s.walk_slot, lnz,
                       (const uint32_t *)pos_of_slot.as<uint32_t>(), s.walk_pos);
    SPRS_TRY_HIP(hipGetLastError());
    s.stats[1] += 6;
    SPRS_TRY_HIP(hipStreamSynchronize(stream));
    return SPRS_HIP_OK;
}

template <typename IDX, typename PTR>
int32_t ldl_factor_impl(LdlSym &s, const sprs_hip_csmat *m, sprs_hip_ldl_num *num, sprs_hip_trisolve_info *info, hipStream_t stream) {
    const uint64_t n = s.n, lnz = s.lnz;
    const IDX *perm = s.perm->identity ? nullptr : (const IDX *)s.perm->perm;
    const IDX *pinv = s.perm->identity ? nullptr : (const IDX *)s.perm->perm_inv;
    DevBuf scratch, words;
    StreamDrain drain{stream};
    SPRS_TRY_HIP(num->l_data.reserve((lnz ? lnz : 1) * 8));
    SPRS_TRY_HIP(num->d.reserve(n * 8));
    SPRS_TRY_HIP(num->row_vals.reserve((lnz ? lnz : 1) * 8));
    SPRS_TRY_HIP(scratch.alloc((lnz ? lnz : 1) * 8));
    SPRS_TRY_HIP(words.alloc(64));
    SPRS_TRY_HIP(hipMemsetAsync(num->l_data.p, 0xFF, (lnz ? lnz : 1) * 8, stream));          // every value "pending"
    SPRS_TRY_HIP(hipMemsetAsync(num->d.p, 0xFF, n * 8, stream));
    SPRS_TRY_HIP(hipMemsetAsync(words.p, 0, 64, stream));
    SPRS_TRY_HIP(hipMemsetAsync(words.as<unsigned int>() + 2, 0xFF, 8, stream));              // atomicMin starts from the top
    unsigned int *w = words.as<unsigned int>();               // [0] rows drawn, [1] status, [2..3] smallest singular row
    int ncu = 0, dev = 0;
    SPRS_TRY_HIP(hipGetDevice(&dev));
    SPRS_TRY_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t need = (n + LDL_BLOCK / 64 - 1) / (LDL_BLOCK / 64);
    uint64_t grid = (uint64_t)(ncu > 0 ? ncu : 1) * 2;
    if (grid > need) grid = need;
    hipLaunchKernelGGL((ldl_factor_kernel<IDX, PTR>), dim3((unsigned)grid), dim3(LDL_BLOCK), 0, stream, (const PTR *)m->indptr, (const IDX *)m->indices,
                       (const double *)m->data, perm, pinv, n, (const uint64_t *)s.colptr, (const uint32_t *)s.l_indices,
                       (const uint32_t *)s.col_of_slot, (const uint64_t *)s.rowptr, (const uint32_t *)s.row_cols, (const uint64_t *)s.walk_slot,
                       (const uint32_t *)s.walk_pos, num->l_data.as<unsigned long long>(), num->d.as<unsigned long long>(),
                       scratch.as<double>(), (uint32_t)options().ldl_lds_cap, w, w + 1, (unsigned long long *)(w + 2));
    SPRS_TRY_HIP(hipGetLastError());
    if (lnz) {
        hipLaunchKernelGGL(ldl_gather_kernel, dim3(ldl_grid(lnz)), dim3(256), 0, stream, (const uint64_t *)s.row_slot, lnz,
                           (const double *)num->l_data.as<double>(), num->row_vals.as<double>());
        SPRS_TRY_HIP(hipGetLastError());
    }
    unsigned int hw[4] = {0, 0, 0, 0};
    SPRS_TRY_HIP(copy_to_host(hw, words.p, sizeof(hw), stream));
    if (hw[1] & GS_TIMEOUT) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "LDL factor: a row waited for a value that was never published");
    if (hw[1] & LDL_BROKEN)
        SPRS_FAIL(SPRS_HIP_HIP_ERROR, "LDL factor: an entry outside the symbolic pattern (the matrix must have the pattern that was analysed)");
    if ((uint64_t)hw[0] < n)
        SPRS_FAIL(SPRS_HIP_HIP_ERROR, "LDL factor: only %llu of %llu rows were factored", (unsigned long long)hw[0], (unsigned long long)n);
    if (hw[1] & LDL_SINGULAR) {
        unsigned long long k = 0;
        memcpy(&k, hw + 2, 8);
        if (info) {
            info->singular_index = k;
            info->singular_reason = 1;
        }
        SPRS_FAIL(SPRS_HIP_SINGULAR_MATRIX, "Singular matrix at index %llu (diagonal element is a numeric 0)", k);   // errors.rs:87-92, lib.rs:586-589
    }
    return SPRS_HIP_OK;
}

// L by rows (lower) or L^T = the column arrays read as CSR (upper), unit diagonal, 4-byte indices under 8-byte pointers
int32_t ldl_own_tri(LdlSym &s, bool upper, const double *vals, double *x, hipStream_t stream) {
    const void *indptr = upper ? (const void *)s.colptr : (const void *)s.rowptr;
    const void *indices = upper ? (const void *)s.l_indices : (const void *)s.row_cols;
    GsPlan &pl = upper ? s.upper : s.lower;
    std::lock_guard<std::mutex> lock(s.mu);
    if (!pl.built) {
        sprs_hip_csmat v;
        view_csmat(SPRS_HIP_CSR, s.n, s.n, s.lnz, indptr, 8, indices, 4, vals, s.device, &v);
        SPRS_TRY(upper ? (gs_plan_build<uint32_t, uint64_t, true>(&v, pl)) : (gs_plan_build<uint32_t, uint64_t, false>(&v, pl)));
    }
    unsigned int hw[4] = {0, 0, 0, 0};
    SPRS_TRY((tri_run<uint32_t, uint64_t>(indptr, indices, vals, pl.order, upper, false, true, x, s.n, hw, stream)));
    if ((uint64_t)hw[0] * 64u < s.n || (hw[1] & GS_TIMEOUT)) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "LDL solve: the triangular solve did not finish");
    return SPRS_HIP_OK;
}

}  // namespace

int32_t ldl_symbolic(const sprs_hip_csmat *m, const sprs_hip_perm *p, LdlSym &s, hipStream_t stream) {
    s.n = m->outer();
    s.idx_bytes = m->idx_bytes;
    s.iptr_bytes = m->iptr_bytes;
    s.decl_idx_bytes = m->decl_idx_bytes;
    SPRS_TRY_HIP(hipGetDevice(&s.device));
    if (!p || p->identity) {
        s.perm.reset(identity_perm(s.n, m->user_idx_bytes()));
    } else {
        OwnedPerm q;
        SPRS_TRY(make_perm(q, p->dim, p->idx_bytes, p->user_idx_bytes()));
        if (p->dim) {
            const uint64_t bytes = p->dim * (uint64_t)p->idx_bytes;
            SPRS_TRY_HIP(hipMemcpyAsync(q->perm, p->perm, bytes, hipMemcpyDeviceToDevice, stream));
            SPRS_TRY_HIP(hipMemcpyAsync(q->perm_inv, p->perm_inv, bytes, hipMemcpyDeviceToDevice, stream));
        }
        s.perm = std::move(q);
    }
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto q) {
        return ldl_symbolic_impl<typename decltype(i)::type, typename decltype(q)::type>(m, s, stream);
    });
}

int32_t ldl_factor_f64(LdlSym &s, const sprs_hip_csmat *m, sprs_hip_ldl_num *num, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto q) {
        return ldl_factor_impl<typename decltype(i)::type, typename decltype(q)::type>(s, m, num, info, stream);
    });
}

// LdlNumeric::l (lib.rs:418-429): colptr, l_indices and l_data as a CSC matrix whose pointers and indices both have the index
// width of the matrix that was analysed (the reference's one I)
int32_t ldl_export_l(const sprs_hip_ldl_num *num, OwnedCsmat &out, hipStream_t stream) {
    const LdlSym &s = *num->s;
    OwnedCsmat res;
    SPRS_TRY(make_csmat(res, SPRS_HIP_CSC, s.n, s.n, s.lnz, s.idx_bytes, s.idx_bytes));
    dispatch_width(s.idx_bytes, [&](auto t) {
        using I = typename decltype(t)::type;
        hipLaunchKernelGGL((ldl_narrow_kernel<uint64_t, I>), dim3(ldl_grid(s.n + 1)), dim3(256), 0, stream, (const uint64_t *)s.colptr, s.n + 1, (I *)res->indptr);
        if (s.lnz)
            hipLaunchKernelGGL((ldl_narrow_kernel<uint32_t, I>), dim3(ldl_grid(s.lnz)), dim3(256), 0, stream, (const uint32_t *)s.l_indices, s.lnz,
                               (I *)res->indices);
    });
    SPRS_TRY_HIP(hipGetLastError());
    if (s.lnz) SPRS_TRY_HIP(hipMemcpyAsync(res->data, num->l_data.p, s.lnz * 8, hipMemcpyDeviceToDevice, stream));
    SPRS_TRY_HIP(hipStreamSynchronize(stream));
    res->decl_idx_bytes = s.decl_idx_bytes;
    res->decl_iptr_bytes = s.decl_idx_bytes;
    out = std::move(res);
    return SPRS_HIP_OK;
}

template <typename T>
static int32_t diag_solve_any(const T *d, T *x, uint64_t n, hipStream_t stream) {
    if (!n) return SPRS_HIP_OK;
    hipLaunchKernelGGL(ldl_diag_kernel, dim3(ldl_grid(n)), dim3(256), 0, stream, d, x, n);
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}
int32_t diag_solve_f64(const double *d, double *x, uint64_t n, hipStream_t stream) { return diag_solve_any(d, x, n, stream); }
int32_t diag_solve_f32(const float *d, float *x, uint64_t n, hipStream_t stream) { return diag_solve_any(d, x, n, stream); }

// LdlNumeric::solve (lib.rs:403-409): P b, lsolve, diag_solve, ltsolve, P^-1 x
int32_t ldl_solve_f64(sprs_hip_ldl_num *num, const double *b, double *x, hipStream_t stream) {
    LdlSym &s = *num->s;
    const uint64_t n = s.n;
    DevBuf tmp;
    StreamDrain drain{stream};
    SPRS_TRY_HIP(tmp.alloc(n * 8));
    SPRS_TRY(perm_mul_vec_f64(s.perm.get(), b, tmp.as<double>(), stream));
    SPRS_TRY(ldl_own_tri(s, false, num->row_vals.as<double>(), tmp.as<double>(), stream));
    SPRS_TRY(diag_solve_f64(num->d.as<double>(), tmp.as<double>(), n, stream));
    SPRS_TRY(ldl_own_tri(s, true, num->l_data.as<double>(), tmp.as<double>(), stream));
    sprs_hip_perm inv;                                         // perm.inv(): a view with the two arrays swapped
    inv.dim = s.perm->dim;
    inv.idx_bytes = s.perm->idx_bytes;
    inv.identity = s.perm->identity;
    inv.perm = s.perm->perm_inv;
    inv.perm_inv = s.perm->perm;
    inv.device = s.perm->device;
    SPRS_TRY(perm_mul_vec_f64(&inv, tmp.as<double>(), x, stream));
    SPRS_TRY_HIP(hipStreamSynchronize(stream));
    return SPRS_HIP_OK;
}

int32_t ldl_tri_f64(sprs_hip_csmat *l, sprs_hip_csmat *csr, bool transposed, double *x, hipStream_t stream) {
    const uint64_t n = l->rows;
    std::lock_guard<std::recursive_mutex> lock(l->mu);
    return dispatch_widths(l->idx_bytes, l->iptr_bytes, [&](auto i, auto p) {
        using IDX = typename decltype(i)::type;
        using PTR = typename decltype(p)::type;
        unsigned int hw[4] = {0, 0, 0, 0};
        if (!transposed) {                                     // columns 0 .. n-1 scatter: row r receives its products by ascending column
            if (!csr->gs.built) SPRS_TRY((gs_plan_build<IDX, PTR, false>(csr, csr->gs)));
            SPRS_TRY((tri_run<IDX, PTR>(csr->indptr, csr->indices, csr->data, csr->gs.order, false, false, true, x, n, hw, stream)));
        } else {
            // columns n-1 .. 0, each a dot product in stored order: the CSC arrays ARE the CSR form of L^T.  Its row order is kept in
            // the CSC handle's own tri_upper, which nothing else uses (the solves of trisolve.hpp run on the CSR copy) and which
            // goes with the values like every plan (invalidate_caches)
            if (!l->tri_upper.built) {
                sprs_hip_csmat v;
                view_csmat(l, true, &v);
                SPRS_TRY((gs_plan_build<IDX, PTR, true>(&v, l->tri_upper)));
            }
            SPRS_TRY((tri_run<IDX, PTR>(l->indptr, l->indices, l->data, l->tri_upper.order, true, false, true, x, n, hw, stream)));
        }
        if ((uint64_t)hw[0] * 64u < n || (hw[1] & GS_TIMEOUT)) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "LDL triangular solve did not finish");
        return (int32_t)SPRS_HIP_OK;
    });
}
