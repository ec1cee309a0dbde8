// Orderings for gfx950 — device twins of
//   cuthill_mckee_custom / reverse_cuthill_mckee, start::{Next, MinimumDegree, PseudoPeripheral}, order::{Forward, Reversed}
//                                                        sprs/src/sparse/linalg/ordering.rs:14-559
//   is_symmetric                                         sprs/src/sparse/symmetric.rs:7-34
//   CsMat::max_outer_nnz / CsMat::degrees                sprs/src/sparse/csmat.rs:1188-1216
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// All of them walk the OUTER dimension as the reference does: a CSC handle is read as the CSR arrays of its transpose.
//
// THE LEVEL FORM.  The reference pops a vertex, collects its unvisited neighbours, sorts them by degree (ties: row order, the
// stable outcome of its sort_unstable_by_key) and pushes them.  That is, exactly: level L + 1 = the unvisited vertices adjacent to
// level L; each is owned by its neighbour of smallest position in the order; inside the level the vertices are ordered by the
// key (owner's position, degree, vertex id).  The key is a total order, so the result does not depend on which lane claims a
// vertex first.  The rooted level structure of the pseudo-peripheral search (ordering.rs:109-216) is the same machine with the
// key (owner's position, id): rows are walked in stored order there.
//
//   mark[j] (64 bits, all ones = never seen) = (0xFFFFFFFF - generation) << 32 | position of j's owner.  One atomicMin per
//   (frontier vertex, neighbour): a vertex of an earlier level keeps its word (its owner's position is smaller than every
//   position of the frontier), a vertex claimed in this level takes the smallest owner, and the lane whose atomicMin returns a
//   word of ANOTHER generation (or all ones) is the first to see the vertex: it appends it to the candidate list.  A newer
//   generation has the smaller high half, so the rooted level structures — one generation each — never clear their marks.
//   The ordering's own marks are generation 1 for the whole call: visited vertices stay visited across components.
//   A frontier is seq[fb, fe): the tail of the order (or of the level structure) itself.
//
// NARROW / WIDE.  cm_narrow_kernel is ONE workgroup that runs the whole state machine — choose a start vertex, the George-Liu
// loop, level after level, component after component — with the frontier, the candidates and their sort in LDS, until a
// frontier has more than `ordering_narrow_cap` vertices or more than OD_NARROW_ENTRIES stored entries, the order is complete,
// or OD_BUDGET steps are used up (a step = one level, one start vertex or one end of a search).  The host then runs that one
// level wide (cm_wide_step: lengths -> scan -> cm_expand_kernel tiled on the ENTRIES of the frontier's rows, so a hub is shared
// among waves -> radix_sort_pairs on the packed key -> commit) and hands the machine back.  No kernel waits for another
// workgroup: workgroup barriers only.  A path of n vertices or eye(n) therefore costs ceil(steps / OD_BUDGET) launches and as
// many read-backs of the state, not n.
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "scan.hpp"

namespace sprs_hip {

int32_t radix_sort_pairs(uint64_t *keys, uint64_t *vals, uint64_t n, const std::vector<std::pair<int, int>> &fields, hipStream_t stream);   // sort.hip

namespace od {

constexpr int OD_BLOCK = 256;
constexpr int OD_TILE = 2048;                       // entries per workgroup of the nnz-tiled kernels
constexpr int OD_ITEMS = OD_TILE / OD_BLOCK;
constexpr int OD_ROWS = 2048;                       // slice starts of a tile kept in LDS; a tile that meets more slices reads them from memory
constexpr int OD_CHUNK = 8192;                      // rows per workgroup of the row passes
constexpr int OD_NARROW_MAX = 1024;                 // largest ordering_narrow_cap: frontier vertices kept in LDS
constexpr int OD_NARROW_PER = OD_NARROW_MAX / OD_BLOCK;
constexpr int OD_NARROW_ENTRIES = 4096;             // stored entries of a frontier's rows (= most candidates) the narrow kernel takes
constexpr uint64_t OD_BUDGET = 16384;               // steps of the state machine per launch
constexpr uint64_t OD_UNSET = ~0ull;
constexpr uint64_t OD_HI_ORD = 0xFFFFFFFEull;       // high half of the ordering's marks (generation 1)
constexpr uint64_t OD_NONE = ~0ull;

enum : uint64_t { PH_START = 0, PH_ORD = 1, PH_RLS = 2, PH_DONE = 3 };
enum : uint64_t { WHY_BUDGET = 0, WHY_WIDE = 1, WHY_DONE = 2, WHY_LOST = 3, WHY_VISITED = 4 };

// The state of the machine.  It lives in device memory between launches; the host reads it back after every launch of the
// narrow kernel and writes it after every wide level.
struct CmState {                                    // (no initialisers: a copy of it lives in LDS)
    uint64_t phase, why;
    uint64_t count;                                 // vertices in the order
    uint64_t n_parts;                               // component delimiters written
    uint64_t cursor;                                // first index (vertex, or place in the degree order) that may still be unvisited
    uint64_t fb, fe, pfb;                           // the active search: frontier seq[fb, fe), the level before it from pfb
    uint64_t current, contender, cur_height;        // George-Liu loop (cur_height OD_NONE: no level structure built yet)
    uint64_t height, gen;                           // the rooted level structure under construction
    uint64_t levels, rls_levels, steps;
};

inline CmState initial_state() {
    CmState s{};
    s.phase = PH_START;
    s.cur_height = OD_NONE;
    s.gen = 1;
    return s;
}

template <typename P, typename I>
struct CmArgs {
    const P *ip;
    const I *ix;
    uint64_t n, nnz;
    const uint64_t *deg;
    uint64_t *mark_ord, *mark_rls;                  // n words each (mark_rls: PseudoPeripheral only)
    uint64_t *order, *rls;                          // the order in discovery order; the level structure (PseudoPeripheral only)
    const uint64_t *by_degree;                      // vertices by (degree, id): MinimumDegree only
    uint64_t *parts;                                // n + 1 delimiters at most
    int32_t strategy;
    uint64_t cap, budget;
};

__device__ __forceinline__ uint64_t load_now(const uint64_t *p) {   // a load that sees the atomics of this very kernel
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the stored entries of outer slice v, inside [0, nnz) whatever the arrays hold
template <typename P>
__device__ __forceinline__ uint64_t slice_of(const P *ip, uint64_t v, uint64_t n, uint64_t nnz, uint64_t *len) {
    *len = 0;
    if (v >= n) return 0;
    uint64_t s = (uint64_t)ip[v], e = (uint64_t)ip[v + 1];
    if (e > nnz) e = nnz;
    if (s > e) s = e;
    *len = e - s;
    return s;
}

// ---- the outer slices a tile of entries meets -----------------------------------------------------------------------------------
// s_edge = the last slice that starts at or before the tile's first / last entry; with at most OD_ROWS slices in between their
// starts relative to the tile go to s_off (-1: in front of it).  Returns whether they were staged.
template <typename P>
__device__ __forceinline__ bool stage_tile_rows(const P *ip, uint64_t outer, uint64_t k0, uint64_t k1, int32_t *s_off, uint64_t *s_edge) {
    const int tid = threadIdx.x;
    if (tid < 2) {
        const uint64_t k = tid == 0 ? k0 : k1 - 1;
        uint64_t lo = 0, hi = outer - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if ((uint64_t)ip[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        s_edge[tid] = lo;
    }
    __syncthreads();
    const uint64_t rlo = s_edge[0], nrows = s_edge[1] - rlo + 1;
    const bool staged = nrows <= (uint64_t)OD_ROWS;
    if (staged) {
        for (uint64_t x = tid; x < nrows; x += OD_BLOCK) {
            const uint64_t start = (uint64_t)ip[rlo + x];
            s_off[x] = start < k0 ? -1 : (int32_t)(start - k0 < (uint64_t)OD_TILE ? start - k0 : (uint64_t)OD_TILE);
        }
    }
    __syncthreads();
    return staged;
}

template <typename P>
__device__ __forceinline__ uint64_t tile_row_of(const P *ip, bool staged, const int32_t *s_off, const uint64_t *s_edge, uint64_t k0, uint64_t pos) {
    const uint64_t rlo = s_edge[0], rhi = s_edge[1];
    if (staged) {
        const int32_t q = (int32_t)(pos - k0);
        int32_t lo = 0, hi = (int32_t)(rhi - rlo);
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= q) lo = mid;
            else hi = mid - 1;
        }
        return rlo + (uint64_t)lo;
    }
    uint64_t lo = rlo, hi = rhi;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t)ip[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- degrees, max_outer_nnz ---------------------------------------------------------------------------------------------------
// deg[r] = stored entries of slice r; the entry kernel below takes one off for a stored diagonal entry (a sorted slice without
// duplicates holds at most one), so the count is "entries with index != outer" (csmat.rs:1205-1216) and no lane walks a hub row.
// With `maxlen`, the max-reduction of the slice lengths (csmat.rs:1188-1193): one atomic per workgroup.
template <typename P>
__global__ void __launch_bounds__(OD_BLOCK) od_len_kernel(const P *ip, uint64_t outer, uint64_t nnz, uint64_t *deg, unsigned long long *maxlen) {
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * OD_CHUNK;
    uint64_t mine = 0;
    for (int it = 0; it < OD_CHUNK / OD_BLOCK; ++it) {
        const uint64_t r = r0 + (uint64_t)it * OD_BLOCK + threadIdx.x;
        if (r >= outer) break;
        uint64_t len;
        (void)slice_of(ip, r, outer, nnz, &len);
        if (deg) deg[r] = len;
        mine = len > mine ? len : mine;
    }
    if (!maxlen) return;
    if (mine) atomicMax(&s_max, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(maxlen, s_max);
}

template <typename P, typename I>
__global__ void __launch_bounds__(OD_BLOCK) od_diag_kernel(const P *ip, const I *ix, uint64_t outer, uint64_t nnz, unsigned long long *deg) {
    __shared__ int32_t s_off[OD_ROWS];
    __shared__ uint64_t s_edge[2];
    const uint64_t k0 = (uint64_t)blockIdx.x * OD_TILE;
    const uint64_t k1 = k0 + OD_TILE < nnz ? k0 + OD_TILE : nnz;
    if (k0 >= k1) return;
    const bool staged = stage_tile_rows(ip, outer, k0, k1, s_off, s_edge);
#pragma unroll
    for (int j = 0; j < OD_ITEMS; ++j) {
        const uint64_t pos = k0 + (uint64_t)(j * OD_BLOCK) + threadIdx.x;
        if (pos >= k1) continue;
        const uint64_t r = tile_row_of(ip, staged, s_off, s_edge, k0, pos);
        if ((uint64_t)ix[pos] == r && pos < (uint64_t)ip[r + 1]) atomicAdd(&deg[r], ~0ull);   // - 1
    }
}

// ---- is_symmetric (symmetric.rs:21-32) ------------------------------------------------------------------------------------------
// Per stored entry (o, i, v): slice i must hold index o, with a value that is not `!=` v — a NaN anywhere is therefore "not
// symmetric" and -0.0 equals 0.0.  A workgroup that finds the flag up already has nothing left to decide.
template <typename P, typename I>
__global__ void __launch_bounds__(OD_BLOCK) od_symmetric_kernel(const P *ip, const I *ix, const double *data, uint64_t outer, uint64_t nnz,
                                                                unsigned int *flag) {
    __shared__ int32_t s_off[OD_ROWS];
    __shared__ uint64_t s_edge[2];
    __shared__ unsigned int s_stop;
    const uint64_t k0 = (uint64_t)blockIdx.x * OD_TILE;
    const uint64_t k1 = k0 + OD_TILE < nnz ? k0 + OD_TILE : nnz;
    if (k0 >= k1) return;
    if (threadIdx.x == 0) s_stop = *(volatile unsigned int *)flag;
    __syncthreads();
    if (s_stop) return;                                      // (one read for the whole workgroup: it leaves together)
    const bool staged = stage_tile_rows(ip, outer, k0, k1, s_off, s_edge);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < OD_ITEMS; ++j) {
        const uint64_t pos = k0 + (uint64_t)(j * OD_BLOCK) + threadIdx.x;
        if (pos >= k1) continue;
        const uint64_t o = tile_row_of(ip, staged, s_off, s_edge, k0, pos), i = (uint64_t)ix[pos];
        uint64_t len;
        const uint64_t s = slice_of(ip, i, outer, nnz, &len);
        uint64_t lo = 0, hi = len;                           // the first entry of slice i with index >= o
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint64_t)ix[s + mid] < o) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= len || (uint64_t)ix[s + lo] != o || data[s + lo] != data[pos]) bad = true;
    }
    if (bad) atomicOr(flag, 1u);
}

// ---- Cuthill-McKee: the narrow kernel -------------------------------------------------------------------------------------------

// the first index >= from whose vertex (list[index], or the index itself) is not in the order yet; n when there is none.
// Called by the whole workgroup; s_min is an LDS word.
__device__ __forceinline__ uint64_t first_unvisited(const uint64_t *mark, const uint64_t *list, uint64_t from, uint64_t n, uint64_t *s_min) {
    for (uint64_t c = from; c < n; c += OD_BLOCK) {
        if (threadIdx.x == 0) *s_min = OD_NONE;
        __syncthreads();
        const uint64_t idx = c + threadIdx.x;
        if (idx < n) {
            const uint64_t v = list ? list[idx] : idx;
            if (v < n && load_now(mark + v) == OD_UNSET) atomicMin((unsigned long long *)s_min, (unsigned long long)idx);
        }
        __syncthreads();
        const uint64_t found = *s_min;
        __syncthreads();
        if (found != OD_NONE) return found;
    }
    return n;
}

template <typename P, typename I>
__global__ void __launch_bounds__(OD_BLOCK) cm_narrow_kernel(CmArgs<P, I> a, CmState *state) {
    __shared__ CmState st;
    __shared__ uint64_t s_k1[OD_NARROW_ENTRIES];    // (owner's position in the frontier) << 32 | degree
    __shared__ uint32_t s_id[OD_NARROW_ENTRIES];    // the candidates
    __shared__ uint32_t s_front[OD_NARROW_MAX];     // the frontier
    __shared__ uint32_t s_off[OD_NARROW_MAX + 1];   // exclusive scan of its rows' lengths
    __shared__ uint32_t s_wt[16];
    __shared__ uint32_t s_cnt;
    __shared__ uint64_t s_min;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        st = *state;
        st.why = WHY_BUDGET;
    }
    __syncthreads();
    bool front_lds = false;                         // s_front holds seq[fb, fe)
    for (uint64_t step = 0; step < a.budget; ++step) {
        const uint64_t phase = st.phase, fb = st.fb, fe = st.fe, pfb = st.pfb, count = st.count, cursor = st.cursor, gen = st.gen;
        __syncthreads();
        if (phase == PH_DONE) break;
        // what thread 0 does to begin a search at vertex v
        auto begin_rls = [&](uint64_t v) {
            st.gen += 1;
            a.rls[0] = v;
            atomicExch((unsigned long long *)(a.mark_rls + v), (unsigned long long)((0xFFFFFFFFull - st.gen) << 32));
            st.fb = st.pfb = 0;
            st.fe = 1;
            st.height = 0;
            st.phase = PH_RLS;
        };
        auto begin_order = [&](uint64_t v) {
            // on a non-symmetric pattern the George-Liu loop can walk into an earlier component and return one of its vertices:
            // the reference's assert!(!visited[new_start_vertex]) (ordering.rs:488-491)
            if (load_now(a.mark_ord + v) != OD_UNSET) {
                st.phase = PH_DONE;
                st.why = WHY_VISITED;
                return;
            }
            const uint64_t at = st.count;
            a.order[at] = v;
            atomicExch((unsigned long long *)(a.mark_ord + v), (unsigned long long)((OD_HI_ORD << 32) | at));
            st.fb = st.pfb = at;
            st.fe = st.count = at + 1;
            st.phase = PH_ORD;
        };
        if (phase == PH_START) {
            if (count >= a.n) {
                if (tid == 0) {
                    a.parts[st.n_parts++] = a.n;     // add_component_delimeter(nb_vertices), ordering.rs:523
                    st.phase = PH_DONE;
                    st.why = WHY_DONE;
                }
                __syncthreads();
                break;
            }
            const uint64_t at = first_unvisited(a.mark_ord, a.strategy == SPRS_HIP_START_MINIMUM_DEGREE ? a.by_degree : nullptr, cursor, a.n, &s_min);
            if (at >= a.n) {                         // (cannot happen while count < n)
                if (tid == 0) st.phase = PH_DONE, st.why = WHY_LOST;
                __syncthreads();
                break;
            }
            if (tid == 0) {
                const uint64_t v = a.strategy == SPRS_HIP_START_MINIMUM_DEGREE ? a.by_degree[at] : at;
                a.parts[st.n_parts++] = count;
                st.cursor = at;
                if (a.strategy == SPRS_HIP_START_PSEUDO_PERIPHERAL && a.deg[v] != 0) {   // an isolated vertex returns at once (ordering.rs:241)
                    st.current = v;
                    st.cur_height = OD_NONE;
                    begin_rls(v);
                } else {
                    begin_order(v);
                }
            }
            front_lds = false;
        } else {
            const bool rls = phase == PH_RLS;
            uint64_t *mark = rls ? a.mark_rls : a.mark_ord, *seq = rls ? a.rls : a.order;
            const uint64_t hi = rls ? 0xFFFFFFFFull - gen : OD_HI_ORD;
            const uint64_t F = fe - fb;
            if (F == 0) {                            // the search is over
                if (!rls) {
                    if (tid == 0) st.phase = PH_START;
                } else {
                    // the contender: the FIRST vertex of minimum degree in the last level (min_by_key, ordering.rs:207-211)
                    if (tid == 0) s_min = OD_NONE;
                    __syncthreads();
                    for (uint64_t k = pfb + tid; k < fb; k += OD_BLOCK) {
                        const uint64_t v = seq[k];
                        atomicMin((unsigned long long *)&s_min, (unsigned long long)(((a.deg[v] & 0xFFFFFFFFull) << 32) | (k - pfb)));
                    }
                    __syncthreads();
                    if (tid == 0) {
                        const uint64_t c = seq[pfb + (s_min & 0xFFFFFFFFull)], h = st.height;
                        if (st.cur_height == OD_NONE) {                  // ordering.rs:245-246
                            st.contender = c;
                            st.cur_height = h;
                            begin_rls(c);
                        } else if (h > st.cur_height) {                  // ordering.rs:257-260
                            st.cur_height = h;
                            st.current = st.contender;
                            st.contender = c;
                            begin_rls(c);
                        } else {
                            begin_order(st.current);
                        }
                    }
                }
                front_lds = false;
            } else if (F > a.cap) {
                if (tid == 0) st.why = WHY_WIDE;
                __syncthreads();
                break;
            } else {
                if (!front_lds)
                    for (uint64_t s = tid; s < F; s += OD_BLOCK) s_front[s] = (uint32_t)seq[fb + s];
                __syncthreads();
                uint32_t len[OD_NARROW_PER], sum = 0;
#pragma unroll
                for (int i = 0; i < OD_NARROW_PER; ++i) {
                    const uint64_t s = (uint64_t)tid * OD_NARROW_PER + i;
                    uint64_t l = 0;
                    if (s < F) (void)slice_of(a.ip, (uint64_t)s_front[s], a.n, a.nnz, &l);
                    len[i] = (uint32_t)(l < (uint64_t)OD_NARROW_ENTRIES + 1 ? l : (uint64_t)OD_NARROW_ENTRIES + 1);
                    sum += len[i];
                }
                uint32_t E;
                uint32_t base = block_excl_scan_u32(sum, s_wt, &E);
#pragma unroll
                for (int i = 0; i < OD_NARROW_PER; ++i) {
                    s_off[tid * OD_NARROW_PER + i] = base;
                    base += len[i];
                }
                if (tid == 0) s_cnt = 0;
                __syncthreads();
                if (E > (uint32_t)OD_NARROW_ENTRIES) {
                    if (tid == 0) st.why = WHY_WIDE;
                    __syncthreads();
                    break;
                }
                // expand: one entry of the frontier's rows per lane and round
                for (uint32_t e = tid; e < E; e += OD_BLOCK) {
                    uint32_t lo = 0, top = (uint32_t)F - 1;
                    while (lo < top) {
                        const uint32_t mid = (lo + top + 1) >> 1;
                        if (s_off[mid] <= e) lo = mid;
                        else top = mid - 1;
                    }
                    const uint64_t v = s_front[lo];
                    uint64_t l;
                    const uint64_t s = slice_of(a.ip, v, a.n, a.nnz, &l);
                    const uint64_t j = e - s_off[lo] < l ? (uint64_t)a.ix[s + (e - s_off[lo])] : v;
                    if (j != v && j < a.n) {
                        const uint64_t old = atomicMin((unsigned long long *)(mark + j), (unsigned long long)((hi << 32) | (fb + lo)));
                        if ((old >> 32) != hi) s_id[atomicAdd(&s_cnt, 1u)] = (uint32_t)j;
                    }
                }
                __syncthreads();
                const uint32_t C = s_cnt;
                if (C) {
                    uint32_t size = 2;
                    while (size < C) size <<= 1;
                    for (uint32_t k = tid; k < size; k += OD_BLOCK) {
                        if (k < C) {
                            const uint64_t j = s_id[k];
                            const uint64_t owner = (load_now(mark + j) & 0xFFFFFFFFull) - fb;
                            s_k1[k] = (owner << 32) | (rls ? 0ull : a.deg[j] & 0xFFFFFFFFull);
                        } else {
                            s_k1[k] = ~0ull;
                            s_id[k] = 0xFFFFFFFFu;
                        }
                    }
                    __syncthreads();
                    for (uint32_t k2 = 2; k2 <= size; k2 <<= 1) {
                        for (uint32_t jj = k2 >> 1; jj > 0; jj >>= 1) {
                            for (uint32_t i = tid; i < size; i += OD_BLOCK) {
                                const uint32_t l = i ^ jj;
                                if (l > i) {
                                    const uint64_t ki = s_k1[i], kl = s_k1[l];
                                    const uint32_t vi = s_id[i], vl = s_id[l];
                                    const bool above = ki > kl || (ki == kl && vi > vl);
                                    if (above == ((i & k2) == 0)) {
                                        s_k1[i] = kl, s_k1[l] = ki;
                                        s_id[i] = vl, s_id[l] = vi;
                                    }
                                }
                            }
                            __syncthreads();
                        }
                    }
                    for (uint32_t k = tid; k < C; k += OD_BLOCK) {
                        seq[fe + k] = s_id[k];
                        if (C <= (uint32_t)OD_NARROW_MAX) s_front[k] = s_id[k];
                    }
                }
                front_lds = C <= (uint32_t)OD_NARROW_MAX;
                if (tid == 0) {
                    st.pfb = fb;
                    st.fb = fe;
                    st.fe = fe + C;
                    if (rls) {
                        st.height += 1;
                        st.rls_levels += 1;
                    } else {
                        st.count = fe + C;
                        st.levels += 1;
                    }
                }
            }
        }
        if (tid == 0) st.steps += 1;
        __syncthreads();
    }
    if (tid == 0) *state = st;
}

// ---- Cuthill-McKee: one wide level ------------------------------------------------------------------------------------------------

template <typename P>
__global__ void __launch_bounds__(OD_BLOCK) cm_front_len_kernel(const P *ip, const uint64_t *front, uint64_t F, uint64_t n, uint64_t nnz, uint64_t *lens) {
    const uint64_t s = (uint64_t)blockIdx.x * OD_BLOCK + threadIdx.x;
    if (s >= F) return;
    uint64_t len;
    (void)slice_of(ip, front[s], n, nnz, &len);
    lens[s] = len;
}

// a tile of OD_TILE entries of the frontier's rows (offs = exclusive scan of their lengths, E entries in all)
template <typename P, typename I>
__global__ void __launch_bounds__(OD_BLOCK) cm_expand_kernel(const P *ip, const I *ix, const uint64_t *front, uint64_t F, const uint64_t *offs, uint64_t E,
                                                             uint64_t n, uint64_t nnz, uint64_t fb, uint64_t hi, uint64_t *mark, uint64_t *cand,
                                                             unsigned long long *cnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t k0 = (uint64_t)blockIdx.x * OD_TILE;
    for (int it = 0; it < OD_ITEMS; ++it) {
        const uint64_t e = k0 + (uint64_t)(it * OD_BLOCK) + threadIdx.x;
        bool claim = false;
        uint64_t j = 0;
        if (e < E) {
            uint64_t lo = 0, top = F - 1;                // the last row that starts at or before entry e
            while (lo < top) {
                const uint64_t mid = (lo + top + 1) >> 1;
                if (offs[mid] <= e) lo = mid;
                else top = mid - 1;
            }
            const uint64_t v = front[lo];
            uint64_t len;
            const uint64_t s = slice_of(ip, v, n, nnz, &len);
            if (e - offs[lo] < len) {
                j = (uint64_t)ix[s + (e - offs[lo])];
                if (j != v && j < n) {
                    const uint64_t old = atomicMin((unsigned long long *)(mark + j), (unsigned long long)((hi << 32) | (fb + lo)));
                    claim = (old >> 32) != hi;
                }
            }
        }
        const uint64_t mask = __ballot(claim);          // one reservation per wave
        unsigned long long first = 0;
        if (lane == 0 && mask) first = atomicAdd(cnt, (unsigned long long)__popcll(mask));
        first = __shfl(first, 0, 64);
        if (claim) {
            const uint64_t at = first + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < n) cand[at] = j;
        }
    }
}

// keys[k] = ((owner's position in the frontier << deg_bits | degree) << id_bits) | id of src[k]; vals[k] = src[k]
__global__ void __launch_bounds__(OD_BLOCK) cm_keys_kernel(const uint64_t *src, uint64_t C, const uint64_t *mark, const uint64_t *deg, uint64_t fb,
                                                           int deg_bits, int id_bits, uint64_t n, uint64_t *keys, uint64_t *vals) {
    const uint64_t k = (uint64_t)blockIdx.x * OD_BLOCK + threadIdx.x;
    if (k >= C) return;
    const uint64_t j = src[k] < n ? src[k] : 0;
    const uint64_t owner = (mark[j] & 0xFFFFFFFFull) - fb;
    uint64_t key = deg_bits ? (owner << deg_bits) | (deg[j] & ((1ull << deg_bits) - 1ull)) : owner;
    if (id_bits) key = (key << id_bits) | j;
    keys[k] = key;
    vals[k] = j;
}

__global__ void __launch_bounds__(OD_BLOCK) cm_copy_kernel(const uint64_t *src, uint64_t C, uint64_t *dst) {
    const uint64_t k = (uint64_t)blockIdx.x * OD_BLOCK + threadIdx.x;
    if (k < C) dst[k] = src[k];
}

__global__ void __launch_bounds__(OD_BLOCK) cm_iota_kernel(const uint64_t *deg, uint64_t n, uint64_t *keys, uint64_t *vals) {
    const uint64_t k = (uint64_t)blockIdx.x * OD_BLOCK + threadIdx.x;
    if (k >= n) return;
    keys[k] = deg[k];
    vals[k] = k;
}

// perm[k] (or perm[n - 1 - k]: order::Reversed, ordering.rs:390-394) = order[k], at the handle's index width
template <typename I>
__global__ void __launch_bounds__(OD_BLOCK) cm_emit_kernel(const uint64_t *order, uint64_t n, bool reversed, I *perm) {
    const uint64_t k = (uint64_t)blockIdx.x * OD_BLOCK + threadIdx.x;
    if (k < n) perm[reversed ? n - 1 - k : k] = (I)order[k];
}

inline unsigned blocks_for(uint64_t n) { return n ? (unsigned)((n + OD_BLOCK - 1) / OD_BLOCK) : 1u; }
inline unsigned chunks_for(uint64_t n) { return n ? (unsigned)((n + OD_CHUNK - 1) / OD_CHUNK) : 1u; }
inline unsigned tiles_for(uint64_t n) { return n ? (unsigned)((n + OD_TILE - 1) / OD_TILE) : 1u; }

inline int bits_for(uint64_t n) {                   // bits needed for values < n
    int b = 1;
    while (b < 63 && (1ull << b) < n) ++b;
    return b;
}

template <typename P, typename I>
int32_t degrees_run(const sprs_hip_csmat *m, uint64_t *deg, uint64_t *maxlen_dev, hipStream_t st) {
    const uint64_t outer = m->outer(), nnz = m->nnz;
    if (outer >= 0xFFFFFFFFull * OD_BLOCK || nnz / OD_TILE > 0x7FFFFFFEull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "degrees: the matrix is too large");
    if (maxlen_dev) SPRS_TRY_HIP(hipMemsetAsync(maxlen_dev, 0, 8, st));
    if (!outer) return SPRS_HIP_OK;
    hipLaunchKernelGGL(od_len_kernel<P>, dim3(chunks_for(outer)), dim3(OD_BLOCK), 0, st, (const P *)m->indptr, outer, nnz, deg,
                       (unsigned long long *)maxlen_dev);
    if (deg && nnz)
        hipLaunchKernelGGL((od_diag_kernel<P, I>), dim3(tiles_for(nnz)), dim3(OD_BLOCK), 0, st, (const P *)m->indptr, (const I *)m->indices, outer, nnz,
                           (unsigned long long *)deg);
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

// the temporaries of the wide levels: made by the first one
struct WideScratch {
    DevBuf lens, offs, cand, keys, cnt;
    bool ready = false;
};

// One level of the active search run wide.  S is the host's copy of the state (read back after the narrow kernel stopped with
// WHY_WIDE, or kept from the wide level before); it is advanced here and written back.
template <typename P, typename I>
int32_t cm_wide_step(const CmArgs<P, I> &a, CmState &S, CmState *state_dev, WideScratch &w, int max_deg_bits, uint64_t *stats, hipStream_t st) {
    const bool rls = S.phase == PH_RLS;
    uint64_t *mark = rls ? a.mark_rls : a.mark_ord, *seq = rls ? a.rls : a.order;
    const uint64_t hi = rls ? 0xFFFFFFFFull - S.gen : OD_HI_ORD, fb = S.fb, fe = S.fe, F = fe - fb, n = a.n;
    if (!w.ready) {
        SPRS_TRY_HIP(w.lens.alloc_for(st, n * 8));
        SPRS_TRY_HIP(w.offs.alloc_for(st, (n + 1) * 8));
        SPRS_TRY_HIP(w.cand.alloc_for(st, n * 8));
        SPRS_TRY_HIP(w.keys.alloc_for(st, n * 8));
        SPRS_TRY_HIP(w.cnt.alloc_for(st, 16));
        w.ready = true;
    }
    hipLaunchKernelGGL(cm_front_len_kernel<P>, dim3(blocks_for(F)), dim3(OD_BLOCK), 0, st, a.ip, (const uint64_t *)seq + fb, F, n, a.nnz, w.lens.u64());
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(w.lens.u64(), w.offs.u64(), F, st));
    uint64_t E = 0, C = 0;
    SPRS_TRY_HIP(copy_to_host(&E, w.offs.u64() + F, 8, st));
    stats[2] += 2, stats[3] += 1;
    if (E / OD_TILE > 0x7FFFFFFEull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "cuthill_mckee: a level with more than 2^42 entries is not supported");
    if (E) {
        SPRS_TRY_HIP(hipMemsetAsync(w.cnt.p, 0, 8, st));
        hipLaunchKernelGGL((cm_expand_kernel<P, I>), dim3(tiles_for(E)), dim3(OD_BLOCK), 0, st, a.ip, a.ix, (const uint64_t *)seq + fb, F,
                           (const uint64_t *)w.offs.u64(), E, n, a.nnz, fb, hi, mark, w.cand.u64(), w.cnt.as<unsigned long long>());
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY_HIP(copy_to_host(&C, w.cnt.p, 8, st));
        stats[2] += 1, stats[3] += 1;
    }
    if (C > n - fe) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "cuthill_mckee: inconsistent candidate count");
    if (C) {
        // the packed key (owner, degree, id) when it fits `ordering_key_bits` (64), else two stable passes: by id, then by (owner, degree)
        const int fbits = bits_for(F), dbits = rls ? 0 : max_deg_bits, ibits = bits_for(n);
        uint64_t *keys = w.keys.u64(), *vals = w.lens.u64();        // (the lengths are spent)
        const bool packed = fbits + dbits + ibits <= (int)options().ordering_key_bits;
        if (packed) {
            hipLaunchKernelGGL(cm_keys_kernel, dim3(blocks_for(C)), dim3(OD_BLOCK), 0, st, (const uint64_t *)w.cand.u64(), C, (const uint64_t *)mark, a.deg,
                               fb, dbits, ibits, n, keys, vals);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY(radix_sort_pairs(keys, vals, C, {{0, fbits + dbits + ibits}}, st));
            stats[2] += 1;
        } else {
            hipLaunchKernelGGL(cm_copy_kernel, dim3(blocks_for(C)), dim3(OD_BLOCK), 0, st, (const uint64_t *)w.cand.u64(), C, keys);
            hipLaunchKernelGGL(cm_copy_kernel, dim3(blocks_for(C)), dim3(OD_BLOCK), 0, st, (const uint64_t *)w.cand.u64(), C, vals);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY(radix_sort_pairs(keys, vals, C, {{0, ibits}}, st));
            hipLaunchKernelGGL(cm_keys_kernel, dim3(blocks_for(C)), dim3(OD_BLOCK), 0, st, (const uint64_t *)vals, C, (const uint64_t *)mark, a.deg, fb, dbits,
                               0, n, keys, w.cand.u64());
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY(radix_sort_pairs(keys, w.cand.u64(), C, {{0, fbits + dbits}}, st));
            vals = w.cand.u64();
            stats[2] += 3;
        }
        hipLaunchKernelGGL(cm_copy_kernel, dim3(blocks_for(C)), dim3(OD_BLOCK), 0, st, (const uint64_t *)vals, C, seq + fe);
        SPRS_TRY_HIP(hipGetLastError());
        stats[2] += 1;
    }
    S.pfb = fb;
    S.fb = fe;
    S.fe = fe + C;
    S.steps += 1;
    if (rls) {
        S.height += 1;
        S.rls_levels += 1;
    } else {
        S.count = fe + C;
        S.levels += 1;
    }
    SPRS_TRY_HIP(copy_to_device(state_dev, &S, sizeof S, st));
    return SPRS_HIP_OK;
}

template <typename P, typename I>
int32_t cm_run(const sprs_hip_csmat *m, int32_t strategy, bool reversed, sprs_hip_ordering *o, hipStream_t st) {
    const uint64_t n = m->outer(), nnz = m->nnz;
    if (n >= (1ull << 31)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "cuthill_mckee: 2^31 or more vertices are not supported");
    const bool pp = strategy == SPRS_HIP_START_PSEUDO_PERIPHERAL, md = strategy == SPRS_HIP_START_MINIMUM_DEGREE;
    uint64_t *stats = o->stats;
    // deg | mark_ord | order | parts (n + 1) | state, max length;  mark_rls | rls;  the vertices by (degree, id) and their keys
    DevBuf main, search, bydeg;
    SPRS_TRY_HIP(main.alloc_for(st, (4 * n + 1) * 8 + sizeof(CmState) + 16));
    uint64_t *deg = main.u64(), *mark_ord = deg + n, *order = mark_ord + n, *parts = order + n, *maxlen = parts + n + 1;
    CmState *state_dev = (CmState *)(maxlen + 2);
    SPRS_TRY((degrees_run<P, I>(m, deg, maxlen, st)));
    SPRS_TRY_HIP(hipMemsetAsync(mark_ord, 0xFF, n * 8, st));
    uint64_t max_len = 0;
    SPRS_TRY_HIP(copy_to_host(&max_len, maxlen, 8, st));
    stats[2] += 2, stats[3] += 1;
    const int max_deg_bits = bits_for(max_len + 1);
    CmArgs<P, I> a{};
    a.ip = (const P *)m->indptr, a.ix = (const I *)m->indices, a.n = n, a.nnz = nnz, a.deg = deg, a.mark_ord = mark_ord, a.order = order, a.parts = parts;
    a.strategy = strategy;
    a.cap = (uint64_t)options().ordering_narrow_cap;
    a.budget = OD_BUDGET;
    if (pp) {
        SPRS_TRY_HIP(search.alloc_for(st, 2 * n * 8));
        a.mark_rls = search.u64(), a.rls = a.mark_rls + n;
        SPRS_TRY_HIP(hipMemsetAsync(a.mark_rls, 0xFF, n * 8, st));
    }
    if (md) {                                        // one stable sort by degree: min_by_key returns the FIRST minimum (ordering.rs:82-87)
        SPRS_TRY_HIP(bydeg.alloc_for(st, 2 * n * 8));
        uint64_t *vals = bydeg.u64(), *keys = vals + n;
        hipLaunchKernelGGL(cm_iota_kernel, dim3(blocks_for(n)), dim3(OD_BLOCK), 0, st, (const uint64_t *)deg, n, keys, vals);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(radix_sort_pairs(keys, vals, n, {{0, max_deg_bits}}, st));
        a.by_degree = vals;
        stats[2] += 2;
    }
    CmState S = initial_state();
    SPRS_TRY_HIP(copy_to_device(state_dev, &S, sizeof S, st));
    WideScratch w;
    while (S.phase != PH_DONE) {
        const bool search_on = S.phase == PH_ORD || S.phase == PH_RLS;
        if (!(search_on && S.fe - S.fb > a.cap)) {   // (a frontier the narrow kernel would hand straight back is not offered to it)
            hipLaunchKernelGGL((cm_narrow_kernel<P, I>), dim3(1), dim3(OD_BLOCK), 0, st, a, state_dev);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY_HIP(copy_to_host(&S, state_dev, sizeof S, st));
            stats[2] += 1, stats[3] += 1;
            if (S.why == WHY_VISITED)
                SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Vertex returned by starting strategy should always be unvisited");   // ordering.rs:488-491
            if (S.why == WHY_LOST) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "cuthill_mckee: no unvisited vertex left before the order was complete");
            if (S.why != WHY_WIDE) continue;
        }
        SPRS_TRY((cm_wide_step<P, I>(a, S, state_dev, w, max_deg_bits, stats, st)));
    }
    if (S.count != n || S.n_parts < 1 || S.n_parts > n + 1) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "cuthill_mckee: inconsistent order");
    o->parts.resize(S.n_parts);
    SPRS_TRY_HIP(copy_to_host(o->parts.data(), parts, S.n_parts * 8, st));
    stats[3] += 1;
    if (reversed) {                                  // order::Reversed::into_ordering (ordering.rs:402-418)
        for (auto &p : o->parts) p = n - p;
        std::reverse(o->parts.begin(), o->parts.end());
    }
    stats[0] = S.n_parts - 1;
    stats[1] = S.levels;
    hipLaunchKernelGGL(cm_emit_kernel<I>, dim3(blocks_for(n)), dim3(OD_BLOCK), 0, st, (const uint64_t *)order, n, reversed, (I *)o->perm->perm);
    SPRS_TRY_HIP(hipGetLastError());
    stats[2] += 1;
    SPRS_TRY(perm_build_inverse(o->perm.get(), false, st));   // (synchronises the stream: the temporaries may go)
    SPRS_TRY_HIP(hipStreamSynchronize(st));
    return SPRS_HIP_OK;
}

}  // namespace od

// is_symmetric (symmetric.rs:7-34); a non-square matrix is not symmetric, without a launch
int32_t csmat_is_symmetric(const sprs_hip_csmat *m, int32_t *flag, hipStream_t st) {
    *flag = 0;
    if (m->rows != m->cols) return SPRS_HIP_OK;
    *flag = 1;
    if (!m->nnz) return SPRS_HIP_OK;
    if (m->nnz / od::OD_TILE > 0x7FFFFFFEull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "is_symmetric: more than 2^42 entries are not supported");
    DevBuf bad;
    SPRS_TRY_HIP(bad.alloc_for(st, 16));
    SPRS_TRY_HIP(hipMemsetAsync(bad.p, 0, 16, st));
    dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((od::od_symmetric_kernel<P, I>), dim3(od::tiles_for(m->nnz)), dim3(od::OD_BLOCK), 0, st, (const P *)m->indptr,
                           (const I *)m->indices, (const double *)m->data, m->outer(), m->nnz, bad.as<unsigned int>());
    });
    SPRS_TRY_HIP(hipGetLastError());
    unsigned int differs = 0;
    SPRS_TRY_HIP(copy_to_host(&differs, bad.p, 4, st));
    *flag = differs ? 0 : 1;
    return SPRS_HIP_OK;
}

// CsMat::degrees (csmat.rs:1205-1216) into a device array of outer() u64; asynchronous on `st`
int32_t csmat_degrees(const sprs_hip_csmat *m, uint64_t *out, hipStream_t st) {
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        return od::degrees_run<typename decltype(p)::type, typename decltype(i)::type>(m, out, nullptr, st);
    });
}

// CsMat::max_outer_nnz (csmat.rs:1188-1193)
int32_t csmat_max_outer_nnz(const sprs_hip_csmat *m, uint64_t *out, hipStream_t st) {
    *out = 0;
    if (!m->outer() || !m->nnz) return SPRS_HIP_OK;
    DevBuf mx;
    SPRS_TRY_HIP(mx.alloc_for(st, 16));
    SPRS_TRY(dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        return od::degrees_run<typename decltype(p)::type, typename decltype(i)::type>(m, nullptr, mx.u64(), st);
    }));
    SPRS_TRY_HIP(copy_to_host(out, mx.p, 8, st));
    return SPRS_HIP_OK;
}

// cuthill_mckee_custom (ordering.rs:440-526) on a square handle: fills o->perm (made here, in m's index widths), o->parts and
// o->stats.  Complete on `st` at return.
int32_t csmat_cuthill_mckee(const sprs_hip_csmat *m, int32_t strategy, bool reversed, sprs_hip_ordering *o, hipStream_t st) {
    const uint64_t n = m->outer();
    o->dim = n;
    SPRS_TRY(make_perm(o->perm, n, m->idx_bytes, m->user_idx_bytes()));
    if (n == 0) {                                    // an empty permutation, connected_parts == [0]
        o->parts.assign(1, 0);
        return SPRS_HIP_OK;
    }
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        return od::cm_run<typename decltype(p)::type, typename decltype(i)::type>(m, strategy, reversed, o, st);
    });
}

}  // namespace sprs_hip
