// Permutations for gfx950 — device twins of sprs/src/sparse/permutation.rs:
//   PermOwned::new / inv / vec / inv_vec / is_identity     permutation.rs:39-66, 113-152, 211-226
//   `&P * x`                                                permutation.rs:255-278    y[i] = x[p[i]]
//   permute_rows / permute_cols / transform_mat_papt / transform_mat_paq   permutation.rs:296-591
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// ONE ALGORITHM.  All four matrix functions are: output outer slice r' is input outer slice o[r'], every inner index j becomes
// g[j], the slice is sorted by the new index (csmat_permute below; o or g null = the identity on that side).  Values are
// moved, never computed: they travel as 64-bit words, so -0.0, explicit zeros, infinities and NaN payloads arrive as they left.
//
//  1. perm_len_kernel: len'[r'] = indptr[o[r'] + 1] - indptr[o[r']] and, with a g, the number of rows per length class;
//     exclusive_scan_u64 (scan.hip) gives the new slice starts, perm_indptr_kernel writes them at the handle's width.  nnz does
//     not change, so nothing is read back to size the result.
//  2. g == identity (a one-sided outer permutation): no sort.  perm_copy_kernel is tiled on the OUTPUT nnz axis — a workgroup
//     takes PM_TILE consecutive result entries and finds their slices by searching the new slice starts (staged in LDS), as the
//     SpMM and binop tiles do.  Stores are coalesced; row lengths do not enter the partition.
//  3. g != identity: perm_list_kernel lists the rows by class (one array, the classes one after the other), then
//       <= 16 / 32 / 64 entries   perm_micro_kernel<G>: lane groups, 4 / 2 / 1 rows per wave, group_sort<G> (lanes.hpp) on the
//                                 64-bit key (g[j] << 6) | slot; the values are gathered by slot after the sort
//       <= PM_WAVE_CAP entries    perm_mid_kernel<64>: one WAVE per row (four rows per workgroup), bitonic sort of
//                                 (g[j] << 12) | slot in LDS, no workgroup barrier
//       <= PM_CAP entries         perm_mid_kernel<256>: the same sort by one workgroup per row
//       >  PM_CAP entries (hubs)  never walked by one workgroup: the entries of all hub rows together get the key
//                                 (hub number << 40) | g[j] and the value "source position" and go through radix_sort_pairs
//                                 (sort.hip); every hub row keeps its segment, so sorted position i is result position
//                                 start'[row] + i - first[hub]
//     Keys are unique inside a slice (a validated handle has no duplicates and g is a bijection), so no sort has to be stable.
//  4. P * x is a gather; the inverse, the validation and is_identity are one small kernel each.
//  5. structure.hpp (new_from_unsorted) runs the same row passes and sorts with o = g = identity and a row mask `pick`: only the
//     masked rows are counted, listed and sorted — keyed on their own indices — and every other row is copied.
// An unvalidated handle or permutation (unsorted, duplicated or out-of-range values) gives an unspecified result but never an
// access outside the arrays: a source row >= outer counts as empty, slice bounds are clamped to nnz, an inner index >= inner
// is not looked up in g, and every store is tested against nnz.
#pragma once

#include <vector>

#include "common.hpp"
#include "lanes.hpp"
#include "scan.hpp"

namespace sprs_hip {

int32_t radix_sort_pairs(uint64_t *keys, uint64_t *vals, uint64_t n, const std::vector<std::pair<int, int>> &fields, hipStream_t stream);   // sort.hip

namespace pm {

constexpr int PM_BLOCK = 256;
constexpr int PM_TILE = 2048;                       // option perm_tile (fixed: min = max = default)
constexpr int PM_ITEMS = PM_TILE / PM_BLOCK;
constexpr int PM_ROWS = 2048;                       // slice starts of a tile kept in LDS; a tile that meets more slices reads them from memory
constexpr int PM_CAP = 4096;                        // option perm_cap (fixed): longest row sorted in LDS by one workgroup
constexpr int PM_CHUNK = 8192;                      // rows per workgroup of the two row passes (one atomic per class and workgroup)
constexpr int PM_WAVE_CAP = 1024;                   // longest row sorted in LDS by ONE wave (four rows per workgroup, no workgroup barrier)
constexpr int PM_CLASSES = 6;                       // <= 16, <= 32, <= 64, <= PM_WAVE_CAP, <= PM_CAP, hubs
constexpr int PM_HUB_SHIFT = 40;                    // hub key = (hub number << 40) | new inner index
constexpr uint64_t PM_PAD = ~0ull;

__device__ __forceinline__ int length_class(uint64_t len) {
    return len == 0 ? -1 : len <= 16 ? 0 : len <= 32 ? 1 : len <= 64 ? 2 : len <= (uint64_t)PM_WAVE_CAP ? 3 : len <= (uint64_t)PM_CAP ? 4 : 5;
}

// the class of row r when only the rows with pick[r] != 0 are sorted (structure.hpp; a null `pick` = every row)
__device__ __forceinline__ int picked_class(const uint8_t *pick, uint64_t r, uint64_t len) {
    return pick && !pick[r] ? -1 : length_class(len);
}

// the source slice of result slice r: [s, s + len) inside [0, nnz), empty when o[r] is no slice of the matrix
template <typename P, typename I>
__device__ __forceinline__ uint64_t source_slice(const P *ip, const I *o, uint64_t r, uint64_t outer, uint64_t nnz, uint64_t *len) {
    const uint64_t sr = o ? (uint64_t)o[r] : r;
    *len = 0;
    if (sr >= outer) return 0;
    uint64_t s = (uint64_t)ip[sr], e = (uint64_t)ip[sr + 1];
    if (e > nnz) e = nnz;
    if (s > e) s = e;
    *len = e - s;
    return s;
}

// the new label of inner index j
template <typename I>
__device__ __forceinline__ uint64_t relabel(const I *g, uint64_t j, uint64_t inner) {
    return (g && j < inner) ? (uint64_t)g[j] : j;
}

// 1. lens[r'] and, when `counts` is given, the rows per length class.  A workgroup takes PM_CHUNK consecutive rows and adds its
// five counts with ONE atomic each: an atomic per wave on the same five words took ~5 ms of the 17 ms of P A P^T on the 4096^2
// Laplacian (16.8 M rows).
template <typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_len_kernel(const P *ip, const I *o, const uint8_t *pick, uint64_t outer, uint64_t nnz,
                                                            uint64_t *lens, unsigned long long *counts) {
    __shared__ uint32_t s_cnt[PM_CLASSES];
    if (threadIdx.x < PM_CLASSES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * PM_CHUNK;
    uint32_t mine[PM_CLASSES] = {};
    for (int it = 0; it < PM_CHUNK / PM_BLOCK; ++it) {
        const uint64_t r = r0 + (uint64_t)it * PM_BLOCK + threadIdx.x;
        if (r >= outer) break;
        uint64_t len;
        (void)source_slice(ip, o, r, outer, nnz, &len);
        lens[r] = len;
        const int cls = picked_class(pick, r, len);
#pragma unroll
        for (int c = 0; c < PM_CLASSES; ++c) mine[c] += cls == c ? 1u : 0u;
    }
    if (!counts) return;
#pragma unroll
    for (int c = 0; c < PM_CLASSES; ++c)
        if (mine[c]) atomicAdd(&s_cnt[c], mine[c]);
    __syncthreads();
    if (threadIdx.x < PM_CLASSES && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// the new indptr at the handle's width (a total above nnz — possible only with an unvalidated permutation — is clamped)
template <typename P>
__global__ void __launch_bounds__(PM_BLOCK) perm_indptr_kernel(const uint64_t *offs, uint64_t n, uint64_t nnz, P *out) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i < n) out[i] = (P)(offs[i] < nnz ? offs[i] : nnz);
}

// 3. list[base[c] ..] = the rows of class c (in no particular order: every row knows its place in the result).  A workgroup
// counts the rows of its PM_CHUNK by class, reserves its five ranges with one atomic each and fills them.
__global__ void __launch_bounds__(PM_BLOCK) perm_list_kernel(const uint64_t *offs, const uint8_t *pick, uint64_t outer,
                                                             const unsigned long long *counts, unsigned long long *cursor, uint64_t *list) {
    __shared__ uint32_t s_cnt[PM_CLASSES], s_cur[PM_CLASSES];
    __shared__ uint64_t s_base[PM_CLASSES];
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x < PM_CLASSES) s_cnt[threadIdx.x] = s_cur[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * PM_CHUNK;
    uint32_t mine[PM_CLASSES] = {};
    for (int it = 0; it < PM_CHUNK / PM_BLOCK; ++it) {
        const uint64_t r = r0 + (uint64_t)it * PM_BLOCK + threadIdx.x;
        if (r >= outer) break;
        const int cls = picked_class(pick, r, offs[r + 1] - offs[r]);
#pragma unroll
        for (int c = 0; c < PM_CLASSES; ++c) mine[c] += cls == c ? 1u : 0u;
    }
#pragma unroll
    for (int c = 0; c < PM_CLASSES; ++c)
        if (mine[c]) atomicAdd(&s_cnt[c], mine[c]);
    __syncthreads();
    if (threadIdx.x < PM_CLASSES) {
        uint64_t base = 0;
        for (uint32_t c = 0; c < threadIdx.x; ++c) base += counts[c];
        s_base[threadIdx.x] = base + (s_cnt[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]) : 0ull);
    }
    __syncthreads();
    for (int it = 0; it < PM_CHUNK / PM_BLOCK; ++it) {
        const uint64_t rw = r0 + (uint64_t)it * PM_BLOCK + (threadIdx.x & ~63u);      // the wave's first row: the waves loop alike
        if (rw >= outer) break;
        const uint64_t r = rw + lane;
        const int cls = r < outer ? picked_class(pick, r, offs[r + 1] - offs[r]) : -1;
        for (int c = 0; c < PM_CLASSES; ++c) {
            const uint64_t mask = __ballot(cls == c);
            uint32_t first = 0;
            if (lane == 0 && mask) first = atomicAdd(&s_cur[c], (uint32_t)__popcll(mask));
            first = __shfl(first, 0, 64);
            if (cls == c) {
                const uint64_t pos = s_base[c] + first + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (pos < outer) list[pos] = r;
            }
        }
    }
}

// 2. one tile of PM_TILE result entries, copied from their source slices
template <typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_copy_kernel(const uint64_t *offs, const P *ip, const I *o, const I *ix, const uint64_t *val,
                                                             uint64_t outer, uint64_t nnz, I *ix_out, uint64_t *v_out) {
    __shared__ int32_t s_off[PM_ROWS + 1];          // slice starts relative to the tile (-1: in front of it)
    __shared__ int64_t s_delta[PM_ROWS];            // source position - result position of the slice's entries
    __shared__ uint64_t s_edge[2];
    const int tid = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * PM_TILE;
    const uint64_t total = offs[outer] < nnz ? offs[outer] : nnz;
    const uint64_t k1 = k0 + PM_TILE < total ? k0 + PM_TILE : total;
    if (k0 >= k1) return;
    if (tid < 2) {                                  // the last slice that starts at or before the tile's first / last entry
        const uint64_t k = tid == 0 ? k0 : k1 - 1;
        uint64_t lo = 0, hi = outer - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        s_edge[tid] = lo;
    }
    __syncthreads();
    const uint64_t rlo = s_edge[0], rhi = s_edge[1];
    const int64_t nrows = (int64_t)(rhi - rlo) + 1;
    const bool staged = nrows <= PM_ROWS;
    if (staged) {
        for (int64_t x = tid; x <= nrows; x += PM_BLOCK) {
            const uint64_t start = offs[rlo + x];
            s_off[x] = start < k0 ? -1 : (int32_t)(start - k0 < (uint64_t)PM_TILE + 1 ? start - k0 : (uint64_t)PM_TILE + 1);
            if (x < nrows) {
                uint64_t len;
                const uint64_t s = source_slice(ip, o, rlo + x, outer, nnz, &len);
                s_delta[x] = (int64_t)s - (int64_t)start;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PM_ITEMS; ++j) {
        const int32_t q = j * PM_BLOCK + tid;
        const uint64_t pos = k0 + (uint64_t)q;
        if (pos >= k1) continue;
        int64_t delta;
        if (staged) {
            int32_t lo = 0, hi = (int32_t)nrows - 1;
            while (lo < hi) {
                const int32_t mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            delta = s_delta[lo];
        } else {
            uint64_t lo = rlo, hi = rhi;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (offs[mid] <= pos) lo = mid;
                else hi = mid - 1;
            }
            uint64_t len;
            delta = (int64_t)source_slice(ip, o, lo, outer, nnz, &len) - (int64_t)offs[lo];
        }
        const uint64_t src = (uint64_t)((int64_t)pos + delta);
        if (src < nnz) {
            ix_out[pos] = ix[src];
            v_out[pos] = val[src];
        }
    }
}

// 3a. rows of at most G entries: a group of G lanes per row
template <int G, typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_micro_kernel(const uint64_t *list, uint64_t count, const uint64_t *offs, const P *ip,
                                                              const I *o, const I *g, const I *ix, const uint64_t *val, uint64_t outer,
                                                              uint64_t inner, uint64_t nnz, I *ix_out, uint64_t *v_out) {
    const uint64_t gid = ((uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x) / G;
    const uint32_t gl = threadIdx.x & (uint32_t)(G - 1);
    uint64_t s = 0, d = 0, len = 0;
    if (gid < count) {
        const uint64_t r = list[gid];
        if (r < outer) {
            s = source_slice(ip, o, r, outer, nnz, &len);
            d = offs[r];
        }
    }
    const bool mine = gl < len && len <= (uint64_t)G && d + gl < nnz;
    uint64_t key = PM_PAD;
    if (mine) key = (relabel(g, (uint64_t)ix[s + gl], inner) << 6) | gl;
    key = group_sort<G>(key);                       // the padding sorts behind the row's entries
    if (mine && key != PM_PAD) {
        ix_out[d + gl] = (I)(key >> 6);
        v_out[d + gl] = val[s + (key & 63)];
    }
}

// 3b. rows of at most CAP entries sorted in LDS by TPR threads: one wave per row (four rows per workgroup, the wave hands its
// LDS data on without a workgroup barrier) up to PM_WAVE_CAP entries, the whole workgroup per row up to PM_CAP
template <int TPR, int CAP, typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_mid_kernel(const uint64_t *list, uint64_t count, const uint64_t *offs, const P *ip,
                                                            const I *o, const I *g, const I *ix, const uint64_t *val, uint64_t outer,
                                                            uint64_t inner, uint64_t nnz, I *ix_out, uint64_t *v_out) {
    constexpr int RPB = PM_BLOCK / TPR;             // rows per workgroup
    __shared__ uint64_t keys_s[RPB][CAP];
    const uint32_t tid = threadIdx.x & (uint32_t)(TPR - 1), sub = threadIdx.x / TPR;
    uint64_t *keys = keys_s[sub];
    const uint64_t at = (uint64_t)blockIdx.x * RPB + sub;
    uint64_t len = 0, s = 0, d = 0;
    if (at < count) {
        const uint64_t r = list[at];
        if (r < outer) {
            s = source_slice(ip, o, r, outer, nnz, &len);
            d = offs[r];
        }
    }
    if (len > (uint64_t)CAP) len = 0;
    uint32_t size = 2;
    while (size < len) size <<= 1;
    if (TPR == PM_BLOCK && len == 0) return;        // (the whole workgroup: no barrier is left behind)
    for (uint32_t i = tid; i < size; i += TPR) keys[i] = i < len ? (relabel(g, (uint64_t)ix[s + i], inner) << 12) | i : PM_PAD;
    if (TPR == PM_BLOCK) __syncthreads();
    else wave_sync_lds();
    for (uint32_t k2 = 2; k2 <= size; k2 <<= 1) {
        for (uint32_t jj = k2 >> 1; jj > 0; jj >>= 1) {
            for (uint32_t i = tid; i < size; i += TPR) {
                const uint32_t l = i ^ jj;
                if (l > i) {
                    const uint64_t ki = keys[i], kl = keys[l];
                    if ((ki > kl) == ((i & k2) == 0)) {
                        keys[i] = kl;
                        keys[l] = ki;
                    }
                }
            }
            if (TPR == PM_BLOCK) __syncthreads();
            else wave_sync_lds();
        }
    }
    for (uint32_t i = tid; i < len; i += TPR) {
        const uint64_t key = keys[i];
        if (d + i < nnz && key != PM_PAD) {
            ix_out[d + i] = (I)(key >> 12);
            v_out[d + i] = val[s + (key & 4095)];
        }
    }
}

// 3c. hub rows.  hub_len[h] = entries of hub h; its exclusive scan `first` places the hubs' entries side by side.
__global__ void __launch_bounds__(PM_BLOCK) perm_hub_len_kernel(const uint64_t *list, uint64_t nhubs, const uint64_t *offs, uint64_t outer,
                                                                uint64_t *hub_len) {
    const uint64_t h = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (h >= nhubs) return;
    const uint64_t r = list[h];
    hub_len[h] = r < outer ? offs[r + 1] - offs[r] : 0;
}

__device__ __forceinline__ uint64_t hub_of(const uint64_t *first, uint64_t nhubs, uint64_t i) {
    uint64_t lo = 0, hi = nhubs - 1;                // the last hub with first[h] <= i (no hub is empty)
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_hub_keys_kernel(const uint64_t *list, uint64_t nhubs, const uint64_t *first, uint64_t n,
                                                                 const P *ip, const I *o, const I *g, const I *ix, uint64_t outer,
                                                                 uint64_t inner, uint64_t nnz, uint64_t *keys, uint64_t *srcs) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = hub_of(first, nhubs, i), r = list[h];
    uint64_t len = 0, s = 0;
    if (r < outer) s = source_slice(ip, o, r, outer, nnz, &len);
    const uint64_t at = i - first[h];
    const bool ok = at < len;                       // (s + at < nnz then)
    const uint64_t p = ok ? s + at : 0;
    const uint64_t nj = ok ? relabel(g, (uint64_t)ix[p], inner) : 0;
    keys[i] = (h << PM_HUB_SHIFT) | (nj & ((1ull << PM_HUB_SHIFT) - 1ull));
    srcs[i] = ok ? p : PM_PAD;
}

template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_hub_emit_kernel(const uint64_t *list, uint64_t nhubs, const uint64_t *first, uint64_t n,
                                                                 const uint64_t *keys, const uint64_t *srcs, const uint64_t *offs,
                                                                 const uint64_t *val, uint64_t outer, uint64_t nnz, I *ix_out,
                                                                 uint64_t *v_out) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i], h = key >> PM_HUB_SHIFT, p = srcs[i];
    if (h >= nhubs || p >= nnz) return;
    const uint64_t r = list[h];
    if (r >= outer || i < first[h]) return;
    const uint64_t pos = offs[r] + (i - first[h]);
    if (pos >= offs[r + 1] || pos >= nnz) return;
    ix_out[pos] = (I)(key & ((1ull << PM_HUB_SHIFT) - 1ull));
    v_out[pos] = val[p];
}

// ---- permutations themselves -----------------------------------------------------------------------------------------------

// inv[p[i]] = i for the values in range (nothing is written out of range whatever p holds); *bad |= 1 for a value >= dim
template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_scatter_inverse_kernel(const I *p, uint64_t dim, I *inv, unsigned int *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= dim) return;
    const uint64_t v = (uint64_t)p[i];
    if (v < dim) inv[v] = (I)i;
    else atomicOr(bad, 1u);
}

// a value that occurs twice was written twice: one of its two positions lost, whichever order the stores took
template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_check_inverse_kernel(const I *p, uint64_t dim, const I *inv, unsigned int *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= dim) return;
    const uint64_t v = (uint64_t)p[i];
    if (v < dim && (uint64_t)inv[v] != i) atomicOr(bad, 2u);
}

template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_not_identity_kernel(const I *p, uint64_t dim, unsigned int *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    // (one atomic per wave, and none once the flag is up: under a random permutation EVERY element differs, and 16.8 M atomics
    // on one word took milliseconds)
    const bool differs = i < dim && (uint64_t)p[i] != i;
    if (__ballot(differs) != 0 && (threadIdx.x & 63) == 0 && *(volatile unsigned int *)flag == 0) atomicOr(flag, 1u);
}

template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) perm_gather_kernel(const I *p, const uint64_t *x, uint64_t n, uint64_t *y) {
    const uint64_t stride = (uint64_t)gridDim.x * PM_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint64_t v = (uint64_t)p[i];
        y[i] = v < n ? x[v] : 0ull;
    }
}

inline unsigned blocks_for(uint64_t n) { return n ? (unsigned)((n + PM_BLOCK - 1) / PM_BLOCK) : 1u; }   // (every kernel tests its own bound)

inline unsigned chunks_for(uint64_t n) { return n ? (unsigned)((n + PM_CHUNK - 1) / PM_CHUNK) : 1u; }

inline int bits_for(uint64_t n) {                   // bits needed for values < n
    int b = 1;
    while (b < 63 && (1ull << b) < n) ++b;
    return b;
}

// `pick` (structure.hpp, with o = g = null): only the rows with pick[r] != 0 go through the sorts, keyed on their own indices;
// every other row is copied as it is
template <typename P, typename I>
int32_t run(const sprs_hip_csmat *m, const void *o_, const void *g_, const uint8_t *pick, sprs_hip_csmat *res, hipStream_t st) {
    const uint64_t outer = m->outer(), inner = m->inner(), nnz = m->nnz;
    const P *ip = (const P *)m->indptr;
    const I *ix = (const I *)m->indices, *o = (const I *)o_, *g = (const I *)g_;
    const uint64_t *val = (const uint64_t *)m->data;
    I *ix_out = (I *)res->indices;
    uint64_t *v_out = (uint64_t *)res->data;
    if (outer >= 0xFFFFFFFFull * PM_BLOCK) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "permutation: more than 2^40 outer slices are not supported");
    // lens (outer) | offs (outer + 1) | counts, cursors (PM_CLASSES each)
    DevBuf tmp, listb;
    SPRS_TRY_HIP(tmp.alloc_for(st, (2 * outer + 1 + 2 * PM_CLASSES) * 8));
    uint64_t *lens = tmp.u64(), *offs = lens + outer;
    unsigned long long *counts = (unsigned long long *)(offs + outer + 1), *cursor = counts + PM_CLASSES;
    const bool sorting = (g != nullptr || pick != nullptr) && nnz != 0;
    SPRS_TRY_HIP(hipMemsetAsync(counts, 0, 2 * PM_CLASSES * 8, st));
    hipLaunchKernelGGL((perm_len_kernel<P, I>), dim3(chunks_for(outer)), dim3(PM_BLOCK), 0, st, ip, o, pick, outer, nnz, lens,
                       sorting ? counts : (unsigned long long *)nullptr);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(lens, offs, outer, st));
    hipLaunchKernelGGL(perm_indptr_kernel<P>, dim3(blocks_for(outer + 1)), dim3(PM_BLOCK), 0, st, (const uint64_t *)offs, outer + 1, nnz,
                       (P *)res->indptr);
    SPRS_TRY_HIP(hipGetLastError());
    if (nnz == 0) {
        SPRS_TRY_HIP(hipStreamSynchronize(st));
        return SPRS_HIP_OK;
    }
    if (!sorting) {
        const uint64_t ntiles = (nnz + PM_TILE - 1) / PM_TILE;
        if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "permutation: more than 2^42 entries are not supported");
        hipLaunchKernelGGL((perm_copy_kernel<P, I>), dim3((unsigned)ntiles), dim3(PM_BLOCK), 0, st, (const uint64_t *)offs, ip, o, ix, val,
                           outer, nnz, ix_out, v_out);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY_HIP(hipStreamSynchronize(st));
        return SPRS_HIP_OK;
    }
    if (inner > (1ull << PM_HUB_SHIFT)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "permutation: an inner dimension above 2^40 is not supported");
    if (pick) {                                     // the rows that no sort rewrites
        SPRS_TRY_HIP(hipMemcpyAsync(ix_out, ix, nnz * sizeof(I), hipMemcpyDeviceToDevice, st));
        SPRS_TRY_HIP(hipMemcpyAsync(v_out, val, nnz * 8, hipMemcpyDeviceToDevice, st));
    }
    SPRS_TRY_HIP(listb.alloc_for(st, outer * 8));
    uint64_t *list = listb.u64();
    hipLaunchKernelGGL(perm_list_kernel, dim3(chunks_for(outer)), dim3(PM_BLOCK), 0, st, (const uint64_t *)offs, pick, outer,
                       (const unsigned long long *)counts, cursor, list);
    SPRS_TRY_HIP(hipGetLastError());
    uint64_t cnt[PM_CLASSES];
    SPRS_TRY_HIP(copy_to_host(cnt, counts, sizeof cnt, st));
    uint64_t base[PM_CLASSES + 1] = {0};
    for (int c = 0; c < PM_CLASSES; ++c) base[c + 1] = base[c] + cnt[c];
    if (base[PM_CLASSES] > outer) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "permutation: inconsistent row count");
    if (cnt[0]) {
        hipLaunchKernelGGL((perm_micro_kernel<16, P, I>), dim3(blocks_for(cnt[0] * 16)), dim3(PM_BLOCK), 0, st, (const uint64_t *)list + base[0],
                           cnt[0], (const uint64_t *)offs, ip, o, g, ix, val, outer, inner, nnz, ix_out, v_out);
    }
    if (cnt[1]) {
        hipLaunchKernelGGL((perm_micro_kernel<32, P, I>), dim3(blocks_for(cnt[1] * 32)), dim3(PM_BLOCK), 0, st, (const uint64_t *)list + base[1],
                           cnt[1], (const uint64_t *)offs, ip, o, g, ix, val, outer, inner, nnz, ix_out, v_out);
    }
    if (cnt[2]) {
        hipLaunchKernelGGL((perm_micro_kernel<64, P, I>), dim3(blocks_for(cnt[2] * 64)), dim3(PM_BLOCK), 0, st, (const uint64_t *)list + base[2],
                           cnt[2], (const uint64_t *)offs, ip, o, g, ix, val, outer, inner, nnz, ix_out, v_out);
    }
    if (cnt[3] > 0x7FFFFFFFull || cnt[4] > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "permutation: more than 2^31 rows above 64 entries are not supported");
    if (cnt[3]) {
        hipLaunchKernelGGL((perm_mid_kernel<64, PM_WAVE_CAP, P, I>), dim3(blocks_for(cnt[3] * 64)), dim3(PM_BLOCK), 0, st,
                           (const uint64_t *)list + base[3], cnt[3], (const uint64_t *)offs, ip, o, g, ix, val, outer, inner, nnz, ix_out, v_out);
    }
    if (cnt[4]) {
        hipLaunchKernelGGL((perm_mid_kernel<PM_BLOCK, PM_CAP, P, I>), dim3((unsigned)cnt[4]), dim3(PM_BLOCK), 0, st,
                           (const uint64_t *)list + base[4], cnt[4], (const uint64_t *)offs, ip, o, g, ix, val, outer, inner, nnz, ix_out, v_out);
    }
    SPRS_TRY_HIP(hipGetLastError());
    const uint64_t nhubs = cnt[5];
    if (nhubs) {
        if (nhubs >= (1ull << (64 - PM_HUB_SHIFT))) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "permutation: more than 2^24 hub rows are not supported");
        const uint64_t *hubs = list + base[5];
        // hub_len (nhubs) | first (nhubs + 1)
        DevBuf hb, keys, srcs;
        SPRS_TRY_HIP(hb.alloc_for(st, (2 * nhubs + 1) * 8));
        uint64_t *hub_len = hb.u64(), *first = hub_len + nhubs;
        hipLaunchKernelGGL(perm_hub_len_kernel, dim3(blocks_for(nhubs)), dim3(PM_BLOCK), 0, st, hubs, nhubs, (const uint64_t *)offs, outer, hub_len);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(exclusive_scan_u64(hub_len, first, nhubs, st));
        uint64_t n = 0;
        SPRS_TRY_HIP(copy_to_host(&n, first + nhubs, 8, st));
        if (n > nnz) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "permutation: inconsistent hub count");
        SPRS_TRY_HIP(keys.alloc_for(st, n * 8));
        SPRS_TRY_HIP(srcs.alloc_for(st, n * 8));
        hipLaunchKernelGGL((perm_hub_keys_kernel<P, I>), dim3(blocks_for(n)), dim3(PM_BLOCK), 0, st, hubs, nhubs, (const uint64_t *)first, n, ip, o,
                           g, ix, outer, inner, nnz, keys.u64(), srcs.u64());
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(radix_sort_pairs(keys.u64(), srcs.u64(), n, {{0, bits_for(inner)}, {PM_HUB_SHIFT, bits_for(nhubs)}}, st));
        hipLaunchKernelGGL(perm_hub_emit_kernel<I>, dim3(blocks_for(n)), dim3(PM_BLOCK), 0, st, hubs, nhubs, (const uint64_t *)first, n,
                           (const uint64_t *)keys.u64(), (const uint64_t *)srcs.u64(), (const uint64_t *)offs, val, outer, nnz, ix_out, v_out);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY_HIP(hipStreamSynchronize(st));     // (the hub temporaries go with this scope)
    }
    SPRS_TRY_HIP(hipStreamSynchronize(st));         // the result is complete when the call returns (and the temporaries may go)
    return SPRS_HIP_OK;
}

}  // namespace pm

// The one algorithm of permutation.rs:296-591 on a handle: result outer slice r' = outer slice o[r'] of m, inner index j -> g[j],
// slices sorted.  o / g: device arrays of m's index type with outer / inner entries, or null for the identity.  A new handle
// in m's storage and widths; m is only read.  Blocks until the result is complete on `st`.
int32_t csmat_permute(const sprs_hip_csmat *m, const void *o, const void *g, OwnedCsmat &out, hipStream_t st) {
    OwnedCsmat res;
    if (!o && !g) {                                 // the reference's shortcuts: a plain copy
        SPRS_TRY(copy_csmat(m, true, res, st));
        SPRS_TRY_HIP(hipStreamSynchronize(st));
    } else {
        SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, m->nnz, m->iptr_bytes, m->idx_bytes));
        SPRS_TRY(dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
            return pm::run<typename decltype(p)::type, typename decltype(i)::type>(m, o, g, nullptr, res.get(), st);
        }));
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

// ---- PermOwned ---------------------------------------------------------------------------------------------------------------

// perm_inv[perm[i]] = i (permutation.rs:52-66) and, with `validate`, perm_is_valid (permutation.rs:39-49) on the device
int32_t perm_build_inverse(sprs_hip_perm *p, bool validate, hipStream_t st) {
    if (p->dim == 0) return SPRS_HIP_OK;
    DevBuf bad;
    SPRS_TRY_HIP(bad.alloc(16));
    SPRS_TRY_HIP(hipMemsetAsync(bad.p, 0, 16, st));
    dispatch_width(p->idx_bytes, [&](auto i) {
        using I = typename decltype(i)::type;
        hipLaunchKernelGGL(pm::perm_scatter_inverse_kernel<I>, dim3(pm::blocks_for(p->dim)), dim3(pm::PM_BLOCK), 0, st, (const I *)p->perm, p->dim,
                           (I *)p->perm_inv, bad.as<unsigned int>());
        if (validate)
            hipLaunchKernelGGL(pm::perm_check_inverse_kernel<I>, dim3(pm::blocks_for(p->dim)), dim3(pm::PM_BLOCK), 0, st, (const I *)p->perm,
                               p->dim, (const I *)p->perm_inv, bad.as<unsigned int>());
    });
    SPRS_TRY_HIP(hipGetLastError());
    unsigned int flag = 0;
    SPRS_TRY_HIP(copy_to_host(&flag, bad.p, 4, st));
    if (validate && flag) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "invalid permutation");
    return SPRS_HIP_OK;
}

// PermOwned::is_identity (permutation.rs:144-152): the Identity variant, or a stored permutation equal to 0..dim
int32_t perm_is_identity(const sprs_hip_perm *p, int32_t *flag, hipStream_t st) {
    *flag = 1;
    if (p->identity || p->dim == 0) return SPRS_HIP_OK;
    DevBuf bad;
    SPRS_TRY_HIP(bad.alloc(16));
    SPRS_TRY_HIP(hipMemsetAsync(bad.p, 0, 16, st));
    dispatch_width(p->idx_bytes, [&](auto i) {
        using I = typename decltype(i)::type;
        hipLaunchKernelGGL(pm::perm_not_identity_kernel<I>, dim3(pm::blocks_for(p->dim)), dim3(pm::PM_BLOCK), 0, st, (const I *)p->perm, p->dim,
                           bad.as<unsigned int>());
    });
    SPRS_TRY_HIP(hipGetLastError());
    unsigned int differs = 0;
    SPRS_TRY_HIP(copy_to_host(&differs, bad.p, 4, st));
    *flag = differs ? 0 : 1;
    return SPRS_HIP_OK;
}

// `&P * x` (permutation.rs:255-278): y[i] = x[p[i]], Identity copies; asynchronous on `st`
int32_t perm_mul_vec_f64(const sprs_hip_perm *p, const double *x, double *y, hipStream_t st) {
    if (p->dim == 0) return SPRS_HIP_OK;
    if (p->identity) {
        SPRS_TRY_HIP(hipMemcpyAsync(y, x, p->dim * sizeof(double), hipMemcpyDeviceToDevice, st));
        return SPRS_HIP_OK;
    }
    uint64_t blocks = pm::blocks_for(p->dim);
    if (blocks > 256 * 32) blocks = 256 * 32;
    dispatch_width(p->idx_bytes, [&](auto i) {
        using I = typename decltype(i)::type;
        hipLaunchKernelGGL(pm::perm_gather_kernel<I>, dim3((unsigned)blocks), dim3(pm::PM_BLOCK), 0, st, (const I *)p->perm, (const uint64_t *)x,
                           p->dim, (uint64_t *)y);
    });
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
