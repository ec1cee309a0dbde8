// Structure checks and unsorted input for gfx950 — device twins of
//   utils::check_compressed_structure                         sprs/src/sparse.rs:300-358 (+ IndPtrBase::check_structure, indptr.rs:37-74)
//   CsMat::new_from_unsorted / new_from_unsorted_csc          csmat.rs:311-401
//   CsVec::new_from_unsorted                                  vec.rs:536-557
// Included by convert.hip behind perm.hpp (one translation unit of the library and of the emulator build, tests/emu).
//
// THE CHECK runs in the reference's order and never lets one array address another before the first is known to be sound:
//  1. the dimensions against the (declared) index widths — host arithmetic;
//  2. indptr_check_kernel, a pass of its own over the outer + 1 slice starts: the first decreasing pair, indptr[0] and
//     indptr[outer] come back in one read.  Any finding returns here.  After a clean pass the starts are monotone, begin at 0
//     and end at nnz, so every one of them is a position inside `indices`.
//  3. rows_check_kernel, tiled on the nnz axis: a workgroup takes PM_TILE consecutive entries and finds their slices by
//     searching the slice starts (staged in LDS), as perm_copy_kernel does; row lengths do not enter the partition.  An entry
//     that is not the first of its slice and is <= its predecessor marks the slice Unsorted, a last entry >= inner marks it
//     OutOfRange.  Every workgroup folds its findings into the key (slice << 1) | (OutOfRange ? 1 : 0) and issues ONE integer
//     atomicMin: the answer is the lowest marked slice, Unsorted wins inside a slice, and the result does not depend on the
//     order the workgroups run in.
// Index arrays are read as UNSIGNED at the handle's width: a negative value of a signed tensor is a large index and reports
// OutOfRange for its slice.  (The reference tests every index for "Indices value out of range of usize" ahead of the slices, so
// it would report that negative value before an Unsorted slice in front of it; this check reports in slice order.)
//
// NEW_FROM_UNSORTED leaves its operand untouched (the reference sorts in place because it owns the arrays) and returns a new
// handle in the operand's storage and widths.  After the indptr pass, rows_check_kernel runs once more with two byte arrays: a
// slice "needs sorting" (some entry <= its predecessor) and / or "holds an index >= inner" (any entry, not only the last).
//   - nothing found at all: the result is a copy (the reference skips sorted slices too, csmat.rs:341);
//   - else pm::run (perm.hpp) with the mask needs && !range: the masked slices go by length class through the lane-group / LDS /
//     radix sorts keyed on their own index, every other slice is copied.  Values travel as 64-bit words.
//   - the check (3.) on the result finds the first slice that is still wrong: a sorted slice with two equal indices is
//     Unsorted ("Indices are not sorted").  Slices that hold an index >= inner never enter the packed-key sorts (their keys would
//     overflow); if such a slice is the first offender its kind must still be the reference's — Unsorted when it also holds a
//     duplicate, else OutOfRange — so that ONE slice is downloaded and sorted on the host, on the error path only.
// The vector follows vec.rs:536-557: check, sort only on Unsorted, check again.  Up to PM_CAP entries (and indices below 2^52,
// so that the packed key fits) the sort is perm_mid_kernel on a one-slice matrix; anything else goes through radix_sort_pairs on
// as many key bits as the largest index needs.
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "perm.hpp"

namespace sprs_hip {

namespace st {

using pm::PM_BLOCK;
using pm::PM_CAP;
using pm::PM_ITEMS;
using pm::PM_ROWS;
using pm::PM_TILE;

constexpr int32_t KIND_OK = 0, KIND_UNSORTED = 1, KIND_SIZE_MISMATCH = 2, KIND_OUT_OF_RANGE = 3;   // StructureErrorKind (errors.rs)
constexpr uint64_t NO_SLICE = ~0ull;
constexpr unsigned long long NO_KEY = ~0ull;

// 2. res[0] = the first i with indptr[i + 1] < indptr[i] (preset to ~0), res[1] = indptr[0], res[2] = indptr[outer]
template <typename P>
__global__ void __launch_bounds__(PM_BLOCK) indptr_check_kernel(const P *ip, uint64_t outer, uint64_t *res) {
    __shared__ unsigned long long s_min;
    if (threadIdx.x == 0) s_min = NO_KEY;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i < outer && (uint64_t)ip[i + 1] < (uint64_t)ip[i]) atomicMin(&s_min, (unsigned long long)i);
    if (i == 0) res[1] = (uint64_t)ip[0];
    if (i == outer) res[2] = (uint64_t)ip[outer];
    __syncthreads();
    if (threadIdx.x == 0 && s_min != NO_KEY) atomicMin((unsigned long long *)&res[0], s_min);
}

// 3. one tile of PM_TILE entries.  *key_out (preset to ~0) = min over the marked slices of (slice << 1) | (OutOfRange ? 1 : 0)
// under the rules of the check; with `needs` / `range` (outer bytes each, zeroed) the two facts new_from_unsorted sorts by.
// Reads indices[p] and indices[p - 1] for 0 < p < nnz only and indptr[r] for r <= outer only, whatever the arrays hold.
template <typename P, typename I>
__global__ void __launch_bounds__(PM_BLOCK) rows_check_kernel(const P *ip, const I *ix, uint64_t outer, uint64_t inner, uint64_t nnz,
                                                              uint8_t *needs, uint8_t *range, unsigned long long *key_out) {
    __shared__ int32_t s_off[PM_ROWS + 1];          // slice starts relative to the tile (-1: in front of it)
    __shared__ uint64_t s_edge[2];
    __shared__ unsigned long long s_key;
    const int tid = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * PM_TILE;
    const uint64_t k1 = k0 + PM_TILE < nnz ? k0 + PM_TILE : nnz;
    if (k0 >= k1 || outer == 0) return;
    if (tid == 0) s_key = NO_KEY;
    // the tile's entries and their predecessors are on their way while the slices are searched
    uint64_t vals[PM_ITEMS], prevs[PM_ITEMS];
#pragma unroll
    for (int j = 0; j < PM_ITEMS; ++j) {
        const uint64_t pos = k0 + (uint64_t)(j * PM_BLOCK + tid);
        vals[j] = pos < k1 ? (uint64_t)ix[pos] : 0;
        prevs[j] = pos < k1 && pos > 0 ? (uint64_t)ix[pos - 1] : 0;
    }
    // The last slice that starts at or before the tile's first (wave 0) / last (wave 1) entry.  The wave probes 64 evenly
    // spaced slice starts per step, so 2^24 slices take four dependent reads, not twenty-four: a tile's life is mostly this
    // search.  The range shrinks at every step whatever indptr holds, and no probe leaves [0, outer).
    if (tid < 128) {
        const uint32_t lane = (uint32_t)tid & 63u;
        const uint64_t k = tid < 64 ? k0 : k1 - 1;
        uint64_t lo = 0, hi = outer - 1;
        while (lo < hi) {
            const uint64_t step = (hi - lo) / 64 + 1;
            const uint64_t at = lo + (uint64_t)(lane + 1) * step;
            const bool le = at <= hi && (uint64_t)ip[at] <= k;
            const uint64_t cnt = (uint64_t)__popcll(__ballot(le));
            const uint64_t top = lo + (cnt + 1) * step - 1;
            lo += cnt * step;
            hi = top < hi ? top : hi;
        }
        if (lane == 0) s_edge[tid >> 6] = lo;
    }
    __syncthreads();
    const uint64_t rlo = s_edge[0], rhi = s_edge[1];
    const int64_t nrows = (int64_t)(rhi - rlo) + 1;
    const bool staged = rhi >= rlo && nrows <= PM_ROWS;
    if (staged) {
        for (int64_t x = tid; x <= nrows; x += PM_BLOCK) {
            const uint64_t start = (uint64_t)ip[rlo + x];
            s_off[x] = start < k0 ? -1 : (int32_t)(start - k0 < (uint64_t)PM_TILE + 1 ? start - k0 : (uint64_t)PM_TILE + 1);
        }
    }
    __syncthreads();
    unsigned long long mine = NO_KEY;
#pragma unroll
    for (int j = 0; j < PM_ITEMS; ++j) {
        const int32_t q = j * PM_BLOCK + tid;
        const uint64_t pos = k0 + (uint64_t)q;
        if (pos >= k1) continue;
        uint64_t r;
        bool first, last;
        if (staged) {
            int32_t lo = 0, hi = (int32_t)nrows - 1;
            while (lo < hi) {
                const int32_t mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            r = rlo + (uint64_t)lo;
            first = s_off[lo] == q;
            last = s_off[lo + 1] == q + 1;
        } else {
            uint64_t lo = rlo, hi = rhi < rlo ? rlo : rhi;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if ((uint64_t)ip[mid] <= pos) lo = mid;
                else hi = mid - 1;
            }
            r = lo;
            first = (uint64_t)ip[r] == pos;
            last = (uint64_t)ip[r + 1] == pos + 1;
        }
        const uint64_t v = vals[j];
        if (!first && pos > 0 && v <= prevs[j]) {
            const unsigned long long k = (unsigned long long)r << 1;
            mine = k < mine ? k : mine;
            if (needs) needs[r] = 1;
        }
        if (v >= inner) {
            if (last) {
                const unsigned long long k = ((unsigned long long)r << 1) | 1ull;
                mine = k < mine ? k : mine;
            }
            if (range) range[r] = 1;
        }
    }
    if (mine != NO_KEY) atomicMin(&s_key, mine);
    __syncthreads();
    // (at most one atomic per workgroup, and none once a lower key is up: on a matrix whose every slice is shuffled all
    // workgroups have a finding, and their atomics on this one word took longer than the pass itself.  The word only ever
    // falls, so a stale read costs an atomic that changes nothing, never an answer)
    if (tid == 0 && s_key != NO_KEY && s_key < *(volatile unsigned long long *)key_out) atomicMin(key_out, s_key);
}

// the mask of the sorts: a slice that needs sorting and holds no index >= inner
__global__ void __launch_bounds__(PM_BLOCK) pick_kernel(uint8_t *needs, const uint8_t *range, uint64_t outer) {
    const uint64_t r = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (r < outer) needs[r] = needs[r] && !range[r] ? 1 : 0;
}

// vectors: the largest index (one atomic per wave), the (index, position) pairs of the radix route and its gather
template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) vec_max_kernel(const I *ix, uint64_t n, unsigned long long *out) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    unsigned long long v = i < n ? (unsigned long long)ix[i] : 0ull;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long w = __shfl_xor(v, d, 64);
        v = w > v ? w : v;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, v);
}

template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) vec_keys_kernel(const I *ix, uint64_t n, uint64_t *keys, uint64_t *srcs) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = (uint64_t)ix[i];
    srcs[i] = i;
}

template <typename I>
__global__ void __launch_bounds__(PM_BLOCK) vec_emit_kernel(const uint64_t *keys, const uint64_t *srcs, const uint64_t *val, uint64_t n,
                                                            I *ix_out, uint64_t *v_out) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n || srcs[i] >= n) return;
    ix_out[i] = (I)keys[i];
    v_out[i] = val[srcs[i]];
}

inline uint64_t width_max(int32_t bytes) { return bytes >= 8 ? ~0ull : ((1ull << (8 * bytes)) - 1ull); }

// fills `info` and, for a finding, records the reference's text
inline int32_t report(sprs_hip_structure_info *info, int32_t kind, uint64_t outer, const char *text) {
    if (info) {
        info->kind = kind;
        info->reserved = 0;
        info->outer = outer;
    }
    if (kind == KIND_OK) return SPRS_HIP_OK;
    SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "%s", text);
}

// steps 1 and 2 of the check
template <typename P>
int32_t indptr_pass(const sprs_hip_csmat *m, sprs_hip_structure_info *info, hipStream_t s) {
    const uint64_t outer = m->outer(), inner = m->inner();
    if (inner > width_max(m->user_idx_bytes())) return report(info, KIND_OUT_OF_RANGE, NO_SLICE, "Index type not large enough for this matrix");
    if (outer + 1 > width_max(m->user_iptr_bytes()) || outer + 1 == 0)
        return report(info, KIND_OUT_OF_RANGE, NO_SLICE, "Iptr type not large enough for this matrix");
    if (outer >= 0xFFFFFFFFull * PM_BLOCK) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "check_structure: more than 2^40 outer slices are not supported");
    DevBuf res;
    SPRS_TRY_HIP(res.alloc_for(s, 24));
    uint64_t host[3] = {NO_SLICE, 0, 0};
    SPRS_TRY_HIP(copy_to_device(res.p, host, sizeof host, s));
    hipLaunchKernelGGL(indptr_check_kernel<P>, dim3(pm::blocks_for(outer + 1)), dim3(PM_BLOCK), 0, s, (const P *)m->indptr, outer, res.u64());
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(copy_to_host(host, res.p, sizeof host, s));
    if (host[0] != NO_SLICE) return report(info, KIND_UNSORTED, NO_SLICE, "Unsorted indptr");
    if (host[2] > (UINT64_MAX >> 1)) return report(info, KIND_OUT_OF_RANGE, NO_SLICE, "An indptr value is larger than allowed");
    if (host[2] - host[1] != m->nnz) return report(info, KIND_SIZE_MISMATCH, NO_SLICE, "Indices length and inpdtr's nnz do not match");
    if (host[1] != 0) {
        if (info) *info = sprs_hip_structure_info{KIND_OK, 0, NO_SLICE};
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "the indptr of a device handle must start at 0");
    }
    return SPRS_HIP_OK;
}

// step 3 on the arrays ip / ix of a matrix shaped like m; *key = the packed answer (NO_KEY: nothing found)
template <typename P, typename I>
int32_t rows_pass(const sprs_hip_csmat *m, const void *ip, const void *ix, uint8_t *needs, uint8_t *range, unsigned long long *key,
                  hipStream_t s) {
    *key = NO_KEY;
    if (m->nnz == 0) return SPRS_HIP_OK;
    const uint64_t ntiles = (m->nnz + PM_TILE - 1) / PM_TILE;
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "check_structure: more than 2^42 entries are not supported");
    DevBuf res;
    SPRS_TRY_HIP(res.alloc_for(s, 8));
    SPRS_TRY_HIP(copy_to_device(res.p, key, 8, s));
    hipLaunchKernelGGL((rows_check_kernel<P, I>), dim3((unsigned)ntiles), dim3(PM_BLOCK), 0, s, (const P *)ip, (const I *)ix, m->outer(),
                       m->inner(), m->nnz, needs, range, res.as<unsigned long long>());
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(copy_to_host(key, res.p, 8, s));
    return SPRS_HIP_OK;
}

inline int32_t report_key(sprs_hip_structure_info *info, unsigned long long key, bool out_of_range) {
    if (out_of_range) return report(info, KIND_OUT_OF_RANGE, key >> 1, "Indice is larger than inner dimension");
    return report(info, KIND_UNSORTED, key >> 1, "Indices are not sorted");
}

template <typename P, typename I>
int32_t check(const sprs_hip_csmat *m, sprs_hip_structure_info *info, hipStream_t s) {
    SPRS_TRY(indptr_pass<P>(m, info, s));
    unsigned long long key;
    SPRS_TRY((rows_pass<P, I>(m, m->indptr, m->indices, nullptr, nullptr, &key, s)));
    if (key == NO_KEY) return report(info, KIND_OK, 0, "");
    return report_key(info, key, (key & 1ull) != 0);
}

// the error path of new_from_unsorted: slice r of m holds an index >= inner and was not sorted; does it hold a duplicate?
template <typename P, typename I>
int32_t slice_has_duplicate(const sprs_hip_csmat *m, uint64_t r, bool *dup, hipStream_t s) {
    P ends[2];
    SPRS_TRY_HIP(copy_to_host(ends, (const P *)m->indptr + r, sizeof ends, s));
    const uint64_t b = (uint64_t)ends[0], e = (uint64_t)ends[1];
    *dup = false;
    if (b >= e || e > m->nnz) return SPRS_HIP_OK;
    std::vector<I> row(e - b);
    SPRS_TRY_HIP(copy_to_host(row.data(), (const I *)m->indices + b, (e - b) * sizeof(I), s));
    std::sort(row.begin(), row.end());
    *dup = std::adjacent_find(row.begin(), row.end()) != row.end();
    return SPRS_HIP_OK;
}

template <typename P, typename I>
int32_t from_unsorted(const sprs_hip_csmat *m, OwnedCsmat &out, sprs_hip_structure_info *info, hipStream_t s) {
    SPRS_TRY(indptr_pass<P>(m, info, s));
    const uint64_t outer = m->outer();
    DevBuf flags;                                   // needs (outer) | range (outer)
    SPRS_TRY_HIP(flags.alloc_for(s, 2 * outer + 16));
    uint8_t *needs = flags.as<uint8_t>(), *range = needs + outer;
    SPRS_TRY_HIP(hipMemsetAsync(needs, 0, 2 * outer + 16, s));
    unsigned long long key;
    SPRS_TRY((rows_pass<P, I>(m, m->indptr, m->indices, needs, range, &key, s)));
    OwnedCsmat res;
    if (key == NO_KEY) {                            // a valid operand: the copy is the result
        SPRS_TRY(copy_csmat(m, true, res, s));
        SPRS_TRY_HIP(hipStreamSynchronize(s));
        out = std::move(res);
        return report(info, KIND_OK, 0, "");
    }
    hipLaunchKernelGGL(pick_kernel, dim3(pm::blocks_for(outer)), dim3(PM_BLOCK), 0, s, needs, (const uint8_t *)range, outer);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, m->nnz, m->iptr_bytes, m->idx_bytes));
    SPRS_TRY((pm::run<P, I>(m, nullptr, nullptr, needs, res.get(), s)));
    SPRS_TRY((rows_pass<P, I>(m, res->indptr, res->indices, nullptr, nullptr, &key, s)));
    if (key == NO_KEY) {
        out = std::move(res);
        return report(info, KIND_OK, 0, "");
    }
    bool out_of_range = (key & 1ull) != 0;
    if (!out_of_range) {
        uint8_t unsortable = 0;
        SPRS_TRY_HIP(copy_to_host(&unsortable, range + (key >> 1), 1, s));
        if (unsortable) {
            bool dup = false;
            SPRS_TRY((slice_has_duplicate<P, I>(m, key >> 1, &dup, s)));
            out_of_range = !dup;
        }
    }
    return report_key(info, key, out_of_range);
}

template <typename I>
int32_t vec_sort(const sprs_hip_csvec *v, sprs_hip_csvec *res, hipStream_t s) {
    const uint64_t n = v->nnz;
    const I *ix = (const I *)v->indices;
    const uint64_t *val = (const uint64_t *)v->data;
    DevBuf small;                                   // the largest index | 0, n: indptr, slice starts and row list of a one-slice matrix
    SPRS_TRY_HIP(small.alloc_for(s, 24));
    uint64_t host[3] = {0, 0, n};
    SPRS_TRY_HIP(copy_to_device(small.p, host, sizeof host, s));
    hipLaunchKernelGGL(vec_max_kernel<I>, dim3(pm::blocks_for(n)), dim3(PM_BLOCK), 0, s, ix, n, small.as<unsigned long long>());
    SPRS_TRY_HIP(hipGetLastError());
    uint64_t top = 0;
    SPRS_TRY_HIP(copy_to_host(&top, small.p, 8, s));
    if (n <= (uint64_t)PM_CAP && top < (1ull << 52)) {
        const uint64_t *one = small.u64() + 1;
        hipLaunchKernelGGL((pm::perm_mid_kernel<PM_BLOCK, PM_CAP, uint64_t, I>), dim3(1), dim3(PM_BLOCK), 0, s, one, (uint64_t)1, one, one,
                           (const I *)nullptr, (const I *)nullptr, ix, val, (uint64_t)1, ~0ull, n, (I *)res->indices, (uint64_t *)res->data);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY_HIP(hipStreamSynchronize(s));
        return SPRS_HIP_OK;
    }
    if (n >= 0xFFFFFFFFull * PM_BLOCK) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "new_from_unsorted: more than 2^40 entries are not supported");
    DevBuf keys, srcs;
    SPRS_TRY_HIP(keys.alloc_for(s, n * 8));
    SPRS_TRY_HIP(srcs.alloc_for(s, n * 8));
    hipLaunchKernelGGL(vec_keys_kernel<I>, dim3(pm::blocks_for(n)), dim3(PM_BLOCK), 0, s, ix, n, keys.u64(), srcs.u64());
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(radix_sort_pairs(keys.u64(), srcs.u64(), n, {{0, (top >> 63) ? 64 : pm::bits_for(top + 1)}}, s));
    hipLaunchKernelGGL(vec_emit_kernel<I>, dim3(pm::blocks_for(n)), dim3(PM_BLOCK), 0, s, (const uint64_t *)keys.u64(),
                       (const uint64_t *)srcs.u64(), val, n, (I *)res->indices, (uint64_t *)res->data);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(hipStreamSynchronize(s));          // (the temporaries go with this scope)
    return SPRS_HIP_OK;
}

}  // namespace st

// check_compressed_structure (sparse.rs:300-358) on a handle; blocks until the answer is known
int32_t csmat_check_structure(const sprs_hip_csmat *m, sprs_hip_structure_info *info, hipStream_t s) {
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        return st::check<typename decltype(p)::type, typename decltype(i)::type>(m, info, s);
    });
}

// new_from_unsorted / new_from_unsorted_csc (csmat.rs:311-401): a new handle with every outer slice sorted, validated; m is only
// read.  `out` stays empty on any finding.
int32_t csmat_from_unsorted(const sprs_hip_csmat *m, OwnedCsmat &out, sprs_hip_structure_info *info, hipStream_t s) {
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        return st::from_unsorted<typename decltype(p)::type, typename decltype(i)::type>(m, out, info, s);
    });
}

// CsVec::new_from_unsorted (vec.rs:536-557): check, sort only on Unsorted, check again
int32_t csvec_from_unsorted(const sprs_hip_csvec *v, OwnedCsvec &out, sprs_hip_structure_info *info, hipStream_t s) {
    sprs_hip_structure_info found{};
    const int32_t first = csvec_check_device(v, s, &found);
    if (info) *info = found;
    if (first != SPRS_HIP_OK && !(first == SPRS_HIP_BAD_STRUCTURE && found.kind == st::KIND_UNSORTED)) return first;
    OwnedCsvec res;
    SPRS_TRY(make_csvec(res, v->dim, v->nnz, v->idx_bytes, v->user_idx_bytes()));
    if (first == SPRS_HIP_OK) {
        if (v->nnz) {
            SPRS_TRY_HIP(hipMemcpyAsync(res->indices, v->indices, v->nnz * (uint64_t)v->idx_bytes, hipMemcpyDeviceToDevice, s));
            SPRS_TRY_HIP(hipMemcpyAsync(res->data, v->data, v->nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
            SPRS_TRY_HIP(hipStreamSynchronize(s));
        }
        out = std::move(res);
        return SPRS_HIP_OK;
    }
    clear_error();
    SPRS_TRY(dispatch_width(v->idx_bytes, [&](auto i) { return st::vec_sort<typename decltype(i)::type>(v, res.get(), s); }));
    SPRS_TRY(csvec_check_device(res.get(), s, info));
    out = std::move(res);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
