// Matrix extraction for gfx950 — device twins of
//   CsMat::outer_view        sprs/src/sparse/csmat.rs:1219-1231   (a borrowing CsVec over one outer slice: zero-copy)
//   CsMat::diag              csmat.rs:1234-1256                   (structural: an explicit 0.0 on the diagonal is kept)
//   nnz_index / get          csmat.rs:1312-1351                   (batched: one query per lane)
//   to_inner_onehot          csmat.rs:1017-1056                   (per outer slice the LAST maximal non-NaN entry, value 1.0)
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// diag and to_inner_onehot share one shape: a kernel decides per outer slice whether it keeps an entry and leaves what it
// keeps, a 64-bit keep mask and a count per group of 64 slices; exclusive_scan_u64 over the counts; an emit kernel
// (csvec_emit_kernel for the diagonal, onehot_emit_kernel for the matrix, which also writes the new indptr).
//
// to_inner_onehot: a wave owns 64 consecutive slices.  Slices of at most EX_LONG entries are scanned by their own lane;
// longer ones (hub slices) by the whole wave, 64 entries per load and EX_UNROLL loads in flight, and the lanes' candidates
// are folded by the key (value, position).  The key is a total order on the non-NaN entries (-0.0 == +0.0, so equal values fall to the later position:
// Iterator::max_by returns the last of equal maxima), hence the result does not depend on the shape of the reduction.
#pragma once

#include "common.hpp"
#include "csvec_shared.hpp"

namespace sprs_hip {
namespace ex {

constexpr int EX_BLOCK = 256;                 // 4 waves
constexpr int EX_WAVES = EX_BLOCK / 64;
constexpr uint64_t EX_LONG = 128;             // slices with more entries are scanned by the whole wave
constexpr int EX_UNROLL = 8;                  // steps of 64 entries of such a slice whose loads are in flight together

inline unsigned blocks_for(uint64_t items) { return (unsigned)((items + EX_BLOCK - 1) / EX_BLOCK); }

// position of `key` among the sorted idx[lo, hi), or `none`; every read is inside [lo, hi)
template <typename I>
__device__ __forceinline__ uint64_t find_inner(const I *idx, uint64_t lo, uint64_t hi, uint64_t key, uint64_t none) {
    const uint64_t end = hi;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)idx[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && (uint64_t)idx[lo] == key ? lo : none;
}

// the slice bounds of outer index o, kept inside [0, nnz) whatever a borrowed, unchecked indptr holds
template <typename P>
__device__ __forceinline__ void slice_bounds(const P *ip, uint64_t o, uint64_t nnz, uint64_t &lo, uint64_t &hi) {
    hi = (uint64_t)ip[o + 1];
    if (hi > nnz) hi = nnz;
    lo = (uint64_t)ip[o];
    if (lo > hi) lo = hi;
}

// diag: lane i < n = min(rows, cols) looks for inner index i in outer slice i
template <typename P, typename I>
__global__ void __launch_bounds__(EX_BLOCK) diag_find_kernel(const P *ip, const I *ix, const double *data, uint64_t n, uint64_t nnz,
                                                             double *vals, uint64_t *masks, uint64_t *counts) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (i - (uint64_t)lane >= n) return;                        // whole wave
    bool keep = false;
    if (i < n) {
        uint64_t lo, hi;
        slice_bounds(ip, i, nnz, lo, hi);
        const uint64_t j = find_inner(ix, lo, hi, i, ~0ull);
        if (j != ~0ull) {
            keep = true;
            vals[i] = data[j];
        }
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        masks[i >> 6] = m;
        counts[i >> 6] = (uint64_t)__popcll(m);
    }
}

// batched nnz_index / get: query q = (rows[q], cols[q]); (outer, inner) = (row, col) for CSR (csc = 0), (col, row) for CSC
template <typename P, typename I>
__global__ void __launch_bounds__(EX_BLOCK) mat_lookup_kernel(const P *ip, const I *ix, const double *data, uint64_t nouter, uint64_t nnz,
                                                              int csc, const uint64_t *rows, const uint64_t *cols, uint64_t nq,
                                                              uint64_t *pos, double *val) {
    const uint64_t q = (uint64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const uint64_t o = csc ? cols[q] : rows[q], k = csc ? rows[q] : cols[q];
    uint64_t j = ~0ull;
    if (o < nouter) {
        uint64_t lo, hi;
        slice_bounds(ip, o, nnz, lo, hi);
        j = find_inner(ix, lo, hi, k, ~0ull);
    }
    pos[q] = j;
    if (val) val[q] = j != ~0ull ? data[j] : 0.0;
}

// candidate (x at position e) against the best so far: later positions win ties
__device__ __forceinline__ void onehot_take(double x, uint64_t e, bool &have, double &best, uint64_t &at) {
    if (x != x) return;                                         // NaNs are skipped
    if (!have || x > best || (x == best && e > at)) {
        have = true;
        best = x;
        at = e;
    }
}

// to_inner_onehot, the choice: hot[o] = the inner index of the last maximal non-NaN entry of every populated slice o
template <typename P, typename I>
__global__ void __launch_bounds__(EX_BLOCK) onehot_pick_kernel(const P *ip, const I *ix, const double *data, uint64_t nouter, uint64_t nnz,
                                                               uint64_t *hot, uint64_t *masks, uint64_t *counts) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t g = (uint64_t)blockIdx.x * EX_WAVES + w;
    const uint64_t o0 = g * 64;
    if (o0 >= nouter) return;                                   // whole wave
    const uint64_t o = o0 + lane;
    uint64_t lo = 0, hi = 0;
    if (o < nouter) slice_bounds(ip, o, nnz, lo, hi);
    bool have = false;
    double best = 0.0;
    uint64_t at = 0;
    uint64_t longs = __ballot(hi - lo > EX_LONG);
    if (hi - lo <= EX_LONG)
        for (uint64_t e = lo; e < hi; ++e) onehot_take(data[e], e, have, best, at);
    while (longs) {                                             // wave-uniform: one hub slice after the other
        const int L = __builtin_ctzll(longs);
        const uint64_t ls = cv::rl_u64(lo, L), le = cv::rl_u64(hi, L);
        bool h = false;
        double b = 0.0;
        uint64_t a = 0;
        for (uint64_t e0 = ls; e0 < le; e0 += 64 * EX_UNROLL) {
            double x[EX_UNROLL];
#pragma unroll
            for (int u = 0; u < EX_UNROLL; ++u) {                  // EX_UNROLL loads in flight; past the end a NaN, which is skipped
                const uint64_t e = e0 + (uint64_t)u * 64 + (uint64_t)lane;
                x[u] = e < le ? data[e] : __builtin_nan("");
            }
#pragma unroll
            for (int u = 0; u < EX_UNROLL; ++u) onehot_take(x[u], e0 + (uint64_t)u * 64 + (uint64_t)lane, h, b, a);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int oh = __shfl_xor((int)h, off, 64);
            const double ob = __shfl_xor(b, off, 64);
            const uint64_t oa = __shfl_xor(a, off, 64);
            if (oh) onehot_take(ob, oa, h, b, a);
        }
        if (lane == L) have = h, best = b, at = a;
        longs &= longs - 1;
    }
    const uint64_t m = __ballot(have);
    if (have) hot[o] = (uint64_t)ix[at];
    if (lane == 0) {
        masks[g] = m;
        counts[g] = (uint64_t)__popcll(m);
    }
}

// to_inner_onehot, the result: indptr = the running count of populated slices, one index and 1.0 per populated slice
template <typename P, typename I>
__global__ void __launch_bounds__(EX_BLOCK) onehot_emit_kernel(const uint64_t *masks, const uint64_t *offs, const uint64_t *hot,
                                                               uint64_t nouter, P *oip, I *oix, double *oval) {
    const uint64_t o = (uint64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (o > nouter) return;
    if (o == nouter) {
        oip[o] = (P)offs[(nouter + 63) / 64];
        return;
    }
    const uint64_t m = masks[o >> 6];
    const int b = (int)(o & 63);
    const uint64_t pos = offs[o >> 6] + (uint64_t)__popcll(m & ((1ull << b) - 1ull));
    oip[o] = (P)pos;
    if ((m >> b) & 1ull) {
        oix[pos] = (I)hot[o];
        oval[pos] = 1.0;
    }
}

}  // namespace ex

// outer_view(i), i < outer (checked by the caller): a borrowing vector over m's arrays; the two indptr values are read back on `st`
int32_t csmat_outer_view(const sprs_hip_csmat *m, uint64_t i, sprs_hip_csvec **out, hipStream_t st) {
    uint64_t bounds[2] = {0, 0};
    const uint64_t pb = (uint64_t)m->iptr_bytes;
    SPRS_TRY_HIP(copy_to_host(bounds, (const char *)m->indptr + i * pb, 2 * pb, st));
    uint64_t lo, hi;
    if (pb == 4) {
        const uint32_t *b32 = (const uint32_t *)bounds;
        lo = b32[0], hi = b32[1];
    } else {
        lo = bounds[0], hi = bounds[1];
    }
    if (hi > m->nnz) hi = m->nnz;                               // (a borrowed, unchecked indptr)
    if (lo > hi) lo = hi;
    sprs_hip_csvec *v = view_csvec(m->inner(), hi - lo, (const char *)m->indices + lo * (uint64_t)m->idx_bytes, m->idx_bytes, m->data + lo, m->device);
    v->decl_idx_bytes = m->decl_idx_bytes;
    *out = v;
    return SPRS_HIP_OK;
}

// diag(): a new owning vector of dim min(rows, cols) in m's index width; complete on `st` at return
int32_t csmat_diag_f64(const sprs_hip_csmat *m, OwnedCsvec &out, hipStream_t st) {
    const uint64_t n = m->rows < m->cols ? m->rows : m->cols, ngroups = (n + 63) / 64;
    OwnedCsvec res;
    if (n == 0 || m->nnz == 0) {
        SPRS_TRY(make_csvec(res, n, 0, m->idx_bytes, m->user_idx_bytes()));
        out = std::move(res);
        return SPRS_HIP_OK;
    }
    DevBuf buf;                                                 // values (n) | masks (ngroups) | counts (ngroups) | offsets (ngroups + 1) | overflow flag
    SPRS_TRY_HIP(buf.alloc_for(st, (n + 3 * ngroups + 2) * 8));
    double *vals = buf.as<double>();
    uint64_t *masks = buf.u64() + n, *counts = masks + ngroups, *offs = counts + ngroups;
    uint32_t *overflow = (uint32_t *)(offs + ngroups + 1);
    dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((ex::diag_find_kernel<P, I>), dim3(ex::blocks_for(n)), dim3(ex::EX_BLOCK), 0, st, (const P *)m->indptr,
                           (const I *)m->indices, (const double *)m->data, n, m->nnz, vals, masks, counts);
    });
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(counts, offs, ngroups, st));
    uint64_t nnz = 0;
    SPRS_TRY_HIP(copy_to_host(&nnz, offs + ngroups, 8, st));
    SPRS_TRY(make_csvec(res, n, nnz, m->idx_bytes, m->user_idx_bytes()));
    if (nnz) {
        // (an index below min(rows, cols) fits the matrix's index type: the limit never bites)
        dispatch_width(m->idx_bytes, [&](auto i) {
            using I = typename decltype(i)::type;
            hipLaunchKernelGGL(cv::csvec_emit_kernel<I>, dim3(cv::blocks_for(n)), dim3(cv::CV_BLOCK), 0, st, (const uint64_t *)masks,
                               (const uint64_t *)offs, (const double *)vals, n, ~0ull, (I *)res->indices, res->data, overflow);
        });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail_hip(e, "csmat diag");
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

// batched nnz_index / get: ordered on `st`
int32_t csmat_lookup(const sprs_hip_csmat *m, uint64_t nq, const uint64_t *rows, const uint64_t *cols, uint64_t *pos, double *val,
                     hipStream_t st) {
    if (nq == 0) return SPRS_HIP_OK;
    if (m->nnz == 0) {                                          // nothing is stored: every answer is None, no kernel
        SPRS_TRY_HIP(hipMemsetAsync(pos, 0xFF, nq * 8, st));
        if (val) SPRS_TRY_HIP(hipMemsetAsync(val, 0, nq * 8, st));
        return SPRS_HIP_OK;
    }
    dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((ex::mat_lookup_kernel<P, I>), dim3(ex::blocks_for(nq)), dim3(ex::EX_BLOCK), 0, st, (const P *)m->indptr,
                           (const I *)m->indices, (const double *)m->data, m->outer(), m->nnz, m->storage == SPRS_HIP_CSC ? 1 : 0, rows, cols,
                           nq, pos, val);
    });
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

// to_inner_onehot(): a new owning matrix of m's shape, storage and index widths; complete on `st` at return
int32_t csmat_onehot_f64(const sprs_hip_csmat *m, OwnedCsmat &out, hipStream_t st) {
    const uint64_t nouter = m->outer(), ngroups = (nouter + 63) / 64;
    OwnedCsmat res;
    if (nouter == 0 || m->nnz == 0) {                           // no slice is populated: an all-zero indptr
        SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, 0, m->iptr_bytes, m->idx_bytes));
        hipError_t e = hipMemsetAsync(res->indptr, 0, (nouter + 1) * (uint64_t)m->iptr_bytes, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail_hip(e, "csmat to_inner_onehot");
        out = std::move(res);
        return SPRS_HIP_OK;
    }
    DevBuf buf;                                                 // hot (nouter) | masks (ngroups) | counts (ngroups) | offsets (ngroups + 1)
    SPRS_TRY_HIP(buf.alloc_for(st, (nouter + 3 * ngroups + 1) * 8));
    uint64_t *hot = buf.u64(), *masks = hot + nouter, *counts = masks + ngroups, *offs = counts + ngroups;
    dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((ex::onehot_pick_kernel<P, I>), dim3((unsigned)((ngroups + ex::EX_WAVES - 1) / ex::EX_WAVES)), dim3(ex::EX_BLOCK), 0, st,
                           (const P *)m->indptr, (const I *)m->indices, (const double *)m->data, nouter, m->nnz, hot, masks, counts);
    });
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(counts, offs, ngroups, st));
    uint64_t nnz = 0;
    SPRS_TRY_HIP(copy_to_host(&nnz, offs + ngroups, 8, st));
    SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, nnz, m->iptr_bytes, m->idx_bytes));
    dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((ex::onehot_emit_kernel<P, I>), dim3(ex::blocks_for(nouter + 1)), dim3(ex::EX_BLOCK), 0, st, (const uint64_t *)masks,
                           (const uint64_t *)offs, (const uint64_t *)hot, nouter, (P *)res->indptr, (I *)res->indices, res->data);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip(e, "csmat to_inner_onehot");
    out = std::move(res);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
