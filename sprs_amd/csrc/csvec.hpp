// Sparse-vector products for gfx950 — device twins of
//   prod::csr_mul_csvec             sprs/src/sparse/prod.rs:161-184   (CSR x CsVec: entries with val != 0 only)
//   `&CsMat(CSC) * &CsVec`          sprs/src/sparse/vec.rs:1104-1131  (A * v.col_view(): structural)
//   `&CsVec * &CsMat`               sprs/src/sparse/vec.rs:1084-1102  (v.row_view() * B: structural)
// Included by spmv.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// THE MASKED ORDERED DOT.  All four operators are one operation: for every outer slice o of a compressed matrix M, the
// ordered sparse dot  M_o . v  (sum from +0.0, unfused products added by ascending inner index — the merge of dot_acc,
// vec.rs:846-880, and the accumulator of smmp's numeric pass, both MulAcc, mul_acc.rs:28-30) and a filter: drop-zero
// (csr_mul_csvec keeps `val != 0`) or structural (every o with at least one matched index, explicit zeros kept).
//   CSR A x v: A itself, drop-zero;  CSC A x v: the CSR form of A, structural;
//   v x CSC B: B itself (its columns), structural;  v x CSR B: the CSC form of B, structural.
//
//  1. LOOK-UP TABLE OF v (per call): a presence bitmap of ceil(n / 32) words, cleared and set from v's indices, and v's
//     values scattered into an n-long array that is never cleared — it is read only where the bit is set.
//  2. csvec_dot_kernel: a wave owns 64 consecutive outer slices and streams their entries (contiguous in M) in chunks of
//     64, CV_UNROLL chunks in flight (CV_UNROLL_LONG on a long slice).  Every lane tests one entry's bit; M's value and
//     v's value are loaded ONLY for matched entries, so a sparse v costs one pass over the indices.  Short slices (<= CV_LONG entries) are summed by
//     their own lane: the matched products of a chunk go through LDS and each lane adds those of its slice in entry order.
//     Longer slices are walked by the whole wave: the matched products of a chunk are added in lane order by one uniform
//     loop over the ballot mask (readlane: no memory round trip on the add chain).  Either way every sum is the
//     reference's left-to-right chain, bit for bit.  Out: the sum of every kept slice, a 64-bit keep mask and a count per
//     wave group.
//  3. exclusive_scan_u64 over the group counts; the result's nnz is read back ON THE CALLER'S STREAM.
//  4. csvec_emit_kernel: kept slices -> sorted (indices, data) of the result.
#pragma once

#include "common.hpp"
#include "csvec_shared.hpp"   // CV_BLOCK, rl_u64 / rl_f64 / span_mask, csvec_emit_kernel (step 4), blocks_for

namespace sprs_hip {
namespace cv {

constexpr int CV_WAVES = CV_BLOCK / 64;
constexpr int CV_UNROLL = 4;                  // chunks of 64 entries whose loads are in flight together (short slices)
constexpr int CV_UNROLL_LONG = 16;            // the same for a slice walked by the whole wave: its walk is a chain of round trips
constexpr uint64_t CV_LONG = 128;             // slices with more entries are walked by the whole wave

// 1. the look-up table: bit k of `bits` and vals[k] = v[k] for every stored k (indices below n: checked at upload; the
// test here keeps a borrowed, unchecked vector from writing outside the table)
template <typename VI>
__global__ void __launch_bounds__(CV_BLOCK) csvec_mark_kernel(const VI *vidx, const double *vdata, uint64_t nnz, uint64_t n,
                                                              uint32_t *bits, double *vals) {
    const uint64_t i = (uint64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t k = (uint64_t)vidx[i];
    if (k >= n) return;
    atomicOr(&bits[k >> 5], 1u << (k & 31));
    vals[k] = vdata[i];
}

// U chunks of 64 entries from `c` on, cut at `end`: matched products and their ballot masks
template <int U, typename I>
__device__ __forceinline__ void load_chunks(const I *ix, const double *mv, uint64_t c, uint64_t end, uint64_t n, const uint32_t *bits,
                                            const double *vals, int lane, double (&p)[U], uint64_t (&hits)[U]) {
    uint64_t k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t e = c + (uint64_t)u * 64 + lane;
        k[u] = e < end ? (uint64_t)ix[e] : ~0ull;
    }
    uint32_t w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = k[u] < n ? bits[k[u] >> 5] : 0u;
    bool hit[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        hit[u] = k[u] < n && ((w[u] >> (k[u] & 31)) & 1u);
        p[u] = 0.0;
        if (hit[u]) p[u] = mv[c + (uint64_t)u * 64 + lane] * vals[k[u]];   // unfused: -ffp-contract=off
    }
#pragma unroll
    for (int u = 0; u < U; ++u) hits[u] = __ballot(hit[u]);
}

// 2. the masked ordered dot of every outer slice of (ip, ix, mv) with v's table.  drop_zero: keep `sum != 0` (NaN is kept),
// else every slice with a matched index.
template <typename P, typename I>
__global__ void __launch_bounds__(CV_BLOCK) csvec_dot_kernel(const P *ip, const I *ix, const double *mv, uint64_t nouter, uint64_t n,
                                                             const uint32_t *bits, const double *vals, int drop_zero, double *sums,
                                                             uint64_t *masks, uint64_t *counts) {
    __shared__ double prod_s[CV_WAVES][CV_UNROLL][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t g = (uint64_t)blockIdx.x * CV_WAVES + w;
    const uint64_t r0 = g * 64;
    if (r0 >= nouter) return;                                   // whole wave
    const uint64_t r1 = r0 + 64 < nouter ? r0 + 64 : nouter;
    const uint64_t hi = (uint64_t)ip[r1];
    const uint64_t r = r0 + lane;
    const uint64_t rs = r < r1 ? (uint64_t)ip[r] : hi, re = r < r1 ? (uint64_t)ip[r + 1] : hi;
    double sum = 0.0;
    bool any = false;
    uint64_t longs = __ballot(re - rs > CV_LONG);               // slices walked by the whole wave, in slice order
    uint64_t seg = (uint64_t)ip[r0];
    for (;;) {
        const int L = longs ? __builtin_ctzll(longs) : 64;
        const uint64_t seg_end = L < 64 ? rl_u64(rs, L) : hi;
        // the short slices between seg and seg_end: one lane per slice
        for (uint64_t c = seg; c < seg_end; c += 64 * CV_UNROLL) {
            double p[CV_UNROLL];
            uint64_t hits[CV_UNROLL];
            load_chunks<CV_UNROLL>(ix, mv, c, seg_end, n, bits, vals, lane, p, hits);
            uint64_t any_hit = 0;
#pragma unroll
            for (int u = 0; u < CV_UNROLL; ++u) any_hit |= hits[u];
            if (!any_hit) continue;                             // wave-uniform
#pragma unroll
            for (int u = 0; u < CV_UNROLL; ++u) prod_s[w][u][lane] = p[u];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < CV_UNROLL; ++u) {
                const uint64_t cu = c + (uint64_t)u * 64;
                const uint64_t a = rs > cu ? rs - cu : 0, b = re > cu ? (re - cu < 64 ? re - cu : 64) : 0;
                uint64_t mine = hits[u] & span_mask(a < 64 ? a : 64, b);
                while (mine) {
                    const int j = __builtin_ctzll(mine);
                    sum = sum + prod_s[w][u][j];
                    any = true;
                    mine &= mine - 1;
                }
            }
        }
        if (L == 64) break;
        // slice r0 + L: the whole wave, products added in lane order
        const uint64_t ls = seg_end, le = rl_u64(re, L);
        double acc = 0.0;
        bool acc_any = false;
        for (uint64_t c = ls; c < le; c += 64 * CV_UNROLL_LONG) {
            double p[CV_UNROLL_LONG];
            uint64_t hits[CV_UNROLL_LONG];
            load_chunks<CV_UNROLL_LONG>(ix, mv, c, le, n, bits, vals, lane, p, hits);
#pragma unroll
            for (int u = 0; u < CV_UNROLL_LONG; ++u) {
                uint64_t mm = hits[u];
                acc_any |= mm != 0;
                while (mm) {
                    const int j = __builtin_ctzll(mm);
                    acc = acc + rl_f64(p[u], j);
                    mm &= mm - 1;
                }
            }
        }
        if (lane == L) {
            sum = acc;
            any = acc_any;
        }
        longs &= longs - 1;
        seg = le;
    }
    const bool keep = r < r1 && (drop_zero ? sum != 0.0 : any);
    const uint64_t kept = __ballot(keep);
    if (keep) sums[r] = sum;
    if (lane == 0) {
        masks[g] = kept;
        counts[g] = (uint64_t)__popcll(kept);
    }
}

// CsVec::scatter / to_dense (vec.rs:621, 965): out[idx[i]] = data[i] on a zeroed out
template <typename VI>
__global__ void __launch_bounds__(CV_BLOCK) csvec_scatter_kernel(const VI *vidx, const double *vdata, uint64_t nnz, uint64_t n,
                                                                 double *out) {
    const uint64_t i = (uint64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t k = (uint64_t)vidx[i];
    if (k < n) out[k] = vdata[i];
}

// the invariants of CsVec::try_new (vec.rs:440-491) on device indices: bad[0] = first position p with idx[p+1] <= idx[p]
// ("Unsorted indices"), bad[1] = 1 when the last index is >= dim ("indices larger than vector size")
template <typename VI>
__global__ void __launch_bounds__(CV_BLOCK) csvec_check_kernel(const VI *vidx, uint64_t nnz, uint64_t dim, uint64_t *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t k = (uint64_t)vidx[i];
    if (i + 1 < nnz && (uint64_t)vidx[i + 1] <= k) atomicMin((unsigned long long *)&bad[0], (unsigned long long)i);
    if (i + 1 == nnz && k >= dim) bad[1] = 1;
}

}  // namespace cv

// the per-handle temporaries of the products (the table of v, the slice sums, the group masks / counts / offsets), made at
// the first product of the handle and kept until refresh / free
static int32_t csvec_scratch(sprs_hip_csmat *m, uint64_t n) {
    CsvecScratch &s = m->cv;
    const uint64_t nouter = m->outer(), ngroups = (nouter + 63) / 64;
    if (s.bits && s.n == n && s.nouter == nouter) return SPRS_HIP_OK;
    s = CsvecScratch();
    CsvecScratch t;                // complete before the handle takes it
    t.n = n;
    t.nouter = nouter;
    const uint64_t words = (n + 31) / 32;
    hipError_t e = alloc_block(t.blocks, t.bits, (words ? words : 1) * 4);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.vals, (n ? n : 1) * 8);
    if (e == hipSuccess) e = alloc_block(t.blocks, t.sums, (nouter ? nouter : 1) * 8);
    // masks | counts | offsets (ngroups + 1) | overflow flag
    if (e == hipSuccess) e = alloc_block(t.blocks, t.groups, (3 * ngroups + 2) * 8);
    if (e != hipSuccess) return fail_hip(e, "csvec scratch");
    s = std::move(t);
    return SPRS_HIP_OK;
}

int32_t csvec_check_device(const sprs_hip_csvec *v, hipStream_t s, sprs_hip_structure_info *info) {
    if (info) *info = sprs_hip_structure_info{0, 0, 0};
    if (v->nnz == 0) return SPRS_HIP_OK;
    DevBuf bad;
    SPRS_TRY_HIP(bad.alloc(16));
    uint64_t host[2] = {~0ull, 0};
    hipError_t e = hipMemcpyAsync(bad.p, host, 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        dispatch_width(v->idx_bytes, [&](auto i) {
            using I = typename decltype(i)::type;
            hipLaunchKernelGGL(cv::csvec_check_kernel<I>, dim3(cv::blocks_for(v->nnz)), dim3(cv::CV_BLOCK), 0, s, (const I *)v->indices,
                               v->nnz, v->dim, bad.u64());
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = copy_to_host(host, bad.p, 16, s);
    if (e != hipSuccess) return fail_hip(e, "csvec_check");
    if (host[0] != ~0ull) {                         // StructureError::Unsorted (vec.rs:472-478)
        if (info) info->kind = 1;
        SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Unsorted indices");
    }
    if (host[1]) {                                  // StructureError::SizeMismatch (vec.rs:479-489)
        if (info) info->kind = 2;
        SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "indices larger than vector size");
    }
    return SPRS_HIP_OK;
}

int32_t csvec_scatter(const sprs_hip_csvec *v, double *out, hipStream_t s) {
    if (v->dim) SPRS_TRY_HIP(hipMemsetAsync(out, 0, v->dim * 8, s));
    if (v->nnz) {
        dispatch_width(v->idx_bytes, [&](auto i) {
            using I = typename decltype(i)::type;
            hipLaunchKernelGGL(cv::csvec_scatter_kernel<I>, dim3(cv::blocks_for(v->nnz)), dim3(cv::CV_BLOCK), 0, s, (const I *)v->indices,
                               v->data, v->nnz, v->dim, out);
        });
        SPRS_TRY_HIP(hipGetLastError());
    }
    return SPRS_HIP_OK;
}

template <typename P, typename I>
static void launch_dot(const sprs_hip_csmat *m, uint64_t n, const CsvecScratch &s, int drop_zero, hipStream_t st) {
    const uint64_t ngroups = (m->outer() + 63) / 64;
    hipLaunchKernelGGL((cv::csvec_dot_kernel<P, I>), dim3((unsigned)((ngroups + cv::CV_WAVES - 1) / cv::CV_WAVES)), dim3(cv::CV_BLOCK), 0,
                       st, (const P *)m->indptr, (const I *)m->indices, (const double *)m->data, m->outer(), n, s.bits,
                       s.vals, drop_zero, s.sums, s.groups, s.groups + ngroups);
}

// The masked ordered dot of every outer slice of m with v (m->inner() == v->dim, checked by the caller).  The result has
// dimension m->outer(), index width idx_bytes on the device (declared decl_bytes).  Blocks until it is complete on `st`.
int32_t csvec_masked_dot(const sprs_hip_csmat *mc, const sprs_hip_csvec *v, bool drop_zero, int32_t idx_bytes, int32_t decl_bytes,
                         OwnedCsvec &out, hipStream_t st) {
    auto *m = const_cast<sprs_hip_csmat *>(mc);
    std::lock_guard<std::recursive_mutex> lock(m->mu);         // the handle's scratch serves one product at a time
    const uint64_t n = v->dim, nouter = m->outer(), ngroups = (nouter + 63) / 64;
    SPRS_TRY(csvec_scratch(m, n));
    const CsvecScratch &s = m->cv;
    if (n) SPRS_TRY_HIP(hipMemsetAsync(s.bits, 0, (n + 31) / 32 * 4, st));
    if (v->nnz) {
        dispatch_width(v->idx_bytes, [&](auto i) {
            using I = typename decltype(i)::type;
            hipLaunchKernelGGL(cv::csvec_mark_kernel<I>, dim3(cv::blocks_for(v->nnz)), dim3(cv::CV_BLOCK), 0, st, (const I *)v->indices,
                               v->data, v->nnz, n, s.bits, s.vals);
        });
    }
    if (ngroups) {
        const int dz = drop_zero ? 1 : 0;
        dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
            launch_dot<typename decltype(p)::type, typename decltype(i)::type>(m, n, s, dz, st);     // (indptr type first)
        });
    }
    SPRS_TRY_HIP(hipGetLastError());
    uint64_t *offs = s.groups + 2 * ngroups;
    uint32_t *overflow = (uint32_t *)(s.groups + 3 * ngroups + 1);
    SPRS_TRY(exclusive_scan_u64(s.groups + ngroups, offs, ngroups, st));
    // the result's nnz, read back in the caller's stream order (a non-blocking stream does not wait for the null stream)
    uint64_t nnz = 0;
    SPRS_TRY_HIP(copy_to_host(&nnz, offs + ngroups, 8, st));
    OwnedCsvec res;
    SPRS_TRY(make_csvec(res, nouter, nnz, idx_bytes, decl_bytes));
    if (nnz) {
        const uint64_t decl = decl_bytes ? decl_bytes : idx_bytes;
        const uint64_t limit = decl >= 8 ? ~0ull : (1ull << (8 * decl)) - 1ull;
        uint32_t flag = 0;
        hipError_t e = hipMemsetAsync(overflow, 0, 4, st);
        if (e == hipSuccess) {
            dispatch_width(idx_bytes, [&](auto i) {
                using I = typename decltype(i)::type;
                hipLaunchKernelGGL(cv::csvec_emit_kernel<I>, dim3(cv::blocks_for(nouter)), dim3(cv::CV_BLOCK), 0, st, s.groups, offs, s.sums,
                                   nouter, limit, (I *)res->indices, res->data, overflow);
            });
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = copy_to_host(&flag, overflow, 4, st);
        if (e != hipSuccess) return fail_hip(e, "csvec product");
        if (flag)
            SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the index of a result entry (dimension %llu)",
                      (unsigned long long)nouter);
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
