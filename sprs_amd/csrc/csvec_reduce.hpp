// Sparse-vector reductions and look-ups for gfx950 — device twins of
//   CsVec::dot / dot_acc            sprs/src/sparse/vec.rs:828-881   (sparse . sparse by merge, sparse . dense)
//   prod::csvec_dot_by_binary_search sprs/src/sparse/prod.rs:14-70   (the same sum, found by binary search)
//   CsVec::dot_dense                vec.rs:894-904
//   squared_l2_norm / l2_norm / l1_norm / norm(p)   vec.rs:907-958
//   unit_normalize                  vec.rs:1051-1061
//   nnz_index / get                 vec.rs:787-805
// Included by spmv.hip after csvec.hpp (one translation unit of the library and of the emulator build, tests/emu).
//
// THE ORDERED SUM.  The reference adds its terms left to right from zero; every sum here is that chain, bit for bit, at every
// size, in two launches:
//  (i)  reduce_terms_kernel, a grid over the stored entries: entry i writes its term into slot i of an nnz-long array.  A slot
//       without a term (dot: the index is not stored in the other vector; dot_dense: the index is outside x) holds -0.0, the
//       one value whose addition changes no double: x + -0.0 == x bit for bit for every x (+0.0 and NaN included), so the chain
//       needs no mask of the present slots.
//  (ii) reduce_chain_kernel, ONE wave: it walks the chunks of 64 slots, RD_UNROLL chunks per step.  Every lane loads one slot of
//       each chunk (coalesced; the next step's loads are in flight while this step is added), the wave passes them through LDS,
//       and the accumulator — the same in every lane — takes them in slot order from uniform (broadcast) LDS reads: one
//       dependent add per slot and nothing else on the chain.  (A first version walked a presence mask and fetched every term
//       with readlane, as the long-slice path of csvec_dot_kernel does: eleven instructions per term, 36 ns per entry on the
//       MI355X against 55 ms for downloading 1e7 values and adding them on the host; DESIGN 4.15 has both measurements.)
// The chain's rate (one dependent add per stored entry) bounds dot and the norms on very long vectors: the price of the
// reference's bits.  No float atomics anywhere: the same bits from run to run.
//
// THE ONE DOCUMENTED DIFFERENCE.  Every chain starts from +0.0.  dot_acc starts from Acc::zero() = +0.0 too; Iterator::sum for
// f64 (dot_dense, the norms) has not had the same neutral element in every Rust toolchain, so the SIGN of a zero result of
// dot_dense and of the norms may differ from a given build of the reference.
//
// norm(+inf), norm(-inf) and norm(0) are order-free (max, min, count): reduce_extrema_kernel leaves one partial per workgroup
// of a fixed grid and the host folds them; exact, hence the same bits whatever the grid.
#pragma once

#include <cmath>

#include "csvec.hpp"
#include "scan.hpp"                            // wave_sync_lds

namespace sprs_hip {
namespace rd {

constexpr int RD_BLOCK = 256;                 // threads of a workgroup of the grid stage (4 chunks of 64 entries)
constexpr int RD_UNROLL = 8;                  // chunks of 64 slots per step of the chain: its loads in flight, its LDS stage
constexpr unsigned RD_EXTREMA_GRID = 256;     // workgroups (at most) of the order-free reductions

enum Term { T_DOT = 0, T_DENSE = 1, T_SQUARE = 2, T_ABS = 3, T_POW = 4 };

inline unsigned blocks_for(uint64_t items) { return (unsigned)((items + RD_BLOCK - 1) / RD_BLOCK); }

// position of `key` in the sorted idx[0, n), or n when it is not stored.  Every read is inside [0, n) whatever the array holds
// (a borrowed, unchecked vector may be unsorted: the answer is then arbitrary, the reads are not)
template <typename I>
__device__ __forceinline__ uint64_t find_index(const I *idx, uint64_t lo, uint64_t hi, uint64_t key, uint64_t none) {
    const uint64_t end = hi;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)idx[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && (uint64_t)idx[lo] == key ? lo : none;
}

// (i) the terms.  `a` is the vector the lanes walk (dot: the one with fewer entries, v on equal counts — prod.rs:25), `b` the
// other operand: the searched vector (T_DOT: bidx / bdata / nb), the dense rhs (T_DENSE: bdata = x, nb = x_len) or nothing.
// swapped: `a` is the caller's rhs (the product is written lhs * rhs either way).  A slot without a term gets -0.0.
template <int KIND, typename AI, typename BI>
__global__ void __launch_bounds__(RD_BLOCK) reduce_terms_kernel(const AI *aidx, const double *adata, uint64_t na, const BI *bidx,
                                                                const double *bdata, uint64_t nb, int swapped, double p, double *terms) {
    const uint64_t i = (uint64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= na) return;
    const double x = adata[i];
    double t = -0.0;
    if (KIND == T_DOT) {
        const uint64_t j = find_index(bidx, 0, nb, (uint64_t)aidx[i], ~0ull);
        if (j != ~0ull) t = swapped ? bdata[j] * x : x * bdata[j];      // unfused: -ffp-contract=off
    } else if (KIND == T_DENSE) {
        const uint64_t k = (uint64_t)aidx[i];
        if (k < nb) t = x * bdata[k];                               // (an index outside x, in a borrowed vector: no term, never read)
    } else {
        t = KIND == T_SQUARE ? x * x : KIND == T_ABS ? fabs(x) : pow(fabs(x), p);
    }
    terms[i] = t;
}

// RD_UNROLL chunks of 64 slots from chunk c on: lane l takes slot l of each (-0.0 past the end)
__device__ __forceinline__ void load_slots(const double *terms, uint64_t n, uint64_t c, int lane, double (&t)[RD_UNROLL]) {
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) {
        const uint64_t e = (c + (uint64_t)u) * 64 + (uint64_t)lane;
        t[u] = e < n ? terms[e] : -0.0;
    }
}

// (ii) the chain: +0.0, then every slot in order
__global__ void __launch_bounds__(64) reduce_chain_kernel(const double *terms, uint64_t n, double *out) {
    __shared__ double stage[RD_UNROLL][64];
    const int lane = threadIdx.x & 63;
    const uint64_t nchunks = (n + 63) / 64;
    double acc = 0.0;
    double t[RD_UNROLL];
    load_slots(terms, n, 0, lane, t);
    for (uint64_t c = 0; c < nchunks; c += RD_UNROLL) {
#pragma unroll
        for (int u = 0; u < RD_UNROLL; ++u) stage[u][lane] = t[u];
        wave_sync_lds();
        load_slots(terms, n, c + RD_UNROLL, lane, t);            // the next step's slots: in flight while this step is added
#pragma unroll
        for (int u = 0; u < RD_UNROLL; ++u) {
            if (c + (uint64_t)u < nchunks) {                      // wave-uniform
#pragma unroll
                for (int j = 0; j < 64; ++j) acc = acc + stage[u][j];
            }
        }
        wave_sync_lds();                                          // every lane has read the stage before it is written again
    }
    if (lane == 0) out[0] = acc;
}

// max |x| (NaN ignored, from -inf: fold(-inf, f64::max)), min |x| (from +inf) and the count of !(|x| == 0) (NaN counted) of a
// workgroup's share: part[3 b .. 3 b + 2].  Exact, so the shape of the tree does not show in the result.
__global__ void __launch_bounds__(RD_BLOCK) reduce_extrema_kernel(const double *data, uint64_t n, double *part) {
    __shared__ double s_mx[RD_BLOCK / 64], s_mn[RD_BLOCK / 64], s_ct[RD_BLOCK / 64];
    double mx = -__builtin_inf(), mn = __builtin_inf(), ct = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * RD_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RD_BLOCK) {
        const double ax = fabs(data[i]);
        if (ax > mx) mx = ax;
        if (ax < mn) mn = ax;
        if (!(ax == 0.0)) ct = ct + 1.0;                        // (a count below 2^53: exact)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double omx = __shfl_xor(mx, off, 64), omn = __shfl_xor(mn, off, 64), oct = __shfl_xor(ct, off, 64);
        if (omx > mx) mx = omx;
        if (omn < mn) mn = omn;
        ct = ct + oct;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_mx[w] = mx, s_mn[w] = mn, s_ct[w] = ct;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < RD_BLOCK / 64; ++k) {
            if (s_mx[k] > mx) mx = s_mx[k];
            if (s_mn[k] < mn) mn = s_mn[k];
            ct = ct + s_ct[k];
        }
        part[3 * (uint64_t)blockIdx.x] = mx;
        part[3 * (uint64_t)blockIdx.x + 1] = mn;
        part[3 * (uint64_t)blockIdx.x + 2] = ct;
    }
}

// unit_normalize's map: a plain IEEE divide by the norm the host took from the chain
__global__ void __launch_bounds__(RD_BLOCK) reduce_divide_kernel(const double *in, uint64_t n, double norm, double *out) {
    const uint64_t i = (uint64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i < n) out[i] = in[i] / norm;
}

// nnz_index / get, one query per lane: pos[q] = the position of index qs[q] in the stored arrays or UINT64_MAX (None);
// val[q] (when asked for) the stored value or 0.0
template <typename I>
__global__ void __launch_bounds__(RD_BLOCK) reduce_lookup_kernel(const I *idx, const double *data, uint64_t nnz, const uint64_t *qs,
                                                                 uint64_t nq, uint64_t *pos, double *val) {
    const uint64_t q = (uint64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const uint64_t j = find_index(idx, 0, nnz, qs[q], ~0ull);
    pos[q] = j;
    if (val) val[q] = j != ~0ull ? data[j] : 0.0;
}

// the two launches of one ordered sum and the read-back of its scalar; launch_terms(terms) enqueues stage (i) on `st`
template <typename F>
static int32_t ordered_sum(uint64_t n, F &&launch_terms, double *out, hipStream_t st) {
    *out = 0.0;
    if (n == 0) return SPRS_HIP_OK;
    DevBuf buf;                                                 // result | terms (n)
    SPRS_TRY_HIP(buf.alloc_for(st, 8 + n * 8));
    double *res = buf.as<double>(), *terms = res + 1;
    launch_terms(terms);
    hipLaunchKernelGGL(reduce_chain_kernel, dim3(1), dim3(64), 0, st, (const double *)terms, n, res);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = copy_to_host(out, res, 8, st);
    return e == hipSuccess ? (int32_t)SPRS_HIP_OK : fail_hip(e, "csvec reduction");
}

template <int KIND, typename AI, typename BI>
static void launch_terms(const sprs_hip_csvec *a, const void *bidx, const double *bdata, uint64_t nb, int swapped, double p, double *terms,
                         hipStream_t st) {
    hipLaunchKernelGGL((reduce_terms_kernel<KIND, AI, BI>), dim3(blocks_for(a->nnz)), dim3(RD_BLOCK), 0, st, (const AI *)a->indices,
                       (const double *)a->data, a->nnz, (const BI *)bidx, bdata, nb, swapped, p, terms);
}

}  // namespace rd

// v . w for two sparse vectors of equal dim (checked by the caller); mixed index widths are fine
int32_t csvec_dot_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, double *out, hipStream_t st) {
    const bool swapped = w->nnz < v->nnz;                       // the lanes walk the shorter vector, v on equal counts (prod.rs:25)
    const sprs_hip_csvec *a = swapped ? w : v, *b = swapped ? v : w;
    if (b->nnz == 0) {                                          // (then a is empty too: no term)
        *out = 0.0;
        return SPRS_HIP_OK;
    }
    return rd::ordered_sum(a->nnz, [&](double *terms) {
        dispatch_widths(a->idx_bytes, b->idx_bytes, [&](auto ai, auto bi) {
            rd::launch_terms<rd::T_DOT, typename decltype(ai)::type, typename decltype(bi)::type>(a, b->indices, b->data, b->nnz, swapped ? 1 : 0,
                                                                                                  0.0, terms, st);
        });
    }, out, st);
}

// v . x for a dense x of x_len = v->dim doubles (checked by the caller)
int32_t csvec_dot_dense_f64(const sprs_hip_csvec *v, const double *x, uint64_t x_len, double *out, hipStream_t st) {
    return rd::ordered_sum(v->nnz, [&](double *terms) {
        dispatch_width(v->idx_bytes, [&](auto i) {
            rd::launch_terms<rd::T_DENSE, typename decltype(i)::type, uint64_t>(v, nullptr, x, x_len, 0, 0.0, terms, st);
        });
    }, out, st);
}

// the chain over x * x (term 0), |x| (1) or pow(|x|, p) (2)
int32_t csvec_sum_f64(const sprs_hip_csvec *v, int32_t term, double p, double *out, hipStream_t st) {
    return rd::ordered_sum(v->nnz, [&](double *terms) {
        if (term == 0) rd::launch_terms<rd::T_SQUARE, uint32_t, uint32_t>(v, nullptr, nullptr, 0, 0, 0.0, terms, st);
        else if (term == 1) rd::launch_terms<rd::T_ABS, uint32_t, uint32_t>(v, nullptr, nullptr, 0, 0, 0.0, terms, st);
        else rd::launch_terms<rd::T_POW, uint32_t, uint32_t>(v, nullptr, nullptr, 0, 0, p, terms, st);   // (the indices are not read)
    }, out, st);
}

// out[0] = max |x| from -inf, out[1] = min |x| from +inf, out[2] = the count of !(|x| == 0)
int32_t csvec_extrema_f64(const sprs_hip_csvec *v, double *out, hipStream_t st) {
    out[0] = -__builtin_inf(), out[1] = __builtin_inf(), out[2] = 0.0;
    if (v->nnz == 0) return SPRS_HIP_OK;
    const unsigned want = rd::blocks_for(v->nnz), grid = want < rd::RD_EXTREMA_GRID ? want : rd::RD_EXTREMA_GRID;
    DevBuf buf;
    SPRS_TRY_HIP(buf.alloc_for(st, (uint64_t)grid * 24));
    hipLaunchKernelGGL(rd::reduce_extrema_kernel, dim3(grid), dim3(rd::RD_BLOCK), 0, st, (const double *)v->data, v->nnz, buf.as<double>());
    hipError_t e = hipGetLastError();
    std::vector<double> part((size_t)grid * 3);
    if (e == hipSuccess) e = copy_to_host(part.data(), buf.p, (uint64_t)grid * 24, st);
    if (e != hipSuccess) return fail_hip(e, "csvec norm");
    for (unsigned b = 0; b < grid; ++b) {
        if (part[3 * b] > out[0]) out[0] = part[3 * b];
        if (part[3 * b + 1] < out[1]) out[1] = part[3 * b + 1];
        out[2] = out[2] + part[3 * b + 2];
    }
    return SPRS_HIP_OK;
}

// a NEW owning vector with v's indices, width and dim whose values are v's divided by `norm` (norm > 0) or copied (norm == 0:
// the zero vector is left unchanged, vec.rs:1057).  Complete on `st` at return.
int32_t csvec_divided_f64(const sprs_hip_csvec *v, double norm, OwnedCsvec &out, hipStream_t st) {
    OwnedCsvec res;
    SPRS_TRY(make_csvec(res, v->dim, v->nnz, v->idx_bytes, v->user_idx_bytes()));
    if (v->nnz) {
        hipError_t e = hipMemcpyAsync(res->indices, v->indices, v->nnz * (uint64_t)v->idx_bytes, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && norm > 0.0) {
            hipLaunchKernelGGL(rd::reduce_divide_kernel, dim3(rd::blocks_for(v->nnz)), dim3(rd::RD_BLOCK), 0, st, (const double *)v->data, v->nnz,
                               norm, res->data);
            e = hipGetLastError();
        } else if (e == hipSuccess) {
            e = hipMemcpyAsync(res->data, v->data, v->nnz * sizeof(double), hipMemcpyDeviceToDevice, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail_hip(e, "csvec unit_normalize");
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

// batched nnz_index / get: ordered on `st`
int32_t csvec_lookup(const sprs_hip_csvec *v, uint64_t nq, const uint64_t *qs, uint64_t *pos, double *val, hipStream_t st) {
    if (nq == 0) return SPRS_HIP_OK;
    if (v->nnz == 0) {                                          // nothing is stored: every answer is None, no kernel
        SPRS_TRY_HIP(hipMemsetAsync(pos, 0xFF, nq * 8, st));
        if (val) SPRS_TRY_HIP(hipMemsetAsync(val, 0, nq * 8, st));
        return SPRS_HIP_OK;
    }
    dispatch_width(v->idx_bytes, [&](auto i) {
        using I = typename decltype(i)::type;
        hipLaunchKernelGGL(rd::reduce_lookup_kernel<I>, dim3(rd::blocks_for(nq)), dim3(rd::RD_BLOCK), 0, st, (const I *)v->indices,
                           (const double *)v->data, v->nnz, qs, nq, pos, val);
    });
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
