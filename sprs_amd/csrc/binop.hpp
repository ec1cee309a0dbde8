// Sparse (+, -, elementwise *) sparse and sparse * scalar for gfx950 — device twins of
//   csmat_binop / csmat_binop_same_storage_raw   sprs/src/sparse/binop.rs:178-271   (`&A + &B`, `&A - &B`, mul_mat_same_storage)
//   csvec_binop                                   sprs/src/sparse/binop.rs:442-479   (`&v + &w`, `&v - &w`)
//   `&A * s` = A.map(|x| x * s)                    sprs/src/sparse/binop.rs:132-163
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// ONE MERGE OVER THE NNZ AXIS.  The reference merges the two sorted index lists of every outer slice (nnz_or_zip): an index
// on one side only gives op(l, +0.0) / op(+0.0, r) — the operation IS performed —, an index on both sides op(l, r); a matrix
// keeps the entry iff !(val == 0.0) (both zeros dropped, NaN kept), a vector keeps every merged index.  Every result entry is
// one IEEE operation, so the result is the reference's bit for bit.
//
//  SLOTS.  The un-combined merge of the two operands has N = nnz(A) + nnz(B) slots; outer slice r starts at slot
//     s_r = indptrA[r] + indptrB[r] (monotone, no array of its own).  Row lengths never enter the partition: a workgroup
//     takes BO_TILE consecutive slots.
//  1. binop_partition_kernel: for every tile edge k = t * BO_TILE the slice that holds slot k (binary search on s_r) and the
//     merge-path split (a, b), a + b = k, of that slice pair (binary search on the inner indices, ties lhs first).
//  2. binop_tile_kernel<count>: the tile's entries of A are A[a_t, a_t+1) and of B B[b_t, b_t+1) — BO_TILE indices together,
//     staged in LDS.  Every slot finds its slice and its split there and is "lhs only", "rhs only", "lhs of a pair" or "rhs
//     of a pair" by its own neighbour: the lhs slot looks at B[b], the rhs slot at A[a - 1] (read from global memory when a
//     tile edge cuts the pair: no communication between tiles).  The lhs slot of a pair carries op(l, r), the rhs slot of a
//     pair nothing.  Out: the number of emitting slots per tile.
//  3. exclusive_scan_u64 over the tile counts; the result's nnz is read back ON THE CALLER'S STREAM and the result is
//     allocated at its exact size.
//  4. binop_tile_kernel<emit>: the same classification; slot q = j * 256 + thread, so the ballots of the 8 rounds x 4 waves,
//     prefix-summed in LDS, give every emitting slot its position and one wave instruction stores to consecutive positions.
//     The tile that holds slot s_r writes indptr_out[r] (runs of empty slices, whose s_r coincide, included); the last tile
//     writes the slices that start at N and indptr_out[outer].
// No float atomics, no look-back between workgroups.  Unsorted or duplicated indices of an unchecked handle give an
// unspecified result but never an access outside the arrays: every split is clamped to its slice and its tile, a tile whose
// edges are inconsistent emits nothing, and both passes count the same way, so positions stay below the allocated nnz.
#pragma once

#include <functional>

#include "common.hpp"

namespace sprs_hip {
namespace bo {

constexpr int BO_BLOCK = 256;
constexpr int BO_WAVES = BO_BLOCK / 64;
constexpr int BO_TILE = 2048;                       // option binop_tile (fixed: min = max = default)
constexpr int BO_ITEMS = BO_TILE / BO_BLOCK;
constexpr int BO_BALLOTS = BO_ITEMS * BO_WAVES;     // one 64-bit emit mask per (round, wave), in slot order
constexpr int BO_ROWS = 2048;                       // slice starts of a tile kept in LDS; a tile that meets more slices reads indptr

// indptr of an operand: a matrix's array, or — a sparse vector, p == nullptr — the one slice [0, nnz)
template <typename P>
struct Ptrs {
    const P *p;
    uint64_t nnz;
    __device__ __forceinline__ int64_t operator()(uint64_t r) const {
        const uint64_t v = p ? (uint64_t)p[r] : (r ? nnz : 0);
        return (int64_t)(v < nnz ? v : nnz);        // (a borrowed, unchecked indptr cannot point past the arrays)
    }
};

struct Operands {
    const void *ipa, *ipb;                          // null for vectors
    const void *ia, *ib;
    const double *va, *vb;
    uint64_t outer, nnza, nnzb;
    int32_t op;
    bool drop_zero;
};

// One IEEE operation.  NaN operands: gfx9 has no subtract instruction — l - r is v_add_f64(l, -r), and the source modifier flips
// the sign of a NaN that comes from r alone, where the reference's subsd / fsub hands r on unchanged (quieted).  That one case is
// put right here, so NaN results carry the reference's bits too whenever the reference's own are defined (with NaNs on BOTH
// sides of a commutative operation the host compiler is free to pick either one).
__device__ __forceinline__ double apply(int op, double l, double r) {
    if (op == SPRS_HIP_BINOP_ADD) return l + r;
    if (op == SPRS_HIP_BINOP_MUL) return l * r;
    const double v = l - r;
    return (r != r && l == l) ? __longlong_as_double(__double_as_longlong(r) | 0x0008000000000000ll) : v;
}

// merge-path split of slot k: the smallest a in [alo, ahi] with A(a) > B(k - 1 - a) (an lhs index goes first on a tie)
template <typename FA, typename FB>
__device__ __forceinline__ int64_t split(int64_t k, int64_t alo, int64_t ahi, FA A, FB B) {
    while (alo < ahi) {
        const int64_t mid = (alo + ahi) >> 1;
        if (A(mid) <= B(k - 1 - mid)) alo = mid + 1;
        else ahi = mid;
    }
    return alo;
}

__device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
// position v relative to a tile of n entries that starts at base: -1 = in front of the tile, n + 1 = behind it
__device__ __forceinline__ int32_t rel(int64_t v, int64_t base, int64_t n) { return (int32_t)imin(imax(v - base, -1), n + 1); }

// 1. tile edge t (slot k = min(t * BO_TILE, N)), t = 0 .. ntiles:
//    cut_first[t] = the first slice that starts at or after slot k;  cut_r[t] = the slice that holds slot k;
//    cut_a[t]     = entries of A in front of slot k (those of B: k - cut_a[t])
template <typename P, typename I>
__global__ void __launch_bounds__(BO_BLOCK) binop_partition_kernel(Ptrs<P> pa, Ptrs<P> pb, const I *ia, const I *ib, uint64_t outer,
                                                                   uint64_t ntiles, uint64_t *cut_a, uint64_t *cut_r,
                                                                   uint64_t *cut_first) {
    const uint64_t t = (uint64_t)blockIdx.x * BO_BLOCK + threadIdx.x;
    if (t > ntiles) return;
    const int64_t N = (int64_t)(pa.nnz + pb.nnz);
    const int64_t k = imin((int64_t)(t * BO_TILE), N);
    uint64_t lo = 0, hi = outer;                    // s_outer = N >= k
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pa(mid) + pb(mid) >= k) hi = mid;
        else lo = mid + 1;
    }
    cut_first[t] = lo;
    if (k >= N || outer == 0) {
        cut_a[t] = pa.nnz;
        cut_r[t] = outer ? outer - 1 : 0;
        return;
    }
    lo = 0;
    hi = outer - 1;
    while (lo < hi) {                               // the last slice with s_r <= k: it is not empty, slot k is inside
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (pa(mid) + pb(mid) <= k) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t r = lo;
    const int64_t ra0 = pa(r), ra1 = pa(r + 1), rb0 = pb(r), rb1 = pb(r + 1);
    int64_t a = split(k, imax(ra0, k - rb1), imin(ra1, k - rb0), [&](int64_t x) { return ia[x]; }, [&](int64_t y) { return ib[y]; });
    a = imin(imax(a, imax(ra0, k - (int64_t)pb.nnz)), imin(ra1, k));   // 0 <= a <= nnz(A), 0 <= k - a <= nnz(B) whatever the indices hold
    cut_a[t] = (uint64_t)a;
    cut_r[t] = r;
}

// 2. / 4. one tile of BO_TILE slots.  EMIT = false: counts[tile] = emitting slots.  EMIT = true: offs[tile] is the tile's
// first position in the result; indices / values of the emitting slots and the indptr entries of the slices that start
// inside the tile are written.
template <typename P, typename I, bool EMIT>
__global__ void __launch_bounds__(BO_BLOCK) binop_tile_kernel(Ptrs<P> pa, Ptrs<P> pb, const I *ia, const I *ib, const double *va,
                                                              const double *vb, uint64_t outer, int op, int drop_zero,
                                                              const uint64_t *cut_a, const uint64_t *cut_r, const uint64_t *cut_first,
                                                              uint64_t ntiles, uint64_t *counts, const uint64_t *offs, P *ip_out,
                                                              I *ix_out, double *v_out, uint64_t nnz_out) {
    __shared__ I s_idx[BO_TILE];                    // A[a0, a1) then B[b0, b1)
    __shared__ int32_t s_rs[BO_ROWS + 1], s_ra[BO_ROWS + 1], s_rb[BO_ROWS + 1];   // slice starts: slot, entry of A, entry of B
    __shared__ uint64_t s_ball[BO_BALLOTS];
    __shared__ uint32_t s_pre[BO_BALLOTS + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t t = blockIdx.x;
    const int64_t N = (int64_t)(pa.nnz + pb.nnz);
    const int64_t k0 = (int64_t)(t * BO_TILE), k1 = imin(k0 + BO_TILE, N);
    const int64_t a0 = (int64_t)cut_a[t], a1 = (int64_t)cut_a[t + 1];
    const int64_t b0 = k0 - a0, b1 = k1 - a1;
    // (edges that do not nest — possible only with unsorted indices — : the tile emits nothing)
    const bool sane = a0 >= 0 && a0 <= a1 && a1 <= (int64_t)pa.nnz && b0 >= 0 && b0 <= b1 && b1 <= (int64_t)pb.nnz;
    const int64_t na = a1 - a0;
    if (sane) {
        for (int64_t x = tid; x < k1 - k0; x += BO_BLOCK) s_idx[x] = x < na ? ia[a0 + x] : ib[b0 + x - na];
    }
    const uint64_t rlo = cut_r[t], rhi = t + 1 < ntiles ? cut_r[t + 1] : (outer ? outer - 1 : 0);
    // the slices rlo .. rhi meet the tile: their starts RELATIVE to the tile (-1: in front of it, n + 1: behind it), from LDS
    // when there are at most BO_ROWS of them, else from the indptr arrays
    const int64_t nb = (k1 - k0) - na, nrows = (int64_t)(rhi - rlo) + 1;
    const bool staged = nrows <= BO_ROWS;
    if (sane && staged) {
        for (int64_t x = tid; x <= nrows; x += BO_BLOCK) {
            const int64_t A = pa(rlo + x), B = pb(rlo + x);
            s_ra[x] = rel(A, a0, na);
            s_rb[x] = rel(B, b0, nb);
            s_rs[x] = rel(A + B, k0, k1 - k0);
        }
    }
    __syncthreads();
    // The BO_ITEMS slots of a thread (slot q = j * BO_BLOCK + thread) are searched side by side: every step of a search is one
    // LDS round trip, and the round trips of the items overlap instead of queueing up.
    const int32_t nq = (int32_t)(k1 - k0);
    int32_t row_a0[BO_ITEMS], row_a1[BO_ITEMS], row_b0[BO_ITEMS], row_b1[BO_ITEMS];   // the slice of slot q: the last one with s_r <= k0 + q
    if (sane && staged) {
        int32_t lo[BO_ITEMS], hi[BO_ITEMS];
#pragma unroll
        for (int j = 0; j < BO_ITEMS; ++j) {
            lo[j] = 0;
            hi[j] = (int32_t)nrows - 1;
        }
        int steps = 0;                              // ceil(log2(nrows)): the same for the whole workgroup
        while ((1ll << steps) < nrows) ++steps;
        for (int s = 0; s < steps; ++s) {
#pragma unroll
            for (int j = 0; j < BO_ITEMS; ++j) {
                const int32_t mid = (lo[j] + hi[j] + 1) >> 1;      // (lo once the search is over: s_rs[lo] <= q holds)
                if (s_rs[mid] <= j * BO_BLOCK + tid) lo[j] = mid;
                else hi[j] = mid - 1;
            }
        }
#pragma unroll
        for (int j = 0; j < BO_ITEMS; ++j) {
            row_a0[j] = s_ra[lo[j]], row_a1[j] = s_ra[lo[j] + 1];
            row_b0[j] = s_rb[lo[j]], row_b1[j] = s_rb[lo[j] + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < BO_ITEMS; ++j) {
            const int64_t q = j * BO_BLOCK + tid;
            row_a0[j] = row_a1[j] = row_b0[j] = row_b1[j] = 0;
            if (sane && q < nq) {
                uint64_t lo = rlo, hi = rhi;
                while (lo < hi) {
                    const uint64_t mid = (lo + hi + 1) >> 1;
                    if (pa(mid) + pb(mid) <= k0 + q) lo = mid;
                    else hi = mid - 1;
                }
                row_a0[j] = rel(pa(lo), a0, na), row_a1[j] = rel(pa(lo + 1), a0, na);
                row_b0[j] = rel(pb(lo), b0, nb), row_b1[j] = rel(pb(lo + 1), b0, nb);
            }
        }
    }
    // the split (a, b), a + b = q, of every slot inside the part of its slice pair that lies in the tile; all positions are
    // relative to (a0, b0)
    int32_t a_lo[BO_ITEMS], a_hi[BO_ITEMS];
#pragma unroll
    for (int j = 0; j < BO_ITEMS; ++j) {
        const int32_t q = j * BO_BLOCK + tid;
        const int32_t ra0 = row_a0[j] > 0 ? row_a0[j] : 0, ra1 = row_a1[j] < (int32_t)na ? row_a1[j] : (int32_t)na;
        const int32_t rb0 = row_b0[j] > 0 ? row_b0[j] : 0, rb1 = row_b1[j] < (int32_t)nb ? row_b1[j] : (int32_t)nb;
        a_lo[j] = ra0 > q - rb1 ? ra0 : q - rb1;
        a_hi[j] = ra1 < q - rb0 ? ra1 : q - rb0;
        if (!sane || q >= nq) a_lo[j] = a_hi[j] = 0;
    }
    bool more = true;
    while (more) {
        more = false;
#pragma unroll
        for (int j = 0; j < BO_ITEMS; ++j) {
            if (a_lo[j] < a_hi[j]) {
                const int32_t mid = (a_lo[j] + a_hi[j]) >> 1;
                if (s_idx[mid] <= s_idx[(int32_t)na + j * BO_BLOCK + tid - 1 - mid]) a_lo[j] = mid + 1;    // an lhs index goes first on a tie
                else a_hi[j] = mid;
                more = true;
            }
        }
    }
    I idx[BO_ITEMS];
    double val[BO_ITEMS];
#pragma unroll
    for (int j = 0; j < BO_ITEMS; ++j) {
        const int64_t q = j * BO_BLOCK + tid;       // the slot, counted from the tile's first
        bool emit = false;
        idx[j] = 0;
        val[j] = 0.0;
        if (sane && q < nq) {
            const int64_t ra0 = imax(row_a0[j], 0), ra1 = imin(row_a1[j], na), rb0 = imax(row_b0[j], 0), rb1 = imin(row_b1[j], nb);
            const int64_t a = a_lo[j], b = q - a;
            const bool has_a = a >= ra0 && a < ra1, has_b = b >= rb0 && b < rb1;
            const I xa = has_a ? s_idx[a] : (I)0, xb = has_b ? s_idx[na + b] : (I)0;
            if (has_a && (!has_b || xa <= xb)) {
                // an lhs slot; its pair, if any, is B[b] (beyond the tile's edge when b == nb: read from memory)
                bool pair = false;
                if (b >= rb0 && b < row_b1[j]) pair = (has_b ? xb : ib[b0 + b]) == xa;
                val[j] = apply(op, va[a0 + a], pair ? vb[b0 + b] : 0.0);
                idx[j] = xa;
                emit = true;
            } else if (has_b) {
                // an rhs slot; the rhs of a pair when A[a - 1] holds the same index: that slot carried op(l, r)
                bool pair = false;
                if (a > row_a0[j] && a <= ra1) pair = (a >= 1 ? s_idx[a - 1] : ia[a0 - 1]) == xb;
                if (!pair) {
                    val[j] = apply(op, 0.0, vb[b0 + b]);
                    idx[j] = xb;
                    emit = true;
                }
            }
            if (emit && drop_zero && val[j] == 0.0) emit = false;      // !is_zero(): +0.0 and -0.0 go, NaN stays
        }
        const uint64_t mask = __ballot(emit);
        if (lane == 0) s_ball[j * BO_WAVES + w] = mask;
    }
    __syncthreads();
    if (tid <= BO_BALLOTS) {
        uint32_t pre = 0;
        for (int x = 0; x < tid; ++x) pre += (uint32_t)__popcll(s_ball[x]);
        s_pre[tid] = pre;
    }
    __syncthreads();
    const uint64_t total = s_pre[BO_BALLOTS];
    if (!EMIT) {
        if (tid == 0) counts[t] = total;
        return;
    }
    const uint64_t base = offs[t];
#pragma unroll
    for (int j = 0; j < BO_ITEMS; ++j) {
        const uint64_t mask = s_ball[j * BO_WAVES + w];
        if ((mask >> lane) & 1ull) {
            const uint64_t pos = base + s_pre[j * BO_WAVES + w] + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (pos < nnz_out) {
                ix_out[pos] = idx[j];
                v_out[pos] = val[j];
            }
        }
    }
    if (ip_out) {
        const uint64_t rfirst = cut_first[t], rend = t + 1 == ntiles ? outer + 1 : cut_first[t + 1];
        for (uint64_t r = rfirst + tid; r < rend; r += BO_BLOCK) {
            const int64_t q = pa(r) + pb(r) - k0;   // 0 <= q <= k1 - k0; == only for the slices that start at N (last tile)
            uint64_t pos = base + total;
            if (q >= 0 && q < k1 - k0) {
                const uint64_t m = s_ball[q >> 6];
                pos = base + s_pre[q >> 6] + (uint64_t)__popcll(m & ((1ull << (q & 63)) - 1ull));
            }
            ip_out[r] = (P)pos;
        }
    }
}

// `&A * s`: one stream over the values, 16 bytes per lane and access
struct alignas(16) Pair {
    double x, y;
};

__global__ void __launch_bounds__(BO_BLOCK) scale_kernel(const double *in, uint64_t n, double alpha, double *out) {
    const uint64_t stride = (uint64_t)gridDim.x * BO_BLOCK;
    const uint64_t first = (uint64_t)blockIdx.x * BO_BLOCK + threadIdx.x;
    if ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
        const Pair *in2 = (const Pair *)in;
        Pair *out2 = (Pair *)out;
        for (uint64_t i = first; i < n / 2; i += stride) {
            const Pair v = in2[i];
            Pair o;
            o.x = v.x * alpha;
            o.y = v.y * alpha;
            out2[i] = o;
        }
        if ((n & 1) && first == 0) out[n - 1] = in[n - 1] * alpha;
    } else {                                        // a borrowed array on an 8-byte boundary
        for (uint64_t i = first; i < n; i += stride) out[i] = in[i] * alpha;
    }
}

// where the result's arrays come from once its nnz is known: (nnz, &indptr | null, &indices, &data)
using Alloc = std::function<int32_t(uint64_t, void **, void **, double **)>;

template <typename P, typename I>
int32_t run(const Operands &o, const Alloc &alloc, hipStream_t st) {
    const uint64_t N = o.nnza + o.nnzb, ntiles = (N + BO_TILE - 1) / BO_TILE;
    void *ip_out = nullptr, *ix_out = nullptr;
    double *v_out = nullptr;
    if (ntiles == 0) {
        SPRS_TRY(alloc(0, &ip_out, &ix_out, &v_out));
        if (ip_out) SPRS_TRY_HIP(hipMemsetAsync(ip_out, 0, (o.outer + 1) * sizeof(P), st));
        SPRS_TRY_HIP(hipStreamSynchronize(st));
        return SPRS_HIP_OK;
    }
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "binop: operands of more than 2^42 entries are not supported");
    // cut_a | cut_r | cut_first (ntiles + 1 each) | counts (ntiles) | offsets (ntiles + 1)
    DevBuf tmp;
    SPRS_TRY_HIP(tmp.alloc_for(st, (5 * ntiles + 4) * 8));
    uint64_t *cut_a = tmp.u64(), *cut_r = cut_a + ntiles + 1, *cut_first = cut_r + ntiles + 1;
    uint64_t *counts = cut_first + ntiles + 1, *offs = counts + ntiles;
    const Ptrs<P> pa{(const P *)o.ipa, o.nnza}, pb{(const P *)o.ipb, o.nnzb};
    const I *ia = (const I *)o.ia, *ib = (const I *)o.ib;
    const int dz = o.drop_zero ? 1 : 0;
    hipLaunchKernelGGL((binop_partition_kernel<P, I>), dim3((unsigned)((ntiles + BO_BLOCK) / BO_BLOCK)), dim3(BO_BLOCK), 0, st, pa, pb, ia,
                       ib, o.outer, ntiles, cut_a, cut_r, cut_first);
    hipLaunchKernelGGL((binop_tile_kernel<P, I, false>), dim3((unsigned)ntiles), dim3(BO_BLOCK), 0, st, pa, pb, ia, ib, o.va, o.vb, o.outer,
                       (int)o.op, dz, cut_a, cut_r, cut_first, ntiles, counts, offs, (P *)nullptr, (I *)nullptr, (double *)nullptr,
                       (uint64_t)0);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(counts, offs, ntiles, st));
    // the result's nnz, read back in the caller's stream order (a non-blocking stream does not wait for the null stream)
    uint64_t nnz = 0;
    SPRS_TRY_HIP(copy_to_host(&nnz, offs + ntiles, 8, st));
    if (nnz > N) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "binop: inconsistent count");
    SPRS_TRY(alloc(nnz, &ip_out, &ix_out, &v_out));
    hipLaunchKernelGGL((binop_tile_kernel<P, I, true>), dim3((unsigned)ntiles), dim3(BO_BLOCK), 0, st, pa, pb, ia, ib, o.va, o.vb, o.outer,
                       (int)o.op, dz, cut_a, cut_r, cut_first, ntiles, counts, offs, (P *)ip_out, (I *)ix_out, v_out, nnz);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(hipStreamSynchronize(st));         // the result is complete when the call returns (and tmp may go)
    return SPRS_HIP_OK;
}

}  // namespace bo

// csmat_binop (binop.rs:178-223) on two handles of equal shape, storage and index widths (checked by the caller): a new
// handle in that storage, proper indptr, entries with !(val == 0.0).  Blocks until it is complete on `st`.
int32_t csmat_binop_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, int32_t op, OwnedCsmat &res, hipStream_t st) {
    bo::Operands o{a->indptr, b->indptr, a->indices, b->indices, a->data, b->data, a->outer(), a->nnz, b->nnz, op, true};
    const bo::Alloc alloc = [&](uint64_t nnz, void **ip, void **ix, double **v) {
        SPRS_TRY(make_csmat(res, a->storage, a->rows, a->cols, nnz, a->iptr_bytes, a->idx_bytes));
        *ip = res->indptr;
        *ix = res->indices;
        *v = res->data;
        return (int32_t)SPRS_HIP_OK;
    };
    return dispatch_widths(a->idx_bytes, a->iptr_bytes, [&](auto i, auto p) {
        return bo::run<typename decltype(p)::type, typename decltype(i)::type>(o, alloc, st);
    });
}

// csvec_binop (binop.rs:442-467) on two vectors of equal index width: the same kernels with one outer slice and the drop
// test off — every merged index is appended.  `dim`: the result's dimension (after csvec_fix_zeros).
int32_t csvec_binop_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, int32_t op, uint64_t dim, OwnedCsvec &res, hipStream_t st) {
    bo::Operands o{nullptr, nullptr, v->indices, w->indices, v->data, w->data, 1, v->nnz, w->nnz, op, false};
    const bo::Alloc alloc = [&](uint64_t nnz, void **ip, void **ix, double **d) {
        SPRS_TRY(make_csvec(res, dim, nnz, v->idx_bytes, v->user_idx_bytes()));
        *ip = nullptr;
        *ix = res->indices;
        *d = res->data;
        return (int32_t)SPRS_HIP_OK;
    };
    return dispatch_widths(v->idx_bytes, 8, [&](auto i, auto p) {
        return bo::run<typename decltype(p)::type, typename decltype(i)::type>(o, alloc, st);
    });
}

// `&m * alpha` (binop.rs:145-147, CsMatBase::map): the structure copied as it is, every stored value times alpha — stored
// zeros stay stored.  Blocks until the result is complete on `st`.
int32_t csmat_scale_f64(const sprs_hip_csmat *m, double alpha, OwnedCsmat &out, hipStream_t st) {
    OwnedCsmat res;
    SPRS_TRY(copy_csmat(m, false, res, st));
    if (m->nnz) {
        uint64_t blocks = (m->nnz / 2 + bo::BO_BLOCK) / bo::BO_BLOCK;
        if (blocks > 256 * 32) blocks = 256 * 32;
        hipLaunchKernelGGL(bo::scale_kernel, dim3((unsigned)blocks), dim3(bo::BO_BLOCK), 0, st, (const double *)m->data, m->nnz, alpha,
                           res->data);
        SPRS_TRY_HIP(hipGetLastError());
    }
    SPRS_TRY_HIP(hipStreamSynchronize(st));
    out = std::move(res);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
