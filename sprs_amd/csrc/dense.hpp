// Dense <-> sparse on gfx950 — device twins of
//   CsMat::csr_from_dense / csc_from_dense                       sprs/src/sparse/csmat.rs:499-549
//   assign_to_dense, CsMat::to_dense                             sprs/src/sparse/to_dense.rs:12-30, csmat.rs:1127-1134
//   csmat_binop_dense_raw with the closures of add_dense_mat_same_ordering / mul_dense_mat_same_ordering
//                                                                sprs/src/sparse/binop.rs:273-433
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
//
// A dense operand is f64 in one of the two contiguous orders with a leading dimension: `lines` lines (rows of a row-major,
// columns of a column-major matrix) of `width` elements, `ld` >= width elements apart.  The unit inner stride is the only one:
// ndarray's general strides (mul_dense_strided walks s![..;2, ..;2]) are out of scope.  Everything below is written in
// line / width terms, which are the outer / inner terms of the sparse storage that matches the layout.
//
// FROM_DENSE (matched pair: CSR with row-major, CSC with column-major).  The logical element axis — lines * width elements in
// line order — is cut into tiles of DN_TILE elements: the shape never enters the partition, 1 x N and N x 1 run alike.
//  1. from_dense_kernel<count>: a thread loads two neighbouring elements per access (16 bytes, non-temporal, where both lie in
//     one line and the address is 16-byte aligned; line starts of an odd width / ld are 8-byte aligned only — those pairs,
//     the pair that straddles a line end and a tile's odd last element go as 8-byte loads) into LDS; element q = j * 256 +
//     thread then votes fabs(x) > eps (NaN, both zeros and |x| == eps drop out), one ballot per (round, wave), one count
//     per tile.  A kept element whose index does not fit the declared index width raises a flag.
//  2. exclusive_scan_u64; nnz and the flag are read back ON THE CALLER'S STREAM; the result is allocated at its exact size.
//  3. from_dense_kernel<emit>: the same votes; the ballots, prefix-summed in LDS, place every kept element, so one wave
//     instruction stores to consecutive positions.  indptr[r] is the position of element r * width, written by the tile that
//     holds it; the last tile writes indptr[lines].  Lines without a kept element, runs of them across tiles included, need
//     nothing special: their first elements have equal positions.
// The two mismatched pairs build the matched storage this way and run to_other_storage on it: the same sorted entries as the
// reference's strided walk.  No look-back between workgroups, no atomics.
//
// ASSIGN / BINOP over the stored entries: tiles of DN_TILE entries on the nnz axis; an entry finds its outer slice by a binary
// search on the slice starts that meet the tile (staged in LDS), as the construction kernels do.  assign moves the value's 64
// bits to out[row, col]; the binop reads rhs there and writes op(l, r).  An inner index at or above the inner dimension (an
// unchecked handle) is skipped: nothing is ever written outside the rows x cols elements.
// BINOP over the dense elements (dense_stream_kernel): out = op(+0.0, r) for EVERY element — the operation is performed, so
// -1 * 0 + 1 * (-0.0) is -0.0 and (alpha * 0) * inf is NaN — 16 bytes per lane and access where both sides allow; the entry
// pass follows on the same stream and overwrites the stored positions.  to_dense's zeroing is the same kernel without a read.
// Arithmetic is unfused (the library is built -ffp-contract=off): alpha * l, beta * r and the sum are three roundings.
#pragma once

#include <cmath>

#include "common.hpp"
#include "construct.hpp"   // ct::start_of, ct::divmod

namespace sprs_hip {
namespace dn {

constexpr int DN_BLOCK = 256;
constexpr int DN_WAVES = DN_BLOCK / 64;
constexpr int DN_TILE = 2048;                       // option dense_tile (fixed: min = max = default)
constexpr int DN_ITEMS = DN_TILE / DN_BLOCK;
constexpr int DN_PAIRS = DN_ITEMS / 2;              // 16-byte accesses of a thread per tile
constexpr int DN_BALLOTS = DN_ITEMS * DN_WAVES;     // one 64-bit keep mask per (round, wave), in element order
constexpr int DN_ROWS = 2048;                       // slice starts of a tile kept in LDS; a tile that meets more slices reads indptr
constexpr int DN_ZERO = -2, DN_ASSIGN = -1;         // modes beside SPRS_HIP_BINOP_ADD / SPRS_HIP_BINOP_MUL
static_assert(DN_ITEMS % 2 == 0, "a thread loads pairs");

typedef double dbl2 __attribute__((ext_vector_type(2)));

// One IEEE operation.  A NaN made out of no NaN (inf * 0, inf - inf) has the sign bit set on the x86 the reference runs on
// (its "real indefinite") and not on gfx9: the reference's bits are put in.  A NaN operand travels through as it does there.
__device__ __forceinline__ double indefinite() { return __longlong_as_double((long long)0xFFF8000000000000ull); }
__device__ __forceinline__ double ieee_mul(double l, double r) {
    const double v = l * r;
    return (v != v && l == l && r == r) ? indefinite() : v;
}
__device__ __forceinline__ double ieee_add(double l, double r) {
    const double v = l + r;
    return (v != v && l == l && r == r) ? indefinite() : v;
}
// the two closures the reference ships (binop.rs:319, 367): &alpha * x + &beta * y  and  alpha * x * y
__device__ __forceinline__ double apply(int op, double alpha, double beta, double l, double r) {
    const double al = ieee_mul(alpha, l);
    return op == SPRS_HIP_BINOP_ADD ? ieee_add(al, ieee_mul(beta, r)) : ieee_mul(al, r);
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---- from_dense ---------------------------------------------------------------------------------------------------------------

// One tile of DN_TILE logical elements of `lines` lines of `width` elements, `ld` apart.  EMIT = false: counts[tile] = kept
// elements; *overflow = 1 when a kept element's index in its line is above c_max or its line above r_max.  EMIT = true:
// offs[tile] is the tile's first position; indices, values and the indptr entries of the lines that start in the tile.
template <typename P, typename I, bool EMIT>
__global__ void __launch_bounds__(DN_BLOCK) from_dense_kernel(const double *m, uint64_t lines, uint64_t width, uint64_t ld, double eps,
                                                              uint64_t c_max, uint64_t r_max, uint64_t ntiles, uint64_t *counts,
                                                              const uint64_t *offs, uint64_t *overflow, P *ip_out, I *ix_out, double *v_out,
                                                              uint64_t nnz_out) {
    __shared__ double s_v[DN_TILE];
    __shared__ I s_c[EMIT ? DN_TILE : 1];           // the element's index in its line (emit pass)
    __shared__ uint64_t s_ball[DN_BALLOTS];
    __shared__ uint32_t s_pre[DN_BALLOTS + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t t = blockIdx.x, N = lines * width;
    const uint64_t k0 = t * DN_TILE, k1 = k0 + DN_TILE < N ? k0 + DN_TILE : N;
    const uint32_t n = (uint32_t)(k1 - k0);
    const bool contig = ld == width;                // one stream: element e sits at m[e]
    const bool check = !EMIT && (width - 1 > c_max || lines - 1 > r_max);
    const bool need_pos = EMIT || !contig || check;
#pragma unroll
    for (int j = 0; j < DN_PAIRS; ++j) {
        const uint32_t q = (uint32_t)(j * DN_BLOCK + tid) * 2;
        if (q >= n) continue;
        const uint64_t e = k0 + q;
        const bool two = q + 1 < n;
        uint64_t line = 0, c = e;
        if (need_pos) ct::divmod(e, width, &line, &c);
        uint64_t line1 = line, c1 = c + 1;          // the pair's second element: the next line's first at a line end
        if (need_pos && c1 == width) line1 = line + 1, c1 = 0;
        const uint64_t a0 = contig ? e : line * ld + c, a1 = contig ? e + 1 : line1 * ld + c1;
        double x0, x1 = 0.0;
        if (two && a1 == a0 + 1 && aligned16(m + a0)) {
            const dbl2 v = __builtin_nontemporal_load((const dbl2 *)(m + a0));
            x0 = v[0], x1 = v[1];
        } else {                                    // head / tail of a line on an 8-byte boundary, a line end, the tile's odd end
            x0 = __builtin_nontemporal_load(m + a0);
            if (two) x1 = __builtin_nontemporal_load(m + a1);
        }
        s_v[q] = x0;
        if (two) s_v[q + 1] = x1;
        if (EMIT) {
            s_c[q] = (I)c;
            if (two) s_c[q + 1] = (I)c1;
        }
        if (check) {                                // I::from_usize of a kept index (csmat.rs:526)
            const bool bad0 = fabs(x0) > eps && (c > c_max || line > r_max);
            const bool bad1 = two && fabs(x1) > eps && (c1 > c_max || line1 > r_max);
            if (bad0 || bad1) *overflow = 1;        // (every writer stores the same word)
        }
    }
    __syncthreads();
    // element q = j * DN_BLOCK + thread: the ballots of the DN_ITEMS rounds x DN_WAVES waves are in element order
    bool keep[DN_ITEMS];
#pragma unroll
    for (int j = 0; j < DN_ITEMS; ++j) {
        const uint32_t q = (uint32_t)(j * DN_BLOCK + tid);
        keep[j] = q < n && fabs(s_v[q]) > eps;      // x.abs() > epsilon: NaN, +-0.0 and |x| == eps are dropped
        const uint64_t mask = __ballot(keep[j]);
        if (lane == 0) s_ball[j * DN_WAVES + w] = mask;
    }
    __syncthreads();
    if (tid <= DN_BALLOTS) {
        uint32_t pre = 0;
        for (int x = 0; x < tid; ++x) pre += (uint32_t)__popcll(s_ball[x]);
        s_pre[tid] = pre;
    }
    __syncthreads();
    const uint64_t total = s_pre[DN_BALLOTS];
    if (!EMIT) {
        if (tid == 0) counts[t] = total;
        return;
    }
    const uint64_t base = offs[t];
#pragma unroll
    for (int j = 0; j < DN_ITEMS; ++j) {
        const uint64_t mask = s_ball[j * DN_WAVES + w];
        if (keep[j]) {
            const uint32_t q = (uint32_t)(j * DN_BLOCK + tid);
            const uint64_t pos = base + s_pre[j * DN_WAVES + w] + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (pos < nnz_out) {
                ix_out[pos] = s_c[q];
                v_out[pos] = s_v[q];                // the element's bits as they are
            }
        }
    }
    // indptr of the lines whose first element k0 <= r * width < k1 lies in the tile; the last tile also writes indptr[lines]
    uint64_t rfirst, rem;
    ct::divmod(k0, width, &rfirst, &rem);
    if (rem) ++rfirst;
    uint64_t rend = lines + 1;
    if (t + 1 < ntiles) {
        ct::divmod(k1, width, &rend, &rem);
        if (rem) ++rend;
    }
    for (uint64_t r = rfirst + tid; r < rend; r += DN_BLOCK) {
        const uint64_t q = r * width - k0;          // == n only for indptr[lines]
        uint64_t pos = base + total;
        if (q < n) pos = base + s_pre[q >> 6] + (uint64_t)__popcll(s_ball[q >> 6] & ((1ull << (q & 63)) - 1ull));
        ip_out[r] = (P)pos;
    }
}

template <typename P, typename I>
int32_t from_dense_run(const double *m, int32_t storage, uint64_t lines, uint64_t width, uint64_t ld, double eps, uint64_t c_max, uint64_t r_max,
                       uint64_t nnz_max, OwnedCsmat &out, hipStream_t st) {
    const bool csr = storage == SPRS_HIP_CSR;
    const uint64_t rows = csr ? lines : width, cols = csr ? width : lines;
    const uint64_t N = lines * width, ntiles = (N + DN_TILE - 1) / DN_TILE;
    OwnedCsmat res;
    if (ntiles == 0) {                              // no element at all: lines + 1 zeros
        SPRS_TRY(make_csmat(res, storage, rows, cols, 0, sizeof(P), sizeof(I)));
        SPRS_TRY_HIP(hipMemsetAsync(res->indptr, 0, (lines + 1) * sizeof(P), st));
        SPRS_TRY_HIP(hipStreamSynchronize(st));
        out = std::move(res);
        return SPRS_HIP_OK;
    }
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "from_dense: more than 2^42 elements are not supported");
    // counts (ntiles) | offsets (ntiles + 1) | overflow flag
    DevBuf tmp;
    SPRS_TRY_HIP(tmp.alloc_for(st, (2 * ntiles + 2) * 8));
    uint64_t *counts = tmp.u64(), *offs = counts + ntiles, *flag = offs + ntiles + 1;
    SPRS_TRY_HIP(hipMemsetAsync(flag, 0, 8, st));
    hipLaunchKernelGGL((from_dense_kernel<P, I, false>), dim3((unsigned)ntiles), dim3(DN_BLOCK), 0, st, m, lines, width, ld, eps, c_max, r_max,
                       ntiles, counts, offs, flag, (P *)nullptr, (I *)nullptr, (double *)nullptr, (uint64_t)0);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(exclusive_scan_u64(counts, offs, ntiles, st));
    // nnz and the flag, read back in the caller's stream order (a non-blocking stream does not wait for the null stream)
    uint64_t back[2] = {0, 0};
    SPRS_TRY_HIP(copy_to_host(back, offs + ntiles, 16, st));
    const uint64_t nnz = back[0];
    if (back[1]) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the index of a kept element");
    if (nnz > nnz_max) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the nnz of the result (%llu)", (unsigned long long)nnz);
    if (nnz > N) SPRS_FAIL(SPRS_HIP_HIP_ERROR, "from_dense: inconsistent count");
    SPRS_TRY(make_csmat(res, storage, rows, cols, nnz, sizeof(P), sizeof(I)));
    hipLaunchKernelGGL((from_dense_kernel<P, I, true>), dim3((unsigned)ntiles), dim3(DN_BLOCK), 0, st, m, lines, width, ld, eps, c_max, r_max,
                       ntiles, counts, offs, flag, (P *)res->indptr, (I *)res->indices, res->data, nnz);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(hipStreamSynchronize(st));         // the result is complete when the call returns (and tmp may go)
    out = std::move(res);
    return SPRS_HIP_OK;
}

// ---- the pass over the dense elements -------------------------------------------------------------------------------------------

// out[line, c] = 0 (DN_ZERO) or op(+0.0, rhs[line, c]) for every element of `lines` lines of `width` elements; rhs lines are ld
// apart, out lines out_ld.  A thread takes two neighbouring elements per step.
template <int MODE>
__global__ void __launch_bounds__(DN_BLOCK) dense_stream_kernel(const double *rhs, uint64_t lines, uint64_t width, uint64_t ld, double alpha,
                                                                double beta, double *out, uint64_t out_ld) {
    const uint64_t N = lines * width, npairs = (N + 1) / 2, stride = (uint64_t)gridDim.x * DN_BLOCK;
    const bool contig = out_ld == width && (MODE == DN_ZERO || ld == width);
    for (uint64_t p = (uint64_t)blockIdx.x * DN_BLOCK + threadIdx.x; p < npairs; p += stride) {
        const uint64_t e = 2 * p;
        const bool two = e + 1 < N;
        uint64_t line = 0, c = e;
        if (!contig) ct::divmod(e, width, &line, &c);
        uint64_t line1 = line, c1 = c + 1;
        if (!contig && c1 == width) line1 = line + 1, c1 = 0;
        const uint64_t o0 = contig ? e : line * out_ld + c, o1 = contig ? e + 1 : line1 * out_ld + c1;
        double y0 = 0.0, y1 = 0.0;
        if (MODE != DN_ZERO) {
            const uint64_t a0 = contig ? e : line * ld + c, a1 = contig ? e + 1 : line1 * ld + c1;
            double x0, x1 = 0.0;
            if (two && a1 == a0 + 1 && aligned16(rhs + a0)) {
                const dbl2 v = __builtin_nontemporal_load((const dbl2 *)(rhs + a0));
                x0 = v[0], x1 = v[1];
            } else {
                x0 = __builtin_nontemporal_load(rhs + a0);
                if (two) x1 = __builtin_nontemporal_load(rhs + a1);
            }
            y0 = apply(MODE, alpha, beta, 0.0, x0);
            y1 = apply(MODE, alpha, beta, 0.0, x1);
        }
        if (two && o1 == o0 + 1 && aligned16(out + o0)) {
            dbl2 v;
            v[0] = y0, v[1] = y1;
            __builtin_nontemporal_store(v, (dbl2 *)(out + o0));
        } else {
            out[o0] = y0;
            if (two) out[o1] = y1;
        }
    }
}

template <int MODE>
int32_t dense_stream(const double *rhs, uint64_t lines, uint64_t width, uint64_t ld, double alpha, double beta, double *out, uint64_t out_ld,
                     hipStream_t st) {
    const uint64_t npairs = (lines * width + 1) / 2;
    if (!npairs) return SPRS_HIP_OK;
    uint64_t blocks = (npairs + DN_BLOCK - 1) / DN_BLOCK;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(dense_stream_kernel<MODE>, dim3((unsigned)blocks), dim3(DN_BLOCK), 0, st, rhs, lines, width, ld, alpha, beta, out, out_ld);
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

// ---- the pass over the stored entries -------------------------------------------------------------------------------------------

// where the outer / inner index of an entry moves in a dense array
struct Strides {
    uint64_t os, is;
};

// One tile of DN_TILE stored entries.  mode DN_ASSIGN: out[o, i] = value; SPRS_HIP_BINOP_ADD / MUL: out[o, i] = op(value, rhs[o, i]).
template <typename P, typename I>
__global__ void __launch_bounds__(DN_BLOCK) entries_kernel(const P *ip, const I *ix, const double *val, uint64_t outer, uint64_t inner,
                                                           uint64_t nnz, int mode, double alpha, double beta, const double *rhs, Strides rs,
                                                           double *out, Strides os) {
    __shared__ uint64_t s_edge[2];
    __shared__ int32_t s_off[DN_ROWS];              // slice starts relative to the tile (-1: in front of it)
    const uint64_t e0 = (uint64_t)blockIdx.x * DN_TILE, e1 = e0 + DN_TILE < nnz ? e0 + DN_TILE : nnz;
    if (e0 >= e1 || outer == 0) return;             // (the whole workgroup)
    if (threadIdx.x < 2) {                          // the last slice that starts at or before the tile's first / last entry
        const uint64_t e = threadIdx.x == 0 ? e0 : e1 - 1;
        uint64_t lo = 0, hi = outer - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (ct::start_of(ip, mid, nnz) <= e) lo = mid;
            else hi = mid - 1;
        }
        s_edge[threadIdx.x] = lo;
    }
    __syncthreads();
    const uint64_t rlo = s_edge[0], rhi = s_edge[1] >= s_edge[0] ? s_edge[1] : s_edge[0];
    const int64_t nrows = (int64_t)(rhi - rlo) + 1;
    const bool staged = nrows <= DN_ROWS;
    if (staged) {
        for (int64_t x = threadIdx.x; x < nrows; x += DN_BLOCK) {
            const uint64_t start = ct::start_of(ip, rlo + x, nnz);
            s_off[x] = start < e0 ? -1 : (int32_t)(start - e0 < (uint64_t)DN_TILE ? start - e0 : (uint64_t)DN_TILE);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DN_ITEMS; ++j) {
        const int32_t q = j * DN_BLOCK + (int32_t)threadIdx.x;
        const uint64_t e = e0 + (uint64_t)q;
        if (e >= e1) continue;
        uint64_t o;
        if (staged) {
            int32_t lo = 0, hi = (int32_t)nrows - 1;
            while (lo < hi) {
                const int32_t mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            o = rlo + (uint64_t)lo;
        } else {
            uint64_t lo = rlo, hi = rhi;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (ct::start_of(ip, mid, nnz) <= e) lo = mid;
                else hi = mid - 1;
            }
            o = lo;
        }
        const uint64_t i = (uint64_t)ix[e];
        if (i >= inner || o >= outer) continue;     // an unchecked handle: never a store outside the rows x cols elements
        const uint64_t at = o * os.os + i * os.is;
        if (mode == DN_ASSIGN) ((uint64_t *)out)[at] = ((const uint64_t *)val)[e];
        else out[at] = apply(mode, alpha, beta, val[e], rhs[o * rs.os + i * rs.is]);
    }
}

inline Strides strides_of(const sprs_hip_csmat *m, int32_t layout, uint64_t ld) {
    const uint64_t row = layout == SPRS_HIP_ROW_MAJOR ? ld : 1, col = layout == SPRS_HIP_ROW_MAJOR ? 1 : ld;
    return m->storage == SPRS_HIP_CSR ? Strides{row, col} : Strides{col, row};
}

inline int32_t entries_run(const sprs_hip_csmat *m, int mode, double alpha, double beta, const double *rhs, Strides rs, double *out, Strides os,
                           hipStream_t st) {
    const uint64_t ntiles = (m->nnz + DN_TILE - 1) / DN_TILE;
    if (!ntiles) return SPRS_HIP_OK;
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "dense: a matrix of more than 2^42 entries is not supported");
    return dispatch_widths(m->idx_bytes, m->iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL((entries_kernel<P, I>), dim3((unsigned)ntiles), dim3(DN_BLOCK), 0, st, (const P *)m->indptr, (const I *)m->indices,
                           (const double *)m->data, m->outer(), m->inner(), m->nnz, mode, alpha, beta, rhs, rs, out, os);
        SPRS_TRY_HIP(hipGetLastError());
        return (int32_t)SPRS_HIP_OK;
    });
}

}  // namespace dn

// csr_from_dense / csc_from_dense (csmat.rs:499-549) on a dense operand whose layout matches `storage`: `lines` outer slices
// of `width` elements, ld apart; eps already clamped.  A kept inner index above c_max, a kept OUTER index above r_max (the
// caller converts the result to the other storage) or more than nnz_max kept elements are INDEX_OVERFLOW.  The handle has the
// given device widths (4 or 8).  Blocks until it is complete on `st`.
int32_t csmat_from_dense_f64(const double *m, int32_t storage, uint64_t lines, uint64_t width, uint64_t ld, double eps, uint64_t c_max,
                             uint64_t r_max, uint64_t nnz_max, int32_t iptr_bytes, int32_t idx_bytes, OwnedCsmat &out, hipStream_t st) {
    return dispatch_widths(idx_bytes, iptr_bytes, [&](auto i, auto p) {
        return dn::from_dense_run<typename decltype(p)::type, typename decltype(i)::type>(m, storage, lines, width, ld, eps, c_max, r_max, nnz_max,
                                                                                          out, st);
    });
}

// assign_to_dense (to_dense.rs:12-30) / to_dense (csmat.rs:1127-1134, zero_first) into a rows x cols array of the given layout
// (dimensions checked by the caller).  Ordered on `st`, not waited for.
int32_t csmat_assign_dense_f64(const sprs_hip_csmat *m, bool zero_first, double *out, int32_t layout, uint64_t ld, hipStream_t st) {
    const bool rowmaj = layout == SPRS_HIP_ROW_MAJOR;
    if (zero_first)
        SPRS_TRY(dn::dense_stream<dn::DN_ZERO>(nullptr, rowmaj ? m->rows : m->cols, rowmaj ? m->cols : m->rows, 0, 0.0, 0.0, out, ld, st));
    const dn::Strides os = dn::strides_of(m, layout, ld);
    return dn::entries_run(m, dn::DN_ASSIGN, 0.0, 0.0, nullptr, os, out, os, st);
}

// csmat_binop_dense_raw (binop.rs:384-433) with op = ADD: (alpha * l) + (beta * r), MUL: (alpha * l) * r; lhs' storage matches
// the layout (checked by the caller); out has rhs' layout and the pitch out_ld.  Ordered on `st`, not waited for.
int32_t csmat_binop_dense_f64(const sprs_hip_csmat *lhs, const double *rhs, int32_t layout, uint64_t ld, int32_t op, double alpha, double beta,
                              double *out, uint64_t out_ld, hipStream_t st) {
    const uint64_t lines = lhs->outer(), width = lhs->inner();
    if (op == SPRS_HIP_BINOP_ADD) SPRS_TRY(dn::dense_stream<SPRS_HIP_BINOP_ADD>(rhs, lines, width, ld, alpha, beta, out, out_ld, st));
    else SPRS_TRY(dn::dense_stream<SPRS_HIP_BINOP_MUL>(rhs, lines, width, ld, alpha, beta, out, out_ld, st));
    return dn::entries_run(lhs, op, alpha, beta, rhs, dn::strides_of(lhs, layout, ld), out, dn::strides_of(lhs, layout, out_ld), st);
}

}  // namespace sprs_hip
