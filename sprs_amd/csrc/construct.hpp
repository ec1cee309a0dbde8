// Construction of sparse matrices on gfx950 — device twins of
//   kronecker_product                                   sprs/src/sparse/kronecker.rs:50-99
//   same_storage_fast_stack / vstack / hstack / bmat    sprs/src/sparse/construct.rs:10-160
// Included by convert.hip (one translation unit of the library and of the emulator build, tests/emu).
// Everything is written in outer / inner terms: a CSC operand is the CSR case on its transposed view, which costs nothing.
//
// KRONECKER.  Result slice s = ia * outer(b) + ib holds, for every stored (ai, av) of slice ia of a and every stored (bi, bv) of
// slice ib of b, both in stored order, the entry (ai * inner(b) + bi, av * bv): one IEEE multiply, nothing dropped.  With
// SA(ia) / SB(ib) the entries of a / b in front of a slice (the base of a sliced indptr taken off), the slice starts at
//     S(ia, ib) = SA(ia) * nnz(b) + lenA(ia) * SB(ib)
// — closed form, no scan, and the result's size nnz(a) * nnz(b) is known on the host: nothing is read back.
//  1. kron_indptr_kernel writes S at the result's indptr width (one division per SLICE to split s into (ia, ib)).
//  2. kron_tile_kernel is tiled on the OUTPUT nnz axis: slice lengths run from 0 to (hub row)^2 and never enter the partition.
//     A workgroup takes CT_TILE consecutive result positions, a thread CT_ITEMS consecutive ones.  The thread finds its first
//     position's (ia, ib) by two binary searches on S — on SA(ia) * nnz(b) over the slices of a that meet the tile, then on
//     lenA * SB(ib) — and (ka, kb) by ONE division (32 bits wide when the operands allow); from there it carries (ka, kb) forward.
//     At a slice's end it steps to the next slice of b when that is not empty and searches again otherwise (runs of empty
//     slices, the end of a slice of a).  a and b are read through the caches; the stream is the two result arrays: the tile is
//     gathered in LDS and leaves as 16-byte non-temporal stores, a contiguous kilobyte per wave instruction.
// STACKING.  One block-assembly family behind all four functions.  Every block is brought to the result's storage first; a
// block (i, j) then has the outer slices R_i .. R_i + rows_i of the result and its inner indices are shifted by its offset.
//  1. stack_rows_kernel, one thread per result slice: indptr_out[R_i + r] = nnz(super-rows above i) + sum_j SB_ij(r), and, where
//     a super-row has several blocks, the result position of each block's part of the slice (a temporary of rows_i words per
//     block).
//  2. stack_copy_kernel is tiled on the nnz axis of each block, ONE launch over the table of blocks: a tile finds its block by
//     its number, an entry its slice by a binary search on the starts of the slices that meet the tile (staged in LDS, as the
//     permutation copy does), and moves.  A block that is alone in its super-row (vstack, the fast stack) is one shifted contiguous copy: no search.
// The table of blocks is built on the host and uploaded on the caller's stream.  Values move as 64-bit words.
// No atomics anywhere.  An unvalidated handle gives an unspecified result but never an access outside the arrays: slice starts
// are clamped to nnz, every load is tested against the operand's nnz and every store against the result's.
#pragma once

#include <cstring>
#include <vector>

#include "common.hpp"

namespace sprs_hip {
namespace ct {

constexpr int CT_BLOCK = 256;
constexpr int CT_TILE = 2048;                       // option construct_tile (fixed: min = max = default)
constexpr int CT_ITEMS = CT_TILE / CT_BLOCK;        // consecutive result entries of a thread
constexpr int CT_ROWS = 2048;                       // slice starts of a tile kept in LDS; a tile that meets more slices reads them from memory
static_assert(CT_ITEMS % 4 == 0, "a thread's entries go out as 16-byte stores");

typedef double ct_dbl2 __attribute__((ext_vector_type(2)));
template <typename I>
struct Vec16 {
    typedef I type __attribute__((ext_vector_type(16 / sizeof(I))));
};

// entries of an operand in front of outer slice r: the base of a sliced indptr taken off, never past the arrays
template <typename P>
__device__ __forceinline__ uint64_t start_of(const P *ip, uint64_t r, uint64_t nnz) {
    const uint64_t v = (uint64_t)ip[r] - (uint64_t)ip[0];
    return v < nnz ? v : nnz;
}

__device__ __forceinline__ void divmod(uint64_t n, uint64_t d, uint64_t *q, uint64_t *r) {
    if (((n | d) >> 32) == 0) {                     // (no 64-bit divide in hardware: the long one only where it is needed)
        *q = (uint32_t)n / (uint32_t)d;
        *r = (uint32_t)n % (uint32_t)d;
    } else {
        *q = n / d;
        *r = n % d;
    }
}

// ---- Kronecker product ---------------------------------------------------------------------------------------------------------

template <typename P, typename I>
struct Kron {
    const P *ap, *bp;
    const I *ai, *bi;
    const double *av, *bv;
    uint64_t outer_a, outer_b, inner_b, nnza, nnzb;
};

// where a thread stands: slice (ia, ib), the entry ranges [a0, a1) / [b0, b1) of the two slices and the pair (a, b) it is at
struct Cursor {
    uint64_t ia, ib, a, a0, a1, b, b0, b1;
};

// the slice pair that holds result position p < nnz(a) * nnz(b), ia searched in [lo, hi]
template <typename P, typename I>
__device__ __forceinline__ void locate(const Kron<P, I> &k, uint64_t p, uint64_t lo, uint64_t hi, Cursor &c) {
    while (lo < hi) {                               // the last ia with SA(ia) * nnz(b) <= p: it is not empty
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (start_of(k.ap, mid, k.nnza) * k.nnzb <= p) lo = mid;
        else hi = mid - 1;
    }
    c.ia = lo;
    c.a0 = start_of(k.ap, lo, k.nnza);
    c.a1 = start_of(k.ap, lo + 1, k.nnza);
    if (c.a1 < c.a0) c.a1 = c.a0;
    const uint64_t len_a = c.a1 - c.a0, in_front = c.a0 * k.nnzb;
    const uint64_t r = p >= in_front ? p - in_front : 0;
    lo = 0;
    hi = k.outer_b - 1;
    while (lo < hi) {                               // the last ib with lenA * SB(ib) <= r
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (len_a * start_of(k.bp, mid, k.nnzb) <= r) lo = mid;
        else hi = mid - 1;
    }
    c.ib = lo;
    c.b0 = start_of(k.bp, lo, k.nnzb);
    c.b1 = start_of(k.bp, lo + 1, k.nnzb);
    if (c.b1 < c.b0) c.b1 = c.b0;
    const uint64_t len_b = c.b1 - c.b0, first = len_a * c.b0;
    uint64_t ka = 0, kb = 0;
    if (len_b) divmod(r >= first ? r - first : 0, len_b, &ka, &kb);
    c.a = c.a0 + ka;
    c.b = c.b0 + kb;
}

// 1. the result's indptr: S(ia, ib) for every slice and nnz(a) * nnz(b) behind the last
template <typename P>
__global__ void __launch_bounds__(CT_BLOCK) kron_indptr_kernel(const P *ap, const P *bp, uint64_t outer_a, uint64_t outer_b, uint64_t nnza,
                                                               uint64_t nnzb, P *out) {
    const uint64_t total = outer_a * outer_b, stride = (uint64_t)gridDim.x * CT_BLOCK;
    for (uint64_t s = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x; s <= total; s += stride) {
        uint64_t v = nnza * nnzb;
        if (s < total) {
            uint64_t ia, ib;
            divmod(s, outer_b, &ia, &ib);
            const uint64_t a0 = start_of(ap, ia, nnza), a1 = start_of(ap, ia + 1, nnza);
            v = a0 * nnzb + (a1 > a0 ? a1 - a0 : 0) * start_of(bp, ib, nnzb);
        }
        out[s] = (P)v;
    }
}

// One IEEE multiply.  inf * 0 makes a NaN out of no NaN: the x86 the reference runs on gives it the sign bit (its "real
// indefinite"), gfx9 does not; the reference's bits are put in.  A NaN operand travels through the multiply as it does there.
__device__ __forceinline__ double kron_mul(double l, double r) {
    const double v = l * r;
    return (v != v && l == l && r == r) ? __longlong_as_double((long long)0xFFF8000000000000ull) : v;
}

// 2. one tile of CT_TILE consecutive result entries
template <typename P, typename I>
__global__ void __launch_bounds__(CT_BLOCK) kron_tile_kernel(Kron<P, I> k, I *ix_out, double *v_out) {
    __shared__ uint64_t s_edge[2];
    const uint64_t total = k.nnza * k.nnzb;
    const uint64_t k0 = (uint64_t)blockIdx.x * CT_TILE, k1 = k0 + CT_TILE < total ? k0 + CT_TILE : total;
    if (k0 >= k1) return;
    if (threadIdx.x < 2) {                          // the slices of a that hold the tile's first / last entry
        Cursor e;
        locate(k, threadIdx.x == 0 ? k0 : k1 - 1, 0, k.outer_a - 1, e);
        s_edge[threadIdx.x] = e.ia;
    }
    __syncthreads();
    // a thread computes CT_ITEMS consecutive entries, the workgroup stores the tile from LDS: every wave instruction writes one
    // contiguous kilobyte instead of 64 pieces 64 bytes apart
    __shared__ I s_ix[CT_TILE];
    __shared__ double s_v[CT_TILE];
    const uint32_t q0 = threadIdx.x * CT_ITEMS;
    const uint64_t p0 = k0 + q0;
    if (p0 < k1) {
        const uint64_t ia_hi = s_edge[1];
        Cursor c;
        locate(k, p0, s_edge[0], ia_hi, c);
        bool ok_a = c.a < k.nnza;
        uint64_t xa = ok_a ? (uint64_t)k.ai[c.a] * k.inner_b : 0;
        double va = ok_a ? k.av[c.a] : 0.0;
#pragma unroll
        for (int j = 0; j < CT_ITEMS; ++j) {
            if (p0 + j >= k1) break;
            const bool ok = ok_a && c.b < k.nnzb;
            s_ix[q0 + j] = ok ? (I)(xa + (uint64_t)k.bi[c.b]) : (I)0;
            s_v[q0 + j] = ok ? kron_mul(va, k.bv[c.b]) : 0.0;
            if (j + 1 == CT_ITEMS || p0 + j + 1 >= k1) break;
            if (++c.b < c.b1) continue;
            c.b = c.b0;                             // the next entry of a's slice against the whole of b's
            if (++c.a >= c.a1) {                    // the slice pair is done
                c.a = c.a0;
                bool found = false;
                if (c.ib + 1 < k.outer_b) {
                    const uint64_t n0 = c.b1, n1 = start_of(k.bp, c.ib + 2, k.nnzb);
                    if (n1 > n0) {
                        ++c.ib;
                        c.b = c.b0 = n0;
                        c.b1 = n1;
                        found = true;
                    }
                }
                if (!found) locate(k, p0 + j + 1, c.ia, ia_hi, c);
            }
            ok_a = c.a < k.nnza;
            xa = ok_a ? (uint64_t)k.ai[c.a] * k.inner_b : 0;
            va = ok_a ? k.av[c.a] : 0.0;
        }
    }
    __syncthreads();
    // (the arrays of a result and a tile's first entry sit on 16-byte boundaries)
    const uint32_t n = (uint32_t)(k1 - k0);
    typedef typename Vec16<I>::type ivec;
    constexpr uint32_t PER = 16 / sizeof(I);
    for (uint32_t q = threadIdx.x * PER; q < n; q += CT_BLOCK * PER) {
        if (q + PER <= n) {
            ivec w;
#pragma unroll
            for (uint32_t x = 0; x < PER; ++x) w[x] = s_ix[q + x];
            __builtin_nontemporal_store(w, (ivec *)(ix_out + k0 + q));
        } else {
            for (uint32_t x = q; x < n; ++x) ix_out[k0 + x] = s_ix[x];
        }
    }
    for (uint32_t q = threadIdx.x * 2; q < n; q += CT_BLOCK * 2) {
        if (q + 2 <= n) {
            ct_dbl2 w;
            w[0] = s_v[q];
            w[1] = s_v[q + 1];
            __builtin_nontemporal_store(w, (ct_dbl2 *)(v_out + k0 + q));
        } else {
            v_out[k0 + q] = s_v[q];
        }
    }
}

inline unsigned grid_for(uint64_t n, uint64_t cap) {
    uint64_t blocks = (n + CT_BLOCK - 1) / CT_BLOCK;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

template <typename P, typename I>
int32_t kron_run(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat *res, hipStream_t st) {
    const Kron<P, I> k{(const P *)a->indptr, (const P *)b->indptr, (const I *)a->indices, (const I *)b->indices, a->data, b->data,
                       a->outer(), b->outer(), b->inner(), a->nnz, b->nnz};
    const uint64_t total = k.nnza * k.nnzb, ntiles = (total + CT_TILE - 1) / CT_TILE;
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "kronecker_product: a result of more than 2^42 entries is not supported");
    hipLaunchKernelGGL(kron_indptr_kernel<P>, dim3(grid_for(k.outer_a * k.outer_b + 1, 256 * 64)), dim3(CT_BLOCK), 0, st, k.ap, k.bp, k.outer_a,
                       k.outer_b, k.nnza, k.nnzb, (P *)res->indptr);
    if (ntiles) hipLaunchKernelGGL((kron_tile_kernel<P, I>), dim3((unsigned)ntiles), dim3(CT_BLOCK), 0, st, k, (I *)res->indices, res->data);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY_HIP(hipStreamSynchronize(st));         // the result is complete when the call returns
    return SPRS_HIP_OK;
}

// ---- stacking --------------------------------------------------------------------------------------------------------------

struct StackBlock {                                 // one present block, in the result's outer / inner terms
    const void *ip, *ix;
    const uint64_t *val;
    uint64_t *dstart;                               // result position of the first entry of each of its slices; null: alone in its super-row
    uint64_t rows, nnz, col_off, tile0, pos0;       // tile0: its first tile; pos0: entries of the result in the super-rows above
};

struct StackRow {                                   // one super-row: its first result slice, the entries above it, its blocks
    uint64_t row0, nnz_above, first, count;
};

// 1. the result's indptr and, in a super-row of several blocks, where each block's part of a slice goes
template <typename P>
__global__ void __launch_bounds__(CT_BLOCK) stack_rows_kernel(const StackBlock *blk, const StackRow *srow, uint64_t nsrows, uint64_t total_rows,
                                                              uint64_t total_nnz, P *ip_out) {
    const uint64_t stride = (uint64_t)gridDim.x * CT_BLOCK;
    for (uint64_t g = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x; g <= total_rows; g += stride) {
        if (g == total_rows) {
            ip_out[g] = (P)total_nnz;
            continue;
        }
        uint64_t lo = 0, hi = nsrows - 1;
        while (lo < hi) {                           // the last super-row that starts at or before g: it is not empty
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (srow[mid].row0 <= g) lo = mid;
            else hi = mid - 1;
        }
        const StackRow sr = srow[lo];
        const uint64_t r = g - sr.row0;
        uint64_t run = sr.nnz_above;
        for (uint64_t x = sr.first; x < sr.first + sr.count; ++x)
            if (r < blk[x].rows) run += start_of((const P *)blk[x].ip, r, blk[x].nnz);
        ip_out[g] = (P)(run < total_nnz ? run : total_nnz);
        if (sr.count < 2) continue;
        for (uint64_t x = sr.first; x < sr.first + sr.count; ++x) {
            if (r >= blk[x].rows) continue;
            const uint64_t s = start_of((const P *)blk[x].ip, r, blk[x].nnz), e = start_of((const P *)blk[x].ip, r + 1, blk[x].nnz);
            blk[x].dstart[r] = run;
            run += e > s ? e - s : 0;
        }
    }
}

// 2. one tile of CT_TILE consecutive entries of one block
template <typename P, typename I>
__global__ void __launch_bounds__(CT_BLOCK) stack_copy_kernel(const StackBlock *blk, uint64_t nblocks, uint64_t total_nnz, I *ix_out,
                                                              uint64_t *v_out) {
    __shared__ uint64_t s_blk, s_edge[2];
    __shared__ int32_t s_off[CT_ROWS];              // slice starts relative to the tile (-1: in front of it)
    __shared__ int64_t s_delta[CT_ROWS];            // result position - block position of the slice's entries
    const uint64_t t = blockIdx.x;
    if (threadIdx.x == 0) {
        uint64_t lo = 0, hi = nblocks - 1;
        while (lo < hi) {                           // the last block whose tiles start at or before t: it has tiles
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (blk[mid].tile0 <= t) lo = mid;
            else hi = mid - 1;
        }
        s_blk = lo;
    }
    __syncthreads();
    const StackBlock b = blk[s_blk];
    const P *ip = (const P *)b.ip;
    const I *ix = (const I *)b.ix;
    const uint64_t e0 = (t - b.tile0) * CT_TILE, e1 = e0 + CT_TILE < b.nnz ? e0 + CT_TILE : b.nnz;
    if (t < b.tile0 || e0 >= e1 || b.rows == 0) return;   // (the whole workgroup)
    if (!b.dstart) {                                // alone in its super-row: one shifted contiguous copy
#pragma unroll
        for (int j = 0; j < CT_ITEMS; ++j) {
            const uint64_t e = e0 + (uint64_t)j * CT_BLOCK + threadIdx.x, pos = b.pos0 + e;
            if (e < e1 && pos < total_nnz) {
                ix_out[pos] = (I)((uint64_t)ix[e] + b.col_off);
                v_out[pos] = b.val[e];
            }
        }
        return;
    }
    if (threadIdx.x < 2) {                          // the last slice that starts at or before the tile's first / last entry
        const uint64_t e = threadIdx.x == 0 ? e0 : e1 - 1;
        uint64_t lo = 0, hi = b.rows - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (start_of(ip, mid, b.nnz) <= e) lo = mid;
            else hi = mid - 1;
        }
        s_edge[threadIdx.x] = lo;
    }
    __syncthreads();
    const uint64_t rlo = s_edge[0], rhi = s_edge[1];
    // the slices rlo .. rhi meet the tile: their starts relative to the tile (-1: in front of it) and where they go, from LDS
    // when there are at most CT_ROWS of them (a tile that meets more — runs of empty slices — reads the arrays)
    const int64_t nrows = (int64_t)(rhi - rlo) + 1;
    const bool staged = nrows <= CT_ROWS;
    if (staged) {
        for (int64_t x = threadIdx.x; x < nrows; x += CT_BLOCK) {
            const uint64_t start = start_of(ip, rlo + x, b.nnz);
            s_off[x] = start < e0 ? -1 : (int32_t)(start - e0 < (uint64_t)CT_TILE ? start - e0 : (uint64_t)CT_TILE);
            s_delta[x] = (int64_t)b.dstart[rlo + x] - (int64_t)start;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CT_ITEMS; ++j) {
        const int32_t q = j * CT_BLOCK + (int32_t)threadIdx.x;
        const uint64_t e = e0 + (uint64_t)q;
        if (e >= e1) continue;
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
                if (start_of(ip, mid, b.nnz) <= e) lo = mid;
                else hi = mid - 1;
            }
            delta = (int64_t)b.dstart[lo] - (int64_t)start_of(ip, lo, b.nnz);
        }
        const uint64_t pos = (uint64_t)((int64_t)e + delta);
        if (pos < total_nnz) {
            ix_out[pos] = (I)((uint64_t)ix[e] + b.col_off);
            v_out[pos] = b.val[e];
        }
    }
}

}  // namespace ct

// kronecker_product (kronecker.rs:61-95) on two handles of equal storage and index widths whose result fits them (both checked
// by the caller): a new handle in that storage at its exact size.  Blocks until it is complete on `st`.
int32_t csmat_kronecker_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &out, hipStream_t st) {
    OwnedCsmat res;
    SPRS_TRY(make_csmat(res, a->storage, a->rows * b->rows, a->cols * b->cols, a->nnz * b->nnz, a->iptr_bytes, a->idx_bytes));
    SPRS_TRY(dispatch_widths(a->idx_bytes, a->iptr_bytes, [&](auto i, auto p) {
        return ct::kron_run<typename decltype(p)::type, typename decltype(i)::type>(a, b, res.get(), st);
    }));
    out = std::move(res);
    return SPRS_HIP_OK;
}

// The assembly behind same_storage_fast_stack, vstack, hstack and bmat (construct.rs:10-160).  `items`: the present blocks, all
// of the result's `storage` and of equal index widths, ordered by super-row and inside a super-row from the first to the last;
// `outer_of[i]`: the outer slices of super-row i (every block of it has that many — the caller's dimension check).  The result
// is rows x cols with the sum of the blocks' entries.  Blocks until it is complete on `st`.
int32_t csmat_stack(const std::vector<StackItem> &items, const std::vector<uint64_t> &outer_of, int32_t storage, uint64_t rows, uint64_t cols,
                    int32_t iptr_bytes, int32_t idx_bytes, OwnedCsmat &out, hipStream_t st) {
    const uint64_t nb = items.size(), ns = outer_of.size();
    std::vector<ct::StackBlock> blk(nb);
    std::vector<ct::StackRow> srow(ns);
    uint64_t total_rows = 0, total_nnz = 0, ntiles = 0, words = 0, x = 0;
    for (uint64_t i = 0; i < ns; ++i) {
        srow[i] = {total_rows, total_nnz, x, 0};
        for (; x < nb && items[x].srow == i; ++x) {
            const sprs_hip_csmat *m = items[x].m;
            blk[x] = {m->indptr, m->indices, (const uint64_t *)m->data, nullptr, m->outer(), m->nnz, items[x].inner_off, ntiles, srow[i].nnz_above};
            ntiles += (m->nnz + ct::CT_TILE - 1) / ct::CT_TILE;
            total_nnz += m->nnz;
            ++srow[i].count;
        }
        if (srow[i].count > 1) words += srow[i].count * outer_of[i];
        total_rows += outer_of[i];
    }
    if (ntiles > 0x7FFFFFFFull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "stacking: more than 2^42 entries are not supported");
    OwnedCsmat res;
    SPRS_TRY(make_csmat(res, storage, rows, cols, total_nnz, iptr_bytes, idx_bytes));
    // the table: blocks | super-rows, and behind it the slice positions of the blocks that share a super-row
    const uint64_t blk_bytes = nb * sizeof(ct::StackBlock), row_bytes = ns * sizeof(ct::StackRow);
    DevBuf table, starts;
    SPRS_TRY_HIP(table.alloc_for(st, blk_bytes + row_bytes));
    SPRS_TRY_HIP(starts.alloc_for(st, words * 8));
    uint64_t at = 0;
    for (uint64_t i = 0; i < ns; ++i) {
        if (srow[i].count < 2) continue;
        for (uint64_t b = srow[i].first; b < srow[i].first + srow[i].count; ++b, at += outer_of[i]) blk[b].dstart = starts.u64() + at;
    }
    std::vector<unsigned char> host(blk_bytes + row_bytes);
    if (blk_bytes) memcpy(host.data(), blk.data(), blk_bytes);
    if (row_bytes) memcpy(host.data() + blk_bytes, srow.data(), row_bytes);
    if (!host.empty()) SPRS_TRY_HIP(copy_to_device(table.p, host.data(), host.size(), st));
    const ct::StackBlock *d_blk = table.as<ct::StackBlock>();
    const ct::StackRow *d_row = (const ct::StackRow *)((const unsigned char *)table.p + blk_bytes);
    SPRS_TRY(dispatch_widths(idx_bytes, iptr_bytes, [&](auto i, auto p) {
        using I = typename decltype(i)::type;
        using P = typename decltype(p)::type;
        hipLaunchKernelGGL(ct::stack_rows_kernel<P>, dim3(ct::grid_for(total_rows + 1, 256 * 64)), dim3(ct::CT_BLOCK), 0, st, d_blk, d_row, ns,
                           total_rows, total_nnz, (P *)res->indptr);
        if (ntiles)
            hipLaunchKernelGGL((ct::stack_copy_kernel<P, I>), dim3((unsigned)ntiles), dim3(ct::CT_BLOCK), 0, st, d_blk, nb, total_nnz,
                               (I *)res->indices, (uint64_t *)res->data);
        SPRS_TRY_HIP(hipGetLastError());
        return (int32_t)SPRS_HIP_OK;
    }));
    SPRS_TRY_HIP(hipStreamSynchronize(st));         // the result is complete when the call returns (and the temporaries may go)
    out = std::move(res);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip
