// Single precision CSR x dense SpMM: the entry-stream kernel of spmm.hip restated for N = f32 — device twin of
//   prod::csr_mulacc_dense_rowmaj   sprs/src/sparse/prod.rs:189-214
// whose MulAcc (mul_acc.rs:17-31) is generic over the scalar (dispatch: csmat.rs:1989-2117).
// Compiled in spmm.hip (included there between the f64 kernels and the host code), so that the library and its emulator build
// (tests/emu, a fixed list of translation units) carry it.
//
// THE DECOMPOSITION is spmm_stream_kernel's: a wave takes a tile of ST_TILE = 256 consecutive entries (non-temporal loads into
// LDS), finds their rows from the indptr values that fall into the tile (marks, then a max-scan), its lane groups walk runs of
// consecutive entries with 16 rhs rows in flight per lane and add in entry order; a row inside one run is stored directly, the
// pieces at run boundaries are joined in run order through LDS, rows that cross tiles through lead / trail carries and the
// fix-up kernel in tile order.  No float atomics, multiply and add unfused (-ffp-contract=off): deterministic.
// What changes with 4-byte values: `eval` in LDS is float (the tile image of a wave is 3 KiB instead of 4), value loads are 4
// bytes, accumulators, carries, the fix-up and the re-layout copy (pitch = the column count of the group in floats) are float.
//
// TWO LANE FORMS (template parameter C = columns per lane; option spmm_f32_pair: 1 auto, 2 paired wherever eligible, 0 scalar):
//  * C = 1, scalar lanes: one column per lane, groups of 8 / 16 / 32 / 64 lanes — correct for every layout.
//  * C = 2, paired lanes: a lane owns two adjacent columns and gathers them with ONE 8-byte load, groups of 4 / 8 / 16 / 32
//    lanes cover 8 / 16 / 32 / 64 columns: twice the runs per wave at the same k, and every gather instruction moves the same
//    8 bytes per lane as the f64 kernel's.  Needs a rhs with unit column stride, an even row pitch and an 8-byte aligned base
//    (always true of the re-laid-out copy).  For odd k the last live lane of a group holds ONE column: it gathers 4 bytes and
//    stores 4 bytes, and touches nothing beyond column k - 1.  Result rows are stored as 8 bytes per lane when `out` allows the
//    same (pair_out), else column by column.
#pragma once

namespace sprs_hip {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the copy: row c of the rhs (any strides) -> row relaid_row(c) of a row-major array with a pitch of KPC floats
template <int KPC>
__global__ __launch_bounds__(MM_BLOCK) void spmm_relayout_f32_kernel(const float *__restrict__ rhs, uint64_t ld_rhs, uint64_t cs_rhs, uint64_t rows_rhs,
                                                                     uint32_t k, float *__restrict__ dst) {
    const uint32_t j = threadIdx.x % KPC;
    const uint64_t c = ((uint64_t)blockIdx.x * MM_BLOCK + threadIdx.x) / KPC;
    if (c >= rows_rhs || j >= k) return;
    __builtin_nontemporal_store(rhs[c * ld_rhs + (uint64_t)j * cs_rhs], dst + (uint64_t)relaid_row((uint32_t)c) * KPC + j);
}

// KP lanes per group, C columns per lane (KP * C = 8 / 16 / 32 / 64 columns); C = 2 requires cs_rhs == 1, an even ld_rhs and an
// 8-byte aligned rhs.  relaid: the column ids go through relaid_row.  pair_out: cs_out == 1, ld_out even, out 8-byte aligned.
template <typename IDX, typename PTR, int KP, int C, bool ACC>
__global__ __launch_bounds__(MM_BLOCK) void spmm_stream_f32_kernel(const PTR *__restrict__ indptr, const IDX *__restrict__ indices,
                                                                   const float *__restrict__ data, uint64_t rows, uint64_t nnz,
                                                                   const uint64_t *__restrict__ tile_row, uint64_t ntiles,
                                                                   const float *__restrict__ rhs, uint64_t ld_rhs, uint64_t cs_rhs, uint32_t k,
                                                                   float *__restrict__ out, uint64_t ld_out, uint64_t cs_out,
                                                                   float *__restrict__ carry, uint32_t relaid, uint32_t pair_out) {
    constexpr int G = WAVE / KP;                         // lane groups = runs of a tile
    constexpr int L = ST_TILE / G;                       // entries of a run
    constexpr int U = L < 16 ? L : 16;                   // rhs rows in flight per lane
    __shared__ uint32_t ecol_s[MM_WAVES][ST_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t erow_s[MM_WAVES][ST_TILE];
    __shared__ __attribute__((aligned(16))) float eval_s[MM_WAVES][ST_TILE];
    __shared__ float seg_s[MM_WAVES][2 * WAVE * C];      // first / last row piece of every run: [which * 64 * C + lane * C + c]
    __shared__ uint32_t segrow_s[MM_WAVES][2 * G];
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const uint32_t j = lane % KP, g = lane / KP;
    const uint64_t t = (uint64_t)blockIdx.x * MM_WAVES + w;
    if (t >= ntiles) return;                             // (whole waves; the kernel has no workgroup barrier)
    uint32_t *ecol = ecol_s[w], *erow = erow_s[w], *segrow = segrow_s[w];
    float *eval = eval_s[w], *seg = seg_s[w];
    const uint64_t e0 = t * ST_TILE;
    const uint32_t nt = (uint32_t)(nnz - e0 < (uint64_t)ST_TILE ? nnz - e0 : (uint64_t)ST_TILE);
    // the entries of the tile (past the end of the matrix: the last entry again, never added)
#pragma unroll
    for (int q = 0; q < ST_Q; ++q) {
        const uint32_t pos = (uint32_t)q * WAVE + lane;
        const uint64_t at = e0 + pos < nnz ? e0 + pos : nnz - 1;
        const uint32_t col = (uint32_t)__builtin_nontemporal_load(indices + at);      // used once: the L2s are for the rhs rows
        eval[pos] = __builtin_nontemporal_load(data + at);
        ecol[pos] = relaid ? relaid_row(col) : col;
        erow[pos] = 0u;
    }
    // rows: as in spmm_stream_kernel — every non-empty row that starts inside the tile marks its first entry with its distance
    // from r0; every EMPTY row is met by exactly one tile, which gives it the zeros of the operator form (csmat.rs:2004)
    const uint64_t r0 = tile_row[t], r1 = tile_row[t + 1];
    const uint64_t s0 = (uint64_t)indptr[r0];
    const uint64_t rhi = r1 < rows ? r1 : rows - 1;
    wave_sync_lds();
    for (uint64_t r = (t == 0 ? 0 : r0 + 1) + lane; r <= rhi; r += WAVE) {
        const uint64_t s = (uint64_t)indptr[r], e = (uint64_t)indptr[r + 1];
        if (e > s) {
            if (r > r0 && s < e0 + nt) erow[s - e0] = (uint32_t)(r - r0);
        } else if constexpr (!ACC) {
            for (uint32_t c = 0; c < k; ++c) out[r * ld_out + (uint64_t)c * cs_out] = 0.0f;
        }
    }
    wave_sync_lds();
    uint32_t run_max = 0;
#pragma unroll
    for (int q = 0; q < ST_Q; ++q) {
        const uint32_t pos = (uint32_t)q * WAVE + lane;
        uint32_t o = wave_incl_max_u32(erow[pos]);
        o = o > run_max ? o : run_max;
        run_max = (uint32_t)__builtin_amdgcn_readlane((int)o, WAVE - 1);
        erow[pos] = o;
    }
    wave_sync_lds();
    const uint32_t row_last = erow[nt - 1];
    // the runs.  A lane's columns are c0 .. c0 + C - 1, of which `live` exist; lanes past the last column load what the last
    // live lane loads (cl, nload columns) and store nothing
    const uint32_t c0 = j * (uint32_t)C;
    const uint32_t clast = ((k - 1) / (uint32_t)C) * (uint32_t)C;
    const uint32_t cl = c0 < clast ? c0 : clast;
    const uint32_t nload = k - cl < (uint32_t)C ? k - cl : (uint32_t)C;
    const uint32_t live = c0 < k ? nload : 0u;
    const float *rbase = rhs + (uint64_t)cl * cs_rhs;
    float *obase = out + r0 * ld_out + (uint64_t)cl * cs_out;
    auto put = [&](uint32_t row, const float (&a)[C]) {   // a finished row of the run: every live column of the lane
        float *dst = obase + (uint64_t)row * ld_out;
        if constexpr (C == 2) {
            if (pair_out && live == 2u) {
                f32x2 v = {a[0], a[1]};
                if constexpr (ACC) {
                    const f32x2 o = *reinterpret_cast<const f32x2 *>(dst);
                    v = f32x2{o[0] + a[0], o[1] + a[1]};
                }
                __builtin_nontemporal_store(v, reinterpret_cast<f32x2 *>(dst));
                return;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
            if ((uint32_t)c < live) {
                float *d = dst + (uint64_t)c * cs_out;
                const float val = ACC ? *d + a[c] : a[c];
                __builtin_nontemporal_store(val, d);
            }
    };
    const uint32_t rb = g * L;
    const uint32_t rn = rb < nt ? (nt - rb < (uint32_t)L ? nt - rb : (uint32_t)L) : 0u;
    uint32_t cur = erow[rb < nt ? rb : 0u], first_row = ST_NONE, last_row = ST_NONE;
    bool first = true;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    for (uint32_t b = 0; b < (uint32_t)L; b += U) {
        if (__ballot(b < rn) == 0ull) break;             // wave-uniform (the last tile only)
        float x[U][C];
        if (C == 1 || nload == 1u) {                      // (one column: 4-byte gathers; the second accumulator of a pair stays 0)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u][0] = rbase[(uint64_t)ecol[rb + b + u] * ld_rhs];
                if constexpr (C == 2) x[u][1] = 0.0f;
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const f32x2 v = *reinterpret_cast<const f32x2 *>(rbase + (uint64_t)ecol[rb + b + u] * ld_rhs);
                x[u][0] = v[0];
                x[u][C - 1] = v[1];
            }
        }
#pragma unroll
        for (int u4 = 0; u4 < U; u4 += 4) {              // rows and values of four entries per LDS read
            const Row4 rw4 = *reinterpret_cast<const Row4 *>(erow + rb + b + u4);
            const f32x4 vv = *reinterpret_cast<const f32x4 *>(eval + rb + b + u4);
            const uint32_t rw[4] = {rw4.x, rw4.y, rw4.z, rw4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = b + (uint32_t)(u4 + e) < rn;
                if (in && rw[e] != cur) {
                    if (first) {
#pragma unroll
                        for (int c = 0; c < C; ++c) seg[lane * C + c] = acc[c];
                        first_row = cur;
                        first = false;
                    } else {
                        put(cur, acc);
                    }
                    cur = rw[e];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float sum = acc[c] + vv[e] * x[u4 + e][c];
                    acc[c] = in ? sum : acc[c];
                }
            }
        }
    }
    if (rn) {
        if (first) {
#pragma unroll
            for (int c = 0; c < C; ++c) seg[lane * C + c] = acc[c];
            first_row = cur;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) seg[WAVE * C + lane * C + c] = acc[c];
            last_row = cur;
        }
    }
    if (j == 0) {
        segrow[2 * g] = first_row;
        segrow[2 * g + 1] = last_row;
    }
    wave_sync_lds();
    // the pieces at the run boundaries, joined in run order by the lanes of the first group (lane = its columns)
    if (lane < (uint32_t)KP && live) {
        const bool lead = s0 < e0;                                    // row r0 began in an earlier tile
        const bool cont = e0 + nt < nnz && r1 == r0 + row_last;       // the last row goes on in the next tile
        float *cbase = carry + 2 * t * (uint64_t)k + c0;
        bool have = false, head = true;
        uint32_t mrow = 0;
        float msum[C];
        auto emit = [&](bool last) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if ((uint32_t)c >= live) continue;
                if (head && lead) cbase[c] = msum[c];                 // (a tile inside one long row: its whole sum is a lead)
                else if (last && cont) cbase[k + c] = msum[c];
                else {
                    float *dst = obase + (uint64_t)mrow * ld_out + (uint64_t)c * cs_out;
                    if constexpr (ACC) *dst = *dst + msum[c];
                    else *dst = msum[c];
                }
            }
            head = false;
        };
        for (int s = 0; s < 2 * G; ++s) {
            const uint32_t row = segrow[s];
            if (row == ST_NONE) continue;
            const float *val = seg + (s & 1) * WAVE * C + ((s >> 1) * KP + (int)j) * C;
            if (have && row == mrow) {
#pragma unroll
                for (int c = 0; c < C; ++c) msum[c] = msum[c] + val[c];
            } else {
                if (have) emit(false);
                mrow = row;
#pragma unroll
                for (int c = 0; c < C; ++c) msum[c] = val[c];
                have = true;
            }
        }
        if (have) emit(true);
    }
}

// rows that cross tiles: spmm_stream_fixup_kernel for float carries.  One lane per column whatever the lane form of the stream
// kernel was (KPC = 8 / 16 / 32 / 64 columns): the carries are laid out by column.
template <typename PTR, int KPC, bool ACC>
__global__ __launch_bounds__(MM_BLOCK) void spmm_stream_fixup_f32_kernel(const PTR *__restrict__ indptr, const uint64_t *__restrict__ tile_row,
                                                                         uint64_t ntiles, const float *__restrict__ carry, uint32_t k,
                                                                         float *__restrict__ out, uint64_t ld_out, uint64_t cs_out) {
    constexpr int G = WAVE / KPC;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t j = lane % KPC, g = lane / KPC;
    const uint32_t jj = j < k ? j : k - 1;
    const uint64_t t = ((uint64_t)blockIdx.x * MM_BLOCK + threadIdx.x) / KPC;
    uint64_t r = 0, tb = 0;
    bool work = false;
    if (t + 1 < ntiles) {                                // (the last tile has no trail)
        const uint64_t e0 = t * ST_TILE, e1 = e0 + ST_TILE;
        r = tile_row[t + 1];                             // the row that holds entry e1
        const uint64_t s = (uint64_t)indptr[r];
        work = s >= e0 && s < e1;                        // it starts in this tile
        if (work) tb = ((uint64_t)indptr[r + 1] - 1) / ST_TILE;       // its last tile
    }
    const bool is_long = work && tb - t > FIX_SPAN;
    if (work && !is_long) {
        float sum = carry[(2 * t + 1) * (uint64_t)k + jj];
        for (uint64_t u = t + 1; u <= tb; ++u) sum = sum + carry[2 * u * (uint64_t)k + jj];
        if (j < k) {
            float *dst = out + r * ld_out + (uint64_t)j * cs_out;
            if constexpr (ACC) *dst = *dst + sum;
            else *dst = sum;
        }
    }
    uint64_t todo = __ballot(is_long && j == 0);
    while (todo) {                                       // (at most one turn: a wave owns G <= 8 consecutive boundaries, a long row spans more than FIX_SPAN = 8 tiles)
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t lt = __shfl(t, src, WAVE), ltb = __shfl(tb, src, WAVE), lr = __shfl(r, src, WAVE);
        float sum = 0.0f;
        for (uint64_t u = lt + 1 + g; u <= ltb; u += G) sum = sum + carry[2 * u * (uint64_t)k + jj];
#pragma unroll
        for (int o = KPC; o < WAVE; o <<= 1) sum += __shfl_xor(sum, o, WAVE);
        if (g == 0 && j < k) {
            sum = carry[(2 * lt + 1) * (uint64_t)k + j] + sum;
            float *dst = out + lr * ld_out + (uint64_t)j * cs_out;
            if constexpr (ACC) *dst = *dst + sum;
            else *dst = sum;
        }
    }
}

// one column block of KPC = 8 / 16 / 32 / 64 columns through the entry stream
template <typename IDX, typename PTR, int KPC>
int32_t launch_stream_f32(sprs_hip_csmat_f32 *a, const float *rhs, uint64_t ld_rhs, uint64_t cs_rhs, uint32_t k, float *out, uint64_t ld_out,
                          uint64_t cs_out, bool acc, float *carry, float *relaid, hipStream_t stream) {
    const SpmmPlan &pl = a->mm;
    const dim3 grid((unsigned)((pl.ntiles + MM_WAVES - 1) / MM_WAVES)), block(MM_BLOCK);
    const dim3 fgrid((unsigned)((pl.ntiles * KPC + MM_BLOCK - 1) / MM_BLOCK));
    if (relaid) {
        hipLaunchKernelGGL((spmm_relayout_f32_kernel<KPC>), dim3((unsigned)((a->cols * KPC + MM_BLOCK - 1) / MM_BLOCK)), block, 0, stream, rhs,
                           ld_rhs, cs_rhs, a->cols, k, relaid);
        rhs = relaid;
        ld_rhs = KPC;
        cs_rhs = 1;
    }
    // the paired form needs a rhs that allows 8-byte gathers (the copy always does).  Option spmm_f32_pair = 1 (auto) takes it
    // where it was measured to win: column groups of 32 and 64 under rows long enough to pay for twice the run
    // ends per wave — R-MAT 1M x 16: 1.4 % and 3.6 % faster; slower at 8 and 16 columns, and at every k on the 5-entry rows of
    // the Laplacian.  2 takes it wherever it is eligible, 0 never.
    const int64_t pf = options().spmm_f32_pair;
    const bool eligible = cs_rhs == 1 && ld_rhs % 2 == 0 && ((uintptr_t)rhs & 7u) == 0;
    const bool pair = eligible && (pf == 2 || (pf == 1 && KPC >= 32 && a->nnz >= 8 * a->rows));
    const uint32_t pair_out = cs_out == 1 && ld_out % 2 == 0 && ((uintptr_t)out & 7u) == 0;
    auto go = [&](auto accv) {
        constexpr bool ACCV = decltype(accv)::value;
        if (pair)
            hipLaunchKernelGGL((spmm_stream_f32_kernel<IDX, PTR, KPC / 2, 2, ACCV>), grid, block, 0, stream, (const PTR *)a->indptr,
                               (const IDX *)a->indices, a->data, a->rows, a->nnz, pl.tile_row, pl.ntiles, rhs, ld_rhs, cs_rhs, k, out, ld_out,
                               cs_out, carry, relaid ? 1u : 0u, pair_out);
        else
            hipLaunchKernelGGL((spmm_stream_f32_kernel<IDX, PTR, KPC, 1, ACCV>), grid, block, 0, stream, (const PTR *)a->indptr,
                               (const IDX *)a->indices, a->data, a->rows, a->nnz, pl.tile_row, pl.ntiles, rhs, ld_rhs, cs_rhs, k, out, ld_out,
                               cs_out, carry, relaid ? 1u : 0u, 0u);
        hipLaunchKernelGGL((spmm_stream_fixup_f32_kernel<PTR, KPC, ACCV>), fgrid, block, 0, stream, (const PTR *)a->indptr, pl.tile_row, pl.ntiles,
                           carry, k, out, ld_out, cs_out);
    };
    if (acc) go(std::true_type{});
    else go(std::false_type{});
    SPRS_TRY_HIP(hipGetLastError());
    return SPRS_HIP_OK;
}

}  // namespace

}  // namespace sprs_hip
