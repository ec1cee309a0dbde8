// Single precision on the product path: CSR x dense-vector SpMV for N = f32 — device twin of
//   prod::mul_acc_mat_vec_csr      sprs/src/sparse/prod.rs:103-127   (accumulate)
//   prod::csr_mulacc_dense_colmaj  sprs/src/sparse/prod.rs:274-298   (1 rhs column; `&A * &x`)
// whose MulAcc (mul_acc.rs:17-31) is generic over the scalar — and what an f32 handle needs around it: to_other_storage
// (csmat.rs:1405-1426) and the value casts CsMat::map(|&v| v as f32) / (|&v| v as f64) (csmat.rs:1289-1305).
// Compiled in spmv.hip, so that the library and its emulator build (tests/emu, a fixed list of translation units) carry it.
//
// THE KERNEL is the nnz-tile kernel of spmv.hip restated for 4-byte values: workgroup c owns the entries [c*T, (c+1)*T);
// every lane streams 4 values (16 bytes) and 4 column ids (16 bytes at 4-byte width, two 16-byte loads at 8) per pass with
// non-temporal loads — 8 bytes of stream per stored entry with 4-byte indices against 12 for f64; products are rounded to
// f32 (-ffp-contract=off), staged in a float LDS array (half the LDS of the f64 kernel) and summed per row segment of the
// tile: segments shorter than LONG_SEG = 64 entries LEFT TO RIGHT FROM 0.0f BY ONE LANE — a row that lies inside one tile
// gets the bits of the reference's chain, which the f32 BiCGSTAB relies on for small systems — longer ones by a wave
// (lane l sums entries l, l + 64, ..., then a shuffle tree).  The part of a tile that belongs to a row which started in
// an earlier tile goes to carry[c]; a second small kernel adds the carries of such a row in tile order.  No float atomics:
// run-to-run deterministic.  Empty rows: the accumulate form leaves y[r]'s bits alone, the operator form writes +0.0f.
// The seams are those of the f64 kernel: T (2048 / 4096), the 4-entry vector path of a full tile against the scalar path
// of the last one, LONG_SEG, SEG_CHUNK = 2048 staged row boundaries, and tile_of_block's runs of tiles per XCD.
//
// THE PLAN is the tile index over the handle's own arrays (build_tile_rows) and one carry array per stream, built at the
// first multiply or by sprs_hip_csmat_f32_prepare — or the BANDED plan of spmv_band.hip with float values, x, partial sums and
// carries (hot slices of up to 32768 labels: option spmv_f32_band_tile).  The policy is the f64 handle's (spmv.hip): a forced plan
// (spmv_band = 1) at once; under auto the first multiply on the tile plan and the banded plan from the second one on, or from
// sprs_hip_csmat_f32_prepare, for matrices of at least 2^22 entries whose x takes 4 MiB (cols * 4) and whose long rows hold half
// the entries; spmv_band = 2 keeps the tile plan.  There is no XCD-sliced plan for f32: spmv_xcs does not apply.
#pragma once
#include "spmv_shared.hpp"

namespace sprs_hip {

typedef float flt4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct TileArgsF32 {
    const void *indptr;          // PTR[rows + 1]
    const void *indices;         // IDX[nnz]
    const float *data;
    const uint64_t *tile_row;    // ntiles + 1
    float *carry;                // ntiles
    float *y;
    uint64_t nnz, ntiles;
};

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}

// 4 consecutive column ids from a 16-byte aligned address, used once
template <typename IDX>
__device__ __forceinline__ void load_idx4(const IDX *p, IDX (&c)[4]) {
    if constexpr (sizeof(IDX) == 4) {
        const u32x4 v = __builtin_nontemporal_load((const u32x4 *)p);
        c[0] = v[0], c[1] = v[1], c[2] = v[2], c[3] = v[3];
    } else {
        const u64x2 lo = __builtin_nontemporal_load((const u64x2 *)p);
        const u64x2 hi = __builtin_nontemporal_load((const u64x2 *)(p + 2));
        c[0] = lo[0], c[1] = lo[1], c[2] = hi[0], c[3] = hi[1];
    }
}

template <typename IDX, typename PTR, bool ACC, int TILE>
__global__ __launch_bounds__(BLOCK) void spmv_f32_tile_kernel(TileArgsF32 a, const float *__restrict__ x) {
    constexpr int V = 4;                          // elements per lane per pass (16 B of data)
    constexpr int PASSES = TILE / (BLOCK * V);

    __shared__ __attribute__((aligned(16))) float prod[TILE];
    __shared__ uint32_t segb[SEG_CHUNK + 1];
    __shared__ uint32_t longlist[TILE / LONG_SEG + 1];
    __shared__ uint32_t nlong;

    const PTR *__restrict__ indptr = (const PTR *)a.indptr;
    float *__restrict__ y = a.y;
    const uint64_t tile = tile_of_block(blockIdx.x, a.ntiles);
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wave = tid / WAVE;
    const uint64_t base = tile * (uint64_t)TILE;
    const uint32_t cnt = (a.nnz - base < (uint64_t)TILE) ? (uint32_t)(a.nnz - base) : (uint32_t)TILE;
    const uint64_t lim = base + cnt;
    const uint64_t R0 = a.tile_row[tile], R1 = a.tile_row[tile + 1];
    const uint64_t S = R1 - R0 + 1;               // head + rows starting in this tile

    if (tid == 0) nlong = 0;

    // ---- phase 1: stream the tile, gather x, products -> LDS ---------------
    const IDX *ip = (const IDX *)a.indices + base;
    const float *dp = a.data + base;
    if (cnt == (uint32_t)TILE) {
        IDX ix[PASSES][V];
        flt4 av[PASSES];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const uint32_t i = p * (BLOCK * V) + tid * V;
            load_idx4<IDX>(ip + i, ix[p]);                                  // used once: keep L2 for x
            av[p] = __builtin_nontemporal_load((const flt4 *)(dp + i));
        }
        float xv[PASSES][V];
#pragma unroll
        for (int p = 0; p < PASSES; ++p)
#pragma unroll
            for (int k = 0; k < V; ++k) xv[p][k] = x[(uint64_t)ix[p][k]];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const uint32_t i = p * (BLOCK * V) + tid * V;
            flt4 pr;
#pragma unroll
            for (int k = 0; k < V; ++k) pr[k] = av[p][k] * xv[p][k];
            *(flt4 *)&prod[i] = pr;
        }
    } else {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const uint32_t i = p * (BLOCK * V) + tid * V;
#pragma unroll
            for (int k = 0; k < V; ++k) prod[i + k] = i + k < cnt ? dp[i + k] * x[(uint64_t)ip[i + k]] : 0.0f;
        }
    }

    // ---- phase 2: per-segment sums -----------------------------------------
    // segment 0 = head (tail of row R0-1), segment j>=1 = row R0+j-1.
    // boundary B[0] = 0, B[j] = min(indptr[R0+j-1], lim) - base   (j = 1..S)
    for (uint64_t j0 = 0; j0 < S; j0 += SEG_CHUNK) {
        const uint32_t n = (S - j0 < (uint64_t)SEG_CHUNK) ? (uint32_t)(S - j0) : (uint32_t)SEG_CHUNK;
        for (uint32_t t = tid; t <= n; t += BLOCK) {
            const uint64_t j = j0 + t;
            uint32_t b = 0;
            if (j != 0) {
                const uint64_t v = (uint64_t)indptr[R0 + j - 1];
                b = (uint32_t)((v < lim ? v : lim) - base);
            }
            segb[t] = b;
        }
        __syncthreads();   // prod[], segb[], nlong visible

        for (uint32_t t = tid; t < n; t += BLOCK) {
            const uint32_t sa = segb[t], sb = segb[t + 1];
            const uint32_t len = sb - sa;
            if (len >= LONG_SEG) {
                longlist[atomicAdd(&nlong, 1u)] = t;
            } else {
                float s = 0.0f;
                for (uint32_t k = sa; k < sb; ++k) s += prod[k];   // the reference's chain
                const uint64_t j = j0 + t;
                if (j == 0) {
                    a.carry[tile] = s;
                } else {
                    const uint64_t r = R0 + j - 1;
                    if constexpr (ACC) {
                        if (len) y[r] = y[r] + s;   // empty rows keep y[r] untouched (prod.rs:120-126)
                    } else {
                        y[r] = s;
                    }
                }
            }
        }
        __syncthreads();   // longlist complete

        const uint32_t nl = nlong;
        for (uint32_t q = wave; q < nl; q += NWAVES) {
            const uint32_t t = longlist[q];
            const uint32_t sa = segb[t], sb = segb[t + 1];
            float s = 0.0f;
            for (uint32_t k = sa + lane; k < sb; k += WAVE) s += prod[k];
            s = wave_sum_f32(s);
            if (lane == 0) {
                const uint64_t j = j0 + t;
                if (j == 0) {
                    a.carry[tile] = s;
                } else {
                    const uint64_t r = R0 + j - 1;
                    if constexpr (ACC) y[r] = y[r] + s;
                    else y[r] = s;
                }
            }
        }
        __syncthreads();   // everyone done with segb/longlist before the next chunk
        if (tid == 0) nlong = 0;
    }
}

// fix-up: a row that spans several tiles gets the heads of the later tiles added in tile order.  One thread per tile.
template <typename PTR>
__global__ void spmv_f32_carry_kernel(TileArgsF32 a, uint32_t TILE) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c + 1 >= a.ntiles) return;
    const uint64_t R0 = a.tile_row[c], R1 = a.tile_row[c + 1];
    if (R1 == R0) return;                                                        // no row starts in tile c
    if ((uint64_t)((const PTR *)a.indptr)[R1] <= (c + 1) * (uint64_t)TILE) return;   // last row ends inside tile c
    float acc = 0.0f;
    for (uint64_t d = c + 1; d < a.ntiles && a.tile_row[d] == R1; ++d) acc += a.carry[d];
    a.y[R1 - 1] += acc;
}

// ---- value casts and the gather behind to_other_storage: one thread per stored entry -------------------------
__global__ void narrow_values_kernel(const double *__restrict__ in, uint64_t n, float *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];          // round to nearest even; overflow -> +-inf; NaN stays NaN
}

__global__ void widen_values_kernel(const float *__restrict__ in, uint64_t n, double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];         // exact
}

__global__ void iota_f64_kernel(uint64_t n, double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)i;
}

// out[k] = in[from[k]]: from = the source position of every converted entry, an integer below n < 2^53 held in a double
__global__ void gather_values_f32_kernel(const float *__restrict__ in, const double *__restrict__ from, uint64_t n,
                                         float *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = (uint64_t)from[i];
    if (src < n) out[i] = in[src];
}

namespace {
constexpr uint64_t ENTRY_TILE = 256;     // entries per workgroup of the four kernels above
inline dim3 entry_grid(uint64_t n) { return dim3((unsigned)((n + ENTRY_TILE - 1) / ENTRY_TILE)); }
}  // namespace

int32_t csmat_f32_from_f64(const sprs_hip_csmat *m, OwnedCsmatF32 &out, hipStream_t stream) {
    if (m->nnz > 0x7fffffffull * ENTRY_TILE) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "too many entries for one launch");
    OwnedCsmatF32 res;
    SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, m->nnz, m->iptr_bytes, m->idx_bytes));
    SPRS_TRY_HIP(hipMemcpyAsync(res->indptr, m->indptr, (m->outer() + 1) * (uint64_t)m->iptr_bytes, hipMemcpyDeviceToDevice, stream));
    if (m->nnz) {
        SPRS_TRY_HIP(hipMemcpyAsync(res->indices, m->indices, m->nnz * (uint64_t)m->idx_bytes, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(narrow_values_kernel, entry_grid(m->nnz), dim3(ENTRY_TILE), 0, stream, m->data, m->nnz, res->data);
        SPRS_TRY_HIP(hipGetLastError());
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

int32_t csmat_f32_to_f64(const sprs_hip_csmat_f32 *m, OwnedCsmat &out, hipStream_t stream) {
    if (m->nnz > 0x7fffffffull * ENTRY_TILE) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "too many entries for one launch");
    OwnedCsmat res;
    SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, m->nnz, m->iptr_bytes, m->idx_bytes));
    SPRS_TRY_HIP(hipMemcpyAsync(res->indptr, m->indptr, (m->outer() + 1) * (uint64_t)m->iptr_bytes, hipMemcpyDeviceToDevice, stream));
    if (m->nnz) {
        SPRS_TRY_HIP(hipMemcpyAsync(res->indices, m->indices, m->nnz * (uint64_t)m->idx_bytes, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(widen_values_kernel, entry_grid(m->nnz), dim3(ENTRY_TILE), 0, stream, m->data, m->nnz, res->data);
        SPRS_TRY_HIP(hipGetLastError());
    }
    out = std::move(res);
    return SPRS_HIP_OK;
}

// to_other_storage of an f32 matrix: the structure is converted ONCE by the f64 routine of convert.hip (unchanged), run on a
// view of m's index arrays whose "values" are the entries' own positions 0, 1, ... (exact in a double); the f32 values then
// follow their positions.  Like the f64 routine it runs on the null stream and is complete at return.
int32_t csmat_f32_to_other_storage(const sprs_hip_csmat_f32 *m, OwnedCsmatF32 &out) {
    hipStream_t stream = nullptr;
    const uint64_t nnz = m->nnz;
    if (nnz > 0x7fffffffull * ENTRY_TILE) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "too many entries for one launch");
    DevBuf pos;
    SPRS_TRY_HIP(pos.alloc(nnz * sizeof(double)));
    if (nnz) {
        hipLaunchKernelGGL(iota_f64_kernel, entry_grid(nnz), dim3(ENTRY_TILE), 0, stream, nnz, pos.as<double>());
        SPRS_TRY_HIP(hipGetLastError());
    }
    sprs_hip_csmat v;                         // stack view: its destructor finds no plan and no block to release
    view_csmat(m->storage, m->rows, m->cols, nnz, m->indptr, m->iptr_bytes, m->indices, m->idx_bytes, pos.as<double>(), m->device, &v);
    OwnedCsmat conv;
    SPRS_TRY(to_other_storage(&v, conv));
    OwnedCsmatF32 res;
    SPRS_TRY(adopt_structure_f32(conv.get(), res));
    if (nnz) {
        hipLaunchKernelGGL(gather_values_f32_kernel, entry_grid(nnz), dim3(ENTRY_TILE), 0, stream, m->data, conv->data, nnz, res->data);
        SPRS_TRY_HIP(hipGetLastError());
    }
    SPRS_TRY_HIP(hipStreamSynchronize(stream));   // conv's value block goes back to the pool with this scope
    out = std::move(res);
    return SPRS_HIP_OK;
}

// ---- host side of the SpMV ---------------------------------------------------------------------------------
// option spmv_tile (0, 2048 or 4096: sprs_hip_set_option admits nothing else), else the f64 rule (profiles/r01f_ab_log.txt): 4096
// for matrices with long rows, 2048 (more workgroups in flight) when rows are short
static uint32_t f32_tile_for(const sprs_hip_csmat_f32 *a) {
    const int64_t t = options().spmv_tile;
    return t ? (uint32_t)t : (a->nnz > 16 * a->rows ? 4096u : 2048u);
}

#ifndef SPRS_HIP_EMU
static bool f32_capturing(hipStream_t stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool yes = hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return yes;
}
#else
static bool f32_capturing(hipStream_t) { return false; }
#endif

// the options an f32 plan depends on: a handle rebuilds its plan when one of them changes
static uint64_t f32_plan_signature(const Options &o) {
    const int64_t v[] = {o.spmv_tile, o.spmv_band, o.spmv_band_hot, o.spmv_f32_band_tile, o.spmv_band_phases, o.spmv_band_split, o.spmv_band_rounds,
                         o.spmv_band_cold_tiles, o.spmv_band_hot_run, o.spmv_band_share, o.spmv_band_balance};
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t x : v) h = (h ^ (uint64_t)x) * 0x100000001b3ull;
    return h | 1ull;
}

// Does the automatic rule (spmv_band = 0) hand big power-law f32 matrices to the banded plan?  Decided by measurement
// (DESIGN 4.16): it stays on only while the f32 banded plan beats the f32 tile plan by more than the spread of the runs.
constexpr bool F32_BAND_AUTO = true;

// (a->mu held) the plan for the current option values — the banded plan or the tile index — and, for the tile plan, `stream`'s
// carry array.  Building either allocates and synchronises, which a stream that is being captured into a hipGraph cannot do.
// light: the handle's first multiply — the banded plan is not built yet unless the options force it; pl.light then says that the
// next multiply should come back here (build_plan, spmv.hip).
template <typename PTR>
static int32_t f32_plan(sprs_hip_csmat_f32 *a, hipStream_t stream, float **carry, bool light) {
    SpmvPlanF32 &pl = a->plan;
    const Options &o = options();
    if (!pl.built || pl.opt_sig != f32_plan_signature(o) || (pl.light && !light)) {
        if (f32_capturing(stream))
            SPRS_FAIL(SPRS_HIP_INVALID_ARG, "SpMV on a capturing stream needs the handle's plan to exist: call sprs_hip_csmat_f32_prepare first");
        pl = SpmvPlanF32();
        pl.opt_sig = f32_plan_signature(o);
        // auto: the f64 rule for 4-byte x — x larger than one L2 (4 MiB) and a matrix big enough to amortise the copy
        bool want_band = o.spmv_band == 1 || (F32_BAND_AUTO && o.spmv_band == 0 && a->cols * 4 >= (4ull << 20) && a->nnz >= (1ull << 22));
        if (light && want_band && o.spmv_band != 1) {
            pl.light = true;
            want_band = false;
        }
        if (want_band) {
            const int32_t st = band_build(a, stream, pl.band);
            // auto mode: a matrix the banded plan cannot be built for (its temporaries did not fit) keeps the tile plan;
            // an explicit spmv_band = 1 reports the failure
            if (st == SPRS_HIP_OUT_OF_MEMORY && o.spmv_band == 0) {
                (void)hipGetLastError();
                clear_error();
            } else if (st != SPRS_HIP_OK) {
                return st;
            }
        }
        if (!pl.band) {
            pl.tile = f32_tile_for(a);
            pl.ntiles = (a->nnz + pl.tile - 1) / pl.tile;
            if (pl.ntiles > 0x7fffffffull) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "too many tiles for one launch");
            SPRS_TRY_HIP(alloc_block(pl.blocks, pl.tile_row, (pl.ntiles + 1) * sizeof(uint64_t)));
            const uint64_t n = pl.ntiles + 1;
            hipLaunchKernelGGL(build_tile_rows<PTR>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const PTR *)a->indptr, a->rows,
                               pl.ntiles, pl.tile, pl.tile_row);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY_HIP(hipStreamSynchronize(stream));   // plan complete and visible to every stream
        }
        pl.built = true;
    }
    if (pl.band) return SPRS_HIP_OK;                      // (its per-stream scratch: band_spmv / band_prepare_stream)
    auto it = pl.carry.find((void *)stream);
    if (it == pl.carry.end()) {
        if (f32_capturing(stream))
            SPRS_FAIL(SPRS_HIP_INVALID_ARG, "SpMV on a capturing stream needs the handle's plan to exist: call sprs_hip_csmat_f32_prepare with this stream first");
        DevBuf c;
        SPRS_TRY_HIP(c.alloc(pl.ntiles * sizeof(float)));
        it = pl.carry.emplace((void *)stream, std::move(c)).first;
    }
    *carry = it->second.as<float>();
    return SPRS_HIP_OK;
}

template <typename IDX, typename PTR, int TILE>
static int32_t f32_launch(const TileArgsF32 &ta, const float *x, bool acc, hipStream_t stream) {
    const dim3 grid((unsigned)ta.ntiles), block(BLOCK);
    if (acc) hipLaunchKernelGGL((spmv_f32_tile_kernel<IDX, PTR, true, TILE>), grid, block, 0, stream, ta, x);
    else hipLaunchKernelGGL((spmv_f32_tile_kernel<IDX, PTR, false, TILE>), grid, block, 0, stream, ta, x);
    SPRS_TRY_HIP(hipGetLastError());
    if (ta.ntiles > 1) {
        hipLaunchKernelGGL(spmv_f32_carry_kernel<PTR>, dim3((unsigned)((ta.ntiles + 255) / 256)), dim3(256), 0, stream, ta, (uint32_t)TILE);
        SPRS_TRY_HIP(hipGetLastError());
    }
    return SPRS_HIP_OK;
}

int32_t spmv_f32_prepare(sprs_hip_csmat_f32 *a, hipStream_t stream) {
    std::lock_guard<std::recursive_mutex> lock(a->mu);
    a->prepared = true;
    if (a->rows == 0 || a->nnz == 0) return SPRS_HIP_OK;
    float *carry = nullptr;
    SPRS_TRY(dispatch_width(a->iptr_bytes, [&](auto p) { return f32_plan<typename decltype(p)::type>(a, stream, &carry, false); }));
    if (a->plan.band) return band_prepare_stream(a, a->plan.band.get(), stream);
    return SPRS_HIP_OK;
}

int32_t spmv_f32(sprs_hip_csmat_f32 *a, const float *x, float *y, bool accumulate, hipStream_t stream) {
    if (a->rows == 0) return SPRS_HIP_OK;
    if (a->nnz == 0) {
        // all rows empty: accumulate leaves y alone, the operator form yields zeros (csmat.rs:2137)
        if (!accumulate) SPRS_TRY_HIP(hipMemsetAsync(y, 0, a->rows * sizeof(float), stream));
        return SPRS_HIP_OK;
    }
    // The handle's lock is held until the kernels are launched, as in launch_tiled (spmv.hip)
    std::lock_guard<std::recursive_mutex> lock(a->mu);
    return dispatch_widths(a->idx_bytes, a->iptr_bytes, [&](auto i, auto p) -> int32_t {
        using IDX = typename decltype(i)::type;
        using PTR = typename decltype(p)::type;
        float *carry = nullptr;
        const bool defer = options().spmv_plan_defer != 0 && a->spmv_calls == 0 && !a->prepared;
        SPRS_TRY(f32_plan<PTR>(a, stream, &carry, defer));
        ++a->spmv_calls;
        const SpmvPlanF32 &pl = a->plan;
        if (pl.band) return band_spmv(a, pl.band.get(), x, y, accumulate, stream);
        const TileArgsF32 ta{a->indptr, a->indices, a->data, pl.tile_row, carry, y, a->nnz, pl.ntiles};
        if (pl.tile == 2048) return f32_launch<IDX, PTR, 2048>(ta, x, accumulate, stream);
        return f32_launch<IDX, PTR, 4096>(ta, x, accumulate, stream);
    });
}

}  // namespace sprs_hip
