// Internal definitions shared by the translation units of libsprs_hip.so.
// Public surface: include/sprs_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sprs_hip.h"

struct sprs_hip_spgemm_plan;      // spgemm.hip
struct sprs_hip_dist;             // dist.hip

namespace sprs_hip {

// ---- thread-local error state ------------------------------------------
void set_error(int32_t status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int32_t fail_hip(hipError_t e, const char *what);   // records + returns status
void clear_error();

#define SPRS_TRY_HIP(expr)                                              \
    do {                                                                \
        hipError_t e__ = (expr);                                        \
        if (e__ != hipSuccess) return ::sprs_hip::fail_hip(e__, #expr); \
    } while (0)

#define SPRS_TRY(expr)                      \
    do {                                    \
        int32_t s__ = (expr);               \
        if (s__ != SPRS_HIP_OK) return s__; \
    } while (0)

#define SPRS_FAIL(status, ...)                        \
    do {                                              \
        ::sprs_hip::set_error((status), __VA_ARGS__); \
        return (status);                              \
    } while (0)

// ---- options -------------------------------------------------------------
// One table for the struct, sprs_hip_set_option and sprs_hip_get_option: X(name, default, min, max, devtools).
// devtools = 1: the option only exists in builds with -DSPRS_HIP_DEVTOOLS (timing experiments that give WRONG results,
// profiling printouts); the release library rejects it with INVALID_ARG and compiles the code behind it out.
#ifdef SPRS_HIP_DEVTOOLS
constexpr bool DEVTOOLS = true;
#else
constexpr bool DEVTOOLS = false;
#endif
#define SPRS_HIP_OPTIONS(X)                                                                                                     \
    X(spmv_kernel, 0, 0, 2, 0)          /* 0 auto, 1 nnz-tiled, 2 wave-per-row (A/B only) */                                     \
    X(spmv_xcs, 0, 0, 2, 0)             /* XCD-sliced plan for long rows: 0 auto, 1 force on, 2 off */                            \
    X(spmv_xcs_split, 32, 2, INT64_MAX, 0) /* rows with >= this many entries go to the sliced part */                             \
    X(spmv_xcs_idx32, 1, 0, 1, 0)       /* plan-owned copies store 32-bit column ids when cols < 2^32 */                          \
    X(spmv_sort_tiles, 0, 0, 1, 0)      /* plan copies: entries of a tile sorted by column (10 % SLOWER: profiles/r01v) */         \
    X(spmv_relabel, 0, 0, 2, 0)         /* sliced plan: columns relabelled by count class: 0 auto (on), 1 on, 2 off */             \
    X(spmv_tile, 0, 0, 4096, 0)         /* nnz per workgroup tile: 0 auto, 2048 or 4096 */                                        \
    X(spmv_lds_pad, 0, 0, 100000, 0)    /* extra dynamic LDS bytes per workgroup: caps workgroups per CU (tuning) */              \
    X(spmv_xmask, -1, INT64_MIN, INT64_MAX, 1) /* TIMING EXPERIMENTS ONLY: gather x[col & mask] (wrong results unless -1) */      \
    X(spmv_plan_defer, 1, 0, 1, 0)      /* 1: a handle's FIRST multiply runs on the plain tile index; the re-laid-out copy plans (banded, XCD-sliced: ~0.1 s to build on a 3e8-entry matrix = 80 SpMVs) are built at the second one, or by sprs_hip_csmat_prepare; 0: at the first (rounds 1-4).  Forced plans (spmv_band = 1, spmv_xcs = 1) are never deferred */ \
    X(spmv_band, 0, 0, 2, 0)            /* banded plan (hot columns from LDS, spmv_band.hip): 0 auto (on), 1 on, 2 off */          \
    X(spmv_band_hot, 0, 0, 384, 0)      /* hot slices (0 = default 128) */                                                        \
    X(spmv_band_tile, 0, 0, 16384, 0)   /* labels per hot slice = doubles of the x tile in LDS: 8192 or 16384 (0 = default 16384) */ \
    X(spmv_f32_band_tile, 0, 0, 32768, 0) /* f32 handles read this one instead: floats of the x tile in LDS, 8192, 16384 or 32768 (0 = default 16384) */ \
    X(spmv_band_phases, 0, 0, 8, 0)     /* label ranges of the cold rest (0 = default 1), 8 hash pieces each */                   \
    X(spmv_band_split, 0, 0, INT64_MAX, 0) /* rows with at least this many entries are cut into pieces (0 = default 24) */        \
    X(spmv_band_rounds, 0, 0, 64, 0)    /* workgroups of the hot kernel per CU, one after the other (0 = default 2) */ \
    X(spmv_band_debug, 0, 0, 255, 1)    /* TIMING EXPERIMENTS ONLY (wrong results): hot kernel 1 no stores of the row sums, 2 one row start per lane, 4 none */ \
    X(spmv_band_tail, 0, 0, 2, 0)       /* with the overlap: 0/1 the reduction of the long rows starts when the hot slices and the cold pieces are done, beside what is left of the short rows; 2 it waits for the whole second stream (rounds 2-4, A/B); on ONE stream (small plans): 0/1 the short rows share the reduction's launch (band_tail_kernel), 2 they run as their own launch in front of the hot slices (round 5) */ \
    X(spmv_band_balance, 0, 0, 2, 0)    /* shares of the hot workgroups: by modelled COST of their tiles (1 + row ends / 180) — 0 auto (small plans, whose hot kernel runs alone on one stream), 1 on, 2 off (equal tile counts) */ \
    X(spmv_band_xcd, 0, 0, 2, 0)        /* hot workgroups: every XCD takes a contiguous run of shares (its L2 serves a slice's x tile to its neighbours) — 0 auto (small plans), 1 on, 2 off (shares dealt round-robin over the XCDs) */ \
    X(spmv_band_pack, 0, 0, 2, 0)       /* hot slices whose wave tiles hold at most two sign / exponent patterns each are stored at 8.5 instead of 10 bytes per entry (lossless, same bits of y): 0/1 on, 2 off (A/B) */ \
    X(spmv_band_share, 0, 0, 1ll << 30, 0) /* wave tiles per workgroup of the hot kernel (0 = default: an equal share for rounds x CUs workgroups) */ \
    X(spmv_band_hot_run, 0, 0, 4096, 0) /* consecutive wave tiles per range of the hot kernel (0 = default 4); a workgroup streams 16 neighbouring ranges */ \
    X(spmv_band_cold_tiles, 0, 0, 64, 0) /* consecutive wave tiles per wave of the cold kernel (0 = default 4) */                 \
    X(spmv_band_overlap, 0, 0, 2, 0)    /* cold pieces + short rows on a second stream beside the hot kernel: 0/1 on, 2 off */     \
    X(spmv_band_split_permute, 0, 0, 2, 0) /* with the overlap: hot labels of x gathered first, the rest scattered on the second stream: 0/1 on, 2 off */ \
    X(spmm_long_row, -1, -1, INT64_MAX, 0) /* SpMM: -1 / 0 default (the entry-stream kernel); L > 0: rows of <= L entries summed in entry order by lane groups, longer ones by 512-entry chunks (reference bits for the short rows, several times slower) */ \
    X(spmm_stream, 1, 0, 1, 0)          /* SpMM: 1 tiles of 256 consecutive entries per wave (default); 0 one wave per row chunk (the kernel of rounds 1-3; also what a matrix with 2^32 or more columns runs) */ \
    X(spgemm_micro, 0, 0, 2, 0)         /* rows of at most 64 products and k's by lane groups, 4 / 2 / 1 rows per wave, no LDS (micro_rows_kernel): 0/1 on, 2 off (the hash kernel, A/B) */ \
    X(spgemm_task_order, 0, 0, 2, 0)    /* large-row tasks: 0/1 costliest first (stable sort by cost class), 2 row order (A/B) */  \
    X(spgemm_xcd_chunk, 0, -1, 0, 0)    /* large-row task list -> XCDs: 0 round-robin, -1 one contiguous run per XCD */            \
    X(spgemm_bucket, 1, 0, 1, 0)        /* column-bucket table of B instead of binary searches (A/B) */                           \
    X(spgemm_prof, 0, 0, 1, 1)          /* print the time of the numeric tasks by class and the longest ones */                   \
    X(spgemm_tokens, 1, 1, 4, 0)        /* token chains of the workgroup kernel's ordered adds: 1, 2 or 4 */                      \
    X(spgemm_keep_bits, 1, 0, 1, 0)     /* the counting pass keeps the bitmaps of the large rows for the numeric pass (one walk of their entries instead of two); 0: the numeric kernel walks for its bits (A/B) */ \
    X(spgemm_lane_order, 0, 0, 2, 0)    /* products of one wave instruction into the LDS accumulators: 0 auto = ONE ds_add_f64 when the device passes the lane-order probe (same-address lanes applied in ascending lane order), else one instruction per k-run; 2 always per k-run (A/B); same bits either way */ \
    X(spgemm_overlap, 0, 0, 1, 0)       /* wave kernels on a second stream beside the large-row kernel */                         \
    X(spgemm_midwin_sym, 14, 14, 16, 0) /* log2 of the window of the wave-per-row COUNTING kernel: 14 or 16 */                        \
    X(spgemm_mid_keep, 8, 4, 8, 0)      /* wave instructions per chunk of the wave-per-row kernel (loads in flight together; kept in registers through a segment): 4 or 8 */ \
    X(spgemm_mid_keep_sym, 8, 8, 16, 0) /* the same for its counting twin: 8 or 16 */ \
    X(spgemm_midwin, 15, 14, 15, 0)     /* log2 of the column window of the wave-per-row kernel: 14 or 15 (measured equal on config 5; 2^16 — 10 waves per CU — slower: profiles/r10d) */ \
    X(spgemm_mid, 65536, 0, 1ll << 31, 0) /* rows of <= 64 k's and at most this many products run one wave per row (0: none) */   \
    X(spgemm_ordered, 1, 0, 1, 0)       /* 1: products are added in the reference's order (values bit-identical to sprs'); 0: the waves of a large-row workgroup add as they arrive (LDS atomics: same products, rounding-level differences, not reproducible run to run; ~20 % faster kernel) */ \
    X(spmm_relayout, 0, 0, 2, 0)        /* SpMM stream kernel: gather from a copy of the rhs whose rows are scattered by a multiplicative hash inside blocks of 4096 rows (hub columns sit at 0, 2^k, 2^j + 2^k: their rhs rows would share a few L2 / fabric channels): 0 auto (a rhs of >= 256 MiB per column block under >= 24 entries per column whose row pitch is a power of two or leaves rows of < 16 columns across lines, or one that is not row-major), 1 on, 2 off */ \
    X(spmm_f32_pair, 1, 0, 2, 0)        /* f32 SpMM stream kernel, paired lanes (a lane owns two adjacent columns, one 8-byte gather; needs a rhs with unit column stride, an even row pitch and an 8-byte aligned base, scalar lanes elsewhere): 1 auto = where eligible AND measured faster (column groups of 32 / 64, at least 8 entries per row); 2 wherever eligible; 0 scalar lanes always.  Same results up to the summation order */ \
    X(spmm_debug, 0, 0, 7, 1)           /* developer A/B of the stream kernel (right results): 1 plain instead of non-temporal entry loads, 2 plain result stores, 4 non-temporal rhs gathers */ \
    X(spgemm_debug, 0, 0, 15, 1)        /* TIMING EXPERIMENTS ONLY (wrong results): 1 no ordering of the adds, 2 no index emission, 4 no value stores and 8 no adds (wave-per-row kernel) */ \
    X(spgemm_occupancy, 3, 2, 3, 0)     /* workgroups per CU the large-row numeric kernel is compiled for: 3 (80 VGPRs) or 2 (128) */ \
    X(spgemm_lds_atomic, 1, 0, 1, 0)    /* value adds as ds_add_f64 (1) or read / add / write (0); same order either way (A/B) */  \
    X(spgemm_winlog, 17, 16, 19, 0)     /* log2 of the widest column window of a large-row task */                                \
    X(spgemm_minwin, 13, 11, 16, 0)     /* log2 of the narrowest column window of a heavy row */                                  \
    X(spgemm_heavy, 524288, 1024, INT64_MAX, 0) /* a row of more products is cut into one task per (narrower) column window */    \
    X(gauss_seidel_blocks, 0, 0, 65536, 0) /* workgroups (4 waves) of the Gauss-Seidel sweep kernel (0 = default: one per CU) */          \
    X(gauss_seidel_chain, 0, 0, 1ll << 30, 0) /* 0 / 1: rows in dependency-level order, one row per lane; S > 1: the band schedule — chains of S consecutive rows per lane, skewed, hand-offs through LDS inside a workgroup (bit-identical; measured not faster as built: DESIGN 4.5) — with this stride, INVALID_ARG when the matrix does not fit it */ \
    X(gauss_seidel_debug, 0, 0, 255, 1) /* TIMING EXPERIMENTS ONLY (wrong results): band kernel without 1 any pipeline work, 2 operand loads, 4 entry loads, 8 index loads */ \
    X(gauss_seidel_xcd, 0, 0, 2, 0)     /* sweep kernel: 1 only the workgroups that find themselves on XCD 0 take part (hand-offs through ONE L2), 0 / 2 every XCD (measured: one XCD is not faster) */ \
    X(gauss_seidel_naps, 0, 0, 64, 0)   /* longest pause of a wave whose rows all wait, in s_sleep(1) units, growing with the wait (0 = default 1) */ \
    X(binop_tile, 2048, 2048, 2048, 0)  /* slots (entries of both operands) per workgroup of the sparse +, -, elementwise * kernels (binop.hpp): fixed, published so that tests can place tile edges */ \
    X(perm_tile, 2048, 2048, 2048, 0)   /* result entries per workgroup of the outer-permutation copy kernel (perm.hpp): fixed, published so that tests can place tile edges */ \
    X(perm_cap, 4096, 4096, 4096, 0)    /* longest row a relabelling permutation sorts in LDS by one workgroup (perm.hpp); longer rows go through the radix sort: fixed, published for the tests */ \
    X(construct_tile, 2048, 2048, 2048, 0) /* result entries (Kronecker product) / block entries (stacking) per workgroup of the construction kernels (construct.hpp): fixed, published so that tests can place tile edges */ \
    X(dense_tile, 2048, 2048, 2048, 0)  /* dense elements (from_dense) / stored entries (assign_to_dense, the sparse-with-dense binops) per workgroup of the dense <-> sparse kernels (dense.hpp): fixed, published so that tests can place tile edges */ \
    X(ordering_narrow_cap, 1024, 0, 1024, 0) /* Cuthill-McKee (ordering.hpp): a frontier of at most this many vertices (and at most 4096 stored entries) is expanded, sorted and committed in LDS by the one-workgroup kernel, which goes on to the next level or component without returning to the host; wider levels run as a grid; 0: every level runs as a grid.  Published so that tests can put the seam at 8 vertices */ \
    X(ordering_key_bits, 64, 1, 64, 0)  /* Cuthill-McKee, wide levels: the key (owner, degree, id) goes through ONE radix sort when it fits this many bits, else through two stable ones (by id, then by owner and degree); 64 = whenever it fits a word.  Published so that tests can take the second route */ \
    X(sptrisolve_budget, 4096, 1, 1ll << 20, 0) /* sparse-rhs triangular solve (sptrisolve.hpp): levels of the reach the one-workgroup kernel runs per launch before it hands the state back to the host; a reach of depth d costs ceil(d / budget) launches and read-backs while its frontiers stay narrow (at most 1024 vertices and 4096 stored entries).  Published so that tests can cross it with a short chain */ \
    X(ldl_lds_cap, 1024, 1, 1024, 0)   /* LDL^T numeric kernel (ldl.hpp): a row of L with at most this many entries keeps its work vector y in LDS, a longer one in its slice of a device array.  Published so that tests can run both paths at small n */ \
    X(pool, 1, 0, 1, 0)                 /* keep released result blocks (>= 1 MiB) for the next result instead of hipFree */        \
    X(pool_max_bytes, 128ll << 30, 0, INT64_MAX, 0) /* cap on the bytes the pool may hold */

struct Options {
#define SPRS_X(name, def, lo, hi, dev) int64_t name = (def);
    SPRS_HIP_OPTIONS(SPRS_X)
#undef SPRS_X
};
Options &options();

// handle.hpp: result-block pool
hipError_t pool_alloc(void **p, uint64_t bytes, uint64_t *cap, int device);
// stream_ordered = true: the block was only ever touched by work enqueued on the NULL stream (or on streams joined back to it)
// and every later user of the pool enqueues there too, so it goes back without waiting for the device
void pool_free(void *p, uint64_t cap, int device, bool stream_ordered = false);
uint64_t pool_trim();
uint64_t pool_cached_bytes();

// One block of the pool and its owner: the block goes back (pool_free, which waits for the device) with the owner.  The handles
// below hold one per array they own; a borrowed handle or a view has its array pointers set and its owners empty.
struct PoolBlock {
    void *p = nullptr;
    uint64_t cap = 0;              // bytes of the block (>= what was asked for: blocks come from the pool)
    int dev = 0;
    PoolBlock() = default;
    PoolBlock(PoolBlock &&o) noexcept : p(o.p), cap(o.cap), dev(o.dev) { o.p = nullptr; }
    PoolBlock &operator=(PoolBlock &&o) noexcept {
        std::swap(p, o.p), std::swap(cap, o.cap), std::swap(dev, o.dev);
        return *this;
    }
    ~PoolBlock() { pool_free(p, cap, dev); }
    hipError_t alloc(uint64_t bytes, int device) {   // (on an empty owner)
        dev = device;
        return pool_alloc(&p, bytes, &cap, dev);
    }
};

// A device block and its owner: a call's temporary, released when it goes out of scope, or an array that a plan or a
// per-stream scratch derives from a handle's arrays, released with the plan.  Move-only.
//   alloc:        a private block (hipMalloc), released with hipFree.
//   alloc_pooled: a block of the pool, handed back in null-stream order (pool_free above); legal only for work ordered on the
//                 null stream.
//   alloc_for:    alloc_pooled for work on the null stream, alloc for any other.
struct DevBuf {
    void *p = nullptr;
    uint64_t cap = 0;              // bytes of the block (a pooled one may be larger than what was asked for)
    int dev = 0;
    bool pooled = false;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), dev(o.dev), pooled(o.pooled) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p, o.p), std::swap(cap, o.cap), std::swap(dev, o.dev), std::swap(pooled, o.pooled);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p && pooled) pool_free(p, cap, dev, true);
        else if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
    hipError_t alloc(uint64_t bytes) {
        release();
        pooled = false;
        if (!bytes) bytes = 16;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    // a private block of at least `bytes` (0: none): the one held stays when it is large enough, else a new one replaces it
    // (contents are not kept; on failure the owner is empty)
    hipError_t reserve(uint64_t bytes) { return cap >= bytes ? hipSuccess : alloc(bytes); }
    hipError_t alloc_pooled(uint64_t bytes) {
        release();
        pooled = true;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        return pool_alloc(&p, bytes ? bytes : 8, &cap, dev);
    }
    // the temporary of work on `stream`: only null-stream work may take (and hand back) a block of the pool
    hipError_t alloc_for(hipStream_t stream, uint64_t bytes) { return stream == nullptr ? alloc_pooled(bytes) : alloc(bytes); }
    template <typename T>
    T *as() const { return (T *)p; }
    uint64_t *u64() const { return (uint64_t *)p; }
};

// The arrays of a plan (or of a per-stream scratch) are DevBufs in one list that goes with it.  A new private block of `bytes`
// at the end of `blocks`; `ptr` = its address as the typed pointer the kernels read (a borrowed array has only the pointer).
template <typename T>
hipError_t alloc_block(std::vector<DevBuf> &blocks, T *&ptr, uint64_t bytes) {
    blocks.emplace_back();
    hipError_t e = blocks.back().alloc(bytes);
    ptr = (T *)blocks.back().p;
    return e;
}

// ---- SpMV plan ---------------------------------------------------------------
constexpr int XCS_SLICES = 8;      // one slice of x lines per XCD (each XCD has a private 4 MiB L2)

// One CSR piece the tile kernel runs over: arrays of the handle (borrowed) or blocks of the plan (SpmvPlan::blocks).
struct CsrPiece {
    void *indptr = nullptr;        // device; PTR of the handle for `main`, uint64 for slices
    void *indices = nullptr;       // device
    double *data = nullptr;        // device
    uint16_t *pos = nullptr;       // device, plan copies only: tile-local origin of each entry (tiles sorted by column)
    uint64_t rows = 0, nnz = 0, ntiles = 0;
    uint64_t *tile_row = nullptr;  // device, ntiles + 1: first row starting at/after tile c
};

struct SpmvScratch {               // per stream: nothing in here is shared between in-flight SpMVs
    double *carry_main = nullptr;
    double *carry_slices = nullptr;
    double *partial = nullptr;     // XCS_SLICES x n_long partial row sums
    double *xp = nullptr;          // x in the plan's column labelling (relabelled plans)
    std::vector<DevBuf> blocks;    // the blocks behind the arrays above
};

struct BandPlan;                   // spmv_band.hip
void band_free(BandPlan *bp);
struct BandDelete {
    void operator()(BandPlan *bp) const { band_free(bp); }
};
using OwnedBandPlan = std::unique_ptr<BandPlan, BandDelete>;   // (BandPlan is complete in spmv_band.hip only: band_free is its `delete`)

// Everything the plan owns goes with it: a plan is reset by assigning a fresh one.
struct SpmvPlan {
    bool built = false;
    bool light = false;            // built as the plain tile index although a copy plan would apply (first multiply of the handle): rebuilt at the next one
    bool xcs = false;
    OwnedBandPlan band;            // banded plan: when set, nothing else below is used
    uint64_t opt_sig = 0;          // hash of the option values the plan was built with (plan_signature, spmv.hip)
    uint32_t tile = 0;             // nnz per tile
    int idx_bytes = 8;             // width of the column ids the kernels read (handle's, or 4 for plan copies)
    CsrPiece main;                 // the whole matrix (plain plan) or its short rows (sliced plan)
    CsrPiece slice[XCS_SLICES];    // long rows, entries whose x line hashes to s, rows = n_long
    uint64_t slice_tile_off[XCS_SLICES + 1] = {0};
    uint64_t n_long = 0;
    uint64_t *long_rows = nullptr; // device: original row of long row j
    uint32_t *perm = nullptr;      // device, cols entries: plan label of column j (relabelled plans), else null
    DevBuf perm_block;             // the block behind perm (build_column_labels hands it over)
    uint64_t cols = 0;
    std::vector<DevBuf> blocks;    // the blocks behind every other array the plan made (tile rows, the copies of a sliced plan)
    std::unordered_map<void *, SpmvScratch> scratch;
};

int32_t exclusive_scan_u64(const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t stream);   // scan.hip

// ---- SpMM plan: rows cut into chunks of <= 512 entries (spmm.hip) -------------------------------
struct SpmmPlan {
    bool built = false;
    uint64_t nchunks = 0, n_multi = 0, long_row = 0;
    uint64_t *first_chunk = nullptr;   // device, rows + 1
    uint64_t *chunk_row = nullptr;     // device, nchunks
    uint64_t *multi_rows = nullptr;    // device, rows spanning several chunks
    uint64_t *tile_row = nullptr;      // device, ntiles + 1: the row that holds entry t * 256 (entry-stream kernel)
    uint64_t ntiles = 0;
    bool stream = false;               // built for the entry-stream kernel (no chunk lists then)
    std::vector<DevBuf> blocks;        // the blocks behind the arrays above
    std::unordered_map<void *, DevBuf> partial;   // per stream: the partial sums / carries of the kernels
    std::unordered_map<void *, DevBuf> relaid;    // per stream: the re-laid-out copy of the rhs (option spmm_relayout)
};

// ---- Gauss-Seidel plan: the rows in dependency-level order (gauss_seidel.hip) ---------------------
struct GsPlan {
    bool built = false;
    uint32_t *order = nullptr;         // device, rows entries: row swept at position q (levels ascending, rows ascending inside a level)
    DevBuf order_block;                // the block behind order
    uint64_t nlevels = 0;
    uint64_t no_diag_row = UINT64_MAX; // first row without a stored diagonal entry (the reference's diag.unwrap() panics there)
    uint64_t chain_tried = 0;          // stride the band schedule was last checked for (0: never) ...
    bool chain_ok = false;             // ... and whether every dependency fits it (gs_band_check_kernel)
    uint32_t *pos = nullptr;           // device, rows entries: pos[order[q]] = q, made by the first sparse-rhs solve (sptrisolve.hpp)
    DevBuf pos_block;                  // the block behind pos
};

// ---- sparse-rhs triangular solve: per-handle scratch (sptrisolve.hpp) ------------------------------
// Lives on the CSR form of the handle, beside the lower level plan.  `clean`: the bitmap is all zero, every granule of the work
// vector reads "absent" and b is +0.0 everywhere — what a solve finds and, by touching only its pattern, leaves behind.  Any
// error in between leaves clean = false and the next solve clears all of it.
struct SpTriScratch {
    uint32_t *bits = nullptr;          // device, ceil(n / 32): the visited bitmap of the reach
    uint32_t *queue = nullptr;         // device, n: the reach in discovery order, then the solve order
    unsigned long long *work = nullptr;   // device, n: the hand-off granules of tri_solve_kernel
    double *b = nullptr;               // device, n: the right-hand side scattered, the solution on return
    uint64_t *keys = nullptr;          // device, 4 n: (index, index) and (position in the level order, index), the two sorts
    uint64_t *words = nullptr;         // device: the state of the reach, the status words of the solve
    uint64_t *lens = nullptr;          // device, 2 n + 1: column lengths of a wide frontier and their scan (made by the first wide level)
    uint64_t n = 0;
    bool clean = false;
    std::vector<DevBuf> blocks;        // the blocks behind the arrays above
};

// ---- sparse-vector products: per-handle temporaries (csvec.hpp) ------------------------------------
struct CsvecScratch {
    uint32_t *bits = nullptr;          // device, ceil(n / 32): presence bitmap of v's indices
    double *vals = nullptr;            // device, n: v's values at their indices (read only where the bit is set; never cleared)
    double *sums = nullptr;            // device, outer: the dot of every kept outer slice
    uint64_t *groups = nullptr;        // device: keep masks (ngroups) | counts (ngroups) | offsets (ngroups + 1) | overflow flag
    uint64_t n = 0, nouter = 0;
    std::vector<DevBuf> blocks;        // the blocks behind the arrays above
};

}  // namespace sprs_hip

// Device twin of CsVecBase (sprs/src/sparse.rs:165-173): dim, sorted indices, data.
struct sprs_hip_csvec {
    uint64_t dim = 0, nnz = 0;
    int32_t idx_bytes = 8;             // width of the device indices (4 or 8)
    int32_t decl_idx_bytes = 0;        // width the caller declared when it differs (2: widened to 4 on upload, narrowed on download)
    int32_t user_idx_bytes() const { return decl_idx_bytes ? decl_idx_bytes : idx_bytes; }
    void *indices = nullptr;           // device, nnz entries, strictly increasing
    double *data = nullptr;            // device, nnz entries
    sprs_hip::PoolBlock own_data, own_indices;   // the blocks behind the arrays when the handle owns them (released indices first)
    int device = 0;
};

// Device twin of PermOwned (sprs/src/sparse/permutation.rs:12-28): the Identity variant (no arrays) or perm and perm_inv.
struct sprs_hip_perm {
    uint64_t dim = 0;
    int32_t idx_bytes = 8;             // width of the device arrays (4 or 8)
    int32_t decl_idx_bytes = 0;        // width the caller declared when it differs (2: widened to 4 on upload, narrowed on download)
    int32_t user_idx_bytes() const { return decl_idx_bytes ? decl_idx_bytes : idx_bytes; }
    bool identity = false;             // PermOwned::Identity: both arrays null
    void *perm = nullptr;              // device, dim entries
    void *perm_inv = nullptr;          // device, dim entries: perm_inv[perm[i]] = i
    sprs_hip::PoolBlock own_inv, own_perm;   // the blocks behind the arrays: every stored permutation owns them (released perm first)
    int device = 0;
};

// Device twin of Ordering (sprs/src/sparse/linalg/ordering.rs:7-12): the permutation and the component delimiters.
struct sprs_hip_ordering {
    uint64_t dim = 0;
    std::unique_ptr<sprs_hip_perm> perm;           // perm and perm_inv in the matrix's index widths
    std::vector<uint64_t> parts;                   // connected_parts
    uint64_t stats[4] = {0, 0, 0, 0};              // components, levels of the ordering pass, launches (a sort or a scan counts as one), host read-backs
};

// Device twin of CsMatBase (sprs/src/sparse.rs:94-122).
struct sprs_hip_csmat;
namespace sprs_hip {
// What LdlSymbolic holds (sprs-ldl/src/lib.rs:94-100) plus the structure of L that the reference only writes during the numeric
// pass: shared by the symbolic handle and by every numeric handle made from it (ldl.hpp).
struct LdlSym {
    uint64_t n = 0, lnz = 0;
    int device = 0;


    int32_t idx_bytes = 8, iptr_bytes = 8, decl_idx_bytes = 0;
    std::unique_ptr<sprs_hip_perm> perm;           // the Identity variant or perm and perm_inv, in the matrix's index width
    uint32_t *parents = nullptr;                   // n: elimination tree, 0xFFFFFFFF for a root
    uint64_t *colptr = nullptr;                    // n + 1: l_colptr
    uint32_t *l_indices = nullptr;                 // lnz: rows of L by column, ascending (the reference's l_indices)
    uint32_t *col_of_slot = nullptr;               // lnz: the column of every slot of the arrays above
    uint64_t *rowptr = nullptr;                    // n + 1: L by rows ...
    uint32_t *row_cols = nullptr;                  // lnz: ... columns ascending ...
    uint64_t *row_slot = nullptr;                  // lnz: ... and the column-form slot of every row entry
    uint64_t *walk_slot = nullptr;                 // lnz: per row, the column-form slots in the order the reference's pattern stack is walked
    uint32_t *walk_pos = nullptr;                  // lnz: the position inside its row (ascending columns) of every walk entry
    std::vector<DevBuf> blocks;                    // the blocks behind the arrays above
    std::mutex mu;                                 // guards the two level plans
    GsPlan lower, upper;                           // level orders of L by rows (lsolve) and of L^T (ltsolve): built at the first solve
    uint64_t stats[4] = {0, 0, 0, 0};              // launches of the etree pass, all launches (a sort or a scan counts as one), host read-backs, 0
};
}  // namespace sprs_hip
struct sprs_hip_ldl_sym {
    std::shared_ptr<sprs_hip::LdlSym> s;
};
struct sprs_hip_ldl_num {
    std::shared_ptr<sprs_hip::LdlSym> s;           // the numeric handle keeps the analysis alive
    sprs_hip::DevBuf l_data, d, row_vals;          // lnz values by column (l_data), n pivots, lnz values by row (for lsolve)
};

namespace sprs_hip {
// What the f64 and the f32 matrix handle share: the structure, the values as T, the owned blocks, the lock, the SpMM plan and the
// cached derived handles.  The public structs below derive from it (Self = the deriving struct) and add only their own plans.
// The owned blocks are members of this base, so they go after everything a deriving struct holds.
template <typename T, typename Self>
struct CsmatCore {
    using value_type = T;
    int32_t storage = SPRS_HIP_CSR;
    uint64_t rows = 0, cols = 0, nnz = 0;
    int32_t iptr_bytes = 8, idx_bytes = 8;       // widths of the device arrays (4 or 8)
    // widths the CALLER declared (2, 4 or 8): sprs' SpIndex covers u16 / i16 too (indexing.rs:124-130).  2-byte arrays are
    // widened to 4 bytes on upload and narrowed on download; every value a result could hold is checked against the
    // declared width where the reference's I::from_usize / Iptr::from_usize would panic.  0 = same as the device width
    // (always so for an f32 handle: its host arrays are 4 or 8 bytes wide).
    int32_t decl_iptr_bytes = 0, decl_idx_bytes = 0;
    int32_t user_iptr_bytes() const { return decl_iptr_bytes ? decl_iptr_bytes : iptr_bytes; }
    int32_t user_idx_bytes() const { return decl_idx_bytes ? decl_idx_bytes : idx_bytes; }
    void *indptr = nullptr;    // device, outer+1 entries, zero based
    void *indices = nullptr;   // device, nnz entries
    T *data = nullptr;         // device, nnz entries
    bool prepared = false;     // the prepare entry was called: the copy plans may be built at once (kept across refresh: the CSR copy of a CSC handle is prepared with it)
    PoolBlock own_data, own_indices, own_indptr;    // the blocks behind the arrays when the handle owns them (released indptr first)
    int device = 0;
    std::recursive_mutex mu;   // guards the plans and as_other / t_view: held from the look-up (or rebuild) of a plan until the kernels that read it are launched
    SpmmPlan mm;               // the SpMM plan (spmm.hip): value-agnostic
    Self *t_view = nullptr;    // transpose view (of the CSC form) kept for dense . sparse products (sprs_hip_dense_dot_csmat_*): its SpMM / SpMV plans live as long as the values do; dropped with as_other
    Self *as_other = nullptr;  // the handle in the OTHER storage order (to_other_storage, csmat.rs:1405-1426): made by the first product that needs it (a CSC operand of a dense product / SpMV runs on its CSR form), dropped by refresh / free

    uint64_t outer() const { return storage == SPRS_HIP_CSR ? rows : cols; }
    uint64_t inner() const { return storage == SPRS_HIP_CSR ? cols : rows; }
};
}  // namespace sprs_hip

struct sprs_hip_csmat : sprs_hip::CsmatCore<double, sprs_hip_csmat> {
    uint64_t spmv_calls = 0;   // multiplies so far: the re-laid-out plan copies (banded / XCD-sliced) are built at the SECOND one (or by sprs_hip_csmat_prepare)
    bool one_shot = false;     // the handle multiplies once (sprs_hip_spmv_f64_host): plain plan, no copies of the matrix
    sprs_hip::SpmvPlan plan;
    sprs_hip::GsPlan gs;                 // rows by the levels of the stored c < row: Gauss-Seidel and the lower triangular solves
    sprs_hip::GsPlan tri_upper;          // the mirror (stored c > row, levels rising from the last row): the upper triangular solves (trisolve.hpp)
    sprs_hip::CsvecScratch cv;           // temporaries of the sparse-vector products that run on this handle (csvec.hpp)
    sprs_hip::SpTriScratch sp;           // scratch of the sparse-rhs triangular solve (sptrisolve.hpp): on the CSR form, beside gs
    ~sprs_hip_csmat();         // handle.hpp: waits for the device when cached copies are held, drops them, then the blocks
};

// ---- single precision (spmv_f32.hpp) ----------------------------------------------------------------
namespace sprs_hip {
// The f32 SpMV runs on the banded plan (spmv_band.hip, floats throughout) or on the plain nnz-tile plan: the tile index over the
// handle's own arrays and one carry array per stream.
struct SpmvPlanF32 {
    bool built = false;
    bool light = false;                // built as the tile index although the banded plan would apply (first multiply of the handle): rebuilt at the next one
    OwnedBandPlan band;                // banded plan: when set, nothing below is used
    uint64_t opt_sig = 0;              // hash of the option values the plan was built with (f32_plan_signature, spmv_f32.hpp)
    uint32_t tile = 0;                 // nnz per tile: 2048 or 4096
    uint64_t ntiles = 0;
    uint64_t *tile_row = nullptr;      // device, ntiles + 1: first row starting at/after tile c
    std::vector<DevBuf> blocks;        // the block behind tile_row
    std::unordered_map<void *, DevBuf> carry;   // per stream: ntiles floats
};
}  // namespace sprs_hip

// Device twin of CsMatBase for N = f32.  A type of its own, not a flag of sprs_hip_csmat: no entry that reads `double *data`
// can be handed one (include/sprs_hip.h).  Index arrays are 4 or 8 bytes wide, on the host as on the device.
struct sprs_hip_csmat_f32 : sprs_hip::CsmatCore<float, sprs_hip_csmat_f32> {
    uint64_t spmv_calls = 0;   // multiplies so far, as in sprs_hip_csmat: the banded plan is built at the SECOND one (or by sprs_hip_csmat_f32_prepare)
    sprs_hip::SpmvPlanF32 plan;
    sprs_hip::GsPlan gs;                 // as in sprs_hip_csmat: the level plans read structure only, so they are the same type
    sprs_hip::GsPlan tri_upper;
    ~sprs_hip_csmat_f32();     // handle.hpp
};

namespace sprs_hip {

// Host copies run on the stream of the work around them and are complete when these return: a read-back sees every kernel
// enqueued on that stream before it.  (A blocking copy would run on the null stream, which a hipStreamNonBlocking stream, as
// every torch.cuda.Stream is, is not ordered with.)
inline hipError_t copy_to_host(void *dst, const void *src, uint64_t bytes, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}
inline hipError_t copy_to_device(void *dst, const void *src, uint64_t bytes, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}

// ---- index-width dispatch ------------------------------------------------------------------------------
// A handle's indices (I) and indptr (Iptr) are 4 or 8 bytes wide.  dispatch_widths calls f(TypeTag<IDX>{}, TypeTag<PTR>{})
// with the two types — a generic lambda names them as `typename decltype(i)::type` — and returns what f returns; every pair
// other than (8, 8), (4, 8), (8, 4) takes (4, 4).  dispatch_width is the same for one width.
template <typename T>
struct TypeTag {
    using type = T;
};
template <typename F>
auto dispatch_widths(int32_t idx_bytes, int32_t iptr_bytes, F &&f) {
    if (idx_bytes == 8 && iptr_bytes == 8) return f(TypeTag<uint64_t>{}, TypeTag<uint64_t>{});
    if (idx_bytes == 4 && iptr_bytes == 8) return f(TypeTag<uint32_t>{}, TypeTag<uint64_t>{});
    if (idx_bytes == 8 && iptr_bytes == 4) return f(TypeTag<uint64_t>{}, TypeTag<uint32_t>{});
    return f(TypeTag<uint32_t>{}, TypeTag<uint32_t>{});
}
template <typename F>
auto dispatch_width(int32_t bytes, F &&f) {
    return bytes == 8 ? f(TypeTag<uint64_t>{}) : f(TypeTag<uint32_t>{});
}

// the same for a HOST index array, which may also be 2 bytes wide (u16 / i16, indexing.rs:124-130)
template <typename F>
auto dispatch_host_width(int32_t bytes, F &&f) {
    return bytes == 2 ? f(TypeTag<uint16_t>{}) : dispatch_width(bytes, f);
}

// A handle and its owner: results travel as these below the ABI and are released to a raw pointer only in the extern "C"
// function; a temporary (a converted operand, a slice) goes with the scope that made it.  `delete` is the whole release and
// leaves the thread's error state alone.
template <typename H>
using Owned = std::unique_ptr<H>;
using OwnedCsmat = Owned<sprs_hip_csmat>;
using OwnedCsvec = Owned<sprs_hip_csvec>;
using OwnedPerm = Owned<sprs_hip_perm>;
using OwnedCsmatF32 = Owned<sprs_hip_csmat_f32>;

// spmv_band.hip
int32_t band_build(sprs_hip_csmat *a, hipStream_t stream, OwnedBandPlan &out);   // out stays empty when the plan does not apply
int32_t band_spmv(sprs_hip_csmat *a, BandPlan *bp, const double *x, double *y, bool accumulate, hipStream_t stream);
int32_t band_build(sprs_hip_csmat_f32 *a, hipStream_t stream, OwnedBandPlan &out);   // the same plan with float values, x, partial sums and carries
int32_t band_spmv(sprs_hip_csmat_f32 *a, BandPlan *bp, const float *x, float *y, bool accumulate, hipStream_t stream);
int32_t band_prepare_stream(sprs_hip_csmat_f32 *a, BandPlan *bp, hipStream_t stream);   // makes `stream`'s scratch now (a capturing stream cannot)
uint64_t band_plan_bytes(const BandPlan *bp);
// spmv.hip
int32_t spmv_prepare(sprs_hip_csmat *a, hipStream_t stream);   // builds the full SpMV plan now (sprs_hip_csmat_prepare)
int32_t spmv_f64(sprs_hip_csmat *a, const double *x, double *y, bool accumulate, hipStream_t stream);
// spgemm.hip
int32_t spgemm_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &c);
int32_t spgemm_symbolic(const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &c);
int32_t spgemm_numeric(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat *c);
int32_t spgemm_plan_create(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_spgemm_plan **out);
int32_t spgemm_plan_structure(sprs_hip_spgemm_plan *pl, const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &out, bool with_values);
int32_t spgemm_plan_numeric(sprs_hip_spgemm_plan *pl, const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat *c);
// A plan holds structure only (task lists, counts, offsets, the bucket table of B): one made from f64 operands serves f32
// handles over the same indptr / indices arrays and the reverse; the {column, value} records of B are packed per call.
uint64_t spgemm_plan_nnz(const sprs_hip_spgemm_plan *pl);
void spgemm_plan_free(sprs_hip_spgemm_plan *pl);
// spmm.hip
int32_t spmm_strided_f64(sprs_hip_csmat *a, const double *rhs, uint64_t k, uint64_t rs_rhs, uint64_t cs_rhs, double *out,
                         uint64_t rs_out, uint64_t cs_out, bool accumulate, hipStream_t stream);
int32_t spmm_strided_f32(sprs_hip_csmat_f32 *a, const float *rhs, uint64_t k, uint64_t rs_rhs, uint64_t cs_rhs, float *out,
                         uint64_t rs_out, uint64_t cs_out, bool accumulate, hipStream_t stream);   // kernels: spmm_f32.hpp
// dist.hip
int32_t dist_unique_id(void *id128);
int32_t dist_create(sprs_hip_dist **out, const void *unique_id128, int32_t world, int32_t rank, uint64_t rows, uint64_t cols,
                    const uint64_t *row_starts, const sprs_hip_csmat *local_block, int32_t nsub);
int32_t dist_spmv(sprs_hip_dist *d, const double *x, double *y, hipStream_t stream);
void dist_free(sprs_hip_dist *d);
uint64_t dist_rows(const sprs_hip_dist *d);
uint64_t dist_cols(const sprs_hip_dist *d);
int32_t dist_comm_count(const sprs_hip_dist *d, int32_t *ranks);
int32_t dist_peer_handle(sprs_hip_dist *d, void *handle64);                       // the peer-store route (dist.hip)
int32_t dist_peer_connect(sprs_hip_dist *d, const void *handles, int32_t world);
int32_t dist_set_route(sprs_hip_dist *d, int32_t route);
int32_t dist_route(const sprs_hip_dist *d, int32_t *route);
// triplet.hip
int32_t triplets_to_cs(uint64_t rows, uint64_t cols, uint64_t n, const void *row_inds, const void *col_inds, int32_t in_idx_bytes,
                       const double *data, int32_t storage, int32_t out_idx_bytes, int32_t out_iptr_bytes, OwnedCsmat &out);
// convert.hip
int32_t to_other_storage(const sprs_hip_csmat *m, OwnedCsmat &out);
// binop.hpp (compiled in convert.hip): operands of equal shape, storage and index widths; complete on `stream` at return
int32_t csmat_binop_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, int32_t op, OwnedCsmat &out, hipStream_t stream);
int32_t csvec_binop_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, int32_t op, uint64_t dim, OwnedCsvec &out, hipStream_t stream);
int32_t csmat_scale_f64(const sprs_hip_csmat *m, double alpha, OwnedCsmat &out, hipStream_t stream);
// perm.hpp (compiled in convert.hip): o / g = device arrays of m's index type (outer / inner entries) or null for the identity
int32_t csmat_permute(const sprs_hip_csmat *m, const void *o, const void *g, OwnedCsmat &out, hipStream_t stream);
int32_t perm_build_inverse(sprs_hip_perm *p, bool validate, hipStream_t stream);
int32_t perm_is_identity(const sprs_hip_perm *p, int32_t *flag, hipStream_t stream);
int32_t perm_mul_vec_f64(const sprs_hip_perm *p, const double *x, double *y, hipStream_t stream);
// structure.hpp (compiled in convert.hip): check_compressed_structure and new_from_unsorted on handles; `info` may be null;
// the answer (and the result) is complete on `stream` at return
int32_t csmat_check_structure(const sprs_hip_csmat *m, sprs_hip_structure_info *info, hipStream_t stream);
int32_t csmat_from_unsorted(const sprs_hip_csmat *m, OwnedCsmat &out, sprs_hip_structure_info *info, hipStream_t stream);
int32_t csvec_from_unsorted(const sprs_hip_csvec *v, OwnedCsvec &out, sprs_hip_structure_info *info, hipStream_t stream);
// ordering.hpp (compiled in convert.hip): everything walks the outer dimension; host results are complete on `stream` at return
int32_t csmat_is_symmetric(const sprs_hip_csmat *m, int32_t *flag, hipStream_t stream);
int32_t csmat_degrees(const sprs_hip_csmat *m, uint64_t *out_dev, hipStream_t stream);   // ordered on `stream`
int32_t csmat_max_outer_nnz(const sprs_hip_csmat *m, uint64_t *out, hipStream_t stream);
int32_t csmat_cuthill_mckee(const sprs_hip_csmat *m, int32_t strategy, bool reversed, sprs_hip_ordering *o, hipStream_t stream);
// construct.hpp (compiled in convert.hip): operands of equal storage and index widths; complete on `stream` at return
int32_t csmat_kronecker_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &out, hipStream_t stream);
// the block assembly behind the four stacking functions: the present blocks by super-row, each with the shift of its inner indices
struct StackItem {
    const sprs_hip_csmat *m;
    uint64_t srow, inner_off;
};
int32_t csmat_stack(const std::vector<StackItem> &items, const std::vector<uint64_t> &outer_of, int32_t storage, uint64_t rows, uint64_t cols,
                    int32_t iptr_bytes, int32_t idx_bytes, OwnedCsmat &out, hipStream_t stream);
// dense.hpp (compiled in convert.hip): a dense operand is `lines` lines of `width` f64, ld apart, in the order that matches the
// sparse storage.  from_dense is complete on `stream` at return; the other two are ordered on it
int32_t csmat_from_dense_f64(const double *m, int32_t storage, uint64_t lines, uint64_t width, uint64_t ld, double eps, uint64_t c_max,
                             uint64_t r_max, uint64_t nnz_max, int32_t iptr_bytes, int32_t idx_bytes, OwnedCsmat &out, hipStream_t stream);
int32_t csmat_assign_dense_f64(const sprs_hip_csmat *m, bool zero_first, double *out, int32_t layout, uint64_t ld, hipStream_t stream);
int32_t csmat_binop_dense_f64(const sprs_hip_csmat *lhs, const double *rhs, int32_t layout, uint64_t ld, int32_t op, double alpha, double beta,
                              double *out, uint64_t out_ld, hipStream_t stream);
// bicgstab.hip
int32_t bicgstab_f64(sprs_hip_csmat *a, const double *x0, const double *b, uint64_t n, double tol, uint64_t max_iter,
                     double soft_restart_threshold, double *x, sprs_hip_bicgstab_info *info, hipStream_t stream);
int32_t bicgstab_f32(sprs_hip_csmat_f32 *a, const float *x0, const float *b, uint64_t n, float tol, uint64_t max_iter,
                     float soft_restart_threshold, float *x, sprs_hip_bicgstab_info *info, hipStream_t stream);
// gauss_seidel.hip
int32_t gauss_seidel_f64(sprs_hip_csmat *a, double *x, const double *rhs, uint64_t n, uint64_t max_iter, double eps,
                         sprs_hip_gauss_seidel_info *info, hipStream_t stream);
// (eps is rounded to f32 first; info->error is the f32 value widened; no band schedule)
int32_t gauss_seidel_f32(sprs_hip_csmat_f32 *a, float *x, const float *rhs, uint64_t n, uint64_t max_iter, double eps,
                         sprs_hip_gauss_seidel_info *info, hipStream_t stream);
// trisolve.hpp (compiled in gauss_seidel.hip): csr = the CSR form of the caller's handle, csc = that handle is CSC
int32_t trisolve_f64(sprs_hip_csmat *csr, bool upper, bool csc, double *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream);
int32_t trisolve_f32(sprs_hip_csmat_f32 *csr, bool upper, bool csc, float *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream);
// sptrisolve.hpp (compiled in gauss_seidel.hip): lsolve_csc_sparse_rhs; l = the caller's CSC handle (its columns are the graph
// of the reach), csr = its CSR form (plan, scratch, the rows the solve walks).  Complete on `stream` at return
int32_t sptrisolve_f64(sprs_hip_csmat *l, sprs_hip_csmat *csr, const sprs_hip_csvec *rhs, OwnedCsvec &out, sprs_hip_sptrisolve_info *info,
                       hipStream_t stream);
// ldl.hpp (compiled in gauss_seidel.hip): twins of sprs-ldl/src/lib.rs; p = null for the identity.  Complete on `stream` at return
int32_t ldl_symbolic(const sprs_hip_csmat *m, const sprs_hip_perm *p, LdlSym &s, hipStream_t stream);
int32_t ldl_factor_f64(LdlSym &s, const sprs_hip_csmat *m, sprs_hip_ldl_num *num, sprs_hip_trisolve_info *info, hipStream_t stream);
int32_t ldl_export_l(const sprs_hip_ldl_num *num, OwnedCsmat &out, hipStream_t stream);
int32_t ldl_solve_f64(sprs_hip_ldl_num *num, const double *b, double *x, hipStream_t stream);
// ldl_lsolve (transposed = false) / ldl_ltsolve (true) on the arrays of a CSC handle (csr = its CSR form, for lsolve)
int32_t ldl_tri_f64(sprs_hip_csmat *l, sprs_hip_csmat *csr, bool transposed, double *x, hipStream_t stream);
int32_t diag_solve_f64(const double *d, double *x, uint64_t n, hipStream_t stream);
int32_t diag_solve_f32(const float *d, float *x, uint64_t n, hipStream_t stream);
int32_t slice_outer(const sprs_hip_csmat *m, uint64_t start, uint64_t end, OwnedCsmat &out);
// csvec.hpp (compiled in spmv.hip)
// the invariants of CsVec::try_new on the device; `info` (may be null): the kind of the finding (a vector is its one slice, 0)
int32_t csvec_check_device(const sprs_hip_csvec *v, hipStream_t stream, sprs_hip_structure_info *info = nullptr);
int32_t csvec_scatter(const sprs_hip_csvec *v, double *out, hipStream_t stream);
int32_t csvec_masked_dot(const sprs_hip_csmat *m, const sprs_hip_csvec *v, bool drop_zero, int32_t idx_bytes, int32_t decl_bytes,
                         OwnedCsvec &out, hipStream_t stream);
// csvec_reduce.hpp (compiled in spmv.hip): every scalar is the reference's left-to-right chain from +0.0 and is complete on
// `stream` at return; csvec_sum_f64: term 0 = x * x, 1 = |x|, 2 = pow(|x|, p); csvec_extrema_f64: out[0..2] = max |x| from -inf,
// min |x| from +inf, the count of !(|x| == 0); csvec_lookup is ordered on `stream`
int32_t csvec_dot_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, double *out, hipStream_t stream);
int32_t csvec_dot_dense_f64(const sprs_hip_csvec *v, const double *x, uint64_t x_len, double *out, hipStream_t stream);
int32_t csvec_sum_f64(const sprs_hip_csvec *v, int32_t term, double p, double *out, hipStream_t stream);
int32_t csvec_extrema_f64(const sprs_hip_csvec *v, double *out, hipStream_t stream);
int32_t csvec_divided_f64(const sprs_hip_csvec *v, double norm, OwnedCsvec &out, hipStream_t stream);
int32_t csvec_lookup(const sprs_hip_csvec *v, uint64_t nq, const uint64_t *qs, uint64_t *pos, double *val, hipStream_t stream);
// extract.hpp (compiled in convert.hip): outer_view (i < outer, a borrowing vector), diag, the batched nnz_index / get (ordered on
// `stream`) and to_inner_onehot; results are complete on `stream` at return
int32_t csmat_outer_view(const sprs_hip_csmat *m, uint64_t i, sprs_hip_csvec **out, hipStream_t stream);
int32_t csmat_diag_f64(const sprs_hip_csmat *m, OwnedCsvec &out, hipStream_t stream);
int32_t csmat_lookup(const sprs_hip_csmat *m, uint64_t nq, const uint64_t *rows, const uint64_t *cols, uint64_t *pos, double *val,
                     hipStream_t stream);
int32_t csmat_onehot_f64(const sprs_hip_csmat *m, OwnedCsmat &out, hipStream_t stream);
// handle.hpp: the one place that makes handles
// an owned matrix / vector / permutation with uninitialised arrays of the given sizes on the current device
int32_t make_csmat(OwnedCsmat &out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes);
int32_t make_csvec(OwnedCsvec &out, uint64_t dim, uint64_t nnz, int32_t idx_bytes, int32_t decl_idx_bytes);
int32_t make_perm(OwnedPerm &out, uint64_t dim, int32_t idx_bytes, int32_t decl_idx_bytes);
// non-owning handles over arrays of the caller's: a matrix (`into` = a stack object to fill, or null for a new heap handle), a
// vector, the Identity permutation (2-byte declared width: 4 on the device)
sprs_hip_csmat *view_csmat(int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *indptr, int32_t iptr_bytes,
                           const void *indices, int32_t idx_bytes, const double *data, int device, sprs_hip_csmat *into = nullptr);
sprs_hip_csvec *view_csvec(uint64_t dim, uint64_t nnz, const void *indices, int32_t idx_bytes, const double *data, int device);
sprs_hip_perm *identity_perm(uint64_t dim, int32_t idx_bytes);
sprs_hip_ordering *make_ordering();                 // empty: csmat_cuthill_mckee fills it
sprs_hip_ldl_sym *make_ldl_symbolic();         // with a fresh, empty LdlSym: ldl_symbolic fills it
sprs_hip_ldl_num *make_ldl_numeric(const sprs_hip_ldl_sym *sym);   // shares sym's analysis; arrays empty
// a view of m's arrays with m's declared widths and device; transpose: transpose_view (csmat.rs:982-991) — free, flips the tag
sprs_hip_csmat *view_csmat(const sprs_hip_csmat *m, bool transpose, sprs_hip_csmat *into = nullptr);
// an owned matrix of m's storage, shape and widths whose indptr, indices and (with_data) values are copies of m's, enqueued
// device to device on `stream` (not waited for)
int32_t copy_csmat(const sprs_hip_csmat *m, bool with_data, OwnedCsmat &out, hipStream_t stream);
// everything a handle derives from its arrays (plans, row orders, the copy in the other storage order, the transpose view)
void invalidate_caches(sprs_hip_csmat *m);
// single precision (handle.hpp): the same constructors for the f32 handle, and an owned f32 matrix that takes over the indptr
// and indices blocks of an owned f64 one (which is left without them) beside a fresh block of nnz floats
int32_t make_csmat(OwnedCsmatF32 &out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes);
sprs_hip_csmat_f32 *view_csmat(int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *indptr, int32_t iptr_bytes,
                               const void *indices, int32_t idx_bytes, const float *data, int device, sprs_hip_csmat_f32 *into = nullptr);
sprs_hip_csmat_f32 *view_csmat(const sprs_hip_csmat_f32 *m, bool transpose, sprs_hip_csmat_f32 *into = nullptr);
int32_t adopt_structure_f32(sprs_hip_csmat *from, OwnedCsmatF32 &out);
void invalidate_caches(sprs_hip_csmat_f32 *m);
// spmv_f32.hpp (compiled in spmv.hip)
int32_t spmv_f32_prepare(sprs_hip_csmat_f32 *a, hipStream_t stream);   // the tile index and `stream`'s carry array, now
int32_t spmv_f32(sprs_hip_csmat_f32 *a, const float *x, float *y, bool accumulate, hipStream_t stream);
int32_t csmat_f32_to_other_storage(const sprs_hip_csmat_f32 *m, OwnedCsmatF32 &out);             // complete at return
int32_t csmat_f32_from_f64(const sprs_hip_csmat *m, OwnedCsmatF32 &out, hipStream_t stream);     // ordered on `stream`
int32_t csmat_f32_to_f64(const sprs_hip_csmat_f32 *m, OwnedCsmat &out, hipStream_t stream);      // ordered on `stream`
// one name per operation for code that is generic over the handle type (abi.hip, bicgstab.hip)
inline int32_t spmv(sprs_hip_csmat *a, const double *x, double *y, bool accumulate, hipStream_t stream) { return spmv_f64(a, x, y, accumulate, stream); }
inline int32_t spmv(sprs_hip_csmat_f32 *a, const float *x, float *y, bool accumulate, hipStream_t stream) { return spmv_f32(a, x, y, accumulate, stream); }
inline int32_t spmv_prepare(sprs_hip_csmat_f32 *a, hipStream_t stream) { return spmv_f32_prepare(a, stream); }
inline int32_t to_other_storage(const sprs_hip_csmat_f32 *m, OwnedCsmatF32 &out) { return csmat_f32_to_other_storage(m, out); }
// spgemm.hip: the f32 products (rounded to f32 after every multiply and every add, in the reference's order)
int32_t spgemm_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, OwnedCsmatF32 &c);
int32_t spgemm_symbolic(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, OwnedCsmatF32 &c);
int32_t spgemm_numeric(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 *c);
int32_t spgemm_plan_create(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_spgemm_plan **out);
int32_t spgemm_plan_structure(sprs_hip_spgemm_plan *pl, const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, OwnedCsmatF32 &out, bool with_values);
int32_t spgemm_plan_numeric(sprs_hip_spgemm_plan *pl, const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 *c);
int64_t spgemm_f32_lds_add_verdict();      // bit 0: lane order holds for the f32 LDS add, bit 1: it keeps subnormals (probed once per device)
inline int32_t spgemm_product(const sprs_hip_csmat *a, const sprs_hip_csmat *b, OwnedCsmat &c) { return spgemm_f64(a, b, c); }
inline int32_t spgemm_product(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, OwnedCsmatF32 &c) { return spgemm_f32(a, b, c); }
inline int32_t spmm_strided(sprs_hip_csmat *a, const double *rhs, uint64_t k, uint64_t rs_rhs, uint64_t cs_rhs, double *out, uint64_t rs_out,
                            uint64_t cs_out, bool accumulate, hipStream_t stream) {
    return spmm_strided_f64(a, rhs, k, rs_rhs, cs_rhs, out, rs_out, cs_out, accumulate, stream);
}
inline int32_t spmm_strided(sprs_hip_csmat_f32 *a, const float *rhs, uint64_t k, uint64_t rs_rhs, uint64_t cs_rhs, float *out, uint64_t rs_out,
                            uint64_t cs_out, bool accumulate, hipStream_t stream) {
    return spmm_strided_f32(a, rhs, k, rs_rhs, cs_rhs, out, rs_out, cs_out, accumulate, stream);
}
inline int32_t gauss_seidel(sprs_hip_csmat *a, double *x, const double *rhs, uint64_t n, uint64_t max_iter, double eps, sprs_hip_gauss_seidel_info *info,
                            hipStream_t stream) {
    return gauss_seidel_f64(a, x, rhs, n, max_iter, eps, info, stream);
}
inline int32_t gauss_seidel(sprs_hip_csmat_f32 *a, float *x, const float *rhs, uint64_t n, uint64_t max_iter, double eps, sprs_hip_gauss_seidel_info *info,
                            hipStream_t stream) {
    return gauss_seidel_f32(a, x, rhs, n, max_iter, eps, info, stream);
}
inline int32_t trisolve(sprs_hip_csmat *csr, bool upper, bool csc, double *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return trisolve_f64(csr, upper, csc, x, n, info, stream);
}
inline int32_t trisolve(sprs_hip_csmat_f32 *csr, bool upper, bool csc, float *x, uint64_t n, sprs_hip_trisolve_info *info, hipStream_t stream) {
    return trisolve_f32(csr, upper, csc, x, n, info, stream);
}
inline int32_t diag_solve(const double *d, double *x, uint64_t n, hipStream_t stream) { return diag_solve_f64(d, x, n, stream); }
inline int32_t diag_solve(const float *d, float *x, uint64_t n, hipStream_t stream) { return diag_solve_f32(d, x, n, stream); }
inline int32_t bicgstab(sprs_hip_csmat *a, const double *x0, const double *b, uint64_t n, double tol, uint64_t max_iter, double threshold, double *x,
                        sprs_hip_bicgstab_info *info, hipStream_t stream) {
    return bicgstab_f64(a, x0, b, n, tol, max_iter, threshold, x, info, stream);
}
inline int32_t bicgstab(sprs_hip_csmat_f32 *a, const float *x0, const float *b, uint64_t n, float tol, uint64_t max_iter, float threshold, float *x,
                        sprs_hip_bicgstab_info *info, hipStream_t stream) {
    return bicgstab_f32(a, x0, b, n, tol, max_iter, threshold, x, info, stream);
}
// abi.hip
// a result inherits the declared index widths of its operand; INDEX_OVERFLOW where a value would not fit them
int32_t inherit_declared_widths(sprs_hip_csmat *result, const sprs_hip_csmat *from);

}  // namespace sprs_hip
