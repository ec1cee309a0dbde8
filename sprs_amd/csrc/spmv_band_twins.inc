// The kernels of the banded SpMV that exist once per scalar UNDER NAMES OF THEIR OWN — included twice by spmv_band_kernels.hpp,
// with BAND_T = double, BAND_KERNEL(name) = name and with BAND_T = float, BAND_KERNEL(name) = name_f32.  Everything else of the
// plan that touches a value is a template on the scalar (spmv_band_kernels.hpp); these two are text, not templates, because the
// f64 kernels must keep their names (tests/test_isa_cpu.py picks the f64 hot kernel by name and must not meet an f32 one) and
// their instructions (scripts/device_code_diff.py: a __device__ body inlined into two wrappers compiles to other instructions).
// No include guard on purpose.

// ---------------------------------------------------------------------------------------------
// hot slices: x tile in LDS, 16-bit local column ids (the description: spmv_band_kernels.hpp)
// ---------------------------------------------------------------------------------------------
template <int XT_LOG2, int PACK>
__global__ __launch_bounds__(HOT_THREADS) SPRS_HOT_WAVES_ATTR void BAND_KERNEL(band_hot_kernel)(const HotSeg *__restrict__ hsegs,
                                                               const HotSeg *__restrict__ wg_first, const BAND_T *__restrict__ vals,
                                                               const uint16_t *__restrict__ cid, const BAND_T *__restrict__ xp,
                                                               BAND_T *__restrict__ partial, BAND_T *__restrict__ carry, uint32_t dbg,
                                                               unsigned long long *__restrict__ prof, uint32_t xcd_shares) {
    typedef BAND_T T;
    typedef typename BandT<T>::vec vecT;
    constexpr int VW = BandT<T>::VW, NV = BandT<T>::NV;
    constexpr int XT = 1 << XT_LOG2;
    constexpr bool PACKED = PACK != 0;
    static_assert(!PACKED || sizeof(T) == 8, "packed slices hold doubles");
    static_assert(XT_LOG2 <= 14 || sizeof(T) == 4, "a slice of doubles is at most 16384 labels");
    // developer builds, option spmv_band_debug & 16 (env SPRS_HIP_HOTPROF): when does each workgroup start, see its first x tile,
    // and end (100 MHz wall clock) — is the hot kernel's time its work or its tail?
    if constexpr (DEVTOOLS) {
        if (prof && threadIdx.x == 0) prof[3 * blockIdx.x] = (unsigned long long)wall_clock64();
    }
    // dynamic LDS (hot_lds_bytes): with the size known at compile time the compiler sees that only 4 waves per SIMD fit and
    // spends up to 128 registers; it is asked for 5 (96 registers) so that two gather waves fit beside each hot wave
#ifdef SPRS_HIP_EMU
    static T BAND_KERNEL(lds)[XT + HOT_WAVES * STG];
#else
    extern __shared__ __attribute__((aligned(16))) T BAND_KERNEL(lds)[];
#endif
    T *xs = BAND_KERNEL(lds);                                            // XT values: the x tile
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    T *stage = BAND_KERNEL(lds) + XT + wave * STG;                  // the wave's window for outgoing sums
    // share of this workgroup.  xcd_shares: block b runs on XCD b % 8 (observed dispatch order; only speed depends on it) and every
    // XCD takes a CONTIGUOUS run of shares — the workgroups that stream one slice then sit behind one L2, which serves its x tile
    // to all but the first of them (dealt round-robin, every XCD's L2 fetched every slice: 256 workgroups x 128 KiB = 32 MB through
    // the fabric in the first microseconds of a small plan's hot kernel).
    uint32_t share = blockIdx.x;
    if (xcd_shares) {
        const uint32_t nq = gridDim.x >> 3, rem = gridDim.x & 7u, k = blockIdx.x & 7u;
        share = k * nq + (k < rem ? k : rem) + (blockIdx.x >> 3);
    }
    // the share's FIRST segment comes with its segment range in one record (wg_first[share]: pad0 / pad1 = first segment, end) —
    // one round trip in front of the first x tile instead of two (wg_seg -> hsegs)
    HotSeg nxt = wg_first[share];
    const uint32_t s0 = nxt.pad0, s1 = nxt.pad1;
    for (uint32_t s = s0; s < s1; ++s) {
        const HotSeg seg = nxt;
        if (s + 1 < s1) nxt = hsegs[s + 1];                              // (requested a whole segment before it is needed)
        struct {
            const SPRS_GLOBAL_AS uint64_t *tile_word;                    // TileWord as one 8-byte word: row | keys << 32
            SPRS_GLOBAL_AS T *out;
            uint64_t ent0, nnz;
            uint32_t x0;
        } d{(const SPRS_GLOBAL_AS uint64_t *)seg.tile_word, (SPRS_GLOBAL_AS T *)(partial + seg.out_off), seg.ent0, seg.nnz, seg.x0};
        if (s != s0) __syncthreads();                                    // every wave is done with the previous x tile
        {   // x tile of the slice -> LDS (xp is padded to a whole number of tiles)
            const vecT *src = (const vecT *)(xp + d.x0);
            vecT v[XT / (VW * HOT_THREADS)];
#pragma unroll
            for (int q = 0; q < XT / (VW * HOT_THREADS); ++q) v[q] = src[q * HOT_THREADS + tid];
#pragma unroll
            for (int q = 0; q < XT / (VW * HOT_THREADS); ++q) *(vecT *)&xs[VW * (q * HOT_THREADS + tid)] = v[q];
        }
        // the wave's tiles, in the order it walks them: ranges r = wave, wave + 16, ...; inside a range tile after tile
        const uint32_t run = seg.run, n = seg.ntiles;
        vecT av[NV];
        u32x4 cw = {0u, 0u, 0u, 0u};
        u32x4 plo[2], pmh;                                               // PACKED: low words, mantissa-high fields (dwords 0 .. 3, 4)
        uint32_t pmh4 = 0;
        uint32_t R0n = 0, Kn = 0;
        auto request = [&](uint32_t w) {
            if constexpr (PACKED) {
                const unsigned char *rec = (const unsigned char *)vals + (d.ent0 / WT + w) * (uint64_t)PK_TILE_BYTES;
#pragma unroll
                for (int p = 0; p < 2; ++p) plo[p] = __builtin_nontemporal_load((const u32x4 *)(rec + p * (WAVE * 16) + lane * 16));
                pmh = __builtin_nontemporal_load((const u32x4 *)(rec + PK_MH + lane * 16));
                pmh4 = __builtin_nontemporal_load((const uint32_t *)(rec + PK_MH4 + lane * 4));
                cw = __builtin_nontemporal_load((const u32x4 *)(rec + PK_ID + lane * 16));
                const uint64_t tw = d.tile_word[w];
                R0n = (uint32_t)tw;
                Kn = (uint32_t)(tw >> 32);
            } else {
                const uint64_t g = d.ent0 + (uint64_t)w * WT;
#pragma unroll
                for (int p = 0; p < NV; ++p) av[p] = __builtin_nontemporal_load((const vecT *)(vals + g + p * (WAVE * VW) + lane * VW));
                cw = __builtin_nontemporal_load((const u32x4 *)(cid + g + lane * EPL));
                R0n = (uint32_t)d.tile_word[w];
            }
        };
        // Which wave walks which range is free (a range's sums do not depend on it).  Raw slices: r = wave, wave + 16, ...
        // Packed slices of a big plan: G = 2 consecutive ranges per wave and turn, i.e. 8 records = 34 KiB in a row — with
        // 4 (17 KiB) the packed kernel ran at 750 us in one SpMV and 925 us in the next beside the gather kernels, 901 us on
        // average against 823 us raw, although ALONE it takes 569 against 641 us; with 8 in a row 804 us (profiles/r29a).
        constexpr uint32_t G = PACKED ? (uint32_t)PACK : 1u;
        uint32_t r = wave * G;                                           // current range
        uint32_t t = r * run;                                            // current tile, relative to the segment
        if (t < n) request(seg.tile0 + t);                               // the first tile is requested before the barrier
        __syncthreads();                                                 // xs complete
        if constexpr (DEVTOOLS) {
            if (prof && threadIdx.x == 0 && s == s0) prof[3 * blockIdx.x + 1] = (unsigned long long)wall_clock64();
        }
        T open = 0.0;
        bool mine = false;
        uint32_t last = 0;
        Pending pd;
        SPRS_GLOBAL_AS T *pd_slot = (SPRS_GLOBAL_AS T *)carry;
        while (t < n) {                                                  // wave-uniform
            const uint32_t w = seg.tile0 + t;
            const uint64_t base = (uint64_t)w * WT;
            const uint32_t cnt = d.nnz - base < (uint64_t)WT ? (uint32_t)(d.nnz - base) : (uint32_t)WT;
            T pr[EPL], xv[EPL];
            uint32_t fb = 0;
            // all eight LDS gathers are issued before the first product needs one (a conditional read per entry compiles to
            // eight branches with a full LDS wait each)
#pragma unroll
            for (int p = 0; p < WPASS; ++p) {
                const uint32_t c2 = cw[p];
                xv[2 * p] = xs[c2 & (XT - 1)];
                xv[2 * p + 1] = xs[(c2 >> 16) & (XT - 1)];
                fb |= ((c2 >> 15) & 1u) << (2 * p);
                fb |= ((c2 >> 31) & 1u) << (2 * p + 1);
            }
            if constexpr (PACKED) {
                // the value of entry q: low word as stored; high word = the key that id bit 14 selects, over the 20-bit field
                const uint32_t m[5] = {pmh[0], pmh[1], pmh[2], pmh[3], pmh4};
                const uint32_t ks = (uint32_t)__builtin_amdgcn_readfirstlane((int)Kn);   // wave-uniform: the tile's word
                const uint32_t k0 = ks << 20, k1 = (ks >> 12) << 20;
#pragma unroll
                for (int q = 0; q < EPL; ++q) {
                    const uint32_t sel = cw[q / 2] & (KEY_SEL << (16 * (q & 1)));
                    const uint32_t hi = pk_field(m, q) | (sel ? k1 : k0);
                    pr[q] = __hiloint2double((int)hi, (int)plo[q / 4][q % 4]) * xv[q];
                }
            } else if constexpr (VW == 2) {
#pragma unroll
                for (int p = 0; p < WPASS; ++p) {
                    pr[2 * p] = av[p][0] * xv[2 * p];
                    pr[2 * p + 1] = av[p][1] * xv[2 * p + 1];
                }
            } else {
#pragma unroll
                for (int q = 0; q < EPL; ++q) pr[q] = av[q / VW][q % VW] * xv[q];
            }
            if (cnt < (uint32_t)WT) {                                    // last tile of a slice (wave-uniform): the padding (value 0, id 0) must not
#pragma unroll                                                           // turn an infinite x[first label] into a NaN
                for (int q = 0; q < EPL; ++q) pr[q] = lane * EPL + q < cnt ? pr[q] : (T)0.0;
            }
            // tile_row[w] is the LAST load of the tile's request: taken here, in front of the flush, so that its wait covers only
            // loads issued a whole tile ago.  (Until round 5 the compiler sank this copy behind the flush's stores, and on gfx950
            // loads and stores count on ONE in-order vmcnt: the wave then waited for the acknowledgement of its stores with no
            // load in flight, once per tile — `s_waitcnt vmcnt(0)` between the flush and the next request in the ISA; the probe
            // scripts/probes/stream_store.hip prices such a drain at 1.0 - 2.3 us per tile.)
            uint32_t R0 = R0n;
#ifndef SPRS_HIP_EMU
            asm volatile("" : "+v"(R0)::"memory");
#endif
            // the tile after this one: the next of the range, or the first of the wave's next range
            const uint32_t rend = (r + 1) * run < n ? (r + 1) * run : n;
            const bool range_ends = t + 1 >= rend;
            const uint32_t rn = G > 1u && (r % G) + 1u < G ? r + 1u : r + 1u + (uint32_t)(HOT_WAVES - 1) * G;   // the wave's next range
            const uint32_t tn = range_ends ? rn * run : t + 1;
            SPRS_GLOBAL_AS T *cslot = (SPRS_GLOBAL_AS T *)carry + seg.range0 + r;
            auto out = [&](uint32_t row, T v) {
                if (DEVTOOLS && (dbg & 1u)) return;                      // no stores of the row sums
                __builtin_nontemporal_store(v, &d.out[row]);              // read again by the reduction, a few GB of traffic later

            };
            if (pd.cnt) band_flush(pd, lane, pd_slot, stage, out);        // the previous tile's sums, before this tile's loads are asked for
            if (tn < n) request(seg.tile0 + tn);                         // streams while this tile is summed
            if constexpr (DEVTOOLS) {                                    // timing experiments (option spmv_band_debug): WRONG results
                if (dbg & 2u) fb &= 0x01u;                               // at most one row start per lane
                if (dbg & 4u) fb = 0;                                    // no row starts at all
            }
            if (DEVTOOLS && (dbg & 8u)) {
                band_tile_sums<false>(pr, fb, lane, R0, open, mine, last, cslot, stage, pd, out);
            } else {
                band_tile_sums<true>(pr, fb, lane, R0, open, mine, last, cslot, stage, pd, out);
                pd_slot = cslot;
            }
            if (range_ends) {
                if (lane == 0) {
                    if (mine) d.out[last] = open;                        // the row still open at the end of the range: its sum so far
                    else *cslot = open;                                  // no row starts in the whole range: all of it belongs to an earlier row
                }
                open = 0.0;
                mine = false;
                r = rn;
            }
            t = tn;
        }
        if (pd.cnt) band_flush(pd, lane, pd_slot, stage, [&](uint32_t row, T v) {
            if (DEVTOOLS && (dbg & 1u)) return;
            d.out[row] = v;
        });
    }
    if constexpr (DEVTOOLS) {
        if (prof) {
            __syncthreads();
            if (threadIdx.x == 0) prof[3 * blockIdx.x + 2] = (unsigned long long)wall_clock64();
        }
    }
}


// ---------------------------------------------------------------------------------------------
// x into the plan's labelling, the scatter form (the description: spmv_band_kernels.hpp)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void BAND_KERNEL(band_permute_kernel)(const BAND_T *__restrict__ x, const uint32_t *__restrict__ perm,
                                                           uint64_t cols, BAND_T *__restrict__ xp, BAND_T *__restrict__ y_zero,
                                                           uint64_t rows, uint32_t first_label, uint32_t nref) {
    typedef BAND_T T;
    const uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const uint32_t span = nref - first_label;                            // label in range <=> label - first_label < span
    if (j + 4 <= cols && (((uintptr_t)x | (uintptr_t)perm) & 15) == 0) {
        const u32x4 l = *(const u32x4 *)(perm + j);
        if constexpr (sizeof(T) == 8) {
            const dbl2 a = *(const dbl2 *)(x + j), b = *(const dbl2 *)(x + j + 2);
            if (l[0] - first_label < span) xp[l[0]] = a[0];
            if (l[1] - first_label < span) xp[l[1]] = a[1];
            if (l[2] - first_label < span) xp[l[2]] = b[0];
            if (l[3] - first_label < span) xp[l[3]] = b[1];
        } else {
            const flt4 a = *(const flt4 *)(x + j);
            if (l[0] - first_label < span) xp[l[0]] = a[0];
            if (l[1] - first_label < span) xp[l[1]] = a[1];
            if (l[2] - first_label < span) xp[l[2]] = a[2];
            if (l[3] - first_label < span) xp[l[3]] = a[3];
        }
    } else {
        for (uint64_t c = j; c < cols && c < j + 4; ++c) {
            const uint32_t l = perm[c];
            if (l - first_label < span) xp[l] = x[c];
        }
    }
    if (y_zero) {
        if (j + 4 <= rows && ((uintptr_t)y_zero & 15) == 0) {
            band_store4(y_zero + j, (T)0.0, (T)0.0, (T)0.0, (T)0.0);
        } else {
            for (uint64_t r = j; r < rows && r < j + 4; ++r) y_zero[r] = 0.0;
        }
    }
}
