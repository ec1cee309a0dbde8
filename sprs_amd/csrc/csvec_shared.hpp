// What the sparse-vector kernels of several translation units share: the lane reads and masks of the ordered sums (csvec.hpp,
// csvec_reduce.hpp in spmv.hip) and the emit step that turns kept slots into a sorted CsVec (csvec.hpp; extract.hpp in convert.hip).
#pragma once

#include "common.hpp"

namespace sprs_hip {
namespace cv {

constexpr int CV_BLOCK = 256;                 // 4 waves, each its own group of 64 outer slices

__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ double rl_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// bits [a, b) of a 64-bit mask, 0 <= a <= b <= 64
__device__ __forceinline__ uint64_t span_mask(uint64_t a, uint64_t b) {
    if (a >= b) return 0;
    const uint64_t upto = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
    return upto & ~((1ull << a) - 1ull);
}

// 4. kept slices -> the result's sorted (indices, data).  An index above `limit` (the declared width's maximum) is not
// written: it raises *overflow instead (I::from_usize would panic, vec.rs append)
template <typename OI>
__global__ void __launch_bounds__(CV_BLOCK) csvec_emit_kernel(const uint64_t *masks, const uint64_t *offs, const double *sums,
                                                              uint64_t nouter, uint64_t limit, OI *oidx, double *oval,
                                                              uint32_t *overflow) {
    const uint64_t o = (uint64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (o >= nouter) return;
    const uint64_t m = masks[o >> 6];
    const int b = (int)(o & 63);
    if (!((m >> b) & 1ull)) return;
    const uint64_t pos = offs[o >> 6] + (uint64_t)__popcll(m & ((1ull << b) - 1ull));
    if (o > limit) {
        atomicOr(overflow, 1u);
        return;
    }
    oidx[pos] = (OI)o;
    oval[pos] = sums[o];
}

inline unsigned blocks_for(uint64_t items) { return (unsigned)((items + CV_BLOCK - 1) / CV_BLOCK); }

}  // namespace cv
}  // namespace sprs_hip
