// Device-resident BiCGSTAB: twin of sprs::linalg::bicgstab::BiCGSTAB::solve
// (sprs/src/sparse/linalg/bicgstab.rs:148-171; new() :117-143, step() :194-229, soft/hard
// restart :175-192) — SURVEY §8 (f3), "callers that loop on SpMV".
//
// The reference keeps x, r, rhat, p as CsVec and forms every product with `&CsMat * &CsVec`; for
// vectors without structural zeros that is the dense arithmetic done here (csr_mul_csvec,
// prod.rs:162-184, is one ascending sparse dot per row; a CSC operand takes the SpGEMM route, which
// also adds ascending k).  Everything stays in HBM: per iteration two SpMVs (the
// hot path of this library), four fused element-wise kernels and three dot launches; the host sees
// five scalars per iteration (alpha, omega, rho need them anyway: the restart decisions are
// data dependent, bicgstab.rs:219-226).
//
// Arithmetic: unfused (-ffp-contract=off), same operand order as the reference's expressions, so
// the element-wise part is bit-identical.  (The SpMV is within its own 1e-10 bar: a row that straddles
// two nnz tiles is summed as tail + head.)  Dot products / norms: the reference sums serially from
// 0 (vec.rs:846-880, 907-918).  For n <= BICG_SERIAL_N one thread does exactly that — the
// reference's own test system (4 x 4, tol 1e-60, bicgstab.rs:336-369) then converges to a residual of
// exactly zero in 45 iterations, as a serial CPU restatement of the reference does; above it a FIXED
// two-level tree (8192-element chunks, 256 threads each, partials summed by one workgroup) —
// deterministic, independent of the
// launch, but rounded differently from a serial sum: iterates agree with the serial ones to
// rounding and the restart counts may differ.
//
// The kernels and the loop are templates on the scalar: the reference instantiates its solver for f64 and f32
// (bicgstab.rs:304-305).  For f32 every vector, dot and host scalar is a float, the SpMV is spmv_f32 (spmv_f32.hpp).
#include "common.hpp"

#include <cmath>

namespace sprs_hip {

namespace {

constexpr uint64_t BICG_SERIAL_N = 2048;
constexpr int DOT_BLOCK = 256;
constexpr uint64_t DOT_CHUNK = 8192;

// fixed-shape block reduction: lane tree inside the wave, then the waves in order
template <typename T>
__device__ __forceinline__ T block_sum_fixed(T v, T *lds /* >= 4 */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    T s = T(0);
    if (threadIdx.x == 0) {
        s = lds[0];
        for (uint32_t w = 1; w < (uint32_t)(DOT_BLOCK / 64); ++w) s += lds[w];
    }
    __syncthreads();
    return s;   // valid in thread 0
}

// out[0] = sum a_i b_i, out[1] = sum c_i d_i (second pair optional), serial order: n <= BICG_SERIAL_N
template <typename T>
__global__ void dot_serial_kernel(const T *__restrict__ a, const T *__restrict__ b,
                                  const T *__restrict__ c, const T *__restrict__ d, uint64_t n,
                                  T *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    T s0 = T(0), s1 = T(0);
    for (uint64_t i = 0; i < n; ++i) {
        const T p0 = a[i] * b[i];
        s0 = s0 + p0;
        if (c) {
            const T p1 = c[i] * d[i];
            s1 = s1 + p1;
        }
    }
    out[0] = s0;
    out[1] = s1;
}

// stage 1: chunk c = [c * DOT_CHUNK, ...): thread t sums elements t, t + 256, ... serially, then the block tree
template <typename T>
__global__ __launch_bounds__(DOT_BLOCK) void dot_partial_kernel(const T *__restrict__ a,
                                                                const T *__restrict__ b,
                                                                const T *__restrict__ c,
                                                                const T *__restrict__ d, uint64_t n,
                                                                T *__restrict__ partial /* 2 x nchunks */) {
    __shared__ T lds[8];
    const uint64_t lo = (uint64_t)blockIdx.x * DOT_CHUNK;
    const uint64_t hi = lo + DOT_CHUNK < n ? lo + DOT_CHUNK : n;
    T s0 = T(0), s1 = T(0);
    for (uint64_t i = lo + threadIdx.x; i < hi; i += DOT_BLOCK) {
        const T p0 = a[i] * b[i];
        s0 = s0 + p0;
        if (c) {
            const T p1 = c[i] * d[i];
            s1 = s1 + p1;
        }
    }
    const T t0 = block_sum_fixed(s0, lds);
    const T t1 = block_sum_fixed(s1, lds + 4);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t0;
        partial[gridDim.x + blockIdx.x] = t1;
    }
}

// stage 2: one workgroup, thread t sums partials t, t + 256, ... serially, then the block tree
template <typename T>
__global__ __launch_bounds__(DOT_BLOCK) void dot_final_kernel(const T *__restrict__ partial, uint64_t nchunks,
                                                              T *__restrict__ out) {
    __shared__ T lds[8];
    T s0 = T(0), s1 = T(0);
    for (uint64_t i = threadIdx.x; i < nchunks; i += DOT_BLOCK) {
        s0 = s0 + partial[i];
        s1 = s1 + partial[nchunks + i];
    }
    const T t0 = block_sum_fixed(s0, lds);
    const T t1 = block_sum_fixed(s1, lds + 4);
    if (threadIdx.x == 0) {
        out[0] = t0;
        out[1] = t1;
    }
}

// ---- element-wise steps, written as the reference writes them --------------------------------
// new(): r = b - A x0 (v holds A x0); rhat = r; p = r; x = x0      (bicgstab.rs:123-128)
template <typename T>
__global__ void init_kernel(const T *__restrict__ b, const T *__restrict__ v, const T *__restrict__ x0,
                            uint64_t n, T *__restrict__ r, T *__restrict__ rhat, T *__restrict__ p,
                            T *__restrict__ x) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T ri = b[i] - v[i];
    r[i] = ri;
    rhat[i] = ri;
    p[i] = ri;
    x[i] = x0[i];
}

// h = x + p * alpha;  s = r - v * alpha                            (bicgstab.rs:200, 203)
template <typename T>
__global__ void hs_kernel(const T *__restrict__ x, const T *__restrict__ p, const T *__restrict__ r,
                          const T *__restrict__ v, T alpha, uint64_t n, T *__restrict__ h,
                          T *__restrict__ s) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T pa = p[i] * alpha;
    h[i] = x[i] + pa;
    const T va = v[i] * alpha;
    s[i] = r[i] - va;
}

// x = h + omega * s;  r = s - t * omega                            (bicgstab.rs:206, 209)
template <typename T>
__global__ void xr_kernel(const T *__restrict__ h, const T *__restrict__ s, const T *__restrict__ t,
                          T omega, uint64_t n, T *__restrict__ x, T *__restrict__ r) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T os = omega * s[i];
    x[i] = h[i] + os;
    const T to = t[i] * omega;
    r[i] = s[i] - to;
}

// p = r + (p - v * omega) * beta                                   (bicgstab.rs:224-226)
template <typename T>
__global__ void p_kernel(const T *__restrict__ r, const T *__restrict__ v, T omega, T beta,
                         uint64_t n, T *__restrict__ p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T vo = v[i] * omega;
    const T d = p[i] - vo;
    const T e = d * beta;
    p[i] = r[i] + e;
}

// soft_restart(): rhat = r; p = r                                  (bicgstab.rs:175-180)
template <typename T>
__global__ void restart_kernel(const T *__restrict__ r, uint64_t n, T *__restrict__ rhat,
                               T *__restrict__ p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rhat[i] = r[i];
    p[i] = r[i];
}

// hard_restart(): r = b - A x (v holds A x)                        (bicgstab.rs:186)
template <typename T>
__global__ void resid_kernel(const T *__restrict__ b, const T *__restrict__ v, uint64_t n,
                             T *__restrict__ r) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    r[i] = b[i] - v[i];
}

// Every host scalar (alpha, omega, beta, rho, err) is computed in T, in the reference's expression order; sqrt in T.
template <typename T, typename MAT>
int32_t bicgstab_impl(MAT *a_in, const T *x0, const T *b, uint64_t n, T tol, uint64_t max_iter, T soft_restart_threshold, T *x,
                      sprs_hip_bicgstab_info *info, hipStream_t stream) {
    // `&a * &x` of a CSC matrix (csmat.rs:1866-1949 route) == CSR SpMV of its CSR form: convert once
    MAT *a = a_in;
    std::unique_ptr<MAT> converted;
    if (a_in->storage != SPRS_HIP_CSR) {
        SPRS_TRY(to_other_storage(a_in, converted));
        a = converted.get();
    }

    const uint64_t nchunks = (n + DOT_CHUNK - 1) / DOT_CHUNK;
    DevBuf work;
    SPRS_TRY_HIP(work.alloc((7 * n + 2 * nchunks + 8) * sizeof(T)));
    T *r = work.as<T>(), *rhat = r + n, *p = rhat + n, *v = p + n, *s = v + n, *t = s + n, *h = t + n;
    T *partial = h + n, *scal = partial + 2 * nchunks;
    const dim3 eg((unsigned)((n + 255) / 256)), eb(256);

    // two dots in one go; returns them on the host (the stream is drained: the next scalar depends on it)
    auto dots = [&](const T *a0, const T *b0, const T *c0, const T *d0, T &o0,
                    T &o1) -> int32_t {
        if (n <= BICG_SERIAL_N) {
            hipLaunchKernelGGL(dot_serial_kernel<T>, dim3(1), dim3(64), 0, stream, a0, b0, c0, d0, n, scal);
        } else {
            hipLaunchKernelGGL(dot_partial_kernel<T>, dim3((unsigned)nchunks), dim3(DOT_BLOCK), 0, stream, a0, b0, c0, d0, n,
                               partial);
            hipLaunchKernelGGL(dot_final_kernel<T>, dim3(1), dim3(DOT_BLOCK), 0, stream, partial, nchunks, scal);
        }
        SPRS_TRY_HIP(hipGetLastError());
        T hst[2];
        SPRS_TRY_HIP(copy_to_host(hst, scal, 2 * sizeof(T), stream));
        o0 = hst[0];
        o1 = hst[1];
        return SPRS_HIP_OK;
    };
    const T *none = nullptr;
    T d0 = T(0), d1 = T(0);

    // ---- new() ---------------------------------------------------------------------------------
    SPRS_TRY(spmv(a, x0, v, false, stream));
    hipLaunchKernelGGL(init_kernel<T>, eg, eb, 0, stream, b, v, x0, n, r, rhat, p, x);
    SPRS_TRY_HIP(hipGetLastError());
    SPRS_TRY(dots(r, r, none, none, d0, d1));
    T err = std::sqrt(d0);
    T rho = err * err;
    uint64_t it = 0, soft = 0, hard = 0;
    int32_t converged = 0;

    for (uint64_t k = 0; k < max_iter && !converged; ++k) {
        // ---- step() ----------------------------------------------------------------------------
        ++it;
        SPRS_TRY(spmv(a, p, v, false, stream));
        SPRS_TRY(dots(rhat, v, none, none, d0, d1));
        const T alpha = rho / d0;
        hipLaunchKernelGGL(hs_kernel<T>, eg, eb, 0, stream, x, p, r, v, alpha, n, h, s);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(spmv(a, s, t, false, stream));
        SPRS_TRY(dots(t, s, t, t, d0, d1));
        const T omega = d0 / d1;
        hipLaunchKernelGGL(xr_kernel<T>, eg, eb, 0, stream, h, s, t, omega, n, x, r);
        SPRS_TRY_HIP(hipGetLastError());
        SPRS_TRY(dots(r, r, rhat, r, d0, d1));
        err = std::sqrt(d0);
        const T rho_prev = rho;
        rho = d1;
        if (std::fabs(rho) / (err * err) < soft_restart_threshold) {
            ++soft;
            hipLaunchKernelGGL(restart_kernel<T>, eg, eb, 0, stream, r, n, rhat, p);
            rho = err * err;
        } else {
            const T beta = (rho / rho_prev) * (alpha / omega);
            hipLaunchKernelGGL(p_kernel<T>, eg, eb, 0, stream, r, v, omega, beta, n, p);
        }
        SPRS_TRY_HIP(hipGetLastError());
        // ---- solve(): check the TRUE error before claiming convergence ---------------------------
        if (err < tol) {
            ++hard;
            SPRS_TRY(spmv(a, x, v, false, stream));
            hipLaunchKernelGGL(resid_kernel<T>, eg, eb, 0, stream, b, v, n, r);
            SPRS_TRY_HIP(hipGetLastError());
            SPRS_TRY(dots(r, r, none, none, d0, d1));
            err = std::sqrt(d0);
            hipLaunchKernelGGL(restart_kernel<T>, eg, eb, 0, stream, r, n, rhat, p);
            SPRS_TRY_HIP(hipGetLastError());
            rho = err * err;
            if (err < tol) converged = 1;
        }
    }
    SPRS_TRY_HIP(hipStreamSynchronize(stream));
    if (info) {
        info->iteration_count = it;
        info->soft_restart_count = soft;
        info->hard_restart_count = hard;
        info->err = (double)err;   // (an f32 widens exactly)
        info->rho = (double)rho;
        info->converged = converged;
    }
    return SPRS_HIP_OK;
}

}  // namespace

int32_t bicgstab_f64(sprs_hip_csmat *a, const double *x0, const double *b, uint64_t n, double tol, uint64_t max_iter,
                     double soft_restart_threshold, double *x, sprs_hip_bicgstab_info *info, hipStream_t stream) {
    return bicgstab_impl<double>(a, x0, b, n, tol, max_iter, soft_restart_threshold, x, info, stream);
}

int32_t bicgstab_f32(sprs_hip_csmat_f32 *a, const float *x0, const float *b, uint64_t n, float tol, uint64_t max_iter,
                     float soft_restart_threshold, float *x, sprs_hip_bicgstab_info *info, hipStream_t stream) {
    return bicgstab_impl<float>(a, x0, b, n, tol, max_iter, soft_restart_threshold, x, info, stream);
}

}  // namespace sprs_hip
