// Kernels of the Anderson mixer (anderson.hpp).  All three stream fp64
// vectors through registers once, 16 bytes a lane (every vector starts at an allocation's start,
// so pairs are aligned); none uses LDS beyond the four wave sums of the reduction, none an atomic.
#include <hip/hip_runtime.h>

#include "anderson.hpp"

// Every product and sum below is rounded on its own: the mix is then the unfused statement of
// include/kkt.h bit for bit, and beta = 1, c = 0 returns the bits of f.
#pragma clang fp contract(off)

namespace kkt {

typedef double d2 __attribute__((ext_vector_type(2)));

static inline int stream_grid(int64_t n) {
    const int64_t g = ((n + 1) / 2 + ANDERSON_THREADS - 1) / ANDERSON_THREADS;
    return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

__global__ __launch_bounds__(ANDERSON_THREADS) void anderson_push_kernel(
    const double *__restrict__ f, double *__restrict__ f_prev, double *__restrict__ dF_new,
    int64_t n) {
    const int64_t pairs = n >> 1, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t q = t; q < pairs; q += step) {
        const d2 a = *reinterpret_cast<const d2 *>(f + 2 * q);
        const d2 b = *reinterpret_cast<const d2 *>(f_prev + 2 * q);
        d2 d;
        d.x = a.x - b.x;
        d.y = a.y - b.y;
        *reinterpret_cast<d2 *>(dF_new + 2 * q) = d;
        *reinterpret_cast<d2 *>(f_prev + 2 * q) = a;
    }
    if ((n & 1) && t == 0) {
        const double a = f[n - 1];
        dF_new[n - 1] = a - f_prev[n - 1];
        f_prev[n - 1] = a;
    }
}

void launch_anderson_push(hipStream_t s, const double *f, double *f_prev, double *dF_new,
                          int64_t n) {
    hipLaunchKernelGGL(anderson_push_kernel, dim3(stream_grid(n)), dim3(ANDERSON_THREADS), 0, s, f,
                       f_prev, dF_new, n);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// acc += the products of one element (fused, as mdot_stage1's): the lower triangle of G row by
// row, then r
template <int C>
__device__ __forceinline__ void gram_accumulate(double (&acc)[anderson_dots(C)],
                                                const double (&v)[C], double fv) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j, ++k) acc[k] = __builtin_fma(v[i], v[j], acc[k]);
#pragma unroll
    for (int i = 0; i < C; ++i)
        acc[C * (C + 1) / 2 + i] = __builtin_fma(v[i], fv, acc[C * (C + 1) / 2 + i]);
}

// Stage 1: ANDERSON_BLOCKS workgroups stride over the pairs of elements; one pass over the C + 1
// vectors feeds all C (C + 1) / 2 + C sums (44 accumulators a thread at C = 8).  A thread's sum
// runs over its elements in index order, a wave's by shuffles, the four waves' in LDS in wave
// order: part[block * ANDERSON_DOTS_MAX + dot].
template <int C>
__global__ __launch_bounds__(ANDERSON_THREADS) void anderson_gram_kernel(
    const AndersonCols cols, const double *__restrict__ f, int64_t n, double *__restrict__ part) {
    constexpr int ND = anderson_dots(C);
    __shared__ double sh[ANDERSON_THREADS / 64][ND];
    double acc[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) acc[k] = 0.0;
    const int64_t pairs = n >> 1, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t q = t; q < pairs; q += step) {
        const d2 fv = *reinterpret_cast<const d2 *>(f + 2 * q);
        double vx[C], vy[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const d2 v = *reinterpret_cast<const d2 *>(cols.dF[i] + 2 * q);
            vx[i] = v.x;
            vy[i] = v.y;
        }
        gram_accumulate<C>(acc, vx, fv.x);
        gram_accumulate<C>(acc, vy, fv.y);
    }
    if ((n & 1) && t == 0) {
        double v[C];
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = cols.dF[i][n - 1];
        gram_accumulate<C>(acc, v, f[n - 1]);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const double w = wave_sum(acc[k]);
        if (lane == 0) sh[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < ND) {
        const int k = threadIdx.x;
        part[(int64_t)blockIdx.x * ANDERSON_DOTS_MAX + k] =
            ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
    }
}

// Stage 2: thread k adds the partials of sum k in workgroup order
__global__ __launch_bounds__(64) void anderson_gram_finish_kernel(const double *__restrict__ part,
                                                                  int nd, double *__restrict__ out) {
    const int k = threadIdx.x;
    if (k >= nd) return;
    double a = 0.0;
    for (int b = 0; b < ANDERSON_BLOCKS; ++b) a += part[(int64_t)b * ANDERSON_DOTS_MAX + k];
    out[k] = a;
}

void launch_anderson_gram(hipStream_t s, const AndersonCols &cols, int c, const double *f,
                          int64_t n, double *part) {
    const dim3 g(ANDERSON_BLOCKS), b(ANDERSON_THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(anderson_gram_kernel<1>, g, b, 0, s, cols, f, n, part); break;
        case 2: hipLaunchKernelGGL(anderson_gram_kernel<2>, g, b, 0, s, cols, f, n, part); break;
        case 3: hipLaunchKernelGGL(anderson_gram_kernel<3>, g, b, 0, s, cols, f, n, part); break;
        case 4: hipLaunchKernelGGL(anderson_gram_kernel<4>, g, b, 0, s, cols, f, n, part); break;
        case 5: hipLaunchKernelGGL(anderson_gram_kernel<5>, g, b, 0, s, cols, f, n, part); break;
        case 6: hipLaunchKernelGGL(anderson_gram_kernel<6>, g, b, 0, s, cols, f, n, part); break;
        case 7: hipLaunchKernelGGL(anderson_gram_kernel<7>, g, b, 0, s, cols, f, n, part); break;
        case 8: hipLaunchKernelGGL(anderson_gram_kernel<8>, g, b, 0, s, cols, f, n, part); break;
        default: return;
    }
    hipLaunchKernelGGL(anderson_gram_finish_kernel, dim3(1), dim3(64), 0, s, part,
                       anderson_dots(c), part + (int64_t)ANDERSON_BLOCKS * ANDERSON_DOTS_MAX);
}

template <int C>
__device__ __forceinline__ double mix_one(double fv, const double (&dx)[C > 0 ? C : 1],
                                          const double (&df)[C > 0 ? C : 1],
                                          const AndersonCols &cols, double beta) {
    double s = beta * fv;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double t = dx[j] + beta * df[j];
        s = s - cols.gamma[j] * t;
    }
    return s;
}

// u holds f and receives s; dX_new may be one of cols.dX (a full ring: the oldest pair's slot),
// so neither it nor the columns are __restrict__: a thread reads all its operands of an element
// before it writes that element, and no other thread touches it.
template <int C>
__global__ __launch_bounds__(ANDERSON_THREADS) void anderson_mix_kernel(const AndersonCols cols,
                                                                        double beta, double *u,
                                                                        double *dX_new, int64_t n) {
    constexpr int K = C > 0 ? C : 1;
    const int64_t pairs = n >> 1, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t q = t; q < pairs; q += step) {
        const d2 fv = *reinterpret_cast<const d2 *>(u + 2 * q);
        double dxx[K], dxy[K], dfx[K], dfy[K];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const d2 a = *reinterpret_cast<const d2 *>(cols.dX[j] + 2 * q);
            const d2 b = *reinterpret_cast<const d2 *>(cols.dF[j] + 2 * q);
            dxx[j] = a.x, dxy[j] = a.y, dfx[j] = b.x, dfy[j] = b.y;
        }
        d2 s;
        s.x = mix_one<C>(fv.x, dxx, dfx, cols, beta);
        s.y = mix_one<C>(fv.y, dxy, dfy, cols, beta);
        *reinterpret_cast<d2 *>(u + 2 * q) = s;
        *reinterpret_cast<d2 *>(dX_new + 2 * q) = s;
    }
    if ((n & 1) && t == 0) {
        double dx[K], df[K];
#pragma unroll
        for (int j = 0; j < C; ++j) dx[j] = cols.dX[j][n - 1], df[j] = cols.dF[j][n - 1];
        const double s = mix_one<C>(u[n - 1], dx, df, cols, beta);
        u[n - 1] = s;
        dX_new[n - 1] = s;
    }
}

void launch_anderson_mix(hipStream_t s, const AndersonCols &cols, int c, double beta, double *u,
                         double *dX_new, int64_t n) {
    const dim3 g(stream_grid(n)), b(ANDERSON_THREADS);
    switch (c) {
        case 0: hipLaunchKernelGGL(anderson_mix_kernel<0>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 1: hipLaunchKernelGGL(anderson_mix_kernel<1>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 2: hipLaunchKernelGGL(anderson_mix_kernel<2>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 3: hipLaunchKernelGGL(anderson_mix_kernel<3>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 4: hipLaunchKernelGGL(anderson_mix_kernel<4>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 5: hipLaunchKernelGGL(anderson_mix_kernel<5>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 6: hipLaunchKernelGGL(anderson_mix_kernel<6>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 7: hipLaunchKernelGGL(anderson_mix_kernel<7>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        case 8: hipLaunchKernelGGL(anderson_mix_kernel<8>, g, b, 0, s, cols, beta, u, dX_new, n); break;
        default: break;
    }
}

}  // namespace kkt
