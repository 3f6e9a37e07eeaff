// Kernels of the batched spectrum estimates (spectrum.cpp): B matrices of one pattern run the
// Lanczos / power recurrences in lock-step, the matrix index on blockIdx.y.  The arithmetic per
// matrix is the one-matrix path's, operation for operation: the dots have mdot_stage1 /
// mdot_stage2's chunks and trees (kernels.hip), the vector updates the roundings axpby_kernel
// compiles to, the scalars of a step (spectrum_host.hpp) are plain IEEE double.  A workgroup of a
// matrix whose `active` word is 0 leaves at once.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include "spectrum_host.hpp"

namespace kkt {

typedef double d2 __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ double spec_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// stage 1 of <x_b, y_b>: mdot_stage1<1> per matrix
__global__ __launch_bounds__(256) void spec_dot_stage1(const double *__restrict__ x,
                                                       const double *__restrict__ y, int64_t stride,
                                                       int64_t n, double *__restrict__ part,
                                                       const uint32_t *__restrict__ active) {
    const int b = blockIdx.y;
    if (!active[b]) return;
    __shared__ double sh[4];
    const double *xv = x + (int64_t)b * stride, *yv = y + (int64_t)b * stride;
    const int64_t chunk = ((n + REDUCE_BLOCKS - 1) / REDUCE_BLOCKS + 1) & ~(int64_t)1;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    int64_t hi = lo + chunk;
    if (hi > n) hi = n;
    double acc = 0.0;
    // chunk, lo and stride are even -> 16-byte aligned double2 accesses
    int64_t p = lo + 2 * (int64_t)threadIdx.x;
    for (; p + 1 < hi; p += 512) {
        const d2 a = *reinterpret_cast<const d2 *>(xv + p);
        const d2 c = *reinterpret_cast<const d2 *>(yv + p);
        acc = __builtin_fma(a.x, c.x, acc);
        acc = __builtin_fma(a.y, c.y, acc);
    }
    if (p < hi) acc = __builtin_fma(xv[p], yv[p], acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double t = spec_wave_sum(acc);
    if (lane == 0) sh[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0)
        part[(int64_t)b * REDUCE_BLOCKS + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage 2: mdot_stage2's tree over the matrix's REDUCE_BLOCKS partials, then the scalars of the step
__global__ __launch_bounds__(256) void spec_dot_stage2(SpecBatch S, int mode, int k) {
    const int b = blockIdx.x;
    if (!S.active[b]) return;
    __shared__ double sh[256];
    const double *part = S.part + (int64_t)b * REDUCE_BLOCKS;
    double a = 0.0;
    for (int q = threadIdx.x; q < REDUCE_BLOCKS; q += 256) a += part[q];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double dot = sh[0];
    switch (mode) {
        case SPEC_DOT_START: {
            double rz;
            if (!spec::lanczos_start(dot, &rz)) S.active[b] = 0u;
            S.rz[b] = rz;
            break;
        }
        case SPEC_DOT_PAP: {
            double al;
            if (!spec::lanczos_alpha(dot, S.rz[b], &al)) {
                S.active[b] = 0u;
                break;
            }
            const int32_t s = S.na[b];
            if (s < S.max_steps) S.alpha[(int64_t)s * S.B + b] = al;
            S.na[b] = s + 1;
            S.coef[b] = al;
            break;
        }
        case SPEC_DOT_RZ: {
            double be;
            if (!spec::lanczos_beta(dot, S.rz[b], &be)) {
                S.active[b] = 0u;
                break;
            }
            const int32_t s = S.nb[b];
            if (s < S.max_steps) S.beta[(int64_t)s * S.B + b] = be;
            S.nb[b] = s + 1;
            S.coef[b] = be;
            S.rz[b] = dot;
            break;
        }
        case SPEC_DOT_NORM0: {
#pragma clang fp contract(off)
            const double nv = __dsqrt_rn(dot);
            if (spec::power_live(nv))
                S.coef[b] = 1.0 / nv;
            else
                S.active[b] = 0u;
            break;
        }
        default: {   // SPEC_DOT_NORM after step k
#pragma clang fp contract(off)
            const double nv = __dsqrt_rn(dot);
            S.mu2[b] = nv;
            S.na[b] = k + 1;
            if (spec::power_settled(k, nv, S.last[b]) || !spec::power_live(nv)) {
                S.active[b] = 0u;
                break;
            }
            S.last[b] = nv;
            S.coef[b] = 1.0 / nv;
            break;
        }
    }
}

// The vector updates, coefficient from S.coef.  axpby_kernel's y = a x + b y compiles to
// fma(a, x, fl(b y)) (v_mul_f64 of b and y, v_fmac_f64 of a and x onto it); the three calls of the
// one-matrix loop in that form:
//   r = -a w + 1 r   ->  fma(-a, w, r)           (1 r is exact)
//   p = 1 z + b p    ->  fma(1, z, fl(b p))
//   v = 0 z + c v    ->  fma(0, z, fl(c v))       (z: the loop's second vector; keeps a NaN's way)
__global__ __launch_bounds__(256) void spec_update_kernel(SpecBatch S, int kind) {
    const int b = blockIdx.y;
    if (!S.active[b]) return;
    const int64_t off = (int64_t)b * S.stride;
    const double c = kind == SPEC_UPD_COPY ? 0.0 : S.coef[b];
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < S.n; q += step) {
#pragma clang fp contract(off)
        const int64_t i = off + q;
        switch (kind) {
            case SPEC_UPD_R: S.r[i] = __builtin_fma(-c, S.w[i], 1.0 * S.r[i]); break;
            case SPEC_UPD_P: S.p[i] = __builtin_fma(1.0, S.z[i], c * S.p[i]); break;
            case SPEC_UPD_SCALE: S.r[i] = __builtin_fma(0.0, S.z[i], c * S.r[i]); break;
            default: S.p[i] = S.z[i]; break;
        }
    }
}

// vals_sym_skew_kernel over a batch: matrix b's values m[b].a into m[b].h / m[b].sk, flag nonsym[b]
__global__ __launch_bounds__(256) void spec_sym_skew_kernel(const SpecSplit *__restrict__ m,
                                                            const int32_t *__restrict__ tpos, int64_t n,
                                                            unsigned *__restrict__ nonsym) {
    const SpecSplit M = m[blockIdx.y];
    bool any = false;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t t = tpos[p];
        const double x = M.a[p];
        if (t < 0) {
            M.h[p] = x;
            M.sk[p] = 0.0;
            continue;
        }
        const double y = M.a[t];
        M.h[p] = 0.5 * (x + y);
        M.sk[p] = 0.5 * (x - y);
        if (x != 0.0 && y != 0.0 && fabs(x - y) > 1e-12 * (fabs(x) + fabs(y))) any = true;
    }
    if (any) atomicOr(nonsym + blockIdx.y, 1u);
}

// Fingerprint of a value array's bits: workgroup g of candidate c folds its strided share in a fixed
// order (per thread, then a fixed LDS tree) into out[c * gridDim.x + g]; the host folds the
// gridDim.x words.  It prunes the twin search only: equality is spec_pairs_differ_kernel's.
__device__ __forceinline__ unsigned long long spec_mix(unsigned long long h, unsigned long long v) {
    h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
    return h * 0xff51afd7ed558ccdull;
}
__global__ __launch_bounds__(256) void spec_fingerprint_kernel(const double *const *__restrict__ vals,
                                                               int64_t n,
                                                               unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sh[256];
    const double *a = vals[blockIdx.y];
    unsigned long long h = 0x2545f4914f6cdd1dull;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x)
        h = spec_mix(h, (unsigned long long)__double_as_longlong(a[p]));
    sh[threadIdx.x] = h;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] = spec_mix(sh[threadIdx.x], sh[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// vals_differ_kernel per pair: flag[q] |= 1 when the arrays of pair q differ in any bit
__global__ __launch_bounds__(256) void spec_pairs_differ_kernel(const SpecPair *__restrict__ pairs,
                                                                int64_t n, unsigned *__restrict__ flag) {
    const SpecPair P = pairs[blockIdx.y];
    bool d = false;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x)
        d |= __double_as_longlong(P.a[p]) != __double_as_longlong(P.b[p]);
    if (d) atomicOr(flag + blockIdx.y, 1u);
}

inline int spec_grid(int64_t n, int cap) {
    int64_t g = (n + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

void launch_spec_dot(hipStream_t s, const SpecBatch &S, const double *x, const double *y, int mode,
                     int k) {
    if (S.B <= 0) return;
    hipLaunchKernelGGL(spec_dot_stage1, dim3(REDUCE_BLOCKS, S.B), dim3(256), 0, s, x, y, S.stride, S.n,
                       S.part, S.active);
    hipLaunchKernelGGL(spec_dot_stage2, dim3(S.B), dim3(256), 0, s, S, mode, k);
}

void launch_spec_update(hipStream_t s, const SpecBatch &S, int kind) {
    if (S.B <= 0 || S.n <= 0) return;
    hipLaunchKernelGGL(spec_update_kernel, dim3(spec_grid(S.n, 256), S.B), dim3(256), 0, s, S, kind);
}

void launch_spec_sym_skew(hipStream_t s, const SpecSplit *d_m, int nmat, const int32_t *tpos, int64_t n,
                          unsigned *nonsym) {
    if (nmat <= 0 || n <= 0) return;
    hipLaunchKernelGGL(spec_sym_skew_kernel, dim3(spec_grid(n, 512), nmat), dim3(256), 0, s, d_m, tpos,
                       n, nonsym);
}

void launch_spec_fingerprint(hipStream_t s, const double *const *d_vals, int nmat, int64_t n,
                             unsigned long long *out) {
    if (nmat <= 0) return;
    hipLaunchKernelGGL(spec_fingerprint_kernel, dim3(spec_fingerprint_blocks(n), nmat), dim3(256), 0, s,
                       d_vals, n, out);
}

void launch_spec_pairs_differ(hipStream_t s, const SpecPair *d_pairs, int npairs, int64_t n,
                              unsigned *flag) {
    if (npairs <= 0) return;
    hipLaunchKernelGGL(spec_pairs_differ_kernel, dim3(spec_grid(n, 256), npairs), dim3(256), 0, s,
                       d_pairs, n, flag);
}

}  // namespace kkt
