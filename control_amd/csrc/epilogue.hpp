// The epilogue of a RowOp (kernels.hpp), once, for every kernel that runs one: the row launches and
// row programs of kernels.hip, pc_tile_sweep (tile_kernels.hip; its narrow-row steps 2..its restate
// epi_cheb, see the comment there) and pc_tile_cheb (mass_tile_kernels.hip).  Device code only:
// include after <hip/hip_runtime.h>.
//
// The functions state the rounding sequence: contraction is off inside them and every fused step
// is a __builtin_fma, so the chain is the source's and not the compiler's choice.  It is candidate
// "ff" of both modes in tests/rowstep_ref.py, pinned bit for bit per launch by
// tests/test_gpu_row_steps.py for pc_rows, pc_row_step, pc_rows_shared<W>, pc_rows_shared_g and
// pc_rows_il<8 | 4>; the other forms (row programs, tile and mass-tile kernels) are held to those
// launches bit for bit by the sweep-form, mass-tile and coarse-ring tests.
//   EPI_CHEB  v = fl(c1 pkm1)                     (0 without pkm1)
//             v = fma(c2, pk, v)                  (with pk)
//             v = fma(c3, fl(dinv fl(b - acc)), v)
//             y = fl(post2 fl(post1 v))
//   EPI_LIN   v = fl(ca acc);  v = fma(cy, yin, v) (with yin);  v = fma(cz, z, v) (with z)
//             y2 = fl(c3 fl(dinv y))
// Without pkm1 the first fma adds to +0.0 -- it is not a product: fma(c, x, +0.0) and fl(c x)
// differ for a product of -0.  Masks, the malpha*mx value of masked linear rows, loads, stores and
// granule packing belong to the kernels, as do per-level post factors and `last ? post : 1.0`.
#pragma once

namespace kkt {

// One Chebyshev step of a row: post2 (post1 (c1 p_{k-1} + c2 p_k + c3 dinv (b - acc))).
// has_old / has_new: p_{k-1} / p_k take part (steps 1 and 2 of a solve lack them).
__device__ __forceinline__ double epi_cheb(const bool has_old, const double c1, const double p0,
                                           const bool has_new, const double c2, const double p1,
                                           const double c3, const double dinv, const double b,
                                           const double acc, const double q1, const double q2) {
#pragma clang fp contract(off)
    double t = has_old ? c1 * p0 : 0.0;
    if (has_new) t = __builtin_fma(c2, p1, t);
    t = __builtin_fma(c3, dinv * (b - acc), t);
    return q2 * (q1 * t);
}

// The linear update of a row: ca acc + cy yin + cz z.
__device__ __forceinline__ double epi_lin(const double ca, const double acc, const bool has_yin,
                                          const double cy, const double yin, const bool has_z,
                                          const double cz, const double z) {
#pragma clang fp contract(off)
    double v = ca * acc;
    if (has_yin) v = __builtin_fma(cy, yin, v);
    if (has_z) v = __builtin_fma(cz, z, v);
    return v;
}

// The first Chebyshev step fused into an update: p_1 = c3 D^-1 y on the row y just formed.
__device__ __forceinline__ double epi_first(const double c3, const double dinv, const double y) {
#pragma clang fp contract(off)
    return c3 * (dinv * y);
}

}  // namespace kkt
