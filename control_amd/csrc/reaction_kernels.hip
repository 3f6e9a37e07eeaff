// Kernels of the scalar reaction re-linearisation (reaction.hpp): element matrices (P1 triangles
// and tetrahedra, P2 triangles, Q2 quadrilaterals) of a polynomial reaction coefficient, the Picard residual of the heat-type optimality system (and of
// the stationary one, n_t == 1), its Crank-Nicolson right-hand side and the update of the iterate.
// gfx950, wave64; every store is a plain vector store, and no floating-point atomics: every sum
// runs in a fixed order.  Gather and composition are relin_kernels.hip's.
#include <hip/hip_runtime.h>

#include "reaction.hpp"

namespace kkt {

constexpr int REACTION_ELEMENT_BLOCKS = 1024;   // grid caps: the rest is grid-stride
constexpr int REACTION_ROW_BLOCKS = 512;
constexpr int REACTION_VECTOR_BLOCKS = 256 * 8;

// One thread per (element, level): E[a][b] = sum_q (W_eq g(s_q)) lam_qa lam_qb with
// s_q = lam_q0 v_0 + lam_q1 v_1 + lam_q2 v_2 summed left to right, g by Horner from c[degree]
// down, q ascending from 0.0 (fem.ReactionTerm.element_matrices on the host).  `contract(off)`
// keeps every product and sum a rounding of its own: hipcc contracts by default.
__global__ __launch_bounds__(256) void reaction_elements_kernel(
    const double *__restrict__ v, int64_t ne, int64_t n1, int n_t,
    const int32_t *__restrict__ cells, const double *__restrict__ W,
    const double *__restrict__ lam, ReactionCoef C, double *__restrict__ E) {
    const int64_t total = ne * n_t;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int64_t l = t / ne, e = t - l * ne;
        const double *vl = v + l * n1;
        const double v0 = vl[cells[e * 3]], v1 = vl[cells[e * 3 + 1]], v2 = vl[cells[e * 3 + 2]];
        double acc[RELIN_EP];
#pragma unroll
        for (int k = 0; k < RELIN_EP; ++k) acc[k] = 0.0;
#pragma unroll
        for (int q = 0; q < RELIN_NQ; ++q) {
            const double l0 = lam[q * 3], l1 = lam[q * 3 + 1], l2 = lam[q * 3 + 2];
            const double p0 = l0 * v0, p1 = l1 * v1, p2 = l2 * v2;
            const double s01 = p0 + p1;
            const double s = s01 + p2;
            double g = C.c[C.degree];
            for (int k = C.degree - 1; k >= 0; --k) {
                const double gs = g * s;
                g = gs + C.c[k];
            }
            const double wg = W[e * RELIN_NQ + q] * g;
            const double la[3] = {l0, l1, l2};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double wa = wg * la[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const double term = wa * la[b];
                    acc[a * 3 + b] = acc[a * 3 + b] + term;
                }
            }
        }
        double *o = E + t * RELIN_EP;
#pragma unroll
        for (int k = 0; k < RELIN_EP; ++k) o[k] = acc[k];
    }
}

constexpr int TET_NV = 4;     // nodes of a tetrahedron
constexpr int TET_NQ = 15;    // Stroud's T3:5-1
constexpr int TET_EP = 16;    // entries of its element matrix

// The same statement on P1 tetrahedra: s_q = ((lam_q0 v_0 + lam_q1 v_1) + lam_q2 v_2) + lam_q3 v_3
// over the 15 points of Stroud's T3:5-1, W_eq = wq_q volume_e, all 16 entries on their own
// ((wg la) lb and (wg lb) la round differently).  The 15 x 4 table is uniform over the wave: through
// const __restrict__ it comes by scalar loads into SGPRs and costs no vector register.  One thread
// owns the 128 contiguous bytes of its element matrix and writes them as eight 16-byte stores
// (E is 256-byte aligned and every matrix starts at a multiple of 128 bytes).
__global__ __launch_bounds__(256) void reaction_elements_tet_kernel(
    const double *__restrict__ v, int64_t ne, int64_t n1, int n_t,
    const int32_t *__restrict__ cells, const double *__restrict__ W,
    const double *__restrict__ lam, ReactionCoef C, double *__restrict__ E) {
    const int64_t total = ne * n_t;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int64_t l = t / ne, e = t - l * ne;
        const double *vl = v + l * n1;
        const int32_t *ce = cells + e * TET_NV;
        const double v0 = vl[ce[0]], v1 = vl[ce[1]], v2 = vl[ce[2]], v3 = vl[ce[3]];
        double acc[TET_EP];
#pragma unroll
        for (int k = 0; k < TET_EP; ++k) acc[k] = 0.0;
        // three rounds of five points: a full unroll hoists all 60 table entries out of the
        // grid-stride loop, 120 SGPRs, and spills 74 of them into vector lanes (100 VGPRs)
#pragma unroll 5
        for (int q = 0; q < TET_NQ; ++q) {
            const double la[TET_NV] = {lam[q * TET_NV], lam[q * TET_NV + 1], lam[q * TET_NV + 2],
                                       lam[q * TET_NV + 3]};
            const double p0 = la[0] * v0, p1 = la[1] * v1, p2 = la[2] * v2, p3 = la[3] * v3;
            const double s01 = p0 + p1;
            const double s012 = s01 + p2;
            const double s = s012 + p3;
            double g = C.c[C.degree];
            for (int k = C.degree - 1; k >= 0; --k) {
                const double gs = g * s;
                g = gs + C.c[k];
            }
            const double wg = W[e * TET_NQ + q] * g;
#pragma unroll
            for (int a = 0; a < TET_NV; ++a) {
                const double wa = wg * la[a];
#pragma unroll
                for (int b = 0; b < TET_NV; ++b) {
                    const double term = wa * la[b];
                    acc[a * TET_NV + b] = acc[a * TET_NV + b] + term;
                }
            }
        }
        double2 *o = reinterpret_cast<double2 *>(E + t * TET_EP);
#pragma unroll
        for (int k = 0; k < TET_EP / 2; ++k) o[k] = make_double2(acc[2 * k], acc[2 * k + 1]);
    }
}

constexpr int P2_NV = 6;      // nodes of a P2 triangle: three vertices, three edge midpoints
constexpr int P2_NQ = 25;     // the 5 x 5 conical product rule, degree 9
constexpr int P2_EP = 36;     // entries of its element matrix

// The same statement on P2 triangles: `phi` holds the 25 x 6 values of the shape functions at the
// points of the conical rule (they are no longer the barycentric coordinates),
// s_q = ((((phi_q0 v_0 + phi_q1 v_1) + phi_q2 v_2) + phi_q3 v_3) + phi_q4 v_4) + phi_q5 v_5,
// W_eq = wq_q area_e, all 36 entries on their own.  One thread per (element, level) keeps the 36
// sums in registers; the table is uniform over the wave and comes by scalar loads.  One thread
// owns the 288 contiguous bytes of its element matrix (288 = 18 x 16 and E is 256-byte aligned,
// so every matrix starts at a multiple of 16 bytes) and writes them as eighteen 16-byte stores.
__global__ __launch_bounds__(256) void reaction_elements_p2_kernel(
    const double *__restrict__ v, int64_t ne, int64_t n1, int n_t,
    const int32_t *__restrict__ cells, const double *__restrict__ W,
    const double *__restrict__ phi, ReactionCoef C, double *__restrict__ E) {
    const int64_t total = ne * n_t;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int64_t l = t / ne, e = t - l * ne;
        const double *vl = v + l * n1;
        const int32_t *ce = cells + e * P2_NV;
        double vn[P2_NV];
#pragma unroll
        for (int k = 0; k < P2_NV; ++k) vn[k] = vl[ce[k]];
        double acc[P2_EP];
#pragma unroll
        for (int k = 0; k < P2_EP; ++k) acc[k] = 0.0;
        // five rounds of five points, 30 table entries (60 SGPRs) a round: 104 SGPRs, 115 VGPRs,
        // no scratch, four waves per SIMD.  A full unroll wants all 150 entries at once and
        // spills 282 SGPRs into vector lanes (185 VGPRs, two waves); one point a round needs
        // 56 SGPRs and 100 VGPRs, with a wait for scalar loads in each of 25 rounds (not timed)
#pragma unroll 5
        for (int q = 0; q < P2_NQ; ++q) {
            double pa[P2_NV];
#pragma unroll
            for (int k = 0; k < P2_NV; ++k) pa[k] = phi[q * P2_NV + k];
            double s = pa[0] * vn[0];
#pragma unroll
            for (int k = 1; k < P2_NV; ++k) {
                const double p = pa[k] * vn[k];
                s = s + p;
            }
            double g = C.c[C.degree];
            for (int k = C.degree - 1; k >= 0; --k) {
                const double gs = g * s;
                g = gs + C.c[k];
            }
            const double wg = W[e * P2_NQ + q] * g;
#pragma unroll
            for (int a = 0; a < P2_NV; ++a) {
                const double wa = wg * pa[a];
#pragma unroll
                for (int b = 0; b < P2_NV; ++b) {
                    const double term = wa * pa[b];
                    acc[a * P2_NV + b] = acc[a * P2_NV + b] + term;
                }
            }
        }
        double2 *o = reinterpret_cast<double2 *>(E + t * P2_EP);
#pragma unroll
        for (int k = 0; k < P2_EP / 2; ++k) o[k] = make_double2(acc[2 * k], acc[2 * k + 1]);
    }
}

constexpr int Q2_NV = 9;      // nodes of a Q2 quadrilateral: 3 j + i, i along x, j along y
constexpr int Q2_NQ = 25;     // the 5 x 5 Gauss-Legendre product rule, degree 9 per variable
constexpr int Q2_EP = 81;     // entries of its element matrix

// The same statement on Q2 quadrilaterals: `phi` holds the 25 x 9 values of the tensor-product
// shape functions at the points, s_q is summed left to right over the nine nodes, W_eq = wq_q
// hx hy, all 81 entries on their own.  81 sums are 162 VGPRs, so three lanes share one (element,
// level): lane t works on pair t / 3 and owns the rows part, part + 3, part + 6 with part = t % 3
// -- 27 sums.  Every lane recomputes s_q, g and W g (about 25 operations a point against 57 of
// its own); every entry is still ((W g) phi_qa) phi_qb summed over q ascending, so the bits do
// not depend on the split.  The nine phi_q. of s_q and of the columns are uniform over the wave
// and come by scalar loads, one point a round (18 SGPRs; P2's rounds of five points would be 90
// and spill); the three phi_qa of the lane's own rows depend on the lane and are read from a copy
// of the table in LDS (1800 bytes, three addresses a wave).
//
// The stores are staged through LDS: a lane's piece of E is only 8-byte aligned (648 bytes a
// matrix), and written directly a store is 64 pieces of 8 bytes 216 bytes apart -- 42 M requests
// for the 340 MB of 128^2 cells x 32 levels, which bound the kernel (profiles/
// reaction_picard_q2.md).  In round r the three lanes of a pair hold the rows 3r, 3r + 1, 3r + 2:
// 27 contiguous doubles.  Each round the wave lays its 64 x 9 values into its own 4608 bytes of
// LDS (slot 9 lane + c) and reads them back slot j 64 + lane, j = 0 .. 8: a store then covers 64
// consecutive slots, which are runs of 216 contiguous bytes of E (slot f belongs to lane-item
// tt = t0 + f / 9, pair tt / 3, and sits at 81 pair + 27 r + 9 (tt % 3) + f % 9 = 9 tt + 54 pair
// + 27 r + f % 9).  The loop bound is uniform over the block (the barriers); lanes past the end
// work on the last lane-item and store nothing.
__global__ __launch_bounds__(256) void reaction_elements_q2_kernel(
    const double *__restrict__ v, int64_t ne, int64_t n1, int n_t,
    const int32_t *__restrict__ cells, const double *__restrict__ W,
    const double *__restrict__ phi, ReactionCoef C, double *__restrict__ E) {
    constexpr int PARTS = 3, ROWS = 3, OWN = ROWS * Q2_NV;
    __shared__ double table[Q2_NQ * Q2_NV];
    __shared__ double stage[256 * Q2_NV];
    for (int k = threadIdx.x; k < Q2_NQ * Q2_NV; k += blockDim.x) table[k] = phi[k];
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x - lane;
    double *mine = stage + wave0 * Q2_NV;
    const int64_t total = ne * n_t * PARTS;
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < total;
         base += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int64_t t = min(base + threadIdx.x, total - 1);
        const int64_t pair = t / PARTS;
        const int part = (int)(t - pair * PARTS);
        const int64_t l = pair / ne, e = pair - l * ne;
        const double *vl = v + l * n1;
        const int32_t *ce = cells + e * Q2_NV;
        double vn[Q2_NV];
#pragma unroll
        for (int k = 0; k < Q2_NV; ++k) vn[k] = vl[ce[k]];
        double acc[OWN];
#pragma unroll
        for (int k = 0; k < OWN; ++k) acc[k] = 0.0;
        __syncthreads();          // the table stands; the last round's slots have been read
        const double *own = table + part;
#pragma unroll 1
        for (int q = 0; q < Q2_NQ; ++q) {
            double pa[Q2_NV];
#pragma unroll
            for (int k = 0; k < Q2_NV; ++k) pa[k] = phi[q * Q2_NV + k];
            double s = pa[0] * vn[0];
#pragma unroll
            for (int k = 1; k < Q2_NV; ++k) {
                const double p = pa[k] * vn[k];
                s = s + p;
            }
            double g = C.c[C.degree];
            for (int k = C.degree - 1; k >= 0; --k) {
                const double gs = g * s;
                g = gs + C.c[k];
            }
            const double wg = W[e * Q2_NQ + q] * g;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const double wa = wg * own[q * Q2_NV + PARTS * r];
#pragma unroll
                for (int b = 0; b < Q2_NV; ++b) {
                    const double term = wa * pa[b];
                    acc[r * Q2_NV + b] = acc[r * Q2_NV + b] + term;
                }
            }
        }
        // the wave's first lane-item t0 = 3 p0 + m0: slot f is at o + 9 d + 54 ((m0 + d) / 3)
        // + 27 r + f % 9 with d = f / 9 and o = E + 9 t0 + 54 p0, and is live for d < live
        const int64_t t0 = base + wave0, p0 = t0 / PARTS;
        const int m0 = (int)(t0 - p0 * PARTS);
        const int live = (int)min((int64_t)64, total - t0);
        double *o = E + 9 * t0 + 54 * p0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (r) __syncthreads();
#pragma unroll
            for (int c = 0; c < Q2_NV; ++c) mine[lane * Q2_NV + c] = acc[r * Q2_NV + c];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < Q2_NV; ++j) {
                const int f = j * 64 + lane, d = f / Q2_NV;
                if (d < live) o[9 * d + 54 * ((m0 + d) / PARTS) + 27 * r + f % Q2_NV] = mine[f];
            }
        }
    }
}

// The kernels' levels are those of the D window: v is passed from the slot of level D_l0 (a time
// shard's v window may start one level below), n_t is D_n.  One rank: the base 0, every level.
void launch_reaction_elements(hipStream_t s, const ReactionPlan &P) {
    const dim3 grid(grid_of(P.ne * P.w.D_n, REACTION_ELEMENT_BLOCKS));
    const double *v = P.d_v + (int64_t)(P.w.D_l0 - P.w.v_l0) * P.n1;
    if (P.nv == Q2_NV)
        hipLaunchKernelGGL(reaction_elements_q2_kernel,
                           dim3(grid_of(P.ne * P.w.D_n * 3, REACTION_ELEMENT_BLOCKS)), dim3(256),
                           0, s, v, P.ne, P.n1, P.w.D_n, P.d_cells, P.d_W, P.d_lam, P.coef, P.d_E);
    else if (P.nv == P2_NV)
        hipLaunchKernelGGL(reaction_elements_p2_kernel, grid, dim3(256), 0, s, v, P.ne, P.n1,
                           P.w.D_n, P.d_cells, P.d_W, P.d_lam, P.coef, P.d_E);
    else if (P.nv == TET_NV)
        hipLaunchKernelGGL(reaction_elements_tet_kernel, grid, dim3(256), 0, s, v, P.ne, P.n1,
                           P.w.D_n, P.d_cells, P.d_W, P.d_lam, P.coef, P.d_E);
    else
        hipLaunchKernelGGL(reaction_elements_kernel, grid, dim3(256), 0, s, v, P.ne, P.n1,
                           P.w.D_n, P.d_cells, P.d_W, P.d_lam, P.coef, P.d_E);
}

// sum_k A[k] x[col[k]] over CSR row r from 0.0 in stored order (tperm: the transposed matrix on
// the symmetric pattern) -- SciPy's order for A @ x and A.T @ x
__device__ inline double reaction_row(const int32_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                      const double *__restrict__ A,
                                      const int32_t *__restrict__ tperm, int64_t r,
                                      const double *__restrict__ x) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int32_t k = ip[r]; k < ip[r + 1]; ++k) {
        const double p = (tperm ? A[tperm[k]] : A[k]) * x[ix[k]];
        acc = acc + p;
    }
    return acc;
}

// M @ (x + y): the vectors are added first, as the host does
__device__ inline double reaction_row_sum(const int32_t *__restrict__ ip,
                                          const int32_t *__restrict__ ix,
                                          const double *__restrict__ A, int64_t r,
                                          const double *__restrict__ x,
                                          const double *__restrict__ y) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int32_t k = ip[r]; k < ip[r + 1]; ++k) {
        const double xy = x[ix[k]] + y[ix[k]];
        const double p = A[k] * xy;
        acc = acc + p;
    }
    return acc;
}

struct ReactionArgs {
    const int32_t *ip, *ix, *tperm;
    const double *M, *D, *data, *v, *zeta;
    const uint8_t *bc;
    int64_t n1, nnz;
    // Level windows of a time shard: the rank owns the block rows [lo, lo + nl) of both families
    // (data and the residual: local row blocks f nl + i - lo); v, zeta and D start at the global
    // levels v_l0, z_l0 and D_l0.  n_t is global, and so are the stencil's guards.
    int n_t, cn, lo, nl, v_l0, z_l0, D_l0;
    double tau, beta;
};

// One thread per (row block, dof): local row blocks 0..nl-1 are the adjoint rows r0 of the blocks
// lo.., nl..2nl-1 the state rows r1 of Instationary.non_linear_res_eval, with its bracketing;
// Dirichlet rows are zero.  i: the global block row.
__global__ __launch_bounds__(256) void reaction_residual_kernel(ReactionArgs A,
                                                                double *__restrict__ r) {
    const int rb = blockIdx.y, fam = rb >= A.nl, i = A.lo + (fam ? rb - A.nl : rb);
    for (int64_t R = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; R < A.n1;
         R += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        double out = 0.0;
        if (!A.bc[R]) {
            auto Mx = [&](const double *x) { return reaction_row(A.ip, A.ix, A.M, nullptr, R, x); };
            auto Dx = [&](int l, const double *x) {
                return reaction_row(A.ip, A.ix, A.D + (int64_t)(l - A.D_l0) * A.nnz, nullptr, R, x);
            };
            auto DTx = [&](int l, const double *x) {
                return reaction_row(A.ip, A.ix, A.D + (int64_t)(l - A.D_l0) * A.nnz, A.tperm, R, x);
            };
            // global level l of v and zeta: its slot in the window
            auto v = [&](int l) { return A.v + (int64_t)(l - A.v_l0) * A.n1; };
            auto z = [&](int l) { return A.zeta + (int64_t)(l - A.z_l0) * A.n1; };
            const double tau = A.tau, d = A.data[(int64_t)rb * A.n1 + R];
            if (!A.cn) {
                if (!fam) {
                    const double tDz = tau * DTx(i, z(i));
                    const double Dz = tDz + Mx(z(i));
                    if (i < A.n_t - 1) {
                        const double tMv = tau * Mx(v(i));
                        const double a = d - tMv;
                        const double b = a - Dz;
                        out = b + Mx(z(i + 1));
                    } else {
                        out = -Dz;
                    }
                } else {
                    const double tDv = tau * Dx(i, v(i));
                    const double Dv = tDv + Mx(v(i));
                    if (i == 0) {
                        out = d - Dv;
                    } else {
                        const double a = d + Mx(v(i - 1));
                        const double b = a - Dv;
                        const double c = (tau / A.beta) * Mx(z(i));
                        out = b + c;
                    }
                }
            } else {
                const double h = 0.5 * tau;
                if (!fam) {
                    const double hMv = h * reaction_row_sum(A.ip, A.ix, A.M, R, v(i), v(i + 1));
                    const double a = d - hMv;
                    const double hD0 = h * DTx(i, z(i));
                    const double t0 = hD0 + Mx(z(i));
                    const double b = a - t0;
                    const double hD1 = h * DTx(i + 1, z(i + 1));
                    const double t1 = hD1 - Mx(z(i + 1));
                    out = b - t1;
                } else {
                    const double hD0 = h * Dx(i, v(i));
                    const double t0 = hD0 - Mx(v(i));
                    const double a = d - t0;
                    const double hD1 = h * Dx(i + 1, v(i + 1));
                    const double t1 = hD1 + Mx(v(i + 1));
                    const double b = a - t1;
                    const double c =
                        (h / A.beta) * reaction_row_sum(A.ip, A.ix, A.M, R, z(i), z(i + 1));
                    out = b + c;
                }
            }
        }
        r[(int64_t)rb * A.n1 + R] = out;
    }
}

void launch_reaction_residual(hipStream_t s, const ReactionPlan &P, double *d_r) {
    ReactionArgs A;
    A.ip = P.d_ip; A.ix = P.d_ix; A.tperm = P.d_tperm;
    A.M = P.d_M; A.D = P.d_D; A.data = P.d_data; A.v = P.d_v; A.zeta = P.d_zeta; A.bc = P.d_bc;
    A.n1 = P.n1; A.nnz = P.nnz; A.n_t = P.w.n_t; A.cn = P.w.CN;
    A.lo = P.w.lo; A.nl = P.w.nl; A.v_l0 = P.w.v_l0; A.z_l0 = P.w.z_l0; A.D_l0 = P.w.D_l0;
    A.tau = P.tau; A.beta = P.beta;
    hipLaunchKernelGGL(reaction_residual_kernel,
                       dim3(grid_of(P.n1, REACTION_ROW_BLOCKS), 2 * P.w.nl), dim3(256), 0, s, A,
                       d_r);
}

struct StationaryArgs {
    const int32_t *ip, *ix, *tperm;
    const double *M, *D, *data, *v, *zeta;
    const uint8_t *bc;
    int64_t n1;
    double ib;   // 1.0 / beta, rounded once on the host
};

// The stationary system (n_t == 1): one thread per (family, dof).  Family 0 is the adjoint row
// r0 = (d0 - M v) - D^T zeta, family 1 the state row r1 = (d1 - D v) + ib (M zeta) of
// Stationary.non_linear_res_eval, with its bracketing; Dirichlet rows are zero.
__global__ __launch_bounds__(256) void reaction_stationary_residual_kernel(
    StationaryArgs A, double *__restrict__ r) {
    const int fam = blockIdx.y;
    for (int64_t R = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; R < A.n1;
         R += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        double out = 0.0;
        if (!A.bc[R]) {
            const double d = A.data[(int64_t)fam * A.n1 + R];
            if (!fam) {
                const double a = d - reaction_row(A.ip, A.ix, A.M, nullptr, R, A.v);
                out = a - reaction_row(A.ip, A.ix, A.D, A.tperm, R, A.zeta);
            } else {
                const double a = d - reaction_row(A.ip, A.ix, A.D, nullptr, R, A.v);
                const double c = A.ib * reaction_row(A.ip, A.ix, A.M, nullptr, R, A.zeta);
                out = a + c;
            }
        }
        r[(int64_t)fam * A.n1 + R] = out;
    }
}

void launch_reaction_stationary_residual(hipStream_t s, const ReactionPlan &P, double *d_r) {
    StationaryArgs A;
    A.ip = P.d_ip; A.ix = P.d_ix; A.tperm = P.d_tperm;
    A.M = P.d_M; A.D = P.d_D; A.data = P.d_data; A.v = P.d_v; A.zeta = P.d_zeta; A.bc = P.d_bc;
    A.n1 = P.n1;
    A.ib = 1.0 / P.beta;
    hipLaunchKernelGGL(reaction_stationary_residual_kernel,
                       dim3(grid_of(P.n1, REACTION_ROW_BLOCKS), 2), dim3(256), 0, s, A, d_r);
}

// Crank-Nicolson: T_1 on the adjoint rows (row i + 1 into i), T_2 on the state rows (i - 1 into i).
// r holds the rank's 2 nl row blocks; where i + 1 or i - 1 leaves the shard the term is the
// neighbour rank's raw row (h_up: adjoint row hi, h_dn: state row lo - 1; ReactionPlan::d_rhalo).
// The guards are those of the global system; one rank never reads a halo.
__global__ __launch_bounds__(256) void reaction_rhs_kernel(const double *__restrict__ r,
                                                           double *__restrict__ b, int m, int lo,
                                                           int nl, int64_t n1,
                                                           const double *__restrict__ h_up,
                                                           const double *__restrict__ h_dn) {
    const int64_t n = 2 * (int64_t)nl * n1;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rb = t / n1, R = t - rb * n1;
        double out = r[t];
        if (rb < nl) {
            if (lo + rb + 1 < m) out += rb + 1 < nl ? r[t + n1] : h_up[R];
        } else if (lo + rb - nl > 0) {
            out += rb > nl ? r[t - n1] : h_dn[R];
        }
        b[t] = out;
    }
}

void launch_reaction_rhs(hipStream_t s, const ReactionPlan &P, const double *d_r, double *d_b) {
    const int64_t n = 2 * (int64_t)P.w.nl * P.n1;
    hipLaunchKernelGGL(reaction_rhs_kernel, dim3(grid_of(n, REACTION_VECTOR_BLOCKS)),
                       dim3(256), 0, s, d_r, d_b, P.w.m, P.w.lo, P.w.nl, P.n1, P.d_rhalo,
                       P.d_rhalo ? P.d_rhalo + P.n1 : nullptr);
}

// Unknown block i: v at level i (Crank-Nicolson: i + 1), zeta at level i.  v keeps its boundary
// values on the Dirichlet dofs, zeta is zero there.  The kernel's block rows are the rank's own:
// v and zeta are passed from the slot of level lo.  z_halo: the level after the owned ones is the
// neighbour's zeta (a time shard); it is zeroed on the Dirichlet dofs like the owned levels, and
// refreshed by the next exchange.  (CN's fixed last level is nobody's block: it is left alone.)
__global__ __launch_bounds__(256) void reaction_update_kernel(double *__restrict__ u,
                                                              double *__restrict__ v,
                                                              double *__restrict__ zeta,
                                                              const uint8_t *__restrict__ bc, int m,
                                                              int64_t n1, int cn, int z_halo) {
    const int64_t n0 = (int64_t)m * n1, n = 2 * n0, all = n + (z_halo ? n1 : 0);
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < all;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rb = t / n1, R = t - rb * n1;
        const bool fixed = bc[R] != 0;
        if (t >= n) {
            if (fixed) zeta[(int64_t)m * n1 + R] = 0.0;
            continue;
        }
        if (rb < m) {
            if (!fixed) v[(rb + cn) * n1 + R] += u[t];
        } else {
            const int64_t at = (rb - m) * n1 + R;
            zeta[at] = fixed ? 0.0 : zeta[at] + u[t];
        }
        u[t] = 0.0;   // consumed: the next solve starts from zero
    }
}

void launch_reaction_update(hipStream_t s, const ReactionPlan &P, double *d_u) {
    const int64_t n = (2 * (int64_t)P.w.nl + (int)P.w.z_halo) * P.n1;
    hipLaunchKernelGGL(reaction_update_kernel, dim3(grid_of(n, REACTION_VECTOR_BLOCKS)),
                       dim3(256), 0, s, d_u, P.d_v + (int64_t)(P.w.lo - P.w.v_l0) * P.n1,
                       P.d_zeta + (int64_t)(P.w.lo - P.w.z_l0) * P.n1, P.d_bc, P.w.nl, P.n1,
                       (int)P.w.CN, (int)P.w.z_halo);
}

}  // namespace kkt
