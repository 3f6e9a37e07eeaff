// Device re-linearisation kernels (relin.hpp): P2-P1 convection element matrices, their
// deterministic gather into stored positions, composition into SELL block values, the Picard
// residual and the update.  gfx950, wave64; every store is a plain vector store, and no
// floating-point atomics: every sum runs in a fixed order.
#include <hip/hip_runtime.h>

#include "relin.hpp"

namespace kkt {

// One thread per (element, level): the velocity element matrix
//   N[a][b] = sum_q W_eq phi_qa (w_q . grad phi_eqb)
// and the pressure one  sum_q W_eq lam_qc (w_q . grad lam_ed)  (fem.py convection_v_data /
// convection_p), w_q the P2 wind (component-major) at the quadrature point.
__global__ __launch_bounds__(256) void relin_elements_kernel(
    const double *__restrict__ vlev, int64_t ne, int64_t n2, int n_t,
    const int32_t *__restrict__ V, const double *__restrict__ W, const double *__restrict__ phi,
    const double *__restrict__ gphi, const double *__restrict__ lam,
    const double *__restrict__ glam, double *__restrict__ Ev, double *__restrict__ Ep) {
    const int64_t total = ne * n_t;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = t / ne, e = t - l * ne;
        const double *w = vlev + l * 2 * n2;
        double wx[6], wy[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int32_t node = V[e * 6 + a];
            wx[a] = w[node];
            wy[a] = w[n2 + node];
        }
        double gl[3][2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gl[c][0] = glam[e * 6 + c * 2];
            gl[c][1] = glam[e * 6 + c * 2 + 1];
        }
        double Nv[6][6], Np[3][3];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) Nv[a][b] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) Np[c][d] = 0.0;
        for (int q = 0; q < RELIN_NQ; ++q) {
            double qx = 0.0, qy = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                qx += wx[a] * phi[q * 6 + a];
                qy += wy[a] * phi[q * 6 + a];
            }
            const double wq = W[e * RELIN_NQ + q];
            const double *g = gphi + (e * RELIN_NQ + q) * 12;
            double adv[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) adv[b] = g[2 * b] * qx + g[2 * b + 1] * qy;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double s = wq * phi[q * 6 + a];
#pragma unroll
                for (int b = 0; b < 6; ++b) Nv[a][b] += s * adv[b];
            }
            double advp[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) advp[d] = gl[d][0] * qx + gl[d][1] * qy;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = wq * lam[q * 3 + c];
#pragma unroll
                for (int d = 0; d < 3; ++d) Np[c][d] += s * advp[d];
            }
        }
        double *ov = Ev + t * RELIN_EV;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; b += 2)
                *reinterpret_cast<double2 *>(ov + a * 6 + b) = make_double2(Nv[a][b], Nv[a][b + 1]);
        double *op = Ep + t * RELIN_EP;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) op[c * 3 + d] = Np[c][d];
    }
}

// a value that is the same in every lane of the wave, moved to scalar registers
__device__ inline int uniform32(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ inline int64_t uniform64(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

constexpr int Q2_KV = 9;      // nodes of a Q2 cell: 3 j + i, i along x, j along y
constexpr int Q2_KP = 4;      // nodes of a Q1 cell: 2 j + i
constexpr int Q2_NQ = 16;     // the 4 x 4 Gauss-Legendre product rule, degree 7 per variable
constexpr int Q2_EP = 16;     // entries of the pressure element matrix (the velocity one: 81)

// The same two element matrices on Q2-Q1 quadrilaterals (fem.py rectangle_q2q1):
//   Nv[a][b] = sum_q W_eq phi_qa (w_q . grad phi_eqb)   9 x 9
//   Np[c][d] = sum_q W_eq lam_qc (w_q . grad lam_eqd)   4 x 4
// with grad phi_eqb = gref_qb * jinv_e per component (one rounding, as the host forms its gphi),
// w_q the Q2 interpolant of the level's wind summed left to right over the nine nodes, every sum
// over q ascending from 0.0 and every entry ((W phi_qa) adv_b), so the bits do not depend on how
// the entries are split over lanes.
//
// The shape is that of reaction_elements_q2_kernel (reaction_kernels.hip): 81 sums are 162 VGPRs,
// so three lanes share one (element, level) pair: lane t works on pair t / 3 and owns the velocity
// rows part, part + 3, part + 6 with part = t % 3 -- 27 sums.  Every lane recomputes the wind at
// the point and the nine advections (72 operations a point against 30 of its own).  The pressure
// sums run in a second loop over the points, after the velocity rows have left for LDS: next to
// the 27 sums, the 18 nodal values of the wind and the nine advections they do not fit 168
// registers without scratch, and forming the wind 16 times more (18 fma each) costs less than a
// wave per SIMD.  Of the pressure matrix the lane owns row `part`, and all three lanes of a pair
// carry row 3 (four sums more than an even split would be, and no lane-dependent register index);
// lane 0's copy is the one stored.  The tables a point needs that are uniform over the wave
// (phi_q., gref_q.., lam_q3, lref_q..) come by scalar loads, one point a round; the values of the
// lane's own rows (phi_q,part+3r and lam_q,part) depend on the lane and are read from copies in
// LDS.  144 VGPRs, three waves per SIMD.
//
// Stores are staged through LDS so that a pair's 648 + 128 bytes leave in contiguous runs.  Ev:
// the rounds of reaction_elements_q2_kernel, word for word (in round r the three lanes of a pair
// hold the rows 3r, 3r + 1, 3r + 2: 27 contiguous doubles; the wave lays 64 x 9 values into its
// own 4608 bytes and reads them back slot j 64 + lane).  Ep: the block's lane-items cover the
// pairs from pb = base / 3 on; every lane lays its pressure rows at 16 (pair - pb) + 4 row of the
// same buffer (at most 86 pairs: 1376 of its 2304 slots), and slot f = 16 (pair - pb) + 4 c + d is
// stored by thread f % 256 if the lane-item that owns row c of that pair (3 pair + c, row 3:
// 3 pair) belongs to this block's round -- a block stores 16 consecutive doubles per pair, and the
// rows of a pair split between two blocks each leave with their owner.  The loop bound is uniform
// over the block (the barriers); lanes past the end work on the last lane-item and store nothing.
__global__ __launch_bounds__(256, 3) void relin_elements_q2q1_kernel(
    const double *__restrict__ vlev, int64_t ne, int64_t n2, int n_t,
    const int32_t *__restrict__ V, const double *__restrict__ W, const double *__restrict__ phi,
    const double *__restrict__ gref, const double *__restrict__ lam,
    const double *__restrict__ lref, const double *__restrict__ jinv, double *__restrict__ Ev,
    double *__restrict__ Ep) {
    constexpr int PARTS = 3, ROWS = 3, OWN = ROWS * Q2_KV;
    __shared__ double tphi[Q2_NQ * Q2_KV];
    __shared__ double tlam[Q2_NQ * Q2_KP];
    __shared__ double stage[256 * Q2_KV];
    for (int k = threadIdx.x; k < Q2_NQ * Q2_KV; k += blockDim.x) tphi[k] = phi[k];
    for (int k = threadIdx.x; k < Q2_NQ * Q2_KP; k += blockDim.x) tlam[k] = lam[k];
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x - lane;
    double *mine = stage + wave0 * Q2_KV;
    const int64_t total = ne * n_t * PARTS;
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < total;
         base += (int64_t)gridDim.x * blockDim.x) {
        // the block's first lane-item is the same in every lane: what follows from it (the
        // staging offsets, the pressure slots) stays in scalar registers
        const int64_t ub = uniform64(base);
        const int64_t t = min(ub + threadIdx.x, total - 1);
        const int64_t pair = t / PARTS;
        const int part = (int)(t - pair * PARTS);
        const int64_t l = pair / ne, e = pair - l * ne;
        const double *w = vlev + l * 2 * n2;
        const int32_t *ce = V + e * Q2_KV;
        double wx[Q2_KV], wy[Q2_KV];
#pragma unroll
        for (int k = 0; k < Q2_KV; ++k) {
            const int32_t node = ce[k];
            wx[k] = w[node];
            wy[k] = w[n2 + node];
        }
        const double jx = jinv[2 * e], jy = jinv[2 * e + 1];
        double acc[OWN];
#pragma unroll
        for (int k = 0; k < OWN; ++k) acc[k] = 0.0;
        __syncthreads();          // the tables stand; the last round's slots have been read
        const double *own = tphi + part, *ownp = tlam + part;
#pragma unroll 1
        for (int q = 0; q < Q2_NQ; ++q) {
            double qx = 0.0, qy = 0.0;
#pragma unroll
            for (int k = 0; k < Q2_KV; ++k) {
                const double p = phi[q * Q2_KV + k];
                qx += wx[k] * p;
                qy += wy[k] * p;
            }
            const double wq = W[e * Q2_NQ + q];
            double adv[Q2_KV];
#pragma unroll
            for (int b = 0; b < Q2_KV; ++b) {
                const double gx = gref[(q * Q2_KV + b) * 2] * jx;
                const double gy = gref[(q * Q2_KV + b) * 2 + 1] * jy;
                adv[b] = gx * qx + gy * qy;
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const double s = wq * own[q * Q2_KV + PARTS * r];
#pragma unroll
                for (int b = 0; b < Q2_KV; ++b) acc[r * Q2_KV + b] += s * adv[b];
            }
        }
        // Ev.  The wave's first lane-item t0 = 3 p0 + m0: slot f is at o + 9 d + 54 ((m0 + d) / 3)
        // + 27 r + f % 9 with d = f / 9 and o = Ev + 9 t0 + 54 p0, and is live for d < live
        // (the lane index is taken afresh: what the store rounds derive from it -- f / 9, f % 9 per
        // slot -- is otherwise kept in registers across the whole loop over the blocks' rounds)
        int ln = lane, tid = threadIdx.x;
        asm volatile("" : "+v"(ln), "+v"(tid));
        const int64_t t0 = ub + uniform32(wave0), p0 = t0 / PARTS;
        const int m0 = (int)(t0 - p0 * PARTS);
        const int live = (int)min((int64_t)64, total - t0);
        double *o = Ev + 9 * t0 + 54 * p0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (r) __syncthreads();
#pragma unroll
            for (int c = 0; c < Q2_KV; ++c) mine[ln * Q2_KV + c] = acc[r * Q2_KV + c];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < Q2_KV; ++j) {
                const int f = j * 64 + ln, d = f / Q2_KV;
                if (d < live) o[9 * d + 54 * ((m0 + d) / PARTS) + 27 * r + f % Q2_KV] = mine[f];
            }
        }
        // the pressure sums in a loop of their own, once the velocity sums have left the
        // registers: the wind at the point is formed again, in the same order
        double accp[2 * Q2_KP];
#pragma unroll
        for (int k = 0; k < 2 * Q2_KP; ++k) accp[k] = 0.0;
#pragma unroll 1
        for (int q = 0; q < Q2_NQ; ++q) {
            double qx = 0.0, qy = 0.0;
#pragma unroll
            for (int k = 0; k < Q2_KV; ++k) {
                const double p = phi[q * Q2_KV + k];
                qx += wx[k] * p;
                qy += wy[k] * p;
            }
            const double wq = W[e * Q2_NQ + q];
            double advp[Q2_KP];
#pragma unroll
            for (int d = 0; d < Q2_KP; ++d) {
                const double gx = lref[(q * Q2_KP + d) * 2] * jx;
                const double gy = lref[(q * Q2_KP + d) * 2 + 1] * jy;
                advp[d] = gx * qx + gy * qy;
            }
            const double sp = wq * ownp[q * Q2_KP], s3 = wq * lam[q * Q2_KP + 3];
#pragma unroll
            for (int d = 0; d < Q2_KP; ++d) {
                accp[d] += sp * advp[d];
                accp[Q2_KP + d] += s3 * advp[d];
            }
        }
        // Ep.  pb: the pair of the block's first lane-item; end: one past its last live one
        __syncthreads();
        const int64_t pb = ub / PARTS, end = min(ub + 256, total);
        if (ub + tid < total) {
            double *row = stage + (pair - pb) * Q2_EP;
#pragma unroll
            for (int d = 0; d < Q2_KP; ++d) row[part * Q2_KP + d] = accp[d];
            if (part == 0) {
#pragma unroll
                for (int d = 0; d < Q2_KP; ++d) row[3 * Q2_KP + d] = accp[Q2_KP + d];
            }
        }
        __syncthreads();
        const int nslots = (int)((end - 1) / PARTS - pb + 1) * Q2_EP;
        for (int f = tid; f < nslots; f += 256) {
            const int64_t pr = pb + f / Q2_EP;
            const int c = (f % Q2_EP) / Q2_KP;
            const int64_t owner = PARTS * pr + (c == 3 ? 0 : c);
            if (owner >= ub && owner < end) Ep[pb * Q2_EP + f] = stage[f];
        }
    }
}

// d_v: the v window; slot s of the D window takes its wind from level D_l0 + s of it
void launch_relin_elements(hipStream_t s, const RelinPlan &P, const double *d_v) {
    if (P.kv == Q2_KV) {
        hipLaunchKernelGGL(relin_elements_q2q1_kernel,
                           dim3(grid_of(P.ne * P.w.D_n * 3, 256 * 64)), dim3(256), 0, s,
                           d_v + (int64_t)(P.w.D_l0 - P.w.v_l0) * P.nv, P.ne, P.n2, P.w.D_n, P.d_V,
                           P.d_W, P.d_phi, P.d_gphi, P.d_lam, P.d_glam, P.d_jinv, P.d_Ev, P.d_Ep);
        return;
    }
    hipLaunchKernelGGL(relin_elements_kernel, dim3(grid_of(P.ne * P.w.D_n, 256 * 64)), dim3(256),
                       0, s, d_v + (int64_t)(P.w.D_l0 - P.w.v_l0) * P.nv, P.ne, P.n2, P.w.D_n,
                       P.d_V, P.d_W, P.d_phi, P.d_gphi, P.d_lam, P.d_glam, P.d_Ev, P.d_Ep);
}

// One thread per (stored position, level): the contributions in ascending element-entry order
// (np.bincount's order), then nu K + C with separate roundings (fem / picard D_v on the host).
// `contract(off)` is what keeps the product and the sum apart: hipcc contracts by default, and
// its __dmul_rn / __dadd_rn are plain operators that fuse into an fma like any others.
__global__ __launch_bounds__(256) void relin_gather_kernel(
    const int32_t *__restrict__ cptr, const int32_t *__restrict__ clist,
    const double *__restrict__ E, int64_t per_level, const double *__restrict__ K, double nu,
    int64_t nnz, int n_t, double *__restrict__ D) {
    const int64_t total = nnz * n_t;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int64_t l = t / nnz, k = t - l * nnz;
        const double *El = E + l * per_level;
        double acc = 0.0;
        for (int32_t j = cptr[k]; j < cptr[k + 1]; ++j) acc += El[clist[j]];
        const double nuK = nu * K[k];
        D[t] = nuK + acc;
    }
}

void launch_relin_gather(hipStream_t s, const RelinPlan &P) {
    hipLaunchKernelGGL(relin_gather_kernel, dim3(grid_of(P.nnz2 * P.w.D_n, 256 * 64)), dim3(256),
                       0, s, P.d_cptr2, P.d_clist2, P.d_Ev, P.ne * P.ev, P.d_K2, P.nu, P.nnz2,
                       P.w.D_n, P.d_D2);
    hipLaunchKernelGGL(relin_gather_kernel, dim3(grid_of(P.nnz1 * P.w.D_n, 256 * 64)), dim3(256),
                       0, s, P.d_cptrp, P.d_clistp, P.d_Ep, P.ne * P.ep, P.d_Kp, P.nu, P.nnz1,
                       P.w.D_n, P.d_Dp);
}

// the same kernel under the same grid rule for one pattern of another plan (reaction.cpp)
void launch_relin_gather_one(hipStream_t s, const int32_t *cptr, const int32_t *clist,
                             const double *E, int64_t per_level, const double *K, double nu,
                             int64_t nnz, int n_t, double *D) {
    hipLaunchKernelGGL(relin_gather_kernel, dim3(grid_of(nnz * n_t, 256 * 64)), dim3(256), 0, s,
                       cptr, clist, E, per_level, K, nu, nnz, n_t, D);
}

// blockIdx.y selects the target block; each SELL slot gets alpha D(^T) + gamma M (blocks.py
// _axpby: two products, one sum, kept apart by `contract(off)` as in the gather), Dirichlet
// columns zeroed as kkt_update_block_values does.
// alpha == 0 (uniform over the block: the job is read through the scalar path): the constant
// block gamma M (blocks.py `mass`: one product), D and the transpose permutation are not read.
__global__ __launch_bounds__(256) void relin_compose_kernel(const ComposeJob *__restrict__ jobs) {
    const ComposeJob J = jobs[blockIdx.y];
    const bool constant = J.alpha == 0.0;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < J.npadded;
         p += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const int32_t k = J.sell2csr[p];
        double v = 0.0;
        if (k >= 0) {
            const int64_t ks = k >= J.nnz_s ? k - J.nnz_s : k;
            if (constant) {
                v = J.gamma * J.M[ks];
            } else {
                const int64_t kd = J.tperm ? J.tperm[ks] : ks;
                const double aD = J.alpha * J.D[kd], gM = J.gamma * J.M[ks];
                v = aD + gM;
            }
            if (J.colmask && J.colmask[J.col[p]]) v = 0.0;
        }
        J.dst[p] = v;
    }
}

void launch_relin_compose(hipStream_t s, const ComposeJob *d_jobs, int njobs, int64_t max_padded) {
    if (njobs <= 0) return;
    hipLaunchKernelGGL(relin_compose_kernel, dim3(grid_of(max_padded, 256), njobs), dim3(256), 0,
                       s, d_jobs);
}

// sum_k A[k] x[off + col[k]] over CSR row r (tperm: the transposed matrix on a symmetric pattern)
__device__ inline double relin_row(const int32_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                   const double *__restrict__ A, const int32_t *__restrict__ tperm,
                                   int64_t r, const double *__restrict__ x) {
    double acc = 0.0;
    for (int32_t k = ip[r]; k < ip[r + 1]; ++k) acc += (tperm ? A[tperm[k]] : A[k]) * x[ix[k]];
    return acc;
}

struct RelinArgs {
    const int32_t *ip2, *ix2, *t2, *Bip, *Bix, *BTip, *BTix;
    const double *M2, *D2, *Bv, *BTv, *data, *v, *zeta, *p, *mu;
    const uint8_t *bc;
    int64_t n2, nv, n1, nnz2;
    // Level windows of a time shard: the rank owns the block rows [lo, lo + nl) of both families
    // (data, p, mu, the residual: local row blocks f nl + i - lo); v, zeta and D2 start at the
    // global levels v_l0, z_l0 and D_l0.  n_t and m are global, and so are the stencil's guards.
    int n_t, m, cn, lo, nl, v_l0, z_l0, D_l0;
    double tau, beta;
};

// Velocity rows (picard.non_linear_res_eval): one thread per (row block, dof).  Local row blocks
// 0..nl-1 are the adjoint rows (r00) of the blocks lo.., nl..2nl-1 the state rows (r01);
// Dirichlet rows are zero.  i: the global block row.
__global__ __launch_bounds__(256) void relin_residual_v_kernel(RelinArgs A, double *__restrict__ r) {
    const int rb = blockIdx.y, fam = rb >= A.nl, il = fam ? rb - A.nl : rb, i = A.lo + il;
    for (int64_t R = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; R < A.nv;
         R += (int64_t)gridDim.x * blockDim.x) {
        double out = 0.0;
        if (!A.bc[R]) {
            const int64_t c = R >= A.n2, row = R - c * A.n2, off = c * A.n2;
            auto Mx = [&](const double *lev) {
                return relin_row(A.ip2, A.ix2, A.M2, nullptr, row, lev + off);
            };
            auto Dx = [&](int l, const double *lev) {
                return relin_row(A.ip2, A.ix2, A.D2 + (l - A.D_l0) * A.nnz2, nullptr, row,
                                 lev + off);
            };
            auto DTx = [&](int l, const double *lev) {
                return relin_row(A.ip2, A.ix2, A.D2 + (l - A.D_l0) * A.nnz2, A.t2, row, lev + off);
            };
            auto BTx = [&](const double *lev) {
                return relin_row(A.BTip, A.BTix, A.BTv, nullptr, R, lev);
            };
            const int64_t nv = A.nv;
            // global level l of v and zeta: its slot in the window
            auto v = [&](int l) { return A.v + (l - A.v_l0) * nv; };
            auto z = [&](int l) { return A.zeta + (l - A.z_l0) * nv; };
            const double tau = A.tau, d = A.data[rb * nv + R];
            if (!A.cn) {
                if (!fam) {
                    const double Dz = tau * DTx(i, z(i)) + Mx(z(i));
                    out = d - Dz;
                    if (i < A.n_t - 1) out += -tau * Mx(v(i)) + Mx(z(i + 1));
                    out -= tau * BTx(A.mu + il * A.n1);
                } else {
                    const double Dv = tau * Dx(i, v(i)) + Mx(v(i));
                    out = d - Dv;
                    if (i >= 1) out += Mx(v(i - 1)) + (tau / A.beta) * Mx(z(i));
                    out -= tau * BTx(A.p + il * A.n1);
                }
            } else {
                const double h = 0.5 * tau;
                const double *v0 = v(i), *v1 = v(i + 1);
                const double *z0 = z(i), *z1 = z(i + 1);
                if (!fam) {
                    out = d - h * (Mx(v0) + Mx(v1)) - (h * DTx(i, z0) + Mx(z0)) -
                          (h * DTx(i + 1, z1) - Mx(z1)) - tau * BTx(A.mu + il * A.n1);
                } else {
                    out = d - (h * Dx(i, v0) - Mx(v0)) - (h * Dx(i + 1, v1) + Mx(v1)) +
                          (h / A.beta) * (Mx(z0) + Mx(z1)) - tau * BTx(A.p + il * A.n1);
                }
            }
        }
        r[rb * A.nv + R] = out;
    }
}

// Pressure rows: -B v (local row blocks 0..nl-1; CN: the level i + 1) and -B zeta.
__global__ __launch_bounds__(256) void relin_residual_p_kernel(RelinArgs A, double *__restrict__ r) {
    const int rb = blockIdx.y, fam = rb >= A.nl, i = A.lo + (fam ? rb - A.nl : rb);
    const double *x = fam ? A.zeta + (i - A.z_l0) * A.nv
                          : A.v + ((A.cn ? i + 1 : i) - A.v_l0) * A.nv;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < A.n1;
         q += (int64_t)gridDim.x * blockDim.x)
        r[rb * A.n1 + q] = -relin_row(A.Bip, A.Bix, A.Bv, nullptr, q, x);
}

static RelinArgs relin_args(const RelinPlan &P) {
    RelinArgs A;
    A.ip2 = P.d_ip2; A.ix2 = P.d_ix2; A.t2 = P.d_t2;
    A.Bip = P.d_Bip; A.Bix = P.d_Bix; A.BTip = P.d_BTip; A.BTix = P.d_BTix;
    A.M2 = P.d_M2; A.D2 = P.d_D2; A.Bv = P.d_Bv; A.BTv = P.d_BTv; A.data = P.d_data;
    A.v = P.d_v; A.zeta = P.d_zeta; A.p = P.d_p; A.mu = P.d_mu; A.bc = P.d_bc;
    A.n2 = P.n2; A.nv = P.nv; A.n1 = P.n1; A.nnz2 = P.nnz2;
    A.n_t = P.w.n_t; A.m = P.w.m; A.cn = P.w.CN;
    A.lo = P.w.lo; A.nl = P.w.nl; A.v_l0 = P.w.v_l0; A.z_l0 = P.w.z_l0; A.D_l0 = P.w.D_l0;
    A.tau = P.tau; A.beta = P.beta;
    return A;
}

void launch_relin_residual(hipStream_t s, const RelinPlan &P, double *d_r) {
    const RelinArgs A = relin_args(P);
    hipLaunchKernelGGL(relin_residual_v_kernel, dim3(grid_of(P.nv, 512), 2 * P.w.nl), dim3(256), 0,
                       s, A, d_r);
    hipLaunchKernelGGL(relin_residual_p_kernel, dim3(grid_of(P.n1, 512), 2 * P.w.nl), dim3(256), 0,
                       s, A, d_r + 2 * (int64_t)P.w.nl * P.nv);
}

// The stationary system (n_t == 1): one thread per (family, velocity dof), the velocity rows of
// Stationary.incompressible_non_linear_solve's evaluate() with its bracketing:
//   family 0 (adjoint)  ((d0 - M v) - D^T zeta) - B^T mu
//   family 1 (state)    ((d1 - D v) + ib (M zeta)) - B^T p
// ib = 1 / beta rounded once on the host; Dirichlet rows are zero.  These are not backward Euler's
// rows at n_t = 1: its last adjoint row drops M v, and its rows carry tau.
__global__ __launch_bounds__(256) void relin_stationary_residual_kernel(RelinArgs A, double ib,
                                                                        double *__restrict__ r) {
    const int fam = blockIdx.y;
    for (int64_t R = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; R < A.nv;
         R += (int64_t)gridDim.x * blockDim.x) {
        double out = 0.0;
        if (!A.bc[R]) {
            const int64_t c = R >= A.n2, row = R - c * A.n2, off = c * A.n2;
            const double d = A.data[fam * A.nv + R];
            if (!fam) {
                const double Mv = relin_row(A.ip2, A.ix2, A.M2, nullptr, row, A.v + off);
                const double DTz = relin_row(A.ip2, A.ix2, A.D2, A.t2, row, A.zeta + off);
                out = ((d - Mv) - DTz) - relin_row(A.BTip, A.BTix, A.BTv, nullptr, R, A.mu);
            } else {
                const double Dv = relin_row(A.ip2, A.ix2, A.D2, nullptr, row, A.v + off);
                const double Mz = relin_row(A.ip2, A.ix2, A.M2, nullptr, row, A.zeta + off);
                out = ((d - Dv) + ib * Mz) - relin_row(A.BTip, A.BTix, A.BTv, nullptr, R, A.p);
            }
        }
        r[fam * A.nv + R] = out;
    }
}

// the pressure rows -B v, -B zeta are relin_residual_p_kernel's with one block per family
void launch_relin_stationary_residual(hipStream_t s, const RelinPlan &P, double *d_r) {
    const RelinArgs A = relin_args(P);
    hipLaunchKernelGGL(relin_stationary_residual_kernel, dim3(grid_of(P.nv, 512), 2), dim3(256), 0,
                       s, A, 1.0 / P.beta, d_r);
    hipLaunchKernelGGL(relin_residual_p_kernel, dim3(grid_of(P.n1, 512), 2), dim3(256), 0, s, A,
                       d_r + 2 * P.nv);
}

// b from r: velocity rows as they are, pressure rows times tau; CN: T_1 on the adjoint rows and
// on the zeta pressure rows, T_2 on the state rows and the v pressure rows (picard.py).  r holds
// the rank's 2 nl row blocks per variable; the transforms' terms from the block rows hi and
// lo - 1 are the neighbour ranks' raw rows in `halo` ([velocity | pressure][family], RelinPlan::
// d_rhalo); the guards are those of the global system.
struct RhsHalo {
    const double *h[2][2];
};

__global__ __launch_bounds__(256) void relin_rhs_kernel(const double *__restrict__ r,
                                                        double *__restrict__ b, int m, int lo,
                                                        int nl, int64_t nv, int64_t n1, int cn,
                                                        double tau, RhsHalo halo) {
    const int64_t n0 = 2 * (int64_t)nl * nv, n = n0 + 2 * (int64_t)nl * n1;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool pres = t >= n0;
        const int64_t nx = pres ? n1 : nv, u = pres ? t - n0 : t;
        const int64_t rb = u / nx;
        const int fam = rb >= nl, il = (int)(fam ? rb - nl : rb), i = lo + il;
        const double c = pres ? tau : 1.0;
        double out = pres ? c * r[t] : r[t];
        if (cn) {
            // T_1 (i + 1 into i): adjoint rows, zeta pressure rows; T_2 (i - 1 into i): the others
            const bool t1 = fam == (int)pres;
            const double *hrow = (pres ? (fam ? halo.h[1][1] : halo.h[1][0])
                                       : (fam ? halo.h[0][1] : halo.h[0][0])) + (u - rb * nx);
            if (t1 && i + 1 < m) {
                const double *nb = il + 1 < nl ? r + t + nx : hrow;
                out += pres ? c * nb[0] : nb[0];
            }
            if (!t1 && i >= 1) {
                const double *nb = il >= 1 ? r + t - nx : hrow;
                out += pres ? c * nb[0] : nb[0];
            }
        }
        b[t] = out;
    }
}

void launch_relin_rhs(hipStream_t s, const RelinPlan &P, const double *d_r, double *d_b) {
    const int64_t n = 2 * P.w.nl * (P.nv + P.n1);
    RhsHalo H;
    H.h[0][0] = P.d_rhalo;
    H.h[0][1] = P.d_rhalo + P.nv;
    H.h[1][0] = P.d_rhalo + 2 * P.nv;
    H.h[1][1] = P.d_rhalo + 2 * P.nv + P.n1;
    hipLaunchKernelGGL(relin_rhs_kernel, dim3(grid_of(n, 256 * 8)), dim3(256), 0, s, d_r, d_b,
                       P.w.m, P.w.lo, P.w.nl, P.nv, P.n1, (int)P.w.CN, P.tau, H);
}

__global__ __launch_bounds__(256) void relin_update_kernel(double *__restrict__ u,
                                                           double *__restrict__ v,
                                                           double *__restrict__ zeta,
                                                           double *__restrict__ mu,
                                                           double *__restrict__ p, int m,
                                                           int64_t nv, int64_t n1, int cn) {
    const int64_t n0 = 2 * (int64_t)m * nv, n = n0 + 2 * (int64_t)m * n1;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        if (t < n0) {
            const int64_t rb = t / nv, R = t - rb * nv;
            if (rb < m)        // unknown block i: v at level i (CN: i + 1), zeta at level i
                v[(rb + cn) * nv + R] += u[t];
            else
                zeta[(rb - m) * nv + R] += u[t];
        } else {
            const int64_t k = t - n0, rb = k / n1, q = k - rb * n1;
            if (rb < m)        // pressure blocks: mu with the v rows, p with the zeta rows
                mu[rb * n1 + q] += u[t];
            else
                p[(rb - m) * n1 + q] += u[t];
        }
        u[t] = 0.0;   // consumed: the next solve starts from zero
    }
}

__global__ __launch_bounds__(256) void relin_zero_bc_kernel(double *__restrict__ zeta,
                                                            const uint8_t *__restrict__ bc,
                                                            int64_t n, int64_t nv) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x)
        if (bc[t % nv]) zeta[t] = 0.0;
}

// the kernel's block rows are the rank's own: v and zeta are passed from the slot of level lo
void launch_relin_update(hipStream_t s, const RelinPlan &P, double *d_u) {
    const int64_t n = 2 * P.w.nl * (P.nv + P.n1);
    hipLaunchKernelGGL(relin_update_kernel, dim3(grid_of(n, 256 * 8)), dim3(256), 0, s, d_u,
                       P.d_v + (int64_t)(P.w.lo - P.w.v_l0) * P.nv,
                       P.d_zeta + (int64_t)(P.w.lo - P.w.z_l0) * P.nv, P.d_mu, P.d_p, P.w.nl, P.nv,
                       P.n1, (int)P.w.CN);
    hipLaunchKernelGGL(relin_zero_bc_kernel, dim3(grid_of(P.w.z_n * P.nv, 256 * 8)), dim3(256), 0,
                       s, P.d_zeta, P.d_bc, P.w.z_n * P.nv, P.nv);
}

}  // namespace kkt
