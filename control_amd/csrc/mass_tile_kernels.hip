// Batched one-matrix Chebyshev solves (the mass solves of the (1,1) block: every time level the
// same M), several steps per launch out of LDS (plan: tiles.hpp).
//
// The plain form (pc_rows_il, kernels.hip) is one launch per step: each reads two iterates and the
// right-hand side and writes one iterate, so a 20-step solve streams every iterate through memory
// 20 times.  Here a workgroup takes one tile of a tile plan -- its own rows plus the rings within
// graph distance K -- and a group of four time levels, loads the two newest iterates on tile and
// rings into LDS, and advances k <= K steps on a region that shrinks by one ring per step
// (redundant flops on the rings, as in pc_tile_sweep).  Nothing is handed over between workgroups:
// the levels are independent and the next launch re-reads the rings from memory.  An ordinary
// launch: no spin, no co-residency requirement.
//
// The matrix values and local columns of the rows a thread computes stay in registers and serve
// several level groups (the matrix is the same for every level).  They come from two arrays of one
// layout, [tile][slot][entry][T] -- the values are mass_tile_gather's copy of the value array in
// that order -- so one round trip brings both; the tile's global rows are read once per launch
// into LDS, and a level group's record comes by scalar loads.
//
// Arithmetic: per (row, level) the chain of pc_rows_il -- acc from 0 by fma over the row's entries
// in SELL order (padding entries: value 0), then epi_cheb (epilogue.hpp) -- so results are
// bit-identical.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include "epilogue.hpp"

namespace kkt {

#define KKT_GLOBAL __attribute__((address_space(1)))
typedef KKT_GLOBAL const double *gcd_p;
typedef KKT_GLOBAL double *gd_p;
typedef KKT_GLOBAL const int32_t *gci_p;
typedef KKT_GLOBAL const uint16_t *gcu16_p;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef KKT_GLOBAL const d4 *gcd4_p;
typedef KKT_GLOBAL d4 *gd4_p;

// workgroup barrier that orders LDS traffic only (tile_kernels.hip): outstanding global loads and
// stores are not drained in the step loop
__device__ __forceinline__ void lds_barrier_mt() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// A level group's record, by scalar loads: the index is the same for the whole workgroup, and the
// host wrote the records before the first launch (constant address space).
__device__ __forceinline__ MassTileGroup mt_group(const MassTileArgs &A, const int g) {
    typedef const __attribute__((address_space(4))) uint64_t *cu64_p;
    constexpr int NW = sizeof(MassTileGroup) / sizeof(uint64_t);
    static_assert(sizeof(MassTileGroup) == NW * sizeof(uint64_t), "whole words");
    const cu64_p p = (cu64_p)(A.groups + g);
    uint64_t w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = p[i];
    MassTileGroup G;
    __builtin_memcpy(&G, w, sizeof(G));
    return G;
}

template <int W, int RPT, int T>
__global__ __launch_bounds__(T) void pc_tile_cheb(const MassTileArgs A) {
    extern __shared__ d4 X4[];                 // [2][nk_pad]: the two newest iterates, four levels;
    __shared__ int sn[TILE_DEPTH_MAX + 1];     // behind them [nk_pad] ints: the tile's global rows
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int nkp = A.nk_pad, k = A.k;
    int *sg = (int *)(X4 + 2 * (size_t)nkp);
    const gci_p nt = (gci_p)A.n + (size_t)tile * (TILE_DEPTH_MAX + 1);
    if (tid <= TILE_DEPTH_MAX) sn[tid] = nt[tid];
    const int n0 = nt[0], nk = nt[k], nk1 = nt[k - 1];
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};
    if (tid == 0) {
        // the zero slot: what columns of boundary rows read
        X4[nkp - 1] = zero4;
        X4[2 * (size_t)nkp - 1] = zero4;
    }
    const gci_p grow = (gci_p)A.grow + (size_t)tile * nkp;
    for (int l = tid; l < nk; l += T) sg[l] = grow[l];
    // ---- what never changes during the launch: the rows this thread computes
    double v[RPT][W], dinv[RPT];
    int col[RPT][W], gr[RPT];
    {
        // (the plan's tables have its own width PW <= W: the entries behind it are padding)
        const int PW = A.W;
        const gcu16_p lcol = (gcu16_p)A.lcol + (size_t)tile * RPT * PW * T + tid;
        const gcd_p tv = (gcd_p)A.tvals + (size_t)tile * RPT * PW * T + tid;
        const gcd_p dv = (gcd_p)A.dinv;
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            const int r = sl * T + tid;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                col[sl][e] = e < PW ? lcol[(size_t)(sl * PW + e) * T] : 0;
                v[sl][e] = e < PW ? tv[(size_t)(sl * PW + e) * T] : 0.0;
            }
            gr[sl] = r < nk1 ? grow[r] : -1;
        }
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) dinv[sl] = gr[sl] >= 0 ? dv[gr[sl]] : 0.0;
    }
    __syncthreads();
    const int64_t nx = A.nx;
    const bool first = A.s0 == 0, last = A.last != 0;
    for (int g = blockIdx.y; g < A.ngroups; g += gridDim.y) {
        const MassTileGroup G = mt_group(A, g);
        const int nlev = G.nlev;
        int cur = 0;
        // ---- the two newest iterates on tile and rings; the right-hand sides on the computed rows
        {
            d4 *Xc = X4, *Xo = X4 + nkp;
            if (first) {
                // (step 1 reads no iterate; the buffers only have to hold numbers)
                for (int l = tid; l < nk; l += T) {
                    Xc[l] = zero4;
                    Xo[l] = zero4;
                }
            } else {
                const gcd4_p pn = (gcd4_p)A.in_new + (size_t)g * nx;
                const gcd4_p po = (gcd4_p)A.in_old + (size_t)g * nx;
                const bool has_old = A.s0 >= 2;
                for (int l = tid; l < nk; l += T) {
                    const int gl = sg[l];
                    Xc[l] = pn[gl];
                    Xo[l] = has_old ? po[gl] : zero4;
                }
            }
        }
        d4 b[RPT];
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            double bb[4];
#pragma unroll
            for (int l = 0; l < 4; ++l)
                bb[l] = (gr[sl] >= 0 && l < nlev) ? ((gcd_p)G.b[l])[gr[sl]] : 0.0;
            b[sl] = d4{bb[0], bb[1], bb[2], bb[3]};
        }
        __syncthreads();
        // ---- k steps, one LDS-only barrier each
        for (int j = 1; j <= k; ++j) {
            const int s = A.s0 + j;
            const int nv = sn[k - j];
            const bool has_new = s >= 2, has_old = s >= 3, fin = last && j == k;
            const double c1 = A.coef[j - 1][0], c2 = A.coef[j - 1][1], c3 = A.coef[j - 1][2];
            d4 q1 = d4{1.0, 1.0, 1.0, 1.0}, q2 = q1;
            if (fin) {
                q1 = d4{G.post1[0], G.post1[1], G.post1[2], G.post1[3]};
                q2 = d4{G.post2[0], G.post2[1], G.post2[2], G.post2[3]};
            }
            const d4 *Xc = X4 + (size_t)cur * nkp;
            d4 *Xo = X4 + (size_t)(cur ^ 1) * nkp;
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl) {
                // wave-uniform: none of this wave's 64 rows of the slot is live on the shrunken region
                if (sl * T + (tid & ~63) >= nv) continue;
                const int r = sl * T + tid;
                d4 acc = zero4;
                if (has_new) {
                    d4 xv[W];
#pragma unroll
                    for (int e = 0; e < W; ++e) xv[e] = Xc[col[sl][e]];
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        acc.x = __builtin_fma(v[sl][e], xv[e].x, acc.x);
                        acc.y = __builtin_fma(v[sl][e], xv[e].y, acc.y);
                        acc.z = __builtin_fma(v[sl][e], xv[e].z, acc.z);
                        acc.w = __builtin_fma(v[sl][e], xv[e].w, acc.w);
                    }
                }
                if (r < nv) {
                    const d4 e0 = Xo[r], e1 = Xc[r];
                    const double a_[4] = {acc.x, acc.y, acc.z, acc.w};
                    const double p0_[4] = {e0.x, e0.y, e0.z, e0.w}, p1_[4] = {e1.x, e1.y, e1.z, e1.w};
                    const double b_[4] = {b[sl].x, b[sl].y, b[sl].z, b[sl].w};
                    const double f1[4] = {q1.x, q1.y, q1.z, q1.w}, f2[4] = {q2.x, q2.y, q2.z, q2.w};
                    double o[4];
#pragma unroll
                    for (int l = 0; l < 4; ++l)
                        o[l] = epi_cheb(has_old, c1, p0_[l], has_new, c2, p1_[l], c3, dinv[sl], b_[l],
                                        a_[l], f1[l], f2[l]);
                    // in place over the older iterate: only this thread reads or writes its row there
                    Xo[r] = d4{o[0], o[1], o[2], o[3]};
                }
            }
            lds_barrier_mt();
            cur ^= 1;
        }
        // ---- the own rows leave: the result in the API layout, or the two newest iterates
        {
            const d4 *Xc = X4 + (size_t)cur * nkp, *Xo = X4 + (size_t)(cur ^ 1) * nkp;
            if (last) {
                for (int l = tid; l < n0; l += T) {
                    const int gl = sg[l];
                    const d4 x = Xc[l];
                    const double o[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nlev) ((gd_p)G.out[q])[gl] = o[q];
                }
                // Dirichlet rows belong to no tile: tile 0 writes their zeros
                if (tile == 0) {
                    const gci_p mr = (gci_p)A.masked;
                    for (int i = tid; i < A.nmasked; i += T) {
                        const int gl = mr[i];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (q < nlev) ((gd_p)G.out[q])[gl] = 0.0;
                    }
                }
            } else {
                const gd4_p pn = (gd4_p)A.out_new + (size_t)g * nx;
                const gd4_p po = (gd4_p)A.out_old + (size_t)g * nx;
                for (int l = tid; l < n0; l += T) {
                    const int gl = sg[l];
                    pn[gl] = Xc[l];
                    po[gl] = Xo[l];
                }
            }
        }
        // the next group's loads overwrite what the stores above read
        __syncthreads();
    }
}

// the matrix rows of the tiles in tile order: out[i] = vals[gpos[i]], +0.0 where gpos[i] < 0
__global__ __launch_bounds__(256) void mass_tile_gather(const double *__restrict__ vals,
                                                        const int32_t *__restrict__ gpos,
                                                        double *__restrict__ out, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t gp = gpos[i];
    out[i] = gp >= 0 ? vals[gp] : 0.0;
}

void launch_mass_tile_gather(hipStream_t s, const double *vals, const int32_t *gpos, double *out,
                             int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mass_tile_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vals, gpos,
                       out, n);
}

typedef void (*mass_tile_fn)(const MassTileArgs);

static mass_tile_fn pick_mass_tile(int W, int rpt, int threads) {
#define KKT_MT(w, r, t) \
    if (W == w && rpt == r && threads == t) return pc_tile_cheb<w, r, t>;
#define KKT_MTW(w)                                                                             \
    KKT_MT(w, 1, 256) KKT_MT(w, 2, 256) KKT_MT(w, 3, 256) KKT_MT(w, 4, 256) KKT_MT(w, 1, 512) \
    KKT_MT(w, 2, 512) KKT_MT(w, 3, 512)
    KKT_MTW(5)
    KKT_MTW(7)
    KKT_MTW(9)
#undef KKT_MTW
#undef KKT_MT
    return nullptr;
}

int mass_tile_kernel_width(int W) { return W < 1 ? 0 : W <= 5 ? 5 : W <= 7 ? 7 : W <= 9 ? 9 : 0; }

int mass_tile_max_rpt(int threads) { return threads == 256 ? 4 : threads == 512 ? 3 : 0; }

size_t mass_tile_lds_bytes(int nk_pad) {
    return 2 * (size_t)nk_pad * sizeof(d4) + (size_t)nk_pad * sizeof(int);
}

int mass_tile_prepare(int W, int rpt, int threads, size_t lds_bytes) {
    const mass_tile_fn f = pick_mass_tile(mass_tile_kernel_width(W), rpt, threads);
    // (the limit is the kernel's, not the plan's: a later, smaller plan of another handle must not
    // lower it under a plan that is still launched)
    constexpr int LDS_LIMIT = 160 * 1024 - 1024;
    if (!f || lds_bytes > (size_t)LDS_LIMIT) return 0;
    if (hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_LIMIT) != hipSuccess)
        return 0;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, lds_bytes) != hipSuccess)
        return 0;
    return per_cu;
}

void launch_mass_tile(hipStream_t s, const MassTileArgs &a, int ntiles, int grid_y, int rpt,
                      int threads) {
    if (ntiles <= 0 || grid_y <= 0 || a.ngroups <= 0) return;
    const mass_tile_fn f = pick_mass_tile(mass_tile_kernel_width(a.W), rpt, threads);
    if (!f) throw TileLaunchError{"mass tile kernel: no variant for this plan"};
    (void)hipGetLastError();
    hipLaunchKernelGGL(f, dim3(ntiles, grid_y), dim3(threads), mass_tile_lds_bytes(a.nk_pad), s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        throw TileLaunchError{std::string("mass tile kernel: launch: ") + hipGetErrorString(e)};
}

}  // namespace kkt
