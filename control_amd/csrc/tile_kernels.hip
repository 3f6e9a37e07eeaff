// Tile sweep program for gfx950: the serial time sweeps of the block-Schur preconditioner
// (reference control/control.py:2263-2295, 2375-2406) as ONE persistent launch in which a
// workgroup advances `depth` dependent SpMV steps per hand-off (matrix-powers kernel; plan and
// rationale: tiles.hpp).
//
// One workgroup per CU owns one tile: its own rows plus the rings within graph distance
// `depth`.  State per workgroup:
//   registers  matrix values and local column indices of the rows it ever computes
//              (rows [0, n[depth-1]) of the tile, RPT per thread), Jacobi diagonal, right-hand side
//   LDS        the two newest iterates on all n[depth] local rows
// A step computes p_s on the rows whose columns are still valid (one ring fewer than the step
// before) out of LDS; when the rings are used up, the own rows of the two newest iterates are
// published as tagged granules and the rings are re-gathered from the owners' granules
// ("the data is the flag", cdna_hip_programming.md Guideline 16 R2: no flag, no drain, no
// grid barrier).  Granule buffers alternate with the hand-off epoch; write-after-read safety
// is the argument of pc_row_program_g at tile granularity (a tile publishes epoch e + 1 only
// after it has seen epoch e of every tile it gathers from, and those tiles gather from it).
//
// Arithmetic: every row keeps the fma chain of the plain kernels (kernels.hip rowops_body:
// CSR order inside a term, terms in order) and the same epilogue expressions, so the results
// equal the plain launches bit for bit (tests/test_gpu_parity.py).
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include "epilogue.hpp"

#include <algorithm>
#include <type_traits>

namespace kkt {

#define KKT_GLOBAL __attribute__((address_space(1)))
typedef KKT_GLOBAL const double *gcd_p;
typedef KKT_GLOBAL double *gd_p;
typedef KKT_GLOBAL const int32_t *gci_p;
typedef KKT_GLOBAL const uint16_t *gcu16_p;
typedef KKT_GLOBAL const uint8_t *gcb_p;
typedef KKT_GLOBAL unsigned long long *gu64_p;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned TILE_SPIN_LIMIT = 1u << 21;

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// counter (s_waitcnt vmcnt(0)): every outstanding global load or write-through store would cost
// a round trip per local step.  Global data is ordered by the granule tags, not by barriers.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// one row's value as a 16-byte granule {lo, tag, hi, tag}: ONE write-through (sc1) store
__device__ __forceinline__ void publish(const __amdgpu_buffer_rsrc_t rs, int grow, double v,
                                        unsigned tag) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const u32x4 g = {(unsigned)bits, tag, (unsigned)(bits >> 32), tag};
    __builtin_amdgcn_raw_buffer_store_b128(g, rs, grow * 16, 0, 16 /* sc1 */);
}

// the fields of a level that are needed before the level begins (its operands are requested
// under the last steps of the level before), by value
struct LevEarly {
    const double *vals, *dinv, *bin, *upd0;
    int32_t n_upd, prev_in_lds;
};
__device__ __forceinline__ LevEarly read_early(const TileLevel *p) {
    LevEarly f;
    f.vals = p->vals;
    f.dinv = p->dinv;
    f.bin = p->bin;
    f.upd0 = p->upd_vals[0];
    f.n_upd = p->n_upd;
    f.prev_in_lds = p->prev_in_lds;
    return f;
}

// (an opaque read of a packed column register: the decode -- shift / mask, times 8 plus the vector's
// base -- then stays inside the step loop instead of being hoisted into registers of its own:
// W registers per row slot)
template <typename P>
__device__ __forceinline__ P opaque_ptr(P p) {
    unsigned long long u = (unsigned long long)p;
    asm volatile("" : "+v"(u));
    return (P)u;
}
__device__ __forceinline__ unsigned opaque(unsigned x) {
    asm volatile("" : "+v"(x));
    return x;
}

// A value every lane holds alike, moved into scalar registers.  The compiler keeps a pointer it
// cannot prove uniform in a vector register pair: a buffer descriptor made from it is applied
// lane by lane (a v_readfirstlane loop around every load, each with a wait of its own), and a
// key compared once per level is spilled to scratch and waited for with everything in flight.
__device__ __forceinline__ unsigned uniform(unsigned x) { return __builtin_amdgcn_readfirstlane(x); }
template <typename P>
__device__ __forceinline__ P uniform_ptr(P p) {
    const unsigned long long u = (unsigned long long)p;
    return (P)(((unsigned long long)uniform((unsigned)(u >> 32)) << 32) | uniform((unsigned)u));
}
// An offset no granule buffer reaches (they hold 16 bytes per row or slot, far below 2 GB): the
// range check of the descriptor answers such a load with zeros -- by the documented behaviour of
// raw buffers without a request to memory; that is reasoned, not measured, and nothing depends on
// it but speed.  A poll slot that is dead or whose granule has arrived "loads" from here, so that
// all polls of a round are one straight run of loads in front of one wait.  The price: such a
// slot still issues an instruction per round where a branch issued none.
constexpr int TILE_NO_POLL = 0x7ffffff0;

// ---- the local parts of a coarse exchange (two-grid variants only).  Each is a handful of flops
// behind LDS reads that depend on each other -- offsets, then indices, then operands -- so what it
// costs is round trips: the reads of one kind are issued together and the add / fma chain comes
// last.  The chains themselves are unchanged: same operands, same order, from +0.0.  A short row
// is predicated, never padded (+0.0 and fma(0, x, a) are no identities for -0.0, infinities and
// NaN); its dead reads go to an index that exists -- and they are not free: where most of a
// group's reads would be dead (restriction lists, a thread's second function or row) the plain
// loop stayed, by the exchange stamps (profiles/exchange_chains.md).

// Lane 0's value of the xor butterfly 32, 16, ..., 1 (`a += __shfl_xor(a, o)`), which is all that
// is published: lane 0 only ever takes the partner above it, a[i] + a[i + o] on lanes i < o, and
// the addition commutes exactly.  Register moves across lanes instead of twelve trips through the
// LDS crossbar: half-wave and row swaps for 32 and 16, row shifts (DPP) for 8 to 1.  Other lanes
// end with values that mean nothing.
__device__ __forceinline__ double wave_sum_lane0(double a) {
    auto halves = [](const double x, unsigned &lo, unsigned &hi) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(x);
        lo = (unsigned)b;
        hi = (unsigned)(b >> 32);
    };
    auto whole = [](const unsigned lo, const unsigned hi) {
        return __longlong_as_double((long long)((unsigned long long)lo | ((unsigned long long)hi << 32)));
    };
    unsigned lo, hi;
    halves(a, lo, hi);
    {   // lanes 32-63 of the first operand change places with lanes 0-31 of the second
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        a = whole(l[0], h[0]) + whole(l[1], h[1]);
    }
    halves(a, lo, hi);
    {   // odd rows of the first operand change places with even rows of the second
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        a = whole(l[0], h[0]) + whole(l[1], h[1]);
    }
#define KKT_ROW_SHL(n)                                                                          \
    {                                                                                           \
        halves(a, lo, hi);                                                                      \
        const unsigned l = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x100 + (n), 0xf, 0xf, true); \
        const unsigned h = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0x100 + (n), 0xf, 0xf, true); \
        a += whole(l, h);                                                                       \
    }
    KKT_ROW_SHL(8)
    KKT_ROW_SHL(4)
    KKT_ROW_SHL(2)
    KKT_ROW_SHL(1)
#undef KKT_ROW_SHL
    return a;
}

// A row of the prolongation: the sum over the entries [e0, e1) of a row of P, in the row's order,
// of weight times product.  Up to U entries are read together; longer rows (3-D, vector-valued
// spaces) go on one entry at a time.
template <int U>
__device__ __forceinline__ double prolong_row(const int e0, const int e1, const uint16_t *pk,
                                              const double *pw, const double *ec) {
    int k[U];
    double w[U], x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = e0 + u < e1 ? e0 + u : 0;
        k[u] = pk[e];
        w[u] = pw[e];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = ec[k[u]];
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (e0 + u < e1) a = __builtin_fma(w[u], x[u], a);
    for (int e = e0 + U; e < e1; ++e) a = __builtin_fma(pw[e], ec[pk[e]], a);
    return a;
}

// HPT_: ring-entry slots per thread of a hand-off (RPT + 1 unless the variant is short of registers)
// COARSE: levels are cycles of [Galerkin coarse correction, `its` smoothing sweeps] (two-grid form
// of the sub-solves); the plain variants compile none of it.
template <int W, int RPT, int TMAX, bool UPD, int HPT_ = RPT + 1, bool COARSE = false>
__global__ __launch_bounds__(TMAX) void pc_tile_sweep(
    const TileArgs A, const TileLevel *__restrict__ levels, const int32_t *__restrict__ n_all,
    const int32_t *__restrict__ grow_all, const uint16_t *__restrict__ lcol_all,
    const int32_t *__restrict__ gpos_all, const uint8_t *__restrict__ rowmask_) {
    constexpr int HPT = HPT_;
    extern __shared__ double X[];
    __shared__ int sn[TILE_DEPTH_MAX + 1];
    __shared__ int sdead;
    __shared__ unsigned long long sstat[8];
    const int T = blockDim.x, tid = threadIdx.x, tile = blockIdx.x;
    const int nkp = A.nk_pad, depth = A.depth, its = A.its;
    const int32_t *nt = n_all + (size_t)tile * (TILE_DEPTH_MAX + 1);
    const int n0 = nt[0], nk = nt[depth], nk1 = nt[depth - 1];
    if (tid <= TILE_DEPTH_MAX) sn[tid] = nt[tid];
    if (tid < 8) sstat[tid] = 0ull;
    if (tid == 0) {
        sdead = 0;
        // the zero slot: what columns of boundary rows read (their iterates are exactly 0)
        X[nkp - 1] = 0.0;
        X[2 * (size_t)nkp - 1] = 0.0;
    }
    // ---- residency check.  The hand-offs below assume that every tile of the grid is running at
    // the same time (one workgroup per CU).  If the device cannot place them all at once -- CUs
    // masked off, another process holding wave slots -- the resident tiles would each spin 2^21
    // times in their first hand-off before giving up.  Instead every tile checks in on a counter
    // (it only ever grows: each launch adds exactly gridDim.x, so the value a tile must see is the
    // next multiple above what its own atomic returned) and waits a bounded ~5 ms for the others;
    // a tile that does not see them all marks the launch as abandoned, and every tile -- those
    // still waiting and those scheduled later -- leaves at once.  The host then falls back to
    // plain launches (kkt_info.program_fallbacks).
    __shared__ int s_bail;
    if (tid == 0) {
        typedef KKT_GLOBAL unsigned long long *gu64a_p;
        const gu64a_p ctr = (gu64a_p)(A.err + 2), bail = (gu64a_p)(A.err + 4);
        const unsigned long long nt_ = gridDim.x;
        const bool skip = A.debug_drop < 0 && tile == 0;      // test hook: tile 0 never checks in
        unsigned long long old = 0ull;
        if (!skip) old = __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else old = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long target = (old / nt_ + 1ull) * nt_;
        int bad = 0;
        unsigned long long seen = old;
        // (4 096 polls of ~1.2 us: 5 ms -- long against any launch skew, 400 times shorter than
        // the bounded spin of a hand-off)
        for (int spin = 0; spin < 4096; ++spin) {
            seen = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen >= target) break;
            if (__hip_atomic_load(bail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target) break;
            __builtin_amdgcn_s_sleep(8);
        }
        if (seen < target) {
            __hip_atomic_store(bail, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bad = 1;
        } else if (__hip_atomic_load(bail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target) {
            bad = 1;
        }
        if (bad) {
            atomicOr(A.err, 8u);
            if (atomicCAS(A.err + 1, 0u, 1u) == 0u) {
                A.err[17] = (unsigned)(seen - (target - nt_));     // tiles that had checked in
                A.err[18] = (unsigned)nt_;
            }
        }
        s_bail = bad;
    }
    __syncthreads();
    if (s_bail) return;

    const gci_p grow = (gci_p)grow_all + (size_t)tile * nkp;
    const gcb_p rowmask = (gcb_p)rowmask_;

    // ---- what never changes during the launch: structure of the rows this thread computes.
    // Narrow rows (2-D P1): local column indices and the positions of the matrix values in a
    // SELL array stay in registers.  Wide rows (3-D P1, P2): columns are packed two to a
    // register and the positions are re-read from memory once per level and matrix.
    constexpr bool PACK = W > 9;
    constexpr int CH = PACK ? 5 : W;   // entries of a row handled at a time
    constexpr int WP = (W + 1) / 2;
    constexpr int CW = PACK ? WP : W, GW = PACK ? 1 : W;
    unsigned cpk[RPT][CW];
    int gpr[RPT][GW];
    int gr[RPT];
    bool msk[RPT];
    const gcu16_p lcol = (gcu16_p)lcol_all + (size_t)tile * RPT * W * T + tid;
    const gci_p gpos = (gci_p)gpos_all + (size_t)tile * RPT * W * T + tid;
    const gci_p gpos_base = gpos;
#pragma unroll
    for (int sl = 0; sl < RPT; ++sl) {
        const int r = sl * T + tid;
        if constexpr (PACK) {
#pragma unroll
            for (int k = 0; k < W; k += 2) {
                const unsigned lo = lcol[(size_t)(sl * W + k) * T];
                const unsigned hi = k + 1 < W ? lcol[(size_t)(sl * W + k + 1) * T] : 0u;
                cpk[sl][k / 2] = lo | (hi << 16);
            }
            gpr[sl][0] = 0;
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                cpk[sl][k] = lcol[(size_t)(sl * W + k) * T];
                gpr[sl][k] = gpos[(size_t)(sl * W + k) * T];
            }
        }
        gr[sl] = r < nk1 ? grow[r] : -1;
        msk[sl] = gr[sl] >= 0 && rowmask != nullptr && rowmask[gr[sl]] != 0;
    }
    // (the 1 024-thread variants -- 128 registers -- read the packed columns opaquely, see
    // opaque(); where the decoded offsets fit into registers, hoisting them is 2 % faster)
    constexpr bool OPQ = PACK && TMAX > 512;
    // The two-grid variants at 128 (168) registers read the indices of their per-level requests
    // opaquely too.  Hoisted out of the level loop, the sign-extended indices and the addresses
    // made of them are a register pair per matrix entry, row and table -- 27 registers in scratch
    // (W = 7), reloaded one by one with a wait each in front of the requests of the next level.
    // Made where they are used they cost three instructions per request and level.
    // The 512-thread two-grid variants do the same although they have the registers: with the
    // update's first term passing through `v` (SEQ) a level has two runs of requests, and hoisted
    // addresses for both cost 2 W registers more than before (W = 9: 152 -> 170, a wave per SIMD
    // less); made in place they cost 13-29 fewer than before.
    constexpr bool TIGHT = COARSE;
    auto idx = [](const int i) { return TIGHT ? (int)opaque((unsigned)i) : i; };
    // p[i] where there is an entry, the 0.0 it stands for where there is none
    auto at = [&](const gcd_p p, const int i, const bool live) -> double {
        return live ? p[idx(i)] : 0.0;
    };
#define KKT_CPK(sl, j) (OPQ ? opaque(cpk[sl][j]) : cpk[sl][j])
#define KKT_COL(sl, k)                                                                       \
    (int)(PACK ? (((k) & 1) ? (KKT_CPK(sl, PACK ? (k) / 2 : 0) >> 16)                         \
                            : (KKT_CPK(sl, PACK ? (k) / 2 : 0) & 0xffffu))                    \
               : cpk[sl][PACK ? 0 : (k)])
#define KKT_GP(sl, k) (PACK ? gpos[(size_t)((sl) * W + (k)) * T] : gpr[sl][PACK ? 0 : (k)])
    // ... and the ring entries it gathers at a hand-off
    int hl[HPT], hg[HPT];
#pragma unroll
    for (int h = 0; h < HPT; ++h) {
        const int l = n0 + h * T + tid;
        hl[h] = l < nk ? l : -1;
        hg[h] = l < nk ? grow[l] : 0;
    }

    // step coefficients live in LDS behind the two iterates: a global load inside the step loop
    // would be drained by every workgroup barrier (vmcnt(0)), a round trip per step
    double *scoef = X + 2 * (size_t)nkp;
    // (coarse levels: the table also holds the first sweep after a correction, `its` entries)
    double *dump = scoef + 3 * (size_t)(COARSE ? (its > 0 ? its : 1) : (its > 1 ? its - 1 : 1));
    // coarse corrections: every tile's partial sums, the coarse residual, this tile's corrections
    double *SL = dump + 1, *RC = nullptr, *EC = nullptr;
    int c_nc = 0, c_jmax = 0, c_pstride = 0, c_nslots = 0, c_nj = 0, c_slot0 = 0;
    // ring form (TileCoarseDev::ring_prolong): the products of J_t+ are polled (c_njp of them,
    // else the c_nj of J_t), at most c_jx per tile
    bool c_rings = false;
    int c_njp = 0, c_jx = 0;
    unsigned cepoch = A.cepoch0;
    // the granule buffers of the exchanges as scalars (uniform_ptr), read once: both of each pair,
    // the exchange number picks one
    void *cg0 = nullptr, *cg1 = nullptr, *eg0 = nullptr, *eg1 = nullptr;
    int cg_bytes = 0, eg_bytes = 0;
    if constexpr (COARSE) {
        const TileCoarseDev *cd = A.coarse;
        cg0 = uniform_ptr((void *)cd->cg[0]);
        cg1 = uniform_ptr((void *)cd->cg[1]);
        eg0 = uniform_ptr((void *)cd->eg[0]);
        eg1 = uniform_ptr((void *)cd->eg[1]);
        cg_bytes = (int)uniform(cd->cg_bytes);
        eg_bytes = (int)uniform(cd->eg_bytes);
        c_nc = cd->nc;
        c_jmax = cd->jmax;
        c_pstride = cd->pstride;
        c_nslots = cd->nslots;
        c_nj = cd->nj[tile];
        c_slot0 = cd->slot0[tile];
        c_rings = cd->ring_prolong != 0;
        c_njp = c_rings ? cd->njx[tile] : c_nj;
        c_jx = c_rings ? cd->jxmax : c_jmax;
        RC = SL + c_nslots;
        EC = RC + c_nc;
    }
    // ... and what never changes between corrections, copied into LDS once (read from memory per
    // correction it was a chain of eight dependent round trips, ~25 us per level): the tile's
    // restriction lists and prolongation entries, the slot -> coarse function map
    double *RWc = nullptr, *PWc = nullptr;
    int *CSLc = nullptr, *CIPc = nullptr, *RIPc = nullptr, *JGc = nullptr;
    int *PIPc = nullptr;     // ring form: entry offsets of all nk local rows (nk + 1 of them)
    uint16_t *RROWc = nullptr, *PKc = nullptr;
    gci_p c_pip = nullptr;   // other forms: entry offsets of the own rows, read per correction
    bool c_cached = true;    // the tile's P entries are in LDS (3-D: 8 per row, they stay in memory)
    int c_re0 = 0, c_pq0 = 0;
    // Rows of (P^T A P)^-1: coarse function j belongs to tile j mod ntiles, which forms
    // (E^-1 r_c)_j for everybody and publishes it as a granule (every tile holds the whole coarse
    // residual anyway).  A tile forming the products for the functions its own rows touch read
    // 12 rows of 1 089 doubles from L2 per correction on cfg 2 -- 27 MB over the chip, 6 of the
    // exchange's 10 us -- four tiles each repeating the same product; the 4-5 rows a tile owns
    // stay in LDS while consecutive levels share the matrix (time-invariant operators).
    double *EINVc = nullptr;
    bool c_einv_cache = false;
    const void *einv_key = nullptr;
    const int c_nown = COARSE ? (c_nc > tile ? (c_nc - tile + (int)gridDim.x - 1) / (int)gridDim.x : 0) : 0;
    // the column range of the first row this wave owns (row j over its diagonal block only,
    // kernels.hpp TileCoarseDev), read once: few tiles own more rows than they have waves
    int c_lo0 = 0, c_hi0 = 0, c_ew = 0;
    if constexpr (COARSE) {
        const TileCoarseDev *cd = A.coarse;
        c_ew = cd->ew;
        if ((int)(threadIdx.x >> 6) < c_nown) {
            const int j0 = tile + (int)(threadIdx.x >> 6) * (int)gridDim.x;
            c_lo0 = cd->e_lo[j0];
            c_hi0 = cd->e_hi[j0];
        }
        c_cached = cd->cache_lists != 0;
        // (the layout tile_sweep_lds_bytes() counts)
        const int nrm = c_cached ? cd->nr_max : 0;
        const int npm = c_rings ? cd->np_max : nrm;
        RWc = EC + c_jx;
        PWc = RWc + nrm;
        CSLc = reinterpret_cast<int *>(PWc + npm);
        CIPc = CSLc + c_nslots;
        RIPc = CIPc + (c_nc + 1);
        JGc = RIPc + (c_jmax + 1);
        PIPc = JGc + c_jx;
        RROWc = reinterpret_cast<uint16_t *>(PIPc + (c_rings ? nkp + 1 : 0));
        PKc = RROWc + nrm;
        c_einv_cache = cd->cache_einv != 0;
        // (8-byte aligned: behind the 2-byte lists, rounded up.  As an offset from X, itself
        // aligned: a pointer made from an integer is no longer known to point into LDS, and the
        // rows were read and written by flat instructions)
        EINVc = X + (static_cast<size_t>(reinterpret_cast<const char *>(PKc + npm) -
                                         reinterpret_cast<const char *>(X)) + 7) / 8;
        const gci_p rip = (gci_p)cd->r_ip + (size_t)tile * c_jmax;
        const gci_p pip = (gci_p)cd->p_ip + (size_t)tile * c_pstride;
        // (ring form: the ring rows' entries lie behind the own rows')
        // (uniform: first entries of the tile)
        const int re0 = (int)uniform((unsigned)rip[0]), re1 = (int)uniform((unsigned)rip[c_nj]);
        const int pq0 = (int)uniform((unsigned)pip[0]);
        const int pq1 = (int)uniform((unsigned)pip[c_rings ? nk : nt[0]]);
        c_re0 = re0;
        c_pq0 = pq0;
        const gcu16_p rrow = (gcu16_p)cd->r_row, pk = (gcu16_p)cd->p_k;
        const gcd_p rw = (gcd_p)cd->r_w, pw = (gcd_p)cd->p_w;
        if (c_cached) {
            for (int i = tid; i < re1 - re0; i += T) {
                RWc[i] = rw[re0 + i];
                RROWc[i] = rrow[re0 + i];
            }
            for (int i = tid; i < pq1 - pq0; i += T) {
                PWc[i] = pw[pq0 + i];
                PKc[i] = pk[pq0 + i];
            }
        }
        const gci_p cslot = (gci_p)cd->c_slot, cip = (gci_p)cd->c_ip;
        for (int i = tid; i < c_nslots; i += T) CSLc[i] = cslot[i];
        for (int i = tid; i <= c_nc; i += T) CIPc[i] = cip[i];
        const gci_p jg = (gci_p)cd->jglob + (size_t)tile * cd->jxmax;
        for (int i = tid; i <= c_nj; i += T) RIPc[i] = rip[i] - re0;
        for (int i = tid; i < c_njp; i += T) JGc[i] = jg[i];
        if (c_rings)
            for (int i = tid; i <= nk; i += T) PIPc[i] = pip[i] - pq0;
        c_pip = pip;
        __syncthreads();
    }
    const void *coef_key = nullptr;
    int cur = 0;             // X + cur * nkp: the newest iterate; the other half: the one before
    unsigned epoch = A.epoch0;   // tags never repeat between the launches of one application
    bool dead = false;       // a spin timed out: stop waiting, run to the end, results invalid
    // (the keys -- vals_key, coef_key, einv_key -- are compared once per level or exchange: scalars,
    // see uniform_ptr())
    const void *vals_key = nullptr;
    double v[RPT][W];

    // diagnostics (option "stamps"): 100 MHz ticks this workgroup spent in hand-offs / local
    // steps / level prologues, counts, poll rounds -- 8 x 64-bit words per tile at err + 64
    unsigned long long *stat = reinterpret_cast<unsigned long long *>(A.err + 64) + (size_t)tile * 8;
    const bool stamps = A.stamps != 0;
    unsigned long long t_mark = stamps ? wall_clock64() : 0ull;
    // (summed in LDS and written out once at the end: a read-modify-write of memory per stamp is
    // a round trip that lands in the NEXT interval)
    auto lap = [&](int slot, unsigned long long count) {
        if (!stamps) return;
        const unsigned long long now = wall_clock64();
#ifndef KKT_XSTAMPS
        if (tid == 0) {
            sstat[slot] += now - t_mark;
            sstat[slot + 3] += count;
        }
#else
        // -DKKT_XSTAMPS: the slots hold the parts of the coarse exchange instead, slot 3 the
        // prolongation (scripts/r03_exchange_stamps.py); nothing is counted
        (void)slot;
        (void)count;
#endif
        t_mark = now;
    };

    // publish the own rows of the newest (and the previous) iterate, re-gather the rings
    // The fields of a level are uniform values behind scalar loads, and the first reader of a
    // line waits for it (1-2 us per dependent batch, every workgroup at the same moment; measured:
    // 2.8 us of a level's first step).  lgkmcnt is shared with LDS, so the wait cannot be pushed
    // past the next LDS barrier -- but a hand-off waits for memory anyway: what the NEXT level
    // needs early is read at the start of the current level's first hand-off, one field from
    // each of the two 64-byte lines of its struct, which the level's own reads then find cached.
    static_assert(sizeof(TileLevel) == 128, "two scalar-cache lines per level");
    LevEarly Nf{};
    bool nf_valid = false;
    const TileLevel *nf_want = nullptr;
    // `early`: the newest iterate's own rows went out from the step that computed them (the last
    // step of the round), under that step's remaining work; only the previous iterate is left
    auto handoff = [&](const bool both, const bool early = false) {
        lap(1, 0);
        if (nf_want != nullptr) {
            Nf = read_early(nf_want);
            nf_want = nullptr;
            nf_valid = true;
        }
        ++epoch;
        double *Xc = X + cur * nkp, *Xo = X + (cur ^ 1) * nkp;
        const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr((void *)A.gnew[epoch & 1]), 0, (int)A.granule_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr((void *)A.gold[epoch & 1]), 0, (int)A.granule_bytes, 0x00020000);
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            const int r = sl * T + tid;
            if (r < n0 && !(tile == 0 && A.debug_drop > 0 && (int)(epoch - A.epoch0) == A.debug_drop)) {
                if (!early) publish(rn, gr[sl], Xc[r], epoch);
                // (at depth 1 no ring row is ever computed: nobody reads the previous iterate)
                if (both && depth > 1) publish(ro, gr[sl], Xo[r], epoch);
            }
        }
        // a granule {lo, tag, hi, tag} is read back by ONE 16-byte sc1 load (half the requests of
        // two 8-byte loads; a torn read shows as unequal tags and is simply read again)
        // Per ring entry only "still wanted": a granule that arrives goes to LDS at once (nobody reads
        // a ring row before the barrier below), so a poll needs registers only while it is in flight.
        bool want_o[HPT], need_n[HPT], need_o[HPT];
#pragma unroll
        for (int h = 0; h < HPT; ++h) {
            want_o[h] = both && hl[h] >= 0 && hl[h] < nk1;
            need_n[h] = hl[h] >= 0;
            need_o[h] = want_o[h];
        }
        auto value = [](const u32x4 g) {
            return __longlong_as_double((long long)((unsigned long long)g.x | ((unsigned long long)g.z << 32)));
        };
        // a poll samples memory about half a round trip after it is issued; the neighbours'
        // granules, stored at about the same time as this tile's, take about one: polling at
        // once mostly fails and costs a second round trip
        for (int i = 0; i < A.poll_delay; ++i) __builtin_amdgcn_s_sleep(1);
        unsigned spins = 0;
        while (true) {
            asm volatile("" ::: "memory");   // the loads below are re-issued every round
            bool ok = true;
            // Every poll of the round is issued before the round's one wait.  Only what has not
            // arrived yet is requested again: the other slots take TILE_NO_POLL, no branch around
            // a load (a branch gives each load a wait of its own -- a round trip per slot).
            u32x4 tn[HPT], to[HPT];
#pragma unroll
            for (int h = 0; h < HPT; ++h) {
                tn[h] = __builtin_amdgcn_raw_buffer_load_b128(
                    rn, need_n[h] ? hg[h] * 16 : TILE_NO_POLL, 0, 16 /* sc1 */);
                to[h] = __builtin_amdgcn_raw_buffer_load_b128(
                    ro, need_o[h] ? hg[h] * 16 : TILE_NO_POLL, 0, 16 /* sc1 */);
            }
            __builtin_amdgcn_sched_barrier(0);
            // the tags seen, for the time-out record (arrived before this round: the number itself)
            unsigned seen[HPT][4];
#pragma unroll
            for (int h = 0; h < HPT; ++h) {
                seen[h][0] = need_n[h] ? tn[h].y : (hl[h] >= 0 ? epoch : 0u);
                seen[h][1] = need_n[h] ? tn[h].w : (hl[h] >= 0 ? epoch : 0u);
                seen[h][2] = need_o[h] ? to[h].y : (want_o[h] ? epoch : 0u);
                seen[h][3] = need_o[h] ? to[h].w : (want_o[h] ? epoch : 0u);
                // (a torn read shows as unequal tags and is simply read again)
                const bool hit_n = need_n[h] && tn[h].y == epoch && tn[h].w == epoch;
                const bool hit_o = need_o[h] && to[h].y == epoch && to[h].w == epoch;
                if (hit_n) Xc[hl[h]] = value(tn[h]);
                if (hit_o) Xo[hl[h]] = value(to[h]);
                need_n[h] = need_n[h] && !hit_n;
                need_o[h] = need_o[h] && !hit_o;
                ok &= !need_n[h] && !need_o[h];
            }
            if (ok || dead) break;
            if (++spins >= TILE_SPIN_LIMIT) {
                // record who waited for what: tile, epoch, local index, global row, tags seen
                dead = true;
                sdead = 1;
                atomicOr(A.err, 4u);
                if (atomicCAS(A.err + 1, 0u, 1u) == 0u) {
#pragma unroll
                    for (int h = 0; h < HPT; ++h)
                        if (need_n[h] || need_o[h]) {
                            A.err[8] = (unsigned)tile;
                            A.err[9] = epoch;
                            A.err[10] = (unsigned)hl[h];
                            A.err[11] = (unsigned)hg[h];
                            A.err[12] = seen[h][0];
                            A.err[13] = seen[h][1];
                            A.err[14] = seen[h][2];
                            A.err[15] = seen[h][3];
                            A.err[16] = both ? 1u : 0u;
                        }
                }
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        // a wave that leaves this barrier knows every wave of the workgroup has finished reading
        // the granules of this epoch; only then may anyone publish the next one
        lds_barrier();
        dead = sdead != 0;
#ifndef KKT_XSTAMPS
        if (stamps && tid == 0) sstat[6] += spins;
#endif
        lap(0, 1);
    };

    // Operands of a level that live in registers through its steps: matrix values (re-loaded
    // only when the pointer changes: per level in mode G, once in mode S), Jacobi diagonal,
    // right-hand side.  Called for level 0 up front and for level l + 1 BEFORE the hand-off that
    // ends level l, so that the HBM fetch (every tile asks for its slice of the next matrix at
    // the same moment) runs under the hand-off's wait instead of after it.
    // (In the 1 024- and 768-thread two-grid variants that was not so while indices came back from
    // scratch with a wait each between these requests; see TIGHT.  Emitted code of W = 7: result
    // store, then all nine requests, no wait before the hand-off's polls.)
    double dinv[RPT], b[RPT];
    // (wide rows: the positions of all slots first, then the values -- two dependent round trips
    // instead of two per chunk of five entries)
    auto load_vals = [&](const double *ptr, const bool update_matrix) {
        vals_key = uniform_ptr((const void *)ptr);
        const gcd_p vp = (gcd_p)ptr;
        if constexpr (PACK) {
            // (the addresses of the positions must not be hoisted out of the level loop: they
            // are 2 W registers per row slot that nothing else could use -- 58 of the 245
            // registers of the two-slot 3-D variant)
            const gci_p gpos = opaque_ptr(gpos_base);
            constexpr int G = RPT * W > 30 ? 1 : RPT;   // slots whose positions are fetched together
#pragma unroll
            for (int s0 = 0; s0 < RPT; s0 += G) {
                int gp[G][W];
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int k = 0; k < W; ++k) gp[q][k] = KKT_GP(s0 + q, k);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int k = 0; k < W; ++k)
                        v[s0 + q][k] = at(vp, gp[q][k],
                                          gp[q][k] >= 0 && (!update_matrix || gr[s0 + q] >= 0));
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    // (TIGHT: the masks are made here from the opaque indices, level by level;
                    // hoisted out of the level loop they are a pair of scalar registers per
                    // entry, and scalar registers that run out are kept in lanes of vector
                    // registers -- a whole register for every 64 of them)
                    const int gp = idx(KKT_GP(sl, k));
                    v[sl][k] = at(vp, gp, gp >= 0 && (!update_matrix || idx(gr[sl]) >= 0));
                }
        }
    };
    auto load_db = [&](const LevEarly &L) {
        const gcd_p dp = (gcd_p)L.dinv, bp = (gcd_p)L.bin;
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            dinv[sl] = at(dp, gr[sl], idx(gr[sl]) >= 0);
            b[sl] = at(bp, gr[sl], idx(gr[sl]) >= 0);
        }
    };
    auto load_level = [&](const LevEarly &L) {
        if (uniform_ptr((const void *)L.vals) != vals_key) load_vals(L.vals, false);
        load_db(L);
    };
    // Wide rows and two-grid levels with the level update in the kernel (SEQ): there are no
    // registers for a second matrix, so the first term of the update passes through the registers
    // of the level matrix -- its values are requested in front of the hand-off that ends a level
    // (the old matrix is dead by then) and land under it, they are multiplied after it, and only
    // then is the new level's own matrix requested.
    // Plain wide levels wait for that request at once: their first sweep multiplies by it (one
    // exposed fetch per level instead of a kernel boundary, a plain update launch and the
    // per-launch structure loads).  A two-grid level multiplies by its matrix only after its first
    // exchange -- cycle 0 restricts r = b, all-gathers, forms the owned products and prolongs --
    // so there the request stays in flight under the exchange and `v` is waited for once, behind
    // cycle 0's prolongation.  Between the update and that point `v` must not be read.
    // `vals_key` names the array whose values `v` holds (or will hold once the requests land),
    // `v_is_u` says that they were requested as an update's term, i.e. zero on rows without a
    // global row -- rows no step computes, so where the update's array is the level's own array
    // the values serve as the level matrix without a second request.
    // Wide rows carry one update term only (tile_sweep_fuses_update()); on narrow rows further
    // terms are read from memory after the first.
    constexpr bool SEQ = (PACK || COARSE) && UPD;
    bool v_is_u = false;
    if (A.nlevels > 0) {
        const LevEarly L0 = read_early(&levels[0]);
        if (SEQ && L0.n_upd > 0) {
            load_vals(L0.upd0, true);
            load_db(L0);
            v_is_u = true;
        } else {
            load_level(L0);
        }
    }

    // Narrow rows leave registers for the NEXT level's operands (its matrix, the matrix of its
    // update, diagonal, right-hand side): they are requested when the last round of local steps
    // of a level begins and land under those steps.  Requested at the level's end they cost an
    // HBM round trip per level twice over -- once in front of the hand-off's polls (loads return
    // in order), once in front of the update (measured: 3 us of level prologue in mode G).
    // Variants without that room (1 024 threads: 128 registers) still keep the values of the next
    // update's matrix out of the level's first step: they are requested together with the next
    // matrix in front of the hand-off that ends the level (PRE_U).
    // (two-grid levels are short -- a correction and a handful of sweeps -- and their exchanges
    // need the registers: no operands of the next level are held across them in registers of
    // their own.  The values of the next update's matrix travel under the hand-off that ends the
    // level all the same, in the registers of the level matrix: SEQ above.)
    constexpr bool PRE = UPD && !COARSE && W * RPT <= 14 && TMAX <= 512;
    constexpr bool PRE_U = UPD && !COARSE && !PRE && W * RPT <= 7;
    constexpr int PR = PRE ? RPT : 1, PW = PRE ? W : 1;
    constexpr int UR = (PRE || PRE_U) ? RPT : 1, UW = (PRE || PRE_U) ? W : 1;
    double vn[PR][PW], un[UR][UW], dn[PR], bn[PR];
    bool pre_v = false, pre_u = false, pre_issued = false, un_loaded = false;
    auto load_un = [&](const LevEarly &N) {
        if constexpr (PRE || PRE_U) {
            pre_u = N.n_upd > 0;
            if (pre_u) {
                const gcd_p up = (gcd_p)N.upd0;
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const int gp = KKT_GP(sl, k);
                        un[sl][k] = (gr[sl] >= 0 && gp >= 0) ? up[gp] : 0.0;
                    }
            }
            un_loaded = true;
        }
    };
    auto prefetch_level = [&](const LevEarly &N) {
        if constexpr (PRE) {
            pre_issued = true;
            pre_v = uniform_ptr((const void *)N.vals) != vals_key;
            if (pre_v) {
                const gcd_p vp = (gcd_p)N.vals;
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const int gp = KKT_GP(sl, k);
                        vn[sl][k] = gp >= 0 ? vp[gp] : 0.0;
                    }
            }
            load_un(N);
            const gcd_p dp = (gcd_p)N.dinv, bp = (gcd_p)N.bin;
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl) {
                dn[sl] = gr[sl] >= 0 ? dp[gr[sl]] : 0.0;
                bn[sl] = gr[sl] >= 0 ? bp[gr[sl]] : 0.0;
            }
        }
    };
    auto adopt_level = [&](const LevEarly &N) {
        if constexpr (PRE) {
            if (pre_v) {
                vals_key = uniform_ptr((const void *)N.vals);
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                    for (int k = 0; k < W; ++k) v[sl][k] = vn[sl][k];
            }
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl) {
                dinv[sl] = dn[sl];
                b[sl] = bn[sl];
            }
        }
    };

    for (int lev = 0; lev < A.nlevels; ++lev) {
        const TileLevel &L = levels[lev];
        nf_valid = false;
        nf_want = lev + 1 < A.nlevels ? &levels[lev + 1] : nullptr;
        const bool have_u = (PRE || PRE_U) && un_loaded && pre_u;   // un = values of upd_vals[0]
        const bool use_v = SEQ && v_is_u;                            // v = values of upd_vals[0]
        pre_issued = false;
        un_loaded = false;
        v_is_u = false;
        // (two-grid levels: the pointer to the level's coarse inverse, read here.  Read where the
        // exchange first needs it, it was a load behind the request of the level matrix, and the
        // wait for it -- loads return in order -- a wait for the matrix.  The table of these
        // pointers is written before the launch and read through the constant address space: a
        // scalar load, counted with the level's fields and not with the requests.)
        const double *einv_lev = nullptr;
        if constexpr (COARSE) {
            typedef const double *einv_entry;
            typedef __attribute__((address_space(4))) const einv_entry *einv_table_p;
            einv_lev = ((einv_table_p)(uintptr_t)A.einv)[lev];
        }
        if (uniform_ptr((const void *)L.coef) != coef_key) {
            coef_key = uniform_ptr((const void *)L.coef);
            const gcd_p cp = (gcd_p)(const double *)L.coef;
            __syncthreads();   // nobody still reads the old table
            for (int i = idx(tid); i < 3 * (COARSE ? its : its - 1); i += T) scoef[i] = cp[i];
            // (the barrier after the first step of the level orders these writes before their use)
        }
        // Everything loaded for the level is pinned in registers here: a value whose load is
        // conditional would otherwise be waited for at its first use INSIDE the step loop
        // (s_waitcnt vmcnt(0) there would also drain whatever the loop keeps in flight).
        // (two-grid levels: `v` is pinned behind cycle 0's prolongation instead, see SEQ)
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            if constexpr (!(SEQ && COARSE)) {
#pragma unroll
                for (int k = 0; k < W; ++k) asm volatile("" : "+v"(v[sl][k]));
            }
            asm volatile("" : "+v"(dinv[sl]));
            asm volatile("" : "+v"(b[sl]));
        }
        if (!COARSE && stamps && tid == 0) sstat[7] += wall_clock64() - t_mark;   // prologue up to the update
        const double post1 = L.post1, post2 = L.post2;
        int cr;
        {
            double *Xc = X + cur * nkp, *Xo = X + (cur ^ 1) * nkp;
            if (UPD && L.n_upd > 0) {
                if (!L.prev_in_lds) {
                    // produced before this launch (or by another rank): plain memory
                    const gcd_p xp = (gcd_p)L.x_prev;
                    for (int l = idx(tid); l < nk; l += T) Xc[l] = xp[grow[l]];
                    lds_barrier();
                }
                // b = ca * (sum_t U_t x_prev) + cy * b_in, 0 on boundary rows; p_1 = scale D^-1 b
                double acc[RPT];
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl) acc[sl] = 0.0;
                if constexpr (PRE || PRE_U) {
                    if (have_u) {
                        // all gathers in flight before the first fma (the chains of the slots
                        // then run side by side instead of one LDS round trip per entry)
                        double xu[UR][UW];
#pragma unroll
                        for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                            for (int k = 0; k < W; ++k) xu[sl][k] = Xc[KKT_COL(sl, k)];
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int k = 0; k < W; ++k)
#pragma unroll
                            for (int sl = 0; sl < RPT; ++sl)
                                acc[sl] = __builtin_fma(un[sl][k], xu[sl][k], acc[sl]);
                    }
                }
                if constexpr (SEQ) {
                    if (use_v) {
#pragma unroll
                        for (int sl = 0; sl < RPT; ++sl) {
                            if (sl * T + (tid & ~63) >= nk1) continue;
#pragma unroll
                            for (int k0 = 0; k0 < W; k0 += CH) {
                                double xv[CH];
#pragma unroll
                                for (int k = 0; k < CH; ++k)
                                    if (k0 + k < W) xv[k] = Xc[KKT_COL(sl, k0 + k)];
#pragma unroll
                                for (int k = 0; k < CH; ++k)
                                    if (k0 + k < W)
                                        acc[sl] = __builtin_fma(v[sl][k0 + k], xv[k], acc[sl]);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                }
                // (wide rows with the update: one term, the host's condition for these variants
                // -- with this loop compiled in, the two-slot variant spills 88 registers)
                if constexpr (!(PACK && SEQ))
                for (int t = (have_u || use_v) ? 1 : 0; t < L.n_upd; ++t) {
                    const gcd_p up = (gcd_p)L.upd_vals[t];
#pragma unroll
                    for (int sl = 0; sl < RPT; ++sl) {
                        if (sl * T + (tid & ~63) >= nk1) continue;
#pragma unroll
                        for (int k0 = 0; k0 < W; k0 += CH) {
                            int gp[CH];
                            double vu[CH];
#pragma unroll
                            for (int k = 0; k < CH; ++k)
                                if (k0 + k < W) gp[k] = idx(KKT_GP(sl, k0 + k));
#pragma unroll
                            for (int k = 0; k < CH; ++k)
                                if (k0 + k < W)
                                    vu[k] = at(up, gp[k], idx(gr[sl]) >= 0 && gp[k] >= 0);
#pragma unroll
                            for (int k = 0; k < CH; ++k)
                                if (k0 + k < W)
                                    acc[sl] = __builtin_fma(vu[k], Xc[KKT_COL(sl, k0 + k)], acc[sl]);
                            if constexpr (PACK) __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                if constexpr (SEQ && COARSE) {
                    // the level's own matrix, now that the update's has been used: requested in
                    // front of the stores below (a wait the compiler puts in front of a request
                    // must not find them in flight) and not waited for before the first exchange
                    // is over
                    if (uniform_ptr((const void *)L.vals) != vals_key) load_vals(L.vals, false);
                }
                const gd_p bo = (gd_p)L.bout;
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl) {
                    const int r = sl * T + tid;
                    const double out =
                        msk[sl] ? 0.0 : epi_lin(L.ca, acc[sl], true, L.cy, b[sl], false, 0.0, 0.0);
                    const double out2 = epi_first(L.p1_scale, dinv[sl], out);
                    b[sl] = out;
                    if (r < nk1) Xo[r] = out2;
                    if (r < n0 && bo != nullptr) bo[idx(gr[sl])] = out;
                }
                if constexpr (SEQ && !COARSE) {
                    // the level's own matrix, now that the update's has been used
                    if (uniform_ptr((const void *)L.vals) != vals_key) load_vals(L.vals, false);
                }
            } else {
                // first step of a solve on a right-hand side that is already final
                const bool last = its == 1;
                const double q1 = last ? post1 : 1.0, q2 = last ? post2 : 1.0;
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl) {
                    const int r = sl * T + tid;
                    double out = 0.0;
                    if (!msk[sl])
                        out = epi_cheb(false, 0.0, 0.0, false, 0.0, 0.0, L.p1_scale, dinv[sl], b[sl],
                                       0.0, q1, q2);
                    if (r < nk1) Xo[r] = out;
                }
            }
            cr = depth - 1;
            lds_barrier();
            cur ^= 1;
        }
        const bool has_next = lev + 1 < A.nlevels;
        if (PRE && has_next && its - 1 <= cr) {
            Nf = read_early(&levels[lev + 1]);        // (a level without a hand-off of its own)
            nf_want = nullptr;
            nf_valid = true;
            prefetch_level(Nf);
        }
#pragma unroll
        for (int sl = 0; sl < RPT; ++sl) {
            if constexpr (SEQ && !COARSE) {
#pragma unroll
                for (int k = 0; k < W; ++k) asm volatile("" : "+v"(v[sl][k]));
            }
            asm volatile("" : "+v"(dinv[sl]));
            asm volatile("" : "+v"(b[sl]));
        }
        lap(2, 1);
        if constexpr (COARSE) {
            // ---- two-grid level: cycles of [coarse correction of the iterate; `its` sweeps]
            // One SpMV step of this path on the rows [0, nv): mode 0 the Chebyshev update
            // p+ = c1 p- + c2 p + c3 D^-1 (b - A p) into the older buffer, mode 1 the residual
            // b - A p.  The fma chain of a row is the plain kernels' (slot order).
            auto cstep = [&](const int mode, const int nv, const double cf1, const double cf2,
                             const double cf3, const bool has_old, const double q1,
                             const double q2) {
                double *Xc = X + cur * nkp, *Xo = X + (cur ^ 1) * nkp;
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl) {
                    if (sl * T + (tid & ~63) >= nv) continue;      // wave-uniform
                    const int r = sl * T + tid;
                    double acc = 0.0;
#pragma unroll
                    for (int k0 = 0; k0 < W; k0 += CH) {
                        double xv[CH];
#pragma unroll
                        for (int k = 0; k < CH; ++k)
                            if (k0 + k < W) xv[k] = Xc[KKT_COL(sl, k0 + k)];
#pragma unroll
                        for (int k = 0; k < CH; ++k)
                            if (k0 + k < W) acc = __builtin_fma(v[sl][k0 + k], xv[k], acc);
                        if constexpr (PACK) __builtin_amdgcn_sched_barrier(0);
                    }
                    if (r < nv) {
                        double out = 0.0;
                        if (!msk[sl]) {
                            if (mode == 0) {
                                // (the row's own entries are read here, behind the chain.  Read
                                // with the gathers, one wait in front of the chain as in the plain
                                // steps, they are four registers more across it: the 1 024-thread
                                // variants spilled again and a step took 0.2 us longer --
                                // profiles/coarse_polls.md)
                                out = epi_cheb(has_old, cf1, Xo[r], true, cf2, Xc[r], cf3, dinv[sl],
                                               b[sl], acc, q1, q2);
                            } else {
                                out = b[sl] - acc;
                            }
                        }
                        Xo[r] = out;
                    }
                }
            };
            const TileCoarseDev *cd = A.coarse;
            const gcd_p einv = (gcd_p)einv_lev;
            const int wave = tid >> 6, lane = tid & 63, nwaves = T >> 6;
            for (int cyc = 0; cyc < A.cycles; ++cyc) {
                // ---- residual of the current iterate on the own rows, into the older buffer
                if (cyc == 0) {
                    double *Xo = X + (cur ^ 1) * nkp;
#pragma unroll
                    for (int sl = 0; sl < RPT; ++sl) {
                        const int r = sl * T + tid;
                        if (r < n0) Xo[r] = b[sl];          // zero guess: r = b
                    }
                } else {
                    // the first ring must be valid; ring form: every ring, the correction is
                    // added to them (the same condition in every tile: they all take the same
                    // sequence of hand-offs, which the alternation of the granule buffers needs)
                    if (cr == 0 || (c_rings && cr < depth)) {
                        handoff(false);
                        cr = depth;
                    }
                    cstep(1, n0, 0.0, 0.0, 0.0, false, 1.0, 1.0);
                }
                lds_barrier();
                lap(1, cyc == 0 ? 0 : 1);      // (stamps: the residual step counts as a step)
#ifdef KKT_XSTAMPS
                unsigned long long xs_t = wall_clock64();
                auto xs = [&](int slot) {
                    const unsigned long long n_ = wall_clock64();
                    if (tid == 0) sstat[slot] += n_ - xs_t;
                    xs_t = n_;
                };
#define KKT_XS(slot) xs(slot)
#else
#define KKT_XS(slot)
#endif
                // ---- restriction: partial sums over the own rows for the coarse functions they
                // touch, a wave per function, lanes stride its list, fixed butterfly
                ++cepoch;
                {
                    // (without the ring form: the entry ranges of the own rows in P, wanted at the
                    // prolongation.  Carried through the whole launch they were two registers per
                    // row slot that the ring form never reads, and the 128-register variants kept
                    // them in scratch.  Requested here they have the exchange, 8 us of polls and
                    // barriers, to land under; that is not measured on its own -- the flagship
                    // runs the ring form -- and costs two loads from L2 per row slot and
                    // correction where the parent read them once per launch.)
                    int pe0[RPT], pe1[RPT];
                    if (!c_rings) {
#pragma unroll
                        for (int sl = 0; sl < RPT; ++sl) {
                            const int r = sl * T + tid;
                            pe0[sl] = r < n0 ? c_pip[r] - c_pq0 : 0;
                            pe1[sl] = r < n0 ? c_pip[r + 1] - c_pq0 : 0;
                        }
                    }
                    const double *Rb = X + (cur ^ 1) * nkp;
                    const __amdgpu_buffer_rsrc_t rc_ = __builtin_amdgcn_make_buffer_rsrc(
                        (cepoch & 1) ? cg1 : cg0, 0, cg_bytes, 0x00020000);
                    for (int k = wave; k < c_nj; k += nwaves) {
                        const int e0 = RIPc[k], e1 = RIPc[k + 1];
                        double a = 0.0;
                        if (c_cached) {
                            // (rows and weights of four entries of a lane read ahead of the
                            // gathers and the chain were slower, 0.81 us against 0.66: most
                            // lists are shorter than 64 entries, and the dead reads of the
                            // other three cost more than the live ones gain --
                            // profiles/exchange_chains.md)
                            for (int e = e0 + lane; e < e1; e += 64)
                                a = __builtin_fma(RWc[e], Rb[RROWc[e]], a);
                        } else {
                            const gcu16_p rrow = (gcu16_p)cd->r_row + c_re0;
                            const gcd_p rw = (gcd_p)cd->r_w + c_re0;
                            for (int e = e0 + lane; e < e1; e += 64)
                                a = __builtin_fma(rw[e], Rb[rrow[e]], a);
                        }
                        a = wave_sum_lane0(a);
                        if (lane == 0) publish(rc_, c_slot0 + k, a, cepoch);
                    }
                    // ---- every tile's partial sums ("the data is the flag"), then the coarse
                    // residual: contributions of a function summed in slot (= tile) order
                    // (4 slots per thread, all of them in flight at once; more slots than 4 T:
                    // further rounds, whose granules have mostly landed by then.  8 in flight made
                    // the compiler spill ~200 registers in the 512-thread variants.)
                    constexpr int CSL = 4;
                    KKT_XS(0);      // restriction + publish
                    for (int i = 0; i < A.poll_delay; ++i) __builtin_amdgcn_s_sleep(1);
                    for (int base = 0; base < c_nslots; base += CSL * T) {
                        // (a partial sum that arrives goes to LDS at once -- nobody reads SL before
                        // the barrier below -- so only "still wanted" is kept per slot)
                        bool need[CSL];
#pragma unroll
                        for (int q = 0; q < CSL; ++q) need[q] = base + q * T + tid < c_nslots;
                        const bool live0 = need[0];
                        unsigned spins = 0;
                        while (true) {
                            asm volatile("" ::: "memory");
                            bool ok = true;
                            // all polls of the round in front of its one wait; a slot that has
                            // arrived is not requested again (TILE_NO_POLL)
                            u32x4 t[CSL];
#pragma unroll
                            for (int q = 0; q < CSL; ++q)
                                t[q] = __builtin_amdgcn_raw_buffer_load_b128(
                                    rc_, need[q] ? (base + q * T + tid) * 16 : TILE_NO_POLL, 0, 16);
                            __builtin_amdgcn_sched_barrier(0);
                            // the tags seen in slot 0, for the time-out record
                            const unsigned seen_y = need[0] ? t[0].y : (live0 ? cepoch : 0u);
                            const unsigned seen_w = need[0] ? t[0].w : (live0 ? cepoch : 0u);
#pragma unroll
                            for (int q = 0; q < CSL; ++q) {
                                const bool hit = need[q] && t[q].y == cepoch && t[q].w == cepoch;
                                if (hit)
                                    SL[base + q * T + tid] = __longlong_as_double((long long)(
                                        (unsigned long long)t[q].x | ((unsigned long long)t[q].z << 32)));
                                need[q] = need[q] && !hit;
                                ok &= !need[q];
                            }
                            if (ok || dead) break;
                            if (++spins >= TILE_SPIN_LIMIT) {
                                dead = true;
                                sdead = 1;
                                atomicOr(A.err, 4u);
                                if (atomicCAS(A.err + 1, 0u, 1u) == 0u) {
                                    A.err[8] = (unsigned)tile;
                                    A.err[9] = cepoch;
                                    A.err[10] = 0xffffu;            // a coarse exchange
                                    A.err[11] = (unsigned)(base + tid);
                                    A.err[12] = seen_y;
                                    A.err[13] = seen_w;
                                    A.err[16] = 2u;
                                }
                                break;
                            }
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    KKT_XS(1);      // polls of this thread
                    lds_barrier();
                    KKT_XS(2);      // barrier: the slowest thread's polls
                    dead = sdead != 0;
                    // (the offsets, then the slots of up to CU contributions, then their partial
                    // sums, then the sum; functions with more contributions -- 3-D, vector-valued
                    // spaces -- go on one at a time.  Two functions of a thread, j and j + T, side
                    // by side so that a partly filled second round costs no chain of its own,
                    // were slower, 0.83 us against 0.70: all threads then issue the reads of a
                    // second function that 6 % of them have -- profiles/exchange_chains.md)
                    constexpr int CU = 4;
                    for (int j = tid; j < c_nc; j += T) {
                        const int q0 = CIPc[j], q1 = CIPc[j + 1];
                        int cs[CU];
                        double cp[CU];
#pragma unroll
                        for (int k = 0; k < CU; ++k) cs[k] = CSLc[q0 + k < q1 ? q0 + k : 0];
#pragma unroll
                        for (int k = 0; k < CU; ++k) cp[k] = SL[cs[k]];
                        // (the first partial sum counts as used whatever the predicate says: the
                        // compiler otherwise moves its two reads into a branch of their own
                        // behind the others -- two more round trips)
                        asm volatile("" : "+v"(cp[0]));
                        double a = 0.0;
#pragma unroll
                        for (int k = 0; k < CU; ++k)
                            if (q0 + k < q1) a += cp[k];
                        for (int q = q0 + CU; q < q1; ++q) a += SL[CSLc[q]];
                        RC[j] = a;
                    }
                    lds_barrier();
                    KKT_XS(4);      // coarse residual
                    // ---- the coarse functions this tile owns (j = tile, tile + ntiles, ...): a wave
                    // per function, the product published as a granule of the same exchange number
                    const __amdgpu_buffer_rsrc_t re_ = __builtin_amdgcn_make_buffer_rsrc(
                        (cepoch & 1) ? eg1 : eg0, 0, eg_bytes, 0x00020000);
                    const int ntl = (int)gridDim.x;
                    // (row j only over the columns of its diagonal block, [e_lo[j], e_hi[j]) with
                    // e_lo a multiple of 64: a lane keeps the columns it had, the terms left out
                    // are exact zeros -- kernels.hpp, TileCoarseDev)
                    const gci_p elo = (gci_p)cd->e_lo, ehi = (gci_p)cd->e_hi;
                    if (c_einv_cache && uniform_ptr((const void *)einv) != einv_key) {
                        // (the iterates' barrier above ordered every earlier read of EINVc)
                        for (int i = wave; i < c_nown; i += nwaves) {
                            const int j = tile + i * ntl;
                            const int lo = i == wave ? c_lo0 : elo[j], hi = i == wave ? c_hi0 : ehi[j];
                            const gcd_p row = einv + (size_t)j * c_nc;
                            for (int q = lo + lane; q < hi; q += 64)
                                EINVc[(size_t)i * c_ew + (q - lo)] = row[q];
                        }
                        einv_key = uniform_ptr((const void *)einv);
                        // (a wave reads back only the row it wrote: no barrier needed)
                    }
                    for (int i = wave; i < c_nown; i += nwaves) {
                        double a = 0.0;
                        const int j = tile + i * ntl;
                        const int lo = i == wave ? c_lo0 : elo[j], hi = i == wave ? c_hi0 : ehi[j];
                        if (c_einv_cache) {
                            // both operands of EG terms of the lane in front of their part of the
                            // chain (a dead term reads the group's first).  (Six entries ahead
                            // was slower while this variant kept 27 registers in scratch -- 128
                            // its/s against 133; it has none there now, profiles/exchange_chains.md)
                            constexpr int EG = 6;
                            const double *row = EINVc + (size_t)i * c_ew;
                            for (int qb = lo + lane; qb < hi; qb += 64 * EG) {
                                double rv[EG], xc[EG];
#pragma unroll
                                for (int u = 0; u < EG; ++u) {
                                    const int q = qb + 64 * u < hi ? qb + 64 * u : qb;
                                    rv[u] = row[q - lo];
                                    xc[u] = RC[q];
                                }
#pragma unroll
                                for (int u = 0; u < EG; ++u)
                                    if (qb + 64 * u < hi) a = __builtin_fma(rv[u], xc[u], a);
                            }
                        } else {
                            // rows from L2: eight loads of a lane in flight before the first fma
                            const gcd_p row = einv + (size_t)j * c_nc;
                            constexpr int EU = 8;
                            for (int q0 = lo + lane; q0 < hi; q0 += 64 * EU) {
                                double rv[EU];
#pragma unroll
                                for (int u = 0; u < EU; ++u) {
                                    const int q = q0 + 64 * u;
                                    rv[u] = q < hi ? row[q] : 0.0;
                                }
#pragma unroll
                                for (int u = 0; u < EU; ++u) {
                                    const int q = q0 + 64 * u;
                                    if (q < hi) a = __builtin_fma(rv[u], RC[q], a);
                                }
                            }
                        }
                        a = wave_sum_lane0(a);
                        if (lane == 0) publish(re_, tile + i * ntl, a, cepoch);
                    }
                    KKT_XS(5);      // owned products + publish
                    // ---- the products for the functions the own rows touch, from their owners
                    // (ring form: and for those its ring rows touch)
                    for (int k0 = 0; k0 < c_njp; k0 += T) {
                        const int k = k0 + tid;
                        u32x4 g = u32x4{0u, 0u, 0u, 0u};
                        unsigned spins = 0;
                        while (true) {
                            asm volatile("" ::: "memory");
                            bool ok = true;
                            if (k < c_njp && (g.y != cepoch || g.w != cepoch)) {
                                g = __builtin_amdgcn_raw_buffer_load_b128(re_, JGc[k] * 16, 0, 16);
                                ok = g.y == cepoch && g.w == cepoch;
                            }
                            if (__all(ok) || dead) break;
                            if (++spins >= TILE_SPIN_LIMIT) {
                                dead = true;
                                sdead = 1;
                                atomicOr(A.err, 4u);
                                if (atomicCAS(A.err + 1, 0u, 1u) == 0u) {
                                    A.err[8] = (unsigned)tile;
                                    A.err[9] = cepoch;
                                    A.err[10] = 0xfffeu;            // products of a coarse exchange
                                    A.err[11] = (unsigned)(k < c_njp ? JGc[k] : 0);
                                    A.err[12] = g.y;
                                    A.err[13] = g.w;
                                    A.err[16] = 2u;
                                }
                                break;
                            }
                            __builtin_amdgcn_s_sleep(1);
                        }
                        if (k < c_njp)
                            EC[k] = __longlong_as_double((long long)(
                                (unsigned long long)g.x | ((unsigned long long)g.z << 32)));
                    }
                    lds_barrier();
                    dead = sdead != 0;
                    KKT_XS(6);      // products polled + barrier
                    // ---- prolongation onto the own rows of the current iterate
                    double *Xc = X + cur * nkp;
                    if (c_rings) {
                        // ... and onto the ring rows: a ring row's chain is its owner's (entries
                        // in the order of P's row, the owners' products), so the value is the one
                        // a hand-off would fetch.  Later cycles: the hand-off in front of the
                        // residual left the current iterate on every ring.
                        // (two rows of a thread, l and l + T, side by side were slower, as in
                        // the coarse residual: few threads have a second row)
                        for (int l = tid; l < nk; l += T) {
                            const int e0 = PIPc[l], e1 = PIPc[l + 1];
                            const double xo = Xc[l];
                            const double a = prolong_row<4>(e0, e1, PKc, PWc, EC);
                            Xc[l] = cyc == 0 ? a : xo + a;
                        }
                    } else {
#pragma unroll
                    for (int sl = 0; sl < RPT; ++sl) {
                        const int r = sl * T + tid;
                        if (r < n0) {
                            double a = 0.0;
                            if (c_cached) {
                                a = prolong_row<4>(pe0[sl], pe1[sl], PKc, PWc, EC);
                            } else {
                                const gcu16_p pk = (gcu16_p)cd->p_k + c_pq0;
                                const gcd_p pw = (gcd_p)cd->p_w + c_pq0;
                                for (int e = pe0[sl]; e < pe1[sl]; ++e)
                                    a = __builtin_fma(pw[e], EC[pk[e]], a);
                            }
                            Xc[r] = cyc == 0 ? a : Xc[r] + a;
                        }
                    }
                    }
                }
                // the first sweep's row count (a full round follows) and coefficients, read in
                // front of the barrier; the table was written at the start of the level, behind
                // barriers long past
                int nv_next = sn[depth - 1];
                double cn1 = scoef[0], cn2 = scoef[1], cn3 = scoef[2];
                // The level matrix, requested at the level's start behind the update (or in front
                // of the hand-off that ended the level before), is pinned in registers here: the
                // one place where a level waits for it, with the exchange between the request and
                // this point.  No step of the sweep loop below then waits for memory on its own.
                // (later cycles: nothing is in flight, the pin costs nothing)
#pragma unroll
                for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                    for (int k = 0; k < W; ++k) asm volatile("" : "+v"(v[sl][k]));
                // (the barrier inside the hand-off orders these stores before anyone's gathers)
                lds_barrier();
                KKT_XS(3);      // prolongation, the pin of the level matrix, barrier
                if (stamps) {      // the coarse exchange, restriction to prolongation: slot 7
                    const unsigned long long now = wall_clock64();
                    if (tid == 0) sstat[7] += now - t_mark;
                    t_mark = now;
                }
                // (ring form: every local row holds the corrected iterate already)
                if (!c_rings) handoff(false);
                cr = depth;
                // ---- smoothing sweeps from the corrected iterate
                // (row count and coefficients of a step are read from LDS one step ahead, as in the
                // plain steps below: they land with the barrier's own wait)
                for (int s = 1; s <= its; ++s) {
                    if (cr == 0) {
                        handoff(s >= 2);
                        cr = depth;
                    }
                    const bool last = cyc + 1 == A.cycles && s == its;
                    cstep(0, nv_next, cn1, cn2, cn3, s >= 2, last ? post1 : 1.0, last ? post2 : 1.0);
                    if (s < its) {
                        nv_next = sn[(cr - 1 == 0 ? depth : cr - 1) - 1];
                        cn1 = scoef[3 * s];
                        cn2 = scoef[3 * s + 1];
                        cn3 = scoef[3 * s + 2];
                    }
                    lds_barrier();
                    cur ^= 1;
                    --cr;
                }
            }
        } else {
            // ---- Chebyshev steps 2 .. its, `depth` of them per hand-off
            // (row count and coefficients of a step are read from LDS one step ahead: they land with
            // the barrier's own wait instead of in front of the step's gathers)
            int nv_next = sn[(cr == 0 ? depth : cr) - 1];
            double cn1 = scoef[0], cn2 = scoef[1], cn3 = scoef[2];
            bool early_done = false;   // the step before published the own rows already
            for (int s = 2; s <= its; ++s) {
                if (cr == 0) {
                    handoff(s >= 3, early_done);
                    early_done = false;
                    cr = depth;
                    // the last round of the level: the next level's operands travel under it
                    if (PRE && has_next && its - s < depth) prefetch_level(Nf);
                }
                const int nv = nv_next;
                const double cf1 = cn1, cf2 = cn2, cf3 = cn3;
                const bool last = s == its;
                const double q1 = last ? post1 : 1.0, q2 = last ? post2 : 1.0;
                const bool has_old = s >= 3;
                double *Xc = X + cur * nkp, *Xo = X + (cur ^ 1) * nkp;
                // a hand-off follows this step inside the level
                // (wide rows only -- on narrow rows at depth 5-7 the stores in the step cost more
                // than the hand-off gains: 0.45 -> 0.51 us per step, 3.58 -> 3.37 us per hand-off)
                const bool pub_next = PACK && cr == 1 && s < its;
                const bool pub_drop =
                    tile == 0 && A.debug_drop > 0 && (int)(epoch + 1 - A.epoch0) == A.debug_drop;
                early_done = pub_next;
                const __amdgpu_buffer_rsrc_t rn_next = __builtin_amdgcn_make_buffer_rsrc(
                    (void *)A.gnew[(epoch + 1) & 1], 0, (int)A.granule_bytes, 0x00020000);
                if constexpr (PACK) {
    #pragma unroll
                    for (int sl = 0; sl < RPT; ++sl) {
                        // wave-uniform: none of this wave's 64 rows of the slot is live on the
                        // shrunken region
                        if (sl * T + (tid & ~63) >= nv) continue;
                        const int r = sl * T + tid;
                        double acc = 0.0;
    #pragma unroll
                        for (int k0 = 0; k0 < W; k0 += CH) {
                            // (wide rows: a bounded number of gathers in flight, or the registers of
                            // the matrix values spill)
                            double xv[CH];
    #pragma unroll
                            for (int k = 0; k < CH; ++k)
                                if (k0 + k < W) xv[k] = Xc[KKT_COL(sl, k0 + k)];
    #pragma unroll
                            for (int k = 0; k < CH; ++k)
                                if (k0 + k < W) acc = __builtin_fma(v[sl][k0 + k], xv[k], acc);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (r < nv) {
                            const double e0 = Xo[r], e1 = Xc[r];
                            double out = 0.0;
                            if (!msk[sl])
                                out = epi_cheb(has_old, cf1, e0, true, cf2, e1, cf3, dinv[sl], b[sl],
                                               acc, q1, q2);
                            Xo[r] = out;
                            // last step of a round: the own rows leave at once, with the number of
                            // the hand-off that follows (the rest of the step runs under their flight)
                            if (pub_next && !pub_drop && r < n0)
                                publish(rn_next, gr[sl], out, epoch + 1);
                        }
                    }
                } else {
                    // Narrow rows: a step is a latency chain (gather, W dependent fmas, epilogue,
                    // store, barrier), not a throughput problem -- the slots of a thread run side by
                    // side: every gather of every live slot is issued before the first fma.  Live
                    // slots are a prefix (rows of a slot lie behind those of the one before); a wave
                    // none of whose 64 rows of a slot is live on the shrunken region skips the slot.
                    int nl = 0;
                    long long keep[RPT];
    #pragma unroll
                    for (int sl = 0; sl < RPT; ++sl) {
                        if (sl * T + (tid & ~63) < nv) nl = sl + 1;
                        keep[sl] = msk[sl] ? 0ll : -1ll;
                        asm volatile("" : "+v"(keep[sl]));
                    }
                    auto body = [&](auto NLc) {
                        constexpr int NL = decltype(NLc)::value;
                        double xv[NL][W], e0[NL], e1[NL], acc[NL];
    #pragma unroll
                        for (int sl = 0; sl < NL; ++sl) {
    #pragma unroll
                            for (int k = 0; k < W; ++k) xv[sl][k] = Xc[KKT_COL(sl, k)];
                            const int r = sl * T + tid;
                            e0[sl] = Xo[r];
                            e1[sl] = Xc[r];
                            acc[sl] = 0.0;
                        }
                        __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                        for (int k = 0; k < W; ++k)
    #pragma unroll
                            for (int sl = 0; sl < NL; ++sl)
                                acc[sl] = __builtin_fma(v[sl][k], xv[sl][k], acc[sl]);
    #pragma unroll
                        for (int sl = 0; sl < NL; ++sl) {
                            const int r = sl * T + tid;
                            // The one copy of the epilogue left in the kernels: it restates
                            // epi_cheb(has_old, cf1, e0, true, cf2, e1, cf3, dinv, b, acc, q1, q2)
                            // (epilogue.hpp) and is held to it bit for bit by the tile plans of
                            // tests/test_gpu_sweep_forms.py.  With the call in its place the compiler
                            // shares more code between the bodies of the slot counts: the 512-thread
                            // kernels of W = 5 / 7 / 9 with two (three) slots come out one (two)
                            // v_mul_f64 and v_fmac_f64 shorter -- 44 -> 43 and 22 -> 21 (W = 5, two
                            // slots) up to 97 -> 95 and 38 -> 36 (W = 9, three) -- and a kernel here
                            // must keep its instruction mix (profiles/one_epilogue.md).
                            // (boundary rows: a bit mask, not a branch or a select the compiler
                            // turns into one -- a branch per slot would put the chains of the slots
                            // one behind the other again)
                            double t = has_old ? cf1 * e0[sl] : 0.0;
                            t += cf2 * e1[sl];
                            t += cf3 * (dinv[sl] * (b[sl] - acc[sl]));
                            const double out = __longlong_as_double(
                                __double_as_longlong(q2 * (q1 * t)) & keep[sl]);
                            // rows behind the live region store into a dump slot: an unconditional
                            // store keeps the compiler from sinking the chain into a branch per slot
                            *(r < nv ? Xo + r : dump) = out;
                        }
                    };
                    if (nl == 1) body(std::integral_constant<int, 1>{});
                    if constexpr (RPT >= 2)
                        if (nl == 2) body(std::integral_constant<int, 2>{});
                    if constexpr (RPT >= 3)
                        if (nl == 3) body(std::integral_constant<int, 3>{});
                }
                if (s < its) {
                    const int crn = cr - 1 == 0 ? depth : cr - 1;
                    nv_next = sn[crn - 1];
                    cn1 = scoef[3 * (s - 1)];
                    cn2 = scoef[3 * (s - 1) + 1];
                    cn3 = scoef[3 * (s - 1) + 2];
                }
                lds_barrier();
                cur ^= 1;
                --cr;
            }
        }
        lap(1, (unsigned long long)(its - 1));
        if constexpr (SEQ && COARSE) {
            // (`v` landed long ago, but the compiler cannot know that the cycle loop with its pin
            // ran at all: without this one it waits -- vmcnt(0) -- before the requests below
            // overwrite `v`, and what that wait then drains is the result store in front of them)
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl)
#pragma unroll
                for (int k = 0; k < W; ++k) asm volatile("" : "+v"(v[sl][k]));
        }
        // ---- result of the level: own rows to memory; the next level's update multiplies it
        {
            double *Xc = X + cur * nkp;
            const gd_p op = (gd_p)L.out;
#pragma unroll
            for (int sl = 0; sl < RPT; ++sl) {
                const int r = sl * T + tid;
                if (r < n0) op[idx(gr[sl])] = Xc[r];
            }
            if (lev + 1 < A.nlevels) {
                if (!nf_valid) Nf = read_early(&levels[lev + 1]);
                nf_want = nullptr;
                const LevEarly &N = Nf;
                if constexpr (SEQ && COARSE) {
                    // one run of requests for either kind of next level -- the first term of its
                    // update or, without one, its matrix: two branches that both write `v` make
                    // the compiler wait in front of the second for loads the first may have
                    // issued, and that wait drains the result store above
                    // (narrow rows, next level on the matrix `v` holds -- operators that do not
                    // change in time, stored once: `v` stays and the update reads its matrix from
                    // memory, out of L2, as all further terms do.  Passing it through `v` there
                    // means requesting the level matrix again at every level, and on the flagship
                    // stored that way it measured 1.2 % slower: profiles/level_fetch.md)
                    const bool upd = N.n_upd > 0 &&
                                     (PACK || uniform_ptr((const void *)N.vals) != vals_key);
                    const double *src = upd ? N.upd0 : N.vals;
                    if (upd || uniform_ptr((const void *)src) != vals_key) load_vals(src, upd);
                    load_db(N);
                    v_is_u = upd;
                } else if (!(PRE && pre_issued)) {
                    if (SEQ && N.n_upd > 0) {
                        load_vals(N.upd0, true);
                        load_db(N);
                        v_is_u = true;
                    } else {
                        load_level(N);
                        if constexpr (PRE_U) load_un(N);
                    }
                }
                if (N.n_upd > 0 && N.prev_in_lds) handoff(false);
                if (PRE && pre_issued) adopt_level(N);
            }
        }
    }
    if (stamps && tid == 0)
        for (int i = 0; i < 8; ++i) stat[i] += sstat[i];
}

#undef KKT_COL
#undef KKT_CPK
#undef KKT_GP

typedef void (*tile_fn)(const TileArgs, const TileLevel *, const int32_t *, const int32_t *,
                        const uint16_t *, const int32_t *, const uint8_t *);
// Register budget per thread by workgroup size: 512 threads -> 256, 1024 -> 128.  Narrow rows
// (2-D P1) run 512 threads with up to three row slots or 1 024 with one, level update fused.
// Wide rows (3-D P1: 15 entries, 30 registers of matrix values per row slot) run 512 threads with
// two slots in the variant without the fused update (244 registers; with it 256 + 78 spilled).
static tile_fn pick_tile_coarse(int W, int rpt, int threads, int hslots);
static tile_fn pick_tile(int W, int rpt, int threads, bool fused = true, int hslots = 0,
                         bool coarse = false) {
    if (coarse) return fused ? pick_tile_coarse(W, rpt, threads, hslots) : nullptr;
    if (hslots <= 0) hslots = 1;
#define KKT_T(w)                                                           \
    if (W == w) {                                                          \
        if (threads <= 512) {                                              \
            switch (rpt) {                                                 \
                case 1: return pc_tile_sweep<w, 1, 512, true>;             \
                case 2: return pc_tile_sweep<w, 2, 512, true>;             \
                case 3: return pc_tile_sweep<w, 3, 512, true>;             \
                default: return nullptr;                                   \
            }                                                              \
        }                                                                  \
        return rpt == 1 ? pc_tile_sweep<w, 1, 1024, true> : nullptr;       \
    }
    KKT_T(5) KKT_T(7) KKT_T(9)
#undef KKT_T
    // Wide rows: with the level update (one term, its matrix passing through the registers of
    // the level matrix) or without (the update stays a plain launch, one tile launch per level)
    // 3-D tiles whose rows and ring fit one slot each: 1 024 threads (16 waves hide the step's
    // latency chain better than 8 with two slots)
    if (W == 15 && threads > 512 && rpt == 1 && hslots <= 1)
        return fused ? pc_tile_sweep<15, 1, 1024, true, 1> : pc_tile_sweep<15, 1, 1024, false, 1>;
    if (W == 15 && threads <= 512) {
        if (rpt == 1) return fused ? pc_tile_sweep<15, 1, 512, true> : pc_tile_sweep<15, 1, 512, false>;
        if (rpt == 2) return fused ? pc_tile_sweep<15, 2, 512, true> : pc_tile_sweep<15, 2, 512, false>;
    }
    // P2 velocity blocks (9 or 19 entries per row, row-sorted storage): one row slot
    if (W == 19 && threads <= 512 && rpt == 1)
        return fused ? pc_tile_sweep<19, 1, 512, true> : pc_tile_sweep<19, 1, 512, false>;
    if (W == 19 && threads <= 512 && rpt == 2)      // 215 registers
        return fused ? pc_tile_sweep<19, 2, 512, true> : pc_tile_sweep<19, 2, 512, false>;
    if (W == 19 && threads > 512 && threads <= 768 && rpt == 1)
        return fused ? pc_tile_sweep<19, 1, 768, true> : pc_tile_sweep<19, 1, 768, false>;
    return nullptr;
}

// variants with coarse corrections (two-grid levels), level update fused
static tile_fn pick_tile_coarse(int W, int rpt, int threads, int hslots) {
    if (hslots <= 0) hslots = 1;
#define KKT_TC(w)                                                                  \
    if (W == w) {                                                                  \
        if (threads <= 512) {                                                      \
            switch (rpt) {                                                         \
                case 1: return pc_tile_sweep<w, 1, 512, true, 2, true>;            \
                case 2: return pc_tile_sweep<w, 2, 512, true, 3, true>;            \
                case 3: return pc_tile_sweep<w, 3, 512, true, 4, true>;            \
                default: return nullptr;                                           \
            }                                                                      \
        }                                                                          \
        return rpt == 1 ? pc_tile_sweep<w, 1, 1024, true, 2, true> : nullptr;      \
    }
    KKT_TC(5) KKT_TC(7) KKT_TC(9)
#undef KKT_TC
    if (W == 15 && threads > 512 && rpt == 1 && hslots <= 1)
        return pc_tile_sweep<15, 1, 1024, true, 1, true>;
    if (W == 15 && threads <= 512) {
        if (rpt == 1) return pc_tile_sweep<15, 1, 512, true, 2, true>;
        if (rpt == 2) return pc_tile_sweep<15, 2, 512, true, 3, true>;
    }
    if (W == 19 && threads <= 512 && rpt == 1) return pc_tile_sweep<19, 1, 512, true, 2, true>;
    if (W == 19 && threads <= 512 && rpt == 2) return pc_tile_sweep<19, 2, 512, true, 3, true>;
    // (two-grid levels are short chains of steps: 16 waves with one row each run a step's 19
    // gathers in half the time of 8 waves with two)
    if (W == 19 && threads > 512 && threads <= 768 && rpt == 1)
        return pc_tile_sweep<19, 1, 768, true, 2, true>;
    return nullptr;
}

bool tile_sweep_coarse_available(int W, int rpt, int threads, int hslots) {
    return threads >= 64 && threads <= 1024 && threads % 64 == 0 && hslots <= rpt + 1 &&
           pick_tile_coarse(W, rpt, threads, hslots) != nullptr;
}

bool tile_sweep_fuses_update(int W, int max_terms) {
    return W <= 9 || ((W == 15 || W == 19) && max_terms <= 1);
}

size_t tile_sweep_lds_bytes(int nk_pad, int its, int coarse_nc, int coarse_nslots, int coarse_jmax,
                            int coarse_nr_max, int coarse_einv_rows, int coarse_einv_width,
                            int coarse_ring_entries, int coarse_jxmax) {
    if (coarse_nc > 0 && coarse_einv_rows > 0)
        return tile_sweep_lds_bytes(nk_pad, its, coarse_nc, coarse_nslots, coarse_jmax,
                                    coarse_nr_max, 0, 0, coarse_ring_entries, coarse_jxmax) +
               (size_t)coarse_einv_rows * (coarse_einv_width > 0 ? coarse_einv_width : coarse_nc) *
                   sizeof(double) + 8;
    if (coarse_nc > 0) {
        // ring form: products of J_t+ instead of J_t, the ring rows' entries behind the own rows',
        // per-row entry offsets of all local rows
        const bool rings = coarse_jxmax > 0;
        const size_t jx = rings ? (size_t)coarse_jxmax : (size_t)coarse_jmax;
        const size_t np = (size_t)coarse_nr_max + (rings ? (size_t)coarse_ring_entries : 0);
        const size_t pip = rings ? (size_t)nk_pad + 1 : 0;
        return (2 * (size_t)nk_pad + 3 * (size_t)std::max(1, its) + 1 + (size_t)coarse_nslots +
                (size_t)coarse_nc + jx + (size_t)coarse_nr_max + np) * sizeof(double) +
               ((size_t)coarse_nslots + (size_t)coarse_nc + 1 + (size_t)coarse_jmax + 1 + jx + pip) *
                   sizeof(int) +
               ((size_t)coarse_nr_max + np) * sizeof(uint16_t) + 16;
    }
    return (2 * (size_t)nk_pad + 3 * (size_t)std::max(1, its - 1) + 1) * sizeof(double);
}

size_t tile_sweep_lds_bytes(int nk_pad, int its, const TileCoarseDev &c, int cache, bool rings) {
    const bool r = rings && cache >= 1;
    return tile_sweep_lds_bytes(nk_pad, its, c.nc, c.nslots, c.jmax, cache >= 1 ? c.nr_max : 0,
                                cache == 2 ? c.nown : 0, c.ew, r ? c.np_max - c.nr_max : 0,
                                r ? c.jxmax : 0);
}

size_t tile_sweep_lds_bytes(int nk_pad, int its, const TileCoarseDev &c) {
    return tile_sweep_lds_bytes(nk_pad, its, c, c.cache_einv ? 2 : c.cache_lists ? 1 : 0,
                                c.ring_prolong != 0);
}

int tile_sweep_max_rpt(int W, int threads) {
    int best = 0;
    for (int rpt = 1; rpt <= 4; ++rpt)
        if (pick_tile(W, rpt, threads, true, 1)) best = rpt;
    return best;
}

int tile_sweep_max_hslots(int W, int rpt, int threads) {
    int best = 0;
    for (int h = 1; h <= rpt + 1; ++h)
        if (pick_tile(W, rpt, threads, true, h)) best = h;
    return best;
}

bool tile_sweep_available(int W, int rpt, int threads, int hslots) {
    return threads >= 64 && threads <= 1024 && threads % 64 == 0 && hslots <= rpt + 1 &&
           pick_tile(W, rpt, threads, true, hslots) != nullptr;
}

int tile_sweep_max_tiles(int W, int rpt, int threads, size_t lds_bytes, int hslots, bool coarse) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    // both variants of a width (with / without the level update) must be resident
    // (coarse: the one variant with corrections)
    for (int fused = coarse ? 1 : 0; fused < 2; ++fused) {
        tile_fn f = pick_tile(W, rpt, threads, fused != 0, hslots, coarse);
        int per_cu = 0;
        if (!f) return 0;
        if (lds_bytes > 48 * 1024 &&
            hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes) != hipSuccess)
            return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, lds_bytes) != hipSuccess)
            return 0;
        if (per_cu < 1) return 0;
    }
    return cus;   // one workgroup per CU
}

void launch_tile_sweep(hipStream_t s, const TileArgs &a, const TileLevel *d_levels,
                       const int32_t *d_n, const int32_t *d_grow, const uint16_t *d_lcol,
                       const int32_t *d_gpos, const uint8_t *d_rowmask, int ntiles, int threads,
                       size_t granule_words, const TileCoarseDev *h_coarse) {
    if (a.nlevels <= 0 || ntiles <= 0) return;
    // tags of an earlier application must not match this one's hand-off numbers
    auto chk = [](hipError_t e, const char *what) {
        if (e != hipSuccess)
            throw TileLaunchError{std::string("tile sweep program: ") + what + ": " +
                                  hipGetErrorString(e)};
    };
    (void)hipGetLastError();
    if (a.clear) {
        if (a.clear & 1)
            for (int i = 0; i < 2; ++i) {
                launch_zero_bytes(s, a.gnew[i], granule_words * sizeof(unsigned long long));
                launch_zero_bytes(s, a.gold[i], granule_words * sizeof(unsigned long long));
            }
        if (h_coarse && (a.clear & 2))
            for (int i = 0; i < 2; ++i) {
                launch_zero_bytes(s, h_coarse->cg[i], h_coarse->cg_bytes);
                launch_zero_bytes(s, h_coarse->eg[i], h_coarse->eg_bytes);
            }
        chk(hipGetLastError(), "clearing the granule buffers");
    }
    const size_t lds = h_coarse ? tile_sweep_lds_bytes(a.nk_pad, a.its, *h_coarse)
                                : tile_sweep_lds_bytes(a.nk_pad, a.its);
    tile_fn f = pick_tile(a.W, a.rpt, threads, a.fused_update != 0, a.hslots, h_coarse != nullptr);
    if (!f) throw TileLaunchError{"tile sweep program: no kernel variant for this plan"};
    (void)hipGetLastError();
    hipLaunchKernelGGL(f, dim3(ntiles), dim3(threads), lds, s, a, d_levels, d_n, d_grow, d_lcol,
                       d_gpos, d_rowmask);
    chk(hipGetLastError(), "launch");
}

}  // namespace kkt
