// Device-kernel interface of libkkt (host-callable launchers).  gfx950 only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <algorithm>

#include <string>

#include "chebyshev.hpp"

namespace kkt {

// thrown by launch_tile_sweep when a memset or the launch itself fails (never silently)
struct TileLaunchError {
    std::string msg;
};

constexpr int MAX_TERMS = 8;      // blocks summed into one block row by one launch
constexpr int MDOT_MAX = 8;       // vectors per fused multi-dot / multi-axpy pass
constexpr int REDUCE_BLOCKS = 1024;  // fixed partial count -> deterministic reductions

// Reference to a vector operand.  base < 0: null; base == 0: `off` holds an absolute
// device pointer; base >= 1: element offset `off` from Bases::p[base - 1], which the
// caller supplies per launch (so one RowOp array serves any input/output vector).
struct VRef {
    int64_t off;
    int32_t base;
    int32_t pad_;
};
struct Bases { const double *p[4]; };

struct SpmvTerm {
    const double *vals;   // padded SELL values (layout of the RowOp's pattern)
    VRef x;               // the column block's vector (length ncols)
};

enum EpiMode : int32_t { EPI_LIN = 0, EPI_CHEB = 1 };

// One block-row operation.  Arrays of RowOp live in device memory; one launch executes
// many of them (blockIdx.y selects the RowOp).  acc = sum_t A_t x_t is accumulated
// term-major with one fused-multiply-add chain per row, in CSR order within a term --
// the order of the reference's sequence of MatMultAdd calls (preconditioner.py:406-432).
// The epilogues and their rounding sequence: epilogue.hpp, the one definition every kernel calls.
struct RowOp {
    const int32_t *col;        // SELL column indices of the shared pattern
    const int32_t *slice_off;  // nslices + 1 offsets, in slots
    const int32_t *perm;       // row stored at each position (-1: none), null: position == row
    int32_t nrows, nslices, nterms, mode;
    int32_t uniform_w;         // >= 0: every slice has this width (slice_off unused)
    int32_t pad0_;
    SpmvTerm t[MAX_TERMS];
    VRef y;
    VRef y2;                   // EPI_LIN only, optional: y2 = c3 * dinv * y
    // EPI_LIN:  y = ca*acc + cy*yin + cz*z;  masked rows: y = malpha * mx[r] (0 if !mx)
    double ca, cy, cz;
    VRef yin, z;
    const uint8_t *rowmask;
    VRef mx;
    double malpha;
    // EPI_CHEB: y = post2*(post1*(c1*pkm1 + c2*pk + c3*dinv*(b - acc))); masked rows use
    //           the exact result of the bc-assembled matrix on a bc-clean rhs: 0
    VRef b, pkm1, pk;
    const double *dinv;
    double c1, c2, c3, post1, post2;
};

// XCD-aware workgroup order of the operator launches (tag 0; tag 1 ignores it), per handle:
// ragged kernels (option "ragged_xcd", default on) and fixed-width ones (option "apply_xcd",
// default off).  Ragged: P2 0.507 -> 0.46-0.48 ms, Stokes outer operator 0.778 -> 0.729 ms.
// (On the fixed-width P1 launches the same relabelling was slower, profiles/DIARY_r01_r02.md
// 8.1b: their traffic is 1.1 x the bytes already; the ragged launches fetched 1.4 x.)
struct XcdOrder { bool ragged = false, fixed = false; };
// Which kernel and instantiation a launch of the preconditioner's row steps gets: the launchers
// below dispatch on these answers, and kkt_debug_row_step / kkt_debug_pc_forms report them.
enum RowFamily : int32_t { ROW_PC_ROWS = 0, ROW_PC_ROW_STEP = 1, ROW_PC_ROWS_SHARED = 2,
                           ROW_PC_ROWS_SHARED_G = 3, ROW_PC_ROWS_IL = 4 };
struct RowKernel {
    RowFamily family;
    int width;               // the instantiation's width argument
    bool declined = false;   // the launcher launches nothing and says so (launch_rowops_shared)
};
// launch_rowops with tag 1: pc_rows<R, WFIX>, or pc_row_step<R, WFIX> for one op that rides in the
// kernel arguments; WFIX 0: the slot loop
inline RowKernel rows_kernel(int R, int uniform_w, int nops, bool single) {
    return {single && nops == 1 ? ROW_PC_ROW_STEP : ROW_PC_ROWS,
            R == 2 && uniform_w >= 1 && uniform_w <= 16 ? uniform_w : 0};
}
// launch_rowops_shared: pc_rows_shared<W, 4>, or pc_rows_shared_g<4, 4> for any other width; it
// serves R = 2 and at least four ops
inline RowKernel shared_kernel(int R, int uniform_w, int nops) {
    const bool declined = R != 2 || nops < 4;
    if (uniform_w >= 1 && uniform_w <= 8) return {ROW_PC_ROWS_SHARED, uniform_w, declined};
    return {ROW_PC_ROWS_SHARED_G, 4, declined};
}
// launch_rowops_il: pc_rows_il<8> or pc_rows_il<4>
inline RowKernel il_kernel(int uniform_w) {
    return {ROW_PC_ROWS_IL, uniform_w >= 1 && uniform_w <= 8 ? 8 : 4};
}
void launch_rowops(hipStream_t s, const RowOp *d_ops, int nops, int max_slices, int R,
                   const Bases &bases, int tag, int uniform_w,
                   const RowOp *h_single = nullptr, XcdOrder xcd = {});
// uniform_w of a launch of ragged structures whose slots lie (>= 75 %) in slices of a width
// ragged_switch_width() accepts: the operator apply then runs kkt_spmv_rows_ragged, where a wave
// picks the body unrolled for its slice's width (other widths: the slot loop, in the same kernel)
constexpr int UNIFORM_W_SWITCH = -2;
// the same with one wave per workgroup, for launches of wide slices (mean width >= 10): the slices
// of a sort window differ in width (P2: 19, 19, 12, 9, 9, ...) and a four-wave workgroup holds its
// registers until its widest slice is done (P2: 0.565 -> 0.510 ms); narrow slices (the B^T blocks
// of the Stokes system: 4 / 5 / 7) move too few bytes per wave to be dispatched one by one
constexpr int UNIFORM_W_SWITCH_1WAVE = -3;
// every slice of the launch at most 7 wide: kkt_spmv_rows_ragged_narrow (bodies 3 .. 7 only, so
// that more waves are resident)
constexpr int UNIFORM_W_SWITCH_NARROW = -4;
bool ragged_switch_width(int w);

// Batched Chebyshev steps on ONE matrix with the iterates of four time levels interleaved
// (element (row r, level l) of a group at 4 r + l): a gather serves four levels with one 32-byte
// load instead of four 8-byte ones.  Right-hand sides and final outputs keep the API layout.
struct IlOp {
    const int32_t *col, *slice_off, *perm;
    const double *vals, *dinv;
    const uint8_t *rowmask;
    int32_t nrows, nslices, uniform_w, nlev;   // nlev <= 4 levels in this group
    const double *b[4];        // right-hand sides of the levels
    double *out[4];            // out[0] != null: the step writes the levels' outputs (last step)
    const double *x;           // interleaved p_k (null: first step, no matrix term)
    const double *pkm1;        // interleaved p_{k-1} or null
    double *y;                 // interleaved output (when out[0] == null)
    double c1, c2, c3;
    double post1[4], post2[4]; // per level (the last step's output scalings)
};
// (xcd: the XCD-aware workgroup order of the batched preconditioner steps, option "pc_xcd")
void launch_rowops_il(hipStream_t s, const IlOp *d_ops, int ngroups, int max_slices, int uniform_w,
                      bool xcd);

// Batched launch for RowOps that all have ONE term with the same matrix and pattern
// (uniform width 1..8, R = 2): four time levels per thread.  Returns false if not applicable.
// (xcd: as for launch_rowops_il)
bool launch_rowops_shared(hipStream_t s, const RowOp *d_ops, int nops, int max_slices, int R,
                          int uniform_w, bool xcd);

// Operator apply for shared values: d_groups[g] = {first op, count <= 4} of runs of EPI_LIN RowOps
// with identical structure (same pattern, same term matrices); fixed slice widths 1..8, R = 2.
constexpr int ROW_GROUP_MAX = 4;
// the launches kkt_spmv_rows_shared serves (launch_rowops_grouped; else the plain kernel runs)
inline bool rowops_grouped_kernel(int R, int uniform_w) { return R == 2 && uniform_w >= 1 && uniform_w <= 8; }
bool launch_rowops_grouped(hipStream_t s, const RowOp *d_ops, const int32_t *d_groups, int ngroups,
                           int max_slices, int R, int uniform_w, const Bases &bases);

// One persistent launch that runs `nphases` single-block RowOps in order, workgroup j
// waiting before each phase for the workgroups d_dep[2j] .. d_dep[2j+1] (kernels.hip).
int prog_flag_words(int nwg);
// data-flow form (tagged granules instead of phase counters), uniform widths 1..16 only
bool row_program_g_available(int R, int uniform_w);
int row_program_g_max_wgs(int uniform_w, int waves_per_wg);
// Compact record of a phase, read through the scalar cache one phase ahead.  kind 1 (STEP): a
// Chebyshev step that inherits matrix, diagonal, right-hand side and mask from the previous
// phase, with p_k = the previous phase's output and p_{k-1} (flags bit 0) the one before.
struct PhaseLite {
    uint32_t kind, flags;
    uint64_t y;
    double c1, c2, c3, post1, post2;
    uint64_t pad_;
};
static_assert(sizeof(PhaseLite) == 64, "one scalar cache line");
void launch_row_program_g(hipStream_t s, const RowOp *d_ops, const PhaseLite *d_lite, int nphases,
                          int nwg, int waves_per_wg, int uniform_w, unsigned long long *g0,
                          unsigned long long *g1, size_t granule_words, unsigned *d_err);
int row_program_max_wgs(int R, int uniform_w, int waves_per_wg, bool lowreg = false);
// data-flow form for any width (R = 2): granule hand-off, matrix re-read from L2 every phase
int row_program_gw_max_wgs(int waves_per_wg);
void launch_row_program_gw(hipStream_t s, const RowOp *d_ops, int nphases, int nwg,
                           int waves_per_wg, unsigned long long *g0, unsigned long long *g1,
                           size_t granule_words, unsigned *d_err);
void launch_row_program(hipStream_t s, const RowOp *d_ops, int nphases, int nwg, int waves_per_wg,
                        int R, int uniform_w, const int32_t *d_dep, unsigned *d_flags,
                        unsigned *d_err, bool lowreg = false);

// ---- tile sweep program (tile_kernels.hip; plan: tiles.hpp)
constexpr int TILE_DEPTH_MAX = 16;
// One time level of a sweep: optional update b = ca * (sum_t U_t x_prev) + cy * bin on the
// boundary-masked rows, then `its` Jacobi-Chebyshev steps with the matrix `vals` on b, result in
// `out` (control.py:2263-2295 / 2375-2406: "b_i += M u_{i-1}; solve").
// (128 bytes, aligned: the two scalar-cache lines of a level hold one level only)
struct alignas(128) TileLevel {
    const double *vals;        // SELL values of the level's matrix F_i
    const double *dinv;        // its Jacobi diagonal, inverted (1 on boundary rows)
    const double *bin;         // right-hand side before the update
    double *bout;              // where the updated right-hand side is stored (may be bin; may be null)
    double *out;               // u_i
    const double *x_prev;      // the vector the update multiplies
    const double *upd_vals[2]; // SELL values of the update terms
    int32_t n_upd;             // 0: no update at this level
    int32_t prev_in_lds;       // x_prev is the previous level's `out` (handed over inside the launch)
    double ca, cy;
    double p1_scale;           // first step: p_1 = p1_scale * dinv * b
    double post1, post2;       // factors of the last step
    const TileCoef *coef;      // steps 2 .. its: p_s = c1 p_{s-2} + c2 p_{s-1} + c3 dinv (b - F p_{s-1})
};
// Coarse corrections inside the tile program (two-grid form of the sub-solves): what a tile needs
// to restrict its own rows' residual to the coarse functions they touch (J_t), to publish those
// partial sums, to assemble the whole coarse residual from every tile's partials in a fixed order,
// to apply its rows of (P^T A P)^-1 and to prolong onto its own rows -- and, with `ring_prolong`,
// onto its ring rows as well, from the products of J_t+ = J_t followed by the coarse functions
// that only ring rows touch (no hand-off after a correction then).  Device-resident plan: lists
// from tiles.cpp (build_tile_coarse_lists), uploaded by SchurPC (csrc/pc.cpp, build_tile_coarse).
struct TileCoarseDev {
    int32_t nc, jmax, pstride, nslots;
    int32_t nr_max;               // most restriction (= own-row prolongation) entries of a tile
    int32_t cache_lists;          // 1: every tile copies its entries into LDS (they fit)
    int32_t cache_einv;           // 1: ... and keeps the rows of (P^T A P)^-1 it owns there
    int32_t nown;                 // most coarse functions a tile owns: ceil(nc / ntiles)
    int32_t jxmax;                // max |J_t+|: stride of jglob (= jmax when the lists have no rings)
    int32_t np_max;               // most prolongation entries of a tile, ring rows included
    int32_t ring_prolong;         // 1: tiles prolong onto their rings (needs cache_lists)
    const int32_t *nj;            // [ntiles] number of coarse functions the own rows touch
    const int32_t *njx;           // [ntiles] ... and with those only ring rows touch, >= nj
    const int32_t *jglob;         // [ntiles][jxmax] their global numbers, J_t first
    const int32_t *slot0;         // [ntiles] first slot of the tile's partial sums
    const int32_t *r_ip;          // [ntiles * jmax + 1] restriction lists, per (tile, k) ...
    const uint16_t *r_row;        // ... local own row
    const double *r_w;            // ... and weight, ascending rows
    const int32_t *p_ip;          // [ntiles * pstride + 1] prolongation entries of the local rows
                                  // (own rows first; ring rows have entries only in lists with rings) ...
    const uint16_t *p_k;          // ... index into the tile's J_t+
    const double *p_w;
    const int32_t *c_ip;          // [nc + 1] slots that contribute to a coarse function ...
    const int32_t *c_slot;        // ... ascending (tile order)
    unsigned long long *cg[2];    // granule buffers of the partial sums, 2 words per slot
    uint32_t cg_bytes;
    unsigned long long *eg[2];    // ... and of the products (E^-1 r_c)_j, 2 words per coarse function
    uint32_t eg_bytes;
    // Columns of row j of (P^T A P)^-1 that can be non-zero: [e_lo[j], e_hi[j]), e_lo a multiple of
    // 64.  P^T A P is block diagonal over the connected components of its graph (a vector-valued
    // space: one block per component of the field) and so is its inverse -- Gauss-Jordan with
    // partial pivoting leaves exact zeros outside the blocks -- so the owned products run over the
    // row's block only and the rows kept in LDS are `ew` = max (e_hi - e_lo) long.
    const int32_t *e_lo, *e_hi;
    int32_t ew;
};
constexpr int TILE_COARSE_SLOTS = 8;   // partial-sum slots polled per thread, at most
struct TileArgs {
    const TileCoarseDev *coarse;              // null: plain Chebyshev levels
    const double *const *einv;                // per level: (P^T A P)^-1 of the level's matrix
    int32_t cycles;                           // coarse cycles per level (its = sweeps per cycle)
    uint32_t cepoch0;                         // coarse exchanges of this launch carry tags cepoch0 + 1, ...
    int32_t nlevels, its, depth, nk_pad, rpt, W;
    unsigned long long *gnew[2], *gold[2];   // granule buffers, 2 words per row each
    unsigned granule_bytes;
    unsigned *err;                            // word 0: error bits; words 8..: first time-out record
    int32_t stamps;                           // diagnostics: per-tile 100 MHz tick sums at err + 64
    int32_t poll_delay;                       // s_sleep units between publishing and the first poll
    int32_t debug_drop;                       // test hook: tile 0 skips publishing hand-off number
                                              // debug_drop (> 0), so its neighbours time out
    uint32_t epoch0;                          // hand-offs of this launch carry tags epoch0 + 1, ...
    int32_t clear;                            // host side, before the launch: 1 zero the hand-off
                                              // granule buffers (the first tile launch of a replayed
                                              // sequence), 2 those of the coarse exchanges (its first
                                              // launch with coarse levels)
    int32_t fused_update;                     // 0: kernel variant without the level update
    int32_t hslots;                           // ring-entry slots per thread the plan needs
};
bool tile_sweep_available(int W, int rpt, int threads, int hslots);   // hslots: ring-entry slots per thread
bool tile_sweep_coarse_available(int W, int rpt, int threads, int hslots);   // variant with coarse corrections
int tile_sweep_max_hslots(int W, int rpt, int threads);
int tile_sweep_max_rpt(int W, int threads);   // most row slots per thread of any variant (0: none)
// whether the variant for this shape computes the level update b -= U u_prev itself (narrow
// rows); wide rows (3-D P1) have no registers for it: the update stays a launch of its own
bool tile_sweep_fuses_update(int W, int max_terms);   // update terms of any level of the run
size_t tile_sweep_lds_bytes(int nk_pad, int its, int coarse_nc = 0, int coarse_nslots = 0,
                            int coarse_jmax = 0, int coarse_nr_max = 0,
                            int coarse_einv_rows = 0,
                            int coarse_einv_width = 0,   // rows of the coarse inverse kept in LDS
                            int coarse_ring_entries = 0,  // ring form: entries of the ring rows ...
                            int coarse_jxmax = 0);        // ... and max |J_t+| (0: no ring form)
// the footprint of a coarse plan as the kernel lays it out: `cache` 0 nothing cached, 1 the lists,
// 2 also the rows of the coarse inverse; `rings`: the ring form (needs cache >= 1)
size_t tile_sweep_lds_bytes(int nk_pad, int its, const TileCoarseDev &c, int cache, bool rings);
// ... with the plan's own settings
size_t tile_sweep_lds_bytes(int nk_pad, int its, const TileCoarseDev &c);
// workgroups of `threads` that are certainly co-resident (one per CU)
int tile_sweep_max_tiles(int W, int rpt, int threads, size_t lds_bytes, int hslots,
                         bool coarse = false);
void launch_tile_sweep(hipStream_t s, const TileArgs &a, const TileLevel *d_levels,
                       const int32_t *d_n, const int32_t *d_grow, const uint16_t *d_lcol,
                       const int32_t *d_gpos, const uint8_t *d_rowmask, int ntiles, int threads,
                       size_t granule_words, const TileCoarseDev *h_coarse = nullptr);

// ---- batched one-matrix Chebyshev solves, several steps per launch out of LDS
// (mass_tile_kernels.hip; plan: tiles.hpp with depth = K)
constexpr int MASS_TILE_MAX_DEPTH = 8;
// a group of (at most) four time levels: right-hand sides, outputs and the last step's factors
struct MassTileGroup {
    const double *b[4];
    double *out[4];
    double post1[4], post2[4];
    int32_t nlev, pad_;
};
// One launch: steps s0 + 1 .. s0 + k of every solve.  Iterates between launches: four levels
// interleaved by global row (element (row r, level l) of group g at 4 (g nx + r) + l), read from
// the pair in_*, written to the pair out_* (another pair: other tiles read their rings from in_*).
struct MassTileArgs {
    const int32_t *n, *grow;          // the plan's tables (TilePlan::d_*)
    const uint16_t *lcol;
    const int32_t *masked;            // the Dirichlet rows (the last launch writes their zeros)
    const double *tvals;              // the matrix values in the layout of lcol (launch_mass_tile_gather)
    const double *dinv;
    const MassTileGroup *groups;
    const double *in_new, *in_old;    // p_{s0}, p_{s0 - 1} (unused where s0 is too small)
    double *out_new, *out_old;        // p_{s0 + k}, p_{s0 + k - 1} (not the last launch)
    int64_t nx;
    int32_t nmasked, ngroups, nk_pad, W;
    int32_t s0, k, last, pad_;
    double coef[MASS_TILE_MAX_DEPTH][3];   // c1, c2, c3 of steps s0 + 1 .. s0 + k
};
int mass_tile_kernel_width(int W);     // the variant's width for rows of W entries (0: none)
int mass_tile_max_rpt(int threads);    // row slots per thread the variants of a workgroup size have
size_t mass_tile_lds_bytes(int nk_pad);
// workgroups per CU of the variant for this plan (0: none or it does not fit); raises its LDS limit
int mass_tile_prepare(int W, int rpt, int threads, size_t lds_bytes);
void launch_mass_tile(hipStream_t s, const MassTileArgs &a, int ntiles, int grid_y, int rpt,
                      int threads);
// out[i] = gpos[i] >= 0 ? vals[gpos[i]] : +0.0 for the n entries of a plan's gpos table
void launch_mass_tile_gather(hipStream_t s, const double *vals, const int32_t *gpos, double *out,
                             int64_t n);

// ---- value-array preparation
void launch_csr_to_sell(hipStream_t s, const double *csr_vals, const int32_t *sell2csr,
                        double *sell_vals, int64_t n_padded);
void launch_mask_columns(hipStream_t s, double *sell_vals, const int32_t *col,
                         const uint8_t *colmask, int64_t n_padded);
// out = a + c * b (no fma contraction: matches "assemble(block + c * M)")
void launch_vals_axpy(hipStream_t s, double *out, const double *a, double c,
                      const double *b, int64_t n_padded);
// *flag |= 1 when a and b differ in any bit
void launch_vals_differ(hipStream_t s, const double *a, const double *b, int64_t n, unsigned *flag);
void launch_vals_sym_skew(hipStream_t s, const double *a, const int32_t *tpos, double *h,
                          double *sk, int64_t n, unsigned *nonsym);
// dinv[r] = rowmask[r] ? 1 : 1 / diag(A)[r]
void launch_extract_dinv(hipStream_t s, const int32_t *col, const int32_t *slice_off,
                         const double *vals, const uint8_t *rowmask, double *dinv,
                         int nrows, int nslices, int R, const int32_t *perm = nullptr);

// ---- vector kernels (all lengths in doubles)
void launch_copy(hipStream_t s, double *y, const double *x, int64_t n);
void launch_fill(hipStream_t s, double *y, double v, int64_t n);
// y = a*x + b*y
void launch_axpby(hipStream_t s, double *y, double a, const double *x, double b, int64_t n);
// y[k*nx + r] = mask_k[r] ? (mx ? alpha_k * mx[k*nx + r] : 0) : x[k*nx + r]
// Called in place (y == x: System::apply, the Krylov drivers' ns_project of an iterate) although
// both are __restrict__: every thread reads x[p] before it writes y[p] and touches no other element,
// which tests/test_gpu_block_kernels.py::test_mask_blocks pins bit for bit against the out-of-place call.
struct MaskJob { const uint8_t *mask; double alpha; };
void launch_mask_blocks(hipStream_t s, double *y, const double *x, const double *mx,
                        const MaskJob *d_jobs, int nblocks, int64_t nx);
// T_1 (kind 1) / T_2 (kind 2) from the raw rows `t` into `y` with the operator's Dirichlet
// post-correction fused (d_jobs: the n blocks' masks, xin: the operator's input at the same offset)
void launch_time_transform_mask(hipStream_t s, double *y, const double *t, const double *xin,
                                const MaskJob *d_jobs, int kind, int n, int64_t nx,
                                const double *lo_halo, const double *hi_halo);
// CN time transforms over `n` consecutive blocks of length nx (block stride nx):
// kind 1: T_1 (new_i = old_i + old_{i+1}); 2: T_2; 3: T_1^{-1}; 4: T_2^{-1}
// (preconditioner.py:33-60, control.py:63-96).  `lo_halo`/`hi_halo` (may be null) stand
// for the block before the first / after the last one on a time-sharded handle.
// Called in place (y == x: StokesPC's launch_time_transform(st, h_, h_, ...)) although both are
// __restrict__: a thread walks its own dof through the levels, reading every level before it writes
// it; tests/test_gpu_block_kernels.py::test_time_transform pins it bit for bit against the
// out-of-place call.
void launch_time_transform(hipStream_t s, double *y, const double *x, int kind, int n,
                           int64_t nx, const double *lo_halo, const double *hi_halo);
// ConstantNullspace on every block that carries one, in two launches:
// y_j -= mean(y_j); second == 1: y_j += mean(b_j); second == 2: y_j += alpha_j * mean(b_j)
struct ConstJob { int64_t off, nx; double c1, c2_one, c2_alpha; };
void launch_const_correct(hipStream_t s, const ConstJob *d_jobs, int njobs, int64_t max_nx,
                          double *y, const double *b, int second, double *sums);
void launch_const_center(hipStream_t s, const ConstJob *d_jobs, int njobs, int64_t max_nx,
                         const double *x, double *xc, double *sums);

// ---- reductions (two fixed stages, no atomics: bitwise reproducible)
struct VecList { const double *v[MDOT_MAX]; };
// out[i] = <w, V_i>, i < nv <= MDOT_MAX.  scratch: REDUCE_BLOCKS * MDOT_MAX doubles.
void launch_mdot(hipStream_t s, const double *w, VecList V, int nv, int64_t n,
                 double *scratch, double *out);
// out[0] = sqrt(<w, w> + extra) where extra = (add ? *add : 0)
void launch_norm2_finish(hipStream_t s, const double *dot, double *out);
void launch_zero_bytes(hipStream_t s, void *p, size_t nbytes);   // kernel node, not a memset node
void launch_add_constant(hipStream_t s, double *y, double v, int64_t n);   // y[i] += v

// ---- batched spectrum estimates (spectrum_kernels.hip): B matrices of one pattern in lock-step.
// Vector b of a family starts at base + b * stride (stride even, >= n); alpha / beta are
// step-major (entry s of matrix b at [s * B + b]); everything per matrix lives on the device.
struct SpecBatch {
    int32_t B, max_steps;
    int64_t n, stride;
    double *r, *z, *p, *w;      // Lanczos: the PCG vectors; power iteration: v = r and z
    double *part;               // B * REDUCE_BLOCKS partial sums
    double *alpha, *beta;       // max_steps * B each
    int32_t *na, *nb;           // entries recorded (power iteration: na = steps taken)
    double *rz, *coef;          // <r, z>; the coefficient of the next vector update
    double *mu2, *last;         // power iteration: the estimate and the one before
    uint32_t *active;           // 0: the matrix is done, its workgroups leave at once
};
// the spacing the estimates give the vectors of n rows: even (double2 accesses), 32 doubles of slack
inline int64_t spec_batch_stride(int64_t n) { return (n + 32 + 1) & ~(int64_t)1; }
// what the second stage of a batched dot does with the sum (spectrum_host.hpp has the scalars)
enum { SPEC_DOT_START, SPEC_DOT_PAP, SPEC_DOT_RZ, SPEC_DOT_NORM0, SPEC_DOT_NORM };
// <x_b, y_b> for every active matrix with mdot_stage1 / mdot_stage2's chunks and trees, then:
// START rz = dot, stop unless positive and finite; PAP a = rz / dot appended to alpha, stop before
// that unless dot is positive and finite; RZ b = dot / rz appended to beta and rz = dot, stop
// before that unless dot > 1e-28 rz and finite; NORM0 / NORM (after power step k) nv = sqrt(dot),
// the 0.5 % rule from step 8 on, coef = 1 / nv.  A stop clears the matrix's `active` word.
void launch_spec_dot(hipStream_t s, const SpecBatch &S, const double *x, const double *y, int mode,
                     int k = 0);
// R: r = -coef w + r; P: p = z + coef p; SCALE: r = coef r; COPY: p = z -- with the roundings of
// launch_axpby(r, -a, w, 1), launch_axpby(p, 1, z, b), launch_axpby(v, 0, z, c)
enum { SPEC_UPD_R, SPEC_UPD_P, SPEC_UPD_SCALE, SPEC_UPD_COPY };
void launch_spec_update(hipStream_t s, const SpecBatch &S, int kind);
// launch_vals_sym_skew over nmat matrices (d_m on the device), one flag word each
struct SpecSplit { const double *a; double *h, *sk; };
void launch_spec_sym_skew(hipStream_t s, const SpecSplit *d_m, int nmat, const int32_t *tpos, int64_t n,
                          unsigned *nonsym);
// 64-bit fingerprints of the bits of nmat value arrays: spec_fingerprint_blocks(n) words per array
// (fixed order, no atomics), folded by the host with spec_fingerprint_fold
inline int spec_fingerprint_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(64, (n + 2047) / 2048));
}
inline uint64_t spec_fingerprint_fold(const unsigned long long *w, int nwords) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < nwords; ++k) h = (h ^ (uint64_t)w[k]) * 0xff51afd7ed558ccdull + (h >> 29);
    return h;
}
void launch_spec_fingerprint(hipStream_t s, const double *const *d_vals, int nmat, int64_t n,
                             unsigned long long *out);
// launch_vals_differ per pair: flag[q] |= 1 when pair q's arrays differ in any bit
struct SpecPair { const double *a, *b; };
void launch_spec_pairs_differ(hipStream_t s, const SpecPair *d_pairs, int npairs, int64_t n,
                              unsigned *flag);

// ---- coarse space of the two-grid sub-solves on the device: P by rows (prolongation) and by
// columns (restriction), scratch for one correction
struct CoarseDev {
    int nc = 0;
    const int32_t *p_ip = nullptr, *p_ix = nullptr;     // P: n rows
    const double *p_v = nullptr;
    const int32_t *pt_ip = nullptr, *pt_ix = nullptr;   // P^T: nc rows
    const double *pt_v = nullptr;
    double *rc = nullptr, *ec = nullptr;                // nc doubles each
};
// x_out = x_in + P E^-1 P^T r (x_in may be null or x_out); three launches, fixed summation orders
void launch_coarse_correction(hipStream_t s, const CoarseDev &c, const double *einv,
                              const double *r, const double *x_in, double *x_out, int64_t n);
// the same for nb vectors `vstride` apart in one launch per stage (c.rc, c.ec: nb * nc doubles)
void launch_coarse_correction_batched(hipStream_t s, const CoarseDev &c, const double *einv,
                                      const double *r, const double *x_in, double *x_out, int64_t n,
                                      int nb, int64_t vstride);
void launch_einv_outside(hipStream_t s, const double *einv, int nc, const int32_t *lo,
                         const int32_t *hi, unsigned *flag);
void launch_coarse_column(hipStream_t s, const CoarseDev &c, int k, double *x, int64_t n);
void launch_coarse_restrict(hipStream_t s, const CoarseDev &c, const double *r, double *rc,
                            int stride = 1);
// inv = a^-1 (n x n row-major, a destroyed) by Gauss-Jordan with partial pivoting on the device
void launch_dense_inverse(hipStream_t s, double *a, double *inv, int n, int *d_piv,
                          double *d_colbuf, unsigned *d_flag);
// Batched coarse set-up.  E_b = P^T A_b P (rows of A_b masked) for nmat level matrices on one
// SELL structure, one launch; the structure of E comes from the host (e_ip / e_ix).  Sums in the
// order of the column path (launch_coarse_column + SpMV + launch_coarse_restrict): bit-identical
// to it.  E: nmat row-major nc x nc matrices (block_n > 0: their diagonal blocks), zeroed by the
// caller.
struct GalerkinDev {
    const int32_t *e_ip = nullptr, *e_ix = nullptr;   // structure of E: nc rows
    const int32_t *col = nullptr, *slice_off = nullptr;   // SELL structure of A
    const int32_t *pos = nullptr;                     // position of each row (null: position == row)
    const uint8_t *mask = nullptr;                    // masked rows of A P are zero
    int R = 2, uniform_w = -1;
    // > 0: E is block diagonal in nc / block_n ranges of this size, and the Galerkin launch writes
    // each diagonal block as a matrix of its own (nmat * nc / block_n contiguous block_n^2 ones)
    int block_n = 0;
};
void launch_galerkin_batched(hipStream_t s, const CoarseDev &c, const GalerkinDev &g,
                             const double *const *d_vals, double *E, int nmat);
// inv[b] = a_b^-1 for nmat n x n row-major matrices stored contiguously at a (destroyed): blocked
// Gauss-Jordan with partial pivoting, 1 + 2 ceil(n / 32) launches for the whole batch (returned).
// d_bad[b] = first column whose pivot is below 1e-13 max|diag a_b| or which holds a non-finite entry
// when its panel is loaded (n: none).  scratch: at least
// dense_inverse_batched_scratch(n, nmat) bytes.
size_t dense_inverse_batched_scratch(int n, int nmat);
int launch_dense_inverse_batched(hipStream_t s, double *a, double *const *d_inv, int n, int nmat,
                                 void *scratch, int *d_bad);
// Block-diagonal E (nc = nblk * bn; block k: indices [k bn, (k+1) bn)), one launch for all nmat
// matrices: every entry of inv[b] (nc x nc) -- the block inverses Ib[b * nblk + k] (bn x bn,
// contiguous) on the diagonal, exact zeros elsewhere.
void launch_coarse_block_scatter(hipStream_t s, const double *Ib, double *const *d_inv, int nc,
                                 int bn, int nmat);
void launch_flag_to_double(hipStream_t s, const unsigned *flag, double *out);
// w += sign * sum_i coef[i] * V_i   (coef in device memory)
void launch_maxpy(hipStream_t s, double *w, VecList V, const double *coef, double sign,
                  int nv, int64_t n);
// the same update, and out_sq[0] = <w, w> of the updated w (summation order of launch_mdot)
void launch_maxpy_norm(hipStream_t s, double *w, VecList V, const double *coef, double sign,
                       int nv, int64_t n, double *scratch, double *out_sq);
// y = x * (1 / *norm)
void launch_scale_inv(hipStream_t s, double *y, const double *x, const double *norm,
                      int64_t n);

}  // namespace kkt
