/*
 * libkkt -- MI355X-native all-at-once KKT solver: C-ABI drop-in boundary.
 *
 * The reference (sleveque/control) has no native code and no FFI; its boundary for this
 * path is the Python class preconditioner/preconditioner.py:216 `MultiBlockSystem` and
 * its method `.solve()` (preconditioner.py:337-786).  Every entry point below cites the
 * reference lines whose work it takes over.  The Python mirror of that class
 * (control_amd/multiblock.py) binds these symbols with ctypes; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ types, no exceptions cross the boundary
 *   - every function returns KKT_OK (0) or a negative KKT_ERR_* code; the message is
 *     available from kkt_last_error()
 *   - host arrays are caller-owned; the library copies during the call and never keeps
 *     a host pointer after returning (pc callback excepted, see kkt_set_pc_callback)
 *   - a handle is bound to one GPU and is not thread-safe
 *   - vectors are fp64; the flat KKT vector is the n_blocks_00 blocks of variable 0
 *     followed by the n_blocks_11 blocks of variable 1, block k at a contiguous offset
 *     (preconditioner.py:286-287)
 */
#ifndef KKT_H
#define KKT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kkt_system *kkt_handle;

enum {
    KKT_OK = 0,
    KKT_ERR_ARG = -1,       /* bad argument / call order */
    KKT_ERR_HIP = -2,       /* HIP runtime error */
    KKT_ERR_STATE = -3,     /* object not in the state the call needs */
    KKT_ERR_CALLBACK = -4,  /* a host preconditioner callback reported failure */
    KKT_ERR_COMM = -5       /* multi-GPU transport error */
};

/* quadrants of the 2x2 block system (preconditioner.py:303) */
enum { KKT_Q00 = 0, KKT_Q01 = 1, KKT_Q10 = 2, KKT_Q11 = 3 };

/* Krylov methods (`solver_parameters["linear_solver"]`, preconditioner.py:733) */
enum { KKT_KSP_GMRES = 0, KKT_KSP_FGMRES = 1, KKT_KSP_MINRES = 2 };
/* `solver_parameters["pc_side"]` (preconditioner.py:735-736); DEFAULT = the method's own */
enum { KKT_PC_SIDE_DEFAULT = -1, KKT_PC_LEFT = 0, KKT_PC_RIGHT = 1 };

/* PETSc KSPConvergedReason values the reference tests against (preconditioner.py:769) */
enum {
    KKT_CONVERGED_RTOL = 2,
    KKT_CONVERGED_ATOL = 3,
    KKT_CONVERGED_HAPPY_BREAKDOWN = 5,
    KKT_DIVERGED_ITS = -3,
    KKT_DIVERGED_DTOL = -4,
    KKT_DIVERGED_BREAKDOWN = -5,
    KKT_DIVERGED_INDEFINITE_PC = -8,   /* minres: r.Br < 0 */
    KKT_DIVERGED_NANORINF = -9,
    KKT_DIVERGED_INDEFINITE_MAT = -10  /* minres: Lanczos r.Br < 0 after the first step */
};

/* ------------------------------------------------------------------ life cycle */

/* One system on GPU `device_id`.  Replaces the MultiBlockSystem object
 * (preconditioner.py:216-335). */
int kkt_create(kkt_handle *out, int device_id);
int kkt_destroy(kkt_handle h);
/* Message of the last failing call on `h` (or of the last failing kkt_create if NULL). */
const char *kkt_last_error(kkt_handle h);

/* Execution options: which kernel form runs, not what is computed (every form of a step
 * performs the same arithmetic in the same order; tests toggle them to assert that).  Set a
 * key before the call that reads it: storage keys before kkt_set_layout / kkt_add_block,
 * preconditioner keys before kkt_set_pc_schur.  Unknown keys, and values outside a key's list,
 * are rejected with KKT_ERR_ARG and leave the handle's options as they were.  Switches take
 * "0" | "1"; the default is given first.  Options are per handle: each handle's launches follow
 * its own.
 *   "sell_r"        "2" | "1"      rows per lane of the SELL-64R storage
 *   "sell_sort"     "1" | "0"      row-sorted storage for ragged structures (read per pattern)
 *   "sell_sigma"    "1".."64"      slices per sorting window (default 8)
 *   "shared_rows"   "1" | "0"      one load of a shared matrix serves several block rows
 *   "ragged_switch" "1" | "0"      operator apply on ragged structures (P2 / Stokes blocks) with the
 *                                  width-switched kernel; "0": the slot loop
 *   "ragged_xcd"    "1" | "0"      ... in the XCD-aware workgroup order; "0": dispatch order
 *   "apply_xcd"     "0" | "1"      XCD-aware order for the fixed-width operator launches too
 *                                  (measured slower; off)
 *   "pc_xcd"        "1" | "0"      batched preconditioner steps in the XCD-aware workgroup order;
 *                                  "0": dispatch order
 *   "interleave"    "1" | "0"      batched mass solves with the iterates of four time levels
 *                                  interleaved; "0": one vector per time level
 *   "kernarg_ops"   "0" | "1"      single-block preconditioner steps take their RowOp as a kernel
 *                                  argument
 *   "no_graph"      "0" | "1"      "1": replay the preconditioner as plain launches, no hipGraph
 *   "persistent"    "1" | "0"      time sweeps as sweep programs; "0": one launch per step
 *   "prog_mode"     "auto" | "tile" | "dataflow" | "flags" | "w"   sweep-program form (auto:
 *                                  tile where it fits, else dataflow, else flags; "tile": the
 *                                  same; "dataflow": the row programs only, data-flow form
 *                                  preferred; "flags": the counter form; "w": the data-flow form
 *                                  for any width)
 *   "prog_waves"    "1".."8"       waves per workgroup of the dataflow / flags forms (default:
 *                                  chosen by shape)
 *   "prog_steps"    "1" | "0"      dataflow form with compact STEP records
 *   "tile_depth"    "1".."16"      SpMV steps per hand-off of the tile form (default: modelled)
 *   "tile_waves"    "1".."16"      waves per workgroup of the tile form (default: modelled)
 *   "tile_unfused"  "0" | "1"      tile form: wide rows keep the level update as a plain launch
 *   "lanes"         "0" | "1"      BE preconditioner in chunks on two streams
 *   "lane_chunks"   integer        ... that many chunks (default 4; at least 2, at most one per
 *                                  four time levels)
 *   "coarse_setup"  "batched" | "columns"   two-grid set-up with batched Galerkin products and
 *                                  blocked Gauss-Jordan on the device; "columns": column by
 *                                  column (the previous path)
 *   "coarse_keep"   "0" | "1"      keep the Galerkin matrices and inverses of the last set-up
 *   "coarse_blocks" "1" | "0"      batched set-up: one inverse per component block of a
 *                                  vector-valued space (the rows keep their full layout, exact
 *                                  zeros outside the block); "0": invert P^T A P as one matrix
 *   "spectrum_batch"  "0".."4096"  sub-solve matrices of a preconditioner build whose spectrum
 *                                  estimates run in lock-step (default 32; further matrices in
 *                                  further batches).  "0": one matrix at a time with a host round
 *                                  trip per reduction (the previous path).  Same intervals, step
 *                                  counts and preconditioner bit for bit; see kkt_spectrum_stats
 *   "pc_alias"      "1" | "0"      Schur preconditioner: value arrays that the twin search of a
 *                                  build proved equal bit for bit (the per-level copies mode G
 *                                  keeps of a time-invariant operator) are read from one array --
 *                                  the formed matrices blk + c M~ and their Jacobi diagonals, and
 *                                  the stored blocks the updates and right-hand-side products
 *                                  multiply with -- and the formed duplicates are not kept.  Proved
 *                                  again by every rebuild after kkt_update_block_values.  "0":
 *                                  every level reads its own arrays (same results bit for bit; see
 *                                  kkt_debug_pc_alias and kkt_spectrum_stats.alias_blocks)
 *   "coarse_rings"  "1" | "0"      two-grid sub-solves in the tile form: a tile prolongs the
 *                                  coarse correction onto its ring rows itself instead of fetching
 *                                  them in a hand-off after every correction (same results; "0":
 *                                  the hand-off; see kkt_info.sweep_coarse_rings)
 *   "tile_coarse_cache"  "auto" | "2" | "1" | "0"   two-grid sub-solves in the tile form: where the
 *                                  tables of the coarse corrections live.  "2": a tile's lists and
 *                                  the rows of the coarse inverse it owns in LDS, "1": the lists
 *                                  only, "0": nothing (all read from memory); "auto": the first of
 *                                  these that fits.  A forced level that does not fit leaves the
 *                                  two-grid levels to another form, as any plan that does not fit
 *                                  (same results; see kkt_info.sweep_coarse_cache).  The ring form
 *                                  stays with "coarse_rings" and needs the lists in LDS.
 *   "tile_coarse_rows"   "block" | "full"   ... a row of the coarse inverse is applied over the
 *                                  columns of its diagonal block of P^T A P, or ("full") over all
 *                                  n_coarse columns -- what the library does by itself when an
 *                                  inverse has entries outside the blocks (same results; see
 *                                  kkt_info.sweep_coarse_ew)
 *   "mass_tiles"    "1" | "0"      batched one-matrix solves (the mass solves) as several Chebyshev
 *                                  steps per launch out of LDS on a tile plan of their own, where
 *                                  the sweeps are programs ("persistent"), "lanes" is off, the
 *                                  rows have at most 9 entries and the plan's rings pay; "0": one
 *                                  launch per step (same results)
 *   "mass_tile_depth"  "0".."8"    ... steps per launch (0: chosen)
 *   "mass_tile_rows"   "0".."65536"  ... own rows per tile (0: chosen).  A caller who sets the
 *                                  depth or the rows gets the form wherever a plan fits.
 *   "mass_tile_levels" "0".."4096" ... time levels a workgroup serves (groups of four; 0: as
 *                                  many workgroups as the device holds at once)
 *   "mass_tile_waves"  "0" | "4" | "8"   ... waves per workgroup (0: 4 where the rows fit)
 *   "stage_timers"  "0" | "1"      HIP events around the stages of every Krylov iteration
 *                                  (kkt_get_stage_times)
 *   "verbose"       "0" | "1"      set-up decisions on stderr
 *   Diagnostics and test hooks of the tile form: "stamps" "0" | "1" (hand-off time stamps in
 *   its diagnostics buffer), "tile_poll_delay" integer (sleep units before the first poll,
 *   default 24), "debug_drop_handoff" integer (default 0; n > 0: tile 0 skips hand-off n;
 *   n < 0: tile 0 never checks in).
 * The library never reads the process environment: a key that was never set has its default.
 * (The Python mirror forwards KKT_<KEY> variables of developer scripts as explicit calls.) */
int kkt_set_option(kkt_handle h, const char *key, const char *value);

/* Optional hint for the tile form of the preconditioner's sweep programs: coordinates of the
 * dofs of the spatial block the sweeps run on (variable 0: n = N_x rows, `dim` = 1..3 doubles
 * each, row-major; the components of a vector-valued space carry their node's coordinates --
 * in Firedrake: the interpolated SpatialCoordinate of the space).  With them the rows are cut
 * into tiles by coordinate bisection (boxes) instead of bisection of the sparsity graph, whose
 * cuts are slanted in meshes with diagonal edges: smaller rings per hand-off (256^2 P1: 630
 * instead of 784 rows at depth 7; 64^3 P1: 764 instead of 1 030).  Speed only: results do not
 * depend on the partition.  Before kkt_set_pc_schur. */
int kkt_set_tile_coordinates(kkt_handle h, int dim, int64_t n, const double *coords);

/* ------------------------------------------------------------------ definition */

/* Block counts and spatial sizes (preconditioner.py:217-222, 276-302).
 * sub_n_blocks_* = -1 means None.  Must precede every other definition call. */
int kkt_set_layout(kkt_handle h, int n_blocks_00, int n_blocks_11,
                   int64_t nx0, int64_t nx1, int CN,
                   int sub_n_blocks_00_0, int sub_n_blocks_11_0);

/* Time sharding (new functionality): this handle owns block rows
 * [lo, hi) of BOTH variables, where [lo, hi) is rank's slice of n_blocks_00 ==
 * n_blocks_11 rows split evenly over `world` ranks.  Vectors passed to every later call
 * are the local shard [x0_lo..x0_hi-1, x1_lo..x1_hi-1].  Only blocks of owned rows may be
 * added.  Omit for a single GPU. */
int kkt_set_shard(kkt_handle h, int rank, int world);
/* The same for systems whose flat blocks are `families` runs of time levels per variable
 * (2: the outer incompressible system -- velocity blocks (v, zeta), pressure blocks (mu, p),
 * control.py:3654-3673): the rank owns levels [lo, hi) of every family, local vectors are
 * [family 0 levels lo..hi-1, family 1 levels lo..hi-1] per variable.  With Crank-Nicolson the
 * sub-block split of the time transforms (sub_n_blocks_*_0, preconditioner.py:471-525) must be
 * the family boundary. */
int kkt_set_shard_families(kkt_handle h, int rank, int world, int families);
/* Row range owned by `rank` of `world` for `m` block rows (pure host arithmetic). */
int kkt_shard_range(int m, int rank, int world, int *lo, int *hi);

/* One assembled block A_ij of a quadrant as CSR (replaces `assemble(block_ij)`,
 * preconditioner.py:305-328; the adapter feeds `petscmat.getValuesCSR()`).
 * Column indices must be sorted within a row.  Blocks with the same share_id >= 0
 * share one copy of the values on the device (time-invariant operators, "mode S");
 * share_id < 0 gives the block its own copy ("mode G", what the reference stores).
 * Blocks with identical sparsity structure always share the index arrays. */
int kkt_add_block(kkt_handle h, int quadrant, int i, int j,
                  int64_t nrows, int64_t ncols,
                  const int32_t *indptr, const int32_t *indices,
                  const double *values, int64_t share_id);
/* The structure of a block whose values are produced on the device.  Registers block (i, j) as
 * kkt_add_block does with share_id < 0 -- shared index arrays, SELL layout, a value array of its
 * own -- but uploads no values: the array is zero-filled and the block is *unset*.
 * kkt_finalize accepts unset blocks.  While a handle holds one, kkt_apply*, kkt_pc_apply*,
 * kkt_solve*, kkt_time_* and kkt_set_pc_schur / kkt_set_pc_stokes (on the handle, its inner or its
 * commutator handle) return KKT_ERR_STATE before anything is launched; kkt_last_error names the
 * first such block as (quadrant, i, j).  A block becomes set when kkt_relinearise_device composes
 * into it or kkt_update_block_values writes it.  kkt_info.blocks_unset counts them. */
int kkt_add_block_structure(kkt_handle h, int quadrant, int i, int j,
                            int64_t nrows, int64_t ncols,
                            const int32_t *indptr, const int32_t *indices);
/* New values on the stored structure of a block (re-linearisation in a Picard loop,
 * control.py:3377-3590); valid after kkt_finalize.  A built-in preconditioner whose matrices
 * are sums with block values is marked stale and rebuilt once, on the device, at its next
 * application -- not per updated block. */
int kkt_update_block_values(kkt_handle h, int quadrant, int i, int j,
                            const double *values);

/* DirichletBCNullspace(bcs, alpha) on flat block k (k < n_blocks_00: variable 0,
 * otherwise variable 1): preconditioner.py:158-197. */
int kkt_set_bc(kkt_handle h, int block_k, int64_t n_idx, const int32_t *idx,
               double alpha);
/* ConstantNullspace(alpha) on flat block k: preconditioner.py:133-155. */
int kkt_set_const_nullspace(kkt_handle h, int block_k, double alpha);

/* Freeze the definition and build the device data (HBM layout: DESIGN.md). */
int kkt_finalize(kkt_handle h);

/* ------------------------------------------------------------- preconditioner */

enum { KKT_PC_STATIONARY = 0, KKT_PC_INSTATIONARY_BE = 1, KKT_PC_INSTATIONARY_CN = 2 };

/* Built-in block Schur-complement preconditioner: the closures built by
 * Control.Stationary.construct_pc (control.py:351-450) and
 * Control.Instationary.construct_pc (control.py:1943-2440; CN 1995-2189, BE 2191-2438).
 * It reads block_10 / block_01 from the blocks already added.  Mass solves are
 * `mass_its` Jacobi-Chebyshev steps on [mass_emin, mass_emax] (control.py:1967-1982;
 * mass_its == 0: one Jacobi application, control.py:1984-1991).  The hypre sub-solves of
 * the reference are replaced by `schur_its` Jacobi-Chebyshev steps on
 * [schur_emin, schur_emax] (BASELINE.json north_star).  A hand-set interval much wider than the
 * spectrum is harmless for symmetric blocks and harmful for blocks with convection: outside the
 * interval's ellipse the Chebyshev polynomial grows with the imaginary part, and a wide interval
 * has a weak normalisation -- give the matrix's own bounds (or let the library estimate them). */
typedef struct kkt_pc_desc {
    int kind;            /* KKT_PC_* */
    int n_t;             /* time levels (ignored for STATIONARY) */
    double tau;          /* time step (ignored for STATIONARY) */
    double beta;         /* regularisation parameter */
    double epsilon;      /* BE final-time scaling, control.py:2836 (1e-3) */
    int64_t nx;          /* spatial dofs of the mass matrix */
    const int32_t *m_indptr;   /* mass matrix `self._M_v` as CSR */
    const int32_t *m_indices;
    const double *m_values;
    int64_t n_bc;        /* homogeneous Dirichlet dofs (bcs_v = bcs_zeta) */
    const int32_t *bc_idx;
    int mass_its;
    double mass_emin, mass_emax;
    int schur_its;       /* -1: 1.6 sqrt(emax / emin) of a typical time level's matrix */
    double schur_emin, schur_emax;   /* schur_emin <= 0: per matrix, from a Lanczos estimate of its
                                        Jacobi-scaled spectrum on the device (spectrum.cpp) */
    double schur_eimag;  /* > 0: the Jacobi-scaled spectrum of the sub-solve matrices lies in the
                            ellipse with real semi-axis (schur_emax - schur_emin) / 2 and imaginary
                            semi-axis schur_eimag around their mid-point (forward operators with a
                            convection term, control.py:1887-1896: the blocks are not symmetric);
                            the sweeps keep their three-term form with the coefficients of that
                            ellipse (Manteuffel 1977).  0: real interval.  With schur_emin <= 0 it
                            is estimated per matrix too (symmetric part for the interval, spectral
                            radius of the skew part for the semi-axis). */
    /* Two-grid form of the Schur sub-solves (coarse_cycles == 0: off).  A sub-solve is
     * `coarse_cycles` times [x += P (P^T A P)^-1 P^T (b - A x); `schur_its` Jacobi-Chebyshev
     * sweeps on [schur_emin, schur_emax] from x] -- the reference calls BoomerAMG here
     * (control.py:2277-2288); the sweeps keep the shape north_star prescribes and only have to
     * cover the part of the spectrum the coarse space does not see (8 sweeps on [emax / 30, emax]
     * instead of 80 on the whole spectrum of 256^2 P1).  P: nx x n_coarse CSR, rows of Dirichlet
     * dofs empty (control_amd.coarse.multilinear_coarse_space builds it from dof coordinates).
     * The Galerkin matrices are formed and inverted at set-up, one per distinct sub-solve matrix.
     * With schur_emin <= 0: emax from the matrix, emin = emax / 30; schur_its = -1: 8. */
    int coarse_cycles;
    int64_t n_coarse;
    const int32_t *p_indptr, *p_indices;
    const double *p_values;
} kkt_pc_desc;

int kkt_set_pc_schur(kkt_handle h, const kkt_pc_desc *desc);

/* Preconditioner of the incompressible control systems: the pc_fn closures of
 * Stationary.incompressible_linear_solve (control.py:986-1085) and of
 * Instationary.incompressible_linear_solve (BE control.py:4515-4687, CN control.py:4318-4513).  `h` is the outer system
 * (variable 0 = velocity blocks v then zeta, variable 1 = pressure blocks mu then p); `inner`
 * is the velocity KKT system with its own preconditioner and KSP options already set
 * (the reference runs 5 GMRES iterations, control.py:1005-1010); `commutator` is the
 * pressure-space block system block_**_int_p (control.py:976-984, 3818-3820).  Both handles
 * must stay alive while `h` uses them.  B = -(div v, q) is the unscaled divergence block. */
typedef struct kkt_pc_stokes_desc {
    int n_p_blocks;          /* pressure blocks per variable (1 stationary, n_t BE, n_t-1 CN) */
    int cn;                  /* 1: Crank-Nicolson branch -- T_2 / T_1 on tau B u_0 before b_1 is
                                subtracted and their inverses after the scaling (control.py:4407-4428) */
    int64_t nv, np;          /* dofs of one velocity / pressure block */
    double b_scale;          /* tau (instationary, control.py:4577) or 1 */
    double post_scale;       /* 1 / tau^2 (control.py:4596-4601) or 1 */
    const int32_t *b_indptr, *b_indices;      /* B: np x nv */
    const double *b_values;
    const int32_t *kp_indptr, *kp_indices;    /* K_p: np x np */
    const double *kp_values;
    const int32_t *mp_indptr, *mp_indices;    /* M_p: np x np */
    const double *mp_values;
    int kp_its;              /* Jacobi-Chebyshev steps replacing the BoomerAMG cycle on K_p;
                                -1: the degree of the inner system's sub-solves (inner sub-solves in
                                two-grid form: 5 sqrt(kappa) of K_p's own non-zero spectrum, <= 600) */
    double kp_emin, kp_emax; /* kp_emin <= 0: lower bound of the inner sub-solves, upper bound
                                estimated from K_p (two-grid inner sub-solves: both ends estimated
                                from K_p, constants deflated) */
    int mp_its;              /* control.py:957-971: 20 (0: one Jacobi application, :973-979) */
    double mp_emin, mp_emax;
    /* Two-grid form of the K_p solve (0 cycles: the plain polynomial above): kp_coarse_cycles x
     * [Galerkin correction on the coarse space P_p (np x kp_n_coarse, CSR; its columns must sum to
     * the constant vector, which K_p annihilates: the Galerkin matrix is inverted with the
     * constants deflated, E + (trace E / n_c^2) 1 1^T); kp_its sweeps on [kp_emin, kp_emax] from
     * the corrected iterate].  Needs kp_its >= 1 and explicit bounds. */
    int kp_coarse_cycles;
    int64_t kp_n_coarse;
    const int32_t *kp_p_indptr, *kp_p_indices;
    const double *kp_p_values;
} kkt_pc_stokes_desc;
int kkt_set_pc_stokes(kkt_handle h, kkt_handle inner, kkt_handle commutator,
                      const kkt_pc_stokes_desc *desc);

/* Arbitrary user `pc_fn(u_0, u_1, b_0, b_1)` (preconditioner.py:337-345, 623-627) on host
 * arrays: slow path kept for API parity (`P=` of every *_solve, control.py:3257-3258).
 * The library downloads b, calls `fn`, uploads u.  Non-zero return -> the solve fails
 * with KKT_ERR_CALLBACK ("Error encountered in PETSc solve", preconditioner.py:771-772). */
typedef int (*kkt_pc_callback)(void *user, const double *b_0, const double *b_1,
                               double *u_0, double *u_1);
int kkt_set_pc_callback(kkt_handle h, kkt_pc_callback fn, void *user);
/* Default pc_fn: u = b (preconditioner.py:342-345). */
int kkt_set_pc_identity(kkt_handle h);

/* ---------------------------------------------------------------------- solve */

/* KSP options (preconditioner.py:732-748): type, side, GMRES restart, tolerances.
 * divtol <= 0 selects PETSc's default 1e4. */
int kkt_set_krylov(kkt_handle h, int type, int pc_side, int restart,
                   double rtol, double atol, double divtol, int max_it);

/* y = A x: MultiBlockSystemMatrix.mult (preconditioner.py:375-543), host arrays. */
int kkt_apply(kkt_handle h, const double *x, double *y);
/* y = P^-1 x: Preconditioner.apply (preconditioner.py:562-656), host arrays. */
int kkt_pc_apply(kkt_handle h, const double *x, double *y);
/* The whole of MultiBlockSystem.solve after the matrices exist (preconditioner.py:
 * 658-766): corrected initial guess and right-hand side, Krylov loop, corrected
 * solution.  `u` holds the initial guess on entry and the solution on return.
 * hist (may be NULL) receives the monitored residual norms, iteration 0 first. */
int kkt_solve(kkt_handle h, const double *b, double *u,
              int *its, int *reason, double *rnorm,
              double *hist, int hist_cap, int *hist_len);

/* ---------------------------------------------------- device-resident variants */

/* Vectors that stay in HBM between calls (benchmarks; callers with resident data). */
int64_t kkt_local_size(kkt_handle h);             /* doubles in one local KKT vector */
int kkt_vec_alloc(kkt_handle h, double **d_vec);
int kkt_vec_free(kkt_handle h, double *d_vec);
int kkt_vec_upload(kkt_handle h, double *d_vec, const double *host);
int kkt_vec_download(kkt_handle h, const double *d_vec, double *host);
int kkt_apply_device(kkt_handle h, const double *d_x, double *d_y);
int kkt_pc_apply_device(kkt_handle h, const double *d_x, double *d_y);
int kkt_solve_device(kkt_handle h, const double *d_b, double *d_u,
                     int *its, int *reason, double *rnorm,
                     double *hist, int hist_cap, int *hist_len);
int kkt_sync(kkt_handle h);

/* ------------------------------------------- Picard re-linearisation on the device */

/* The Navier-Stokes Picard loop of Instationary.incompressible_non_linear_solve
 * (control.py:4886-5232) with its iterate in HBM: the convection blocks are re-assembled from
 * the device iterate (construct_D_v, control.py:1887-1896 on the velocity space, 3779-3785 on
 * the pressure space), the non-linear residual is evaluated there (control.py:2442-2620 and
 * 4976-5082) and the update is added in place.  Taylor-Hood P2-P1 triangles, Radon's 7-point
 * rule (control_amd/fem.py rectangle_p2p1: the arrays of its `elem` dict).
 *
 * The plan lives on the handle it is set on, which must be the outer incompressible system of
 * the loop: n_blocks_00 = n_blocks_11 = 2m (m = n_t, CN: n_t - 1), nx0 = 2 n2, nx1 = n1.
 * Scalar P2 pattern: the structure of one velocity component of K_v / M_v (sorted CSR; the
 * velocity blocks carry it once per component, component-major); P1 pattern: K_p / M_p.
 * Both must be structurally symmetric: *_tperm[k] is the position of the transposed entry of
 * position k.  Contribution lists: for stored position k, the flat element-entry indices
 * (e * 36 + 6 a + b for the P2 element matrix rows a / columns b, e * 9 + 3 c + d for P1) in
 * *_clist[*_cptr[k] .. *_cptr[k + 1]), ascending; the assembly sums them in that order, the
 * order of np.bincount on the host, so it is deterministic (no atomics).  D = nu K + C(w) per
 * level.  B: the divergence block (n1 x 2 n2, sorted CSR).  data: the 2m x 2 n2 velocity rows
 * of the residual at the zero iterate (desired state, forces, the initial condition); bc_idx:
 * Dirichlet velocity dofs.  Arrays are copied; KKT_ERR_ARG on sizes, ranges or patterns that do
 * not fit.
 *
 * On a time-sharded handle (kkt_set_shard with two families: the outer system) the descriptor is
 * the same global one on every rank, and the plan keeps the rank's part only.  With [lo, hi) the
 * rank's unknown blocks (kkt_shard_range of m) it holds the levels its block rows read:
 *   backward Euler   v [lo - 1, hi), zeta [lo, hi], D [lo, hi)   (no level -1, no level n_t)
 *   Crank-Nicolson   v [lo, hi],     zeta [lo, hi], D [lo, hi]
 * p, mu and the data rows of its blocks.  The first v level and the last zeta level are halos:
 * kkt_relinearise_device refreshes them from the neighbour ranks before it assembles (one level
 * of v up, one of zeta down), and assembles CN's D_lo from the halo v.  kkt_picard_window reports
 * the windows.
 *
 * n_t = 1 is the stationary system of Stationary.incompressible_non_linear_solve
 * (control.py:1112-1480): cn must be 0, tau is ignored, and the handle must be the stationary outer
 * system -- n_blocks_00 = n_blocks_11 = 2 (v, zeta | mu, p), nx0 = 2 n2, nx1 = n1, not
 * Crank-Nicolson, not time-sharded; each violation is a KKT_ERR_ARG that names it.  data: the
 * 2 x 2 n2 rows [M v_d | M f].  Every window is [0, 1), the iterate is one level of each field.
 * The velocity rows of the residual are
 *   ((d_0 - M v) - D^T zeta) - B^T mu   and   ((d_1 - D v) + (1 / beta) (M zeta)) - B^T p
 * (not backward Euler's with n_t = 1: those carry tau, and the last adjoint row drops M v), the
 * pressure rows -B v and -B zeta; with rhs = 1 kkt_picard_residual_device returns the same rows:
 * the stationary right-hand side has no tau and no time transform.  Recipes name level 0
 * (blocks.stationary_incompressible_build_recipes).
 *
 * nv selects the element (the field fills what was padding after nq: every offset is unchanged).
 * nv = 0 is the P2-P1 descriptor described above: nq must be 7 and jinv is not read.  nv = 9 with
 * nq = 16 is Q2-Q1 on axis-parallel quadrilaterals (fem.rectangle_q2q1): local velocity node
 * 3 j + i and pressure node 2 j + i (i along x, j along y), the 4 x 4 Gauss-Legendre product rule
 * on the unit square (point q = 4 r + s is (t_s, t_r); degree 7 per variable, the convection
 * integrand with a Q2 wind has degree 6).  gphi and glam then hold the gradients on the unit
 * square, one table for all cells, and jinv the cells' 1 / hx, 1 / hy (non-NULL): the physical
 * gradient is the one rounded product ref * jinv per component.  The contribution lists run over
 * ne * 81 (e * 81 + 9 a + b) and ne * 16 (e * 16 + 4 c + d) entries.  Any other (nv, nq) is
 * KKT_ERR_ARG naming nv. */
typedef struct kkt_relin_desc {
    int n_t, cn, nq;              /* time levels (1: stationary), CN (1) or backward Euler, points */
    int nv;                       /* 0: P2-P1 triangles (nq = 7); 9: Q2-Q1 quadrilaterals (nq = 16) */
    int64_t ne, n2, n1;           /* cells, velocity nodes (one component), pressure nodes */
    double nu, tau, beta;
    const int32_t *V;             /* ne x 6 P2 nodes per triangle           | ne x 9 Q2 nodes */
    const double *W;              /* ne x nq quadrature weights times |det J| (Q2-Q1: hx hy) */
    const double *phi;            /* nq x 6 P2 basis at the points          | 16 x 9 Q2 basis */
    const double *gphi;           /* ne x nq x 6 x 2 their gradients        | 16 x 9 x 2, reference */
    const double *lam;            /* nq x 3 P1 basis (barycentric)          | 16 x 4 Q1 basis */
    const double *glam;           /* ne x 3 x 2 their gradients             | 16 x 4 x 2, reference */
    int64_t nnz2;                 /* scalar velocity pattern */
    const int32_t *v_indptr, *v_indices, *v_tperm, *v_cptr, *v_clist;
    const double *K2, *M2;        /* nnz2 values: grad-grad and mass of one component */
    int64_t nnz1;                 /* pressure pattern */
    const int32_t *p_indptr, *p_indices, *p_tperm, *p_cptr, *p_clist;
    const double *Kp, *Mp;
    int64_t nnz_b;
    const int32_t *b_indptr, *b_indices;
    const double *b_values;
    int64_t n_bc;
    const int32_t *bc_idx;
    const double *data;
    const double *jinv;           /* nv = 9: ne x 2, 1 / hx and 1 / hy per cell; nv = 0: ignored */
} kkt_relin_desc;
int kkt_set_relinearisation(kkt_handle h, const kkt_relin_desc *desc);

/* One block a recipe rewrites: block (quadrant; i, j) = alpha D_level(^T) + gamma M, with D, M
 * on the velocity (space 0, both components) or pressure (space 1) pattern -- the `comb`
 * coefficients of blocks.instationary_blocks (control.py:2889-2978, 3851-3885).  alpha = 0: the
 * constant block gamma M (its `mass` coefficients); D is not read. */
typedef struct kkt_relin_recipe {
    int quadrant, i, j;
    int space;
    int level;
    int transpose;
    double alpha, gamma;
} kkt_relin_recipe;
/* Rewrites the recipes' blocks of handle h from the plan on handle `plan`.  d_v (device, the
 * levels of the plan's v window x 2 n2, component-major; one rank: all n_t; a time shard: the
 * plan's own iterate) != NULL first re-assembles D at that velocity (collective on a time shard:
 * the halo levels travel first); NULL
 * composes from the last assembly (so the outer, inner and commutator handles of one
 * linearisation share one).  n = 0 only assembles.  The blocks are written on the device as
 * kkt_update_block_values would write them (Dirichlet columns zeroed, a value array shared with
 * other blocks is first made private) and a built-in preconditioner is marked stale.  The
 * target pattern must be the plan's.  Time shards: h is sharded as the plan's handle, recipes
 * keep their global (i, j) and level, and one whose block row the rank does not own, or whose
 * level lies outside the rank's D window, is KKT_ERR_ARG naming the block. */
int kkt_relinearise_device(kkt_handle h, kkt_handle plan, const double *d_v, int n,
                           const kkt_relin_recipe *recipes);
/* The plan's iterate (v, zeta: n_t x 2 n2; p, mu: m x n1) in HBM: host copies in (download 0)
 * or out (download 1), and its device addresses (any out pointer may be NULL).  The host arrays
 * always have the global shapes.  A time shard uploads its windows from them, halo levels
 * included, and downloads only what it owns -- its blocks' levels, and the fixed levels (CN: v_0;
 * zeta of the last level) on the rank whose window holds them -- leaving the rest untouched; the
 * device addresses are those of the windows' first levels.
 * kkt_picard_window: out = [v, zeta, D, block rows] as half-open ranges [first, end) of global
 * levels (one rank: [0, n_t) three times and [0, m)). */
int kkt_picard_state(kkt_handle plan, int download, double *v, double *zeta, double *p,
                     double *mu);
int kkt_picard_iterate(kkt_handle plan, double **d_v, double **d_zeta, double **d_p,
                       double **d_mu);
int kkt_picard_window(kkt_handle plan, int out[8]);
/* Non-linear residual at the plan's iterate, with D of the last assembly (assemble at the
 * iterate's v first).  rhs = 0: d_out (one local vector of the plan's handle) receives the
 * residual rows [r00, r01, r10, r11] of picard.non_linear_res_eval, Dirichlet rows zero;
 * rhs = 1: the right-hand side of the linearised solve (pressure rows times tau, CN: T_1 / T_2,
 * control.py:4266-4269).  *norm (host) = ||[r00, r01, r10, r11]||_2 by the deterministic
 * reduction.  Time shards (collective): the rank's rows [lo, hi) of the four families, each
 * bit for bit the row of the one-rank result; CN takes the transforms' terms across the shard
 * boundary from the neighbours' raw rows; the norm is the all-reduced sum of the ranks' sums of
 * squares, the same on every rank. */
int kkt_picard_residual_device(kkt_handle plan, double *d_out, int rhs, double *norm);
/* v, zeta, mu, p += the blocks of the update d_u (one local vector; CN: v from level 1);
 * then zeta = 0 on the Dirichlet dofs of every level (control.py:5127-5147).  d_u is zeroed:
 * the initial guess of the next linearised solve.  Time shards: the rank's own levels; its halo
 * levels are refreshed by the next assembly. */
int kkt_picard_update_device(kkt_handle plan, double *d_u);

/* Test hooks of the device re-linearisation: plain copies of what the kernels left, no launches.
 * kkt_debug_relin_array downloads one array of the plan's last assembly (cap: doubles available
 * at out): the element matrices Ev (n_t x ne x 36; Q2-Q1: 81) and Ep (n_t x ne x 9; Q2-Q1: 16),
 * or the assembled D2 (n_t x nnz2) and Dp (n_t x nnz1) -- on a time shard the levels of the D
 * window, in order.
 * KKT_ERR_STATE before any assembly, KKT_ERR_ARG when cap is too small.  KKT_RELIN_V and
 * KKT_RELIN_ZETA: the v and zeta windows of the iterate as they are, halo levels included. */
enum { KKT_RELIN_EV = 0, KKT_RELIN_EP = 1, KKT_RELIN_D2 = 2, KKT_RELIN_DP = 3, KKT_RELIN_V = 4,
       KKT_RELIN_ZETA = 5 };
int kkt_debug_relin_array(kkt_handle plan, int which, double *out, int64_t cap);
/* ---- Device re-linearisation of the scalar reaction problem.
 *
 * The forward operator is (L u, w) + (g(v_old) u, w) on P1 or P2 triangles, P1 tetrahedra or Q2
 * quadrilaterals with the polynomial g(s) = sum_k c[k] s^k, degree <= 4 (fem.ReactionTerm).  nq
 * and nv (nodes per cell) select the element; nv = 0 leaves it to nq (7 -> 3, 15 -> 4, 25 -> 6):
 *   nq = 7:  P1 triangles (nv = 3), Radon's 7 points; cells ne x 3, lam 7 x 3, E ne x 9 per level;
 *   nq = 15: P1 tetrahedra (nv = 4), the 15 points of Stroud's T3:5-1 (degree 5, positive
 *            weights); cells ne x 4, lam 15 x 4, E ne x 16 per level, W = weight times the volume;
 *   nq = 25: P2 triangles (nv = 6: vertices 0, 1, 2, then the midpoints of edges (0,1), (1,2),
 *            (0,2)), the 25 points of the 5 x 5 conical product rule (degree 9, positive weights,
 *            interior points); cells ne x 6, lam 25 x 6, W ne x 25 (weight times the area of the
 *            vertex triangle), E ne x 36 per level;
 *   nq = 25, nv = 9: Q2 quadrilaterals (axis-parallel cells, local node 3 j + i with i along x
 *            and j along y), the 25 points of the 5 x 5 Gauss-Legendre product rule (degree 9 per
 *            variable, positive weights, interior points; point 5 r + s is (t_s, t_r)); cells
 *            ne x 9, lam 25 x 9, W ne x 25 (weight times hx hy), E ne x 81 per level;
 * any other nq, any other non-zero nv and an nv that contradicts nq (nv = 9 with nq = 7, nv = 6
 * with nq = 15) are KKT_ERR_ARG naming the field.  lam holds the nq x nv values of the element's shape functions at
 * the points (barycentric coordinates on P1 elements).  Per (element, level) the element matrix
 *   E[a][b] = sum_q (W_eq g(s_q)) lam_qa lam_qb,   s_q = sum_c lam_qc v_c summed left to right,
 * over the points q ascending from 0.0, g by Horner from c[degree] down, every product and sum
 * rounded separately, all nv * nv entries computed on their own; the entries are gathered into the
 * scalar pattern through the contribution lists (flat entry e * nv * nv + nv * a + b, ascending:
 * np.bincount's order) and D = L + C with one rounding per entry.  The element matrices of all
 * levels are kept: n_t * ne * nv * nv doubles beside D (n_t * nnz) -- on 64^3 cells x 128 levels
 * of tetrahedra 25.8 GB and 4 GB, on 256^2 cells x 64 levels of P2 triangles 2.4 GB of element
 * matrices, on 256^2 cells x 64 levels of Q2 quadrilaterals (81 doubles per matrix) 2.7 GB.  The handle must be a scalar instationary layout
 * (n_blocks_00 = n_blocks_11 = m, nx0 = nx1 = n1; m = n_t, Crank-Nicolson n_t - 1), finalized.
 * A time-sharded handle (kkt_set_shard: one block family) takes its share of the same global
 * descriptor: with [lo, hi) its block rows it keeps the levels those rows read -- backward Euler
 * v [lo - 1, hi), zeta [lo, hi], D and E [lo, hi) (level -1 and level n_t do not exist);
 * Crank-Nicolson [lo, hi] of all four -- and the data rows lo .. hi - 1 and m + lo .. m + hi - 1;
 * E is then (levels of the D window) * ne * nv * nv doubles per rank.  A handle sharded in two
 * families (kkt_set_shard_families) is KKT_ERR_ARG.  A handle carries at most one plan, of this kind or of kkt_set_relinearisation's:
 * setting the other kind is KKT_ERR_STATE.  data: the 2m x n1 rows [adjoint | state] of
 * Instationary.non_linear_res_eval at the zero iterate (desired state, forces, backward Euler's
 * initial-condition row tau D(v_0) v_0 + M v_0), Dirichlet rows zero.  c: the Gauss-Newton
 * coefficients (k + 1) c_k when that linearisation is on.  Arrays are copied; patterns, lists and
 * permutations are validated as kkt_set_relinearisation validates its own (KKT_ERR_ARG naming what
 * does not fit).
 *
 * n_t == 1 selects the stationary system [[M, D^T], [D, -(1/beta) M]] of Control.Stationary (no
 * instationary system has one level): cn must be 0 and tau is ignored; the handle must be the
 * stationary layout -- n_blocks_00 = n_blocks_11 = 1, nx0 = nx1 = n1, not Crank-Nicolson, not
 * sharded -- each violation KKT_ERR_ARG naming it; data is 2 x n1, [M v_d | M f] with the
 * Dirichlet rows zero; every window is [0, 1).  Every entry point below then works on that one
 * level: the rows of kkt_reaction_residual_device are those of Stationary.non_linear_res_eval,
 *   r0 = (d0 - M v) - D^T zeta,   r1 = (d1 - D v) + (1.0 / beta) (M zeta),
 * and they are the right-hand side themselves (rhs = 1 gives the bits of rhs = 0). */
typedef struct kkt_reaction_desc {
    int n_t, cn, nq;              /* time levels (1: the stationary system), Crank-Nicolson (1)
                                     or backward Euler; nq = 7: P1 triangles (nv = 3), nq = 15:
                                     P1 tetrahedra (nv = 4), nq = 25: P2 triangles (nv = 6) or
                                     Q2 quadrilaterals (nv = 9) */
    int nv;                       /* nodes per cell; 0: inferred from nq (25: P2 triangles).  It
                                     sits in what was padding before ne: a zeroed descriptor of
                                     the earlier layout reads as nv = 0 */
    int64_t ne, n1;               /* cells, dofs of the space */
    double tau, beta;
    const int32_t *cells;         /* ne x nv nodes per cell */
    const double *W;              /* ne x nq quadrature weights times the area / the volume */
    const double *lam;            /* the nq x nv values of the element's shape functions at the
                                     points (barycentric coordinates on P1 elements) */
    int64_t nnz;                  /* the scalar pattern (that of M) */
    const int32_t *indptr, *indices, *tperm, *cptr, *clist;
    const double *L, *M;          /* nnz values: the linear part and the mass matrix */
    int degree;
    double c[5];
    int64_t n_bc;
    const int32_t *bc_idx;
    const double *data;
} kkt_reaction_desc;
int kkt_set_reaction_relinearisation(kkt_handle h, const kkt_reaction_desc *desc);
/* assemble != 0 first forms the element matrices and D of all n_t levels at the plan's iterate
 * (a time shard, collective: its halo levels first -- one level of v from the rank below, one of
 * zeta from the rank above -- then the levels of its D window, Crank-Nicolson's D_lo from the
 * halo v); then the n recipes (space = 0) rewrite blocks of handle h exactly as kkt_relinearise_device
 * does: Dirichlet columns zeroed, shared value arrays made private first, alpha = 0 recipes give
 * gamma M, a built-in preconditioner is marked stale.  n = 0 only assembles.  Time shards: h
 * must be sharded as the plan's handle (KKT_ERR_ARG otherwise); recipes keep their global
 * indices, and one for a block row of another rank, or whose level lies outside the rank's D
 * window, is KKT_ERR_ARG naming the block, before anything is written. */
int kkt_reaction_relinearise(kkt_handle h, kkt_handle plan, int assemble, int n,
                             const kkt_relin_recipe *recipes);
/* The iterate (v, zeta: n_t x n1) in HBM: host copies in (download 0) or out (download 1), and
 * its device addresses (either out pointer may be NULL).  The host arrays always have the global
 * shapes.  A time shard uploads its windows from them, halo levels included, and downloads only
 * what it owns -- its blocks' levels, and the fixed levels (Crank-Nicolson: v_0; zeta of the last
 * level) on the rank whose window holds them -- leaving the rest untouched; the device addresses
 * are those of the windows' first levels.
 * kkt_reaction_window: out = [v, zeta, D, block rows] as half-open ranges [first, end) of global
 * levels, as kkt_picard_window (one rank: [0, n_t) three times and [0, m)). */
int kkt_reaction_state(kkt_handle plan, int download, double *v, double *zeta);
int kkt_reaction_iterate(kkt_handle plan, double **d_v, double **d_zeta);
int kkt_reaction_window(kkt_handle plan, int out[8]);
/* The rows [r0, r1] of Instationary.non_linear_res_eval at the plan's iterate with D of the last
 * assembly (backward Euler: n_t rows per family, Crank-Nicolson n_t - 1), Dirichlet rows zero, in
 * d_out (one local vector of the plan's handle); rhs = 1: the right-hand side of the linearised
 * solve (Crank-Nicolson: T_1 on the adjoint rows, T_2 on the state rows).  *norm (host): the
 * 2-norm of the untransformed rows by the deterministic reduction.  KKT_ERR_STATE before any
 * assembly.  Time shards (collective): the rank's rows [lo, hi) of both families, each bit for
 * bit the row of the one-rank result; Crank-Nicolson takes the transforms' terms across the shard
 * boundary from the neighbours' raw rows; the norm is the all-reduced sum of the ranks' sums of
 * squares, the same on every rank. */
int kkt_reaction_residual_device(kkt_handle plan, double *d_out, int rhs, double *norm);
/* v, zeta += the blocks of the update d_u (Crank-Nicolson: v from level 1, zeta levels
 * 0 .. n_t - 2); v is left untouched on the Dirichlet dofs (they hold the boundary values), zeta
 * is zero there; d_u is zeroed: the initial guess of the next solve.  Time shards: the rank's own
 * levels (and zeta's halo level zeroed on the Dirichlet dofs); the halo levels are refreshed by
 * the next assembly. */
int kkt_reaction_update_device(kkt_handle plan, double *d_u);
/* Test hook: the element matrices E (n_t x ne x nv x nv: 9 doubles per P1 triangle, 16 per
 * tetrahedron, 36 per P2 triangle, 81 per Q2 quadrilateral) or D (n_t x nnz) of the last assembly
 * (KKT_ERR_STATE before one), or v / zeta (n_t x n1) of the iterate, copied to the host; cap:
 * doubles available at out (KKT_ERR_ARG when too small).  On a time shard the levels of the
 * windows, in order: E and D those of the D window, v and zeta their own, halo levels included. */
enum { KKT_REACTION_E = 0, KKT_REACTION_D = 1, KKT_REACTION_V = 2, KKT_REACTION_ZETA = 3 };
int kkt_debug_reaction_array(kkt_handle plan, int which, double *out, int64_t cap);
/* The stored values of block (quadrant, i, j) in the CSR order of its pattern, read from the
 * SELL value array through the pattern's slot -> CSR map.  *nnz: the stored entries (out == NULL:
 * only that); *padding_zero: 1 when every padding slot of the value array holds 0.0.  A value
 * array that several blocks share is read as it is. */
int kkt_debug_block_values(kkt_handle h, int quadrant, int i, int j, double *out, int64_t cap,
                           int64_t *nnz, int *padding_zero);

/* ---- Anderson acceleration of a device Picard loop, in update space.
 * Call k = 0, 1, ... of kkt_anderson_step receives in d_u (a local vector of the handle,
 * kkt_vec_alloc) the update f_k of the linearised solve and leaves there the step s_k the loop
 * adds to its iterate:
 *   history   k >= 1: the pair dF = f_k - f_{k-1}, dX = s_{k-1} enters a ring of at most `depth`
 *             pairs; the oldest falls out
 *   Gram      with c pairs kept, G = dF^T dF (c x c) and r = dF^T f_k, every entry recomputed at
 *             every call by one deterministic two-stage reduction (no atomics: equal input gives
 *             equal bits on every run and device)
 *   condition G = L L^T by unpivoted Cholesky on the host in double, columns oldest first;
 *             accepted when every pivot is positive and max L_ii / min L_ii <= cond_max; otherwise
 *             the oldest pair leaves the ring and the rest is factored again
 *   solve     gamma from the two triangular solves
 *   step      s = beta f[i]; for j = oldest .. newest kept: t = dX_j[i] + beta dF_j[i],
 *             s = s - gamma_j t; every product and sum rounded on its own.  c = 0: s = beta f,
 *             which for beta = 1 leaves the bits of f alone.
 * s_k is also kept as the next dX, f_k as f_prev: the caller may zero d_u afterwards.
 * kkt_anderson_set: depth 1 .. KKT_ANDERSON_MAX_DEPTH allocates the history (2 depth + 1 vectors
 * in one pool of the handle, released by kkt_destroy or by depth 0, which removes the mixer) and
 * starts at k = 0; KKT_ERR_ARG naming the argument for another depth, a beta that is not finite
 * or is zero, or cond_max <= 1; KKT_ERR_STATE before kkt_finalize and on a time-sharded handle
 * (the Gram sums would have to ride the ranks' all-reduce).  kkt_anderson_reset: the next call is
 * k = 0 again.  kkt_anderson_step / _reset without a mixer: KKT_ERR_STATE.
 * info (may be NULL): the pairs used by the call and dropped by the condition rule, and the
 * system gamma solves: G (columns x columns, row-major, both triangles, oldest first) and r of
 * the pairs used; with option "stage_timers" the three kernels' times by HIP events (else 0). */
#define KKT_ANDERSON_MAX_DEPTH 8
typedef struct kkt_anderson_info {
    int32_t columns, dropped;
    double gamma[KKT_ANDERSON_MAX_DEPTH];
    double G[KKT_ANDERSON_MAX_DEPTH * KKT_ANDERSON_MAX_DEPTH];
    double r[KKT_ANDERSON_MAX_DEPTH];
    double push_ms, gram_ms, mix_ms;
} kkt_anderson_info;
int kkt_anderson_set(kkt_handle h, int depth, double beta, double cond_max);
int kkt_anderson_step(kkt_handle h, double *d_u, kkt_anderson_info *info);
int kkt_anderson_reset(kkt_handle h);
/* Test hook: one kernel of the mixer on host data, once, on the handle's stream (works on a
 * created handle; every pointer is host memory), or a read-out of the handle's ring.
 *   PUSH  f (n); f_prev (n + slack, read and written); out = dF_new (n + slack)
 *   GRAM  c in 0 .. 8 columns dF (c x n, oldest first), f (n); G (c x c, both triangles filled),
 *         r (c); c = 0 launches nothing
 *   MIX   c, dF, dX (c x n), f (n), gamma (c), beta; out = s (n + slack), out2 = the new dX slot
 *         (n + slack).  alias != 0 (c >= 1): the slot IS column 0 of dX, as in a full ring
 *   READ  which (0 dF, 1 dX: ring slot `slot`; 2: f_prev) of the handle's mixer, n = the
 *         handle's local size, into out (n); ring[0] = head (the slot the next pair enters),
 *         ring[1] = pairs kept (the slots before the head, oldest first), ring[2] = 1 when a
 *         previous call is held, ring[3] = depth.  dX of the head slot holds the last step; in a
 *         full ring that slot is also the oldest pair's, whose dX the step replaced after
 *         reading it (the pair leaves with the next call)
 * The `slack` doubles behind a written array go up as the caller filled them and come back, so
 * that a write past n can be recognised.  inputs_changed: how many read-only arrays came back
 * different.  KKT_ERR_ARG for an unknown op, n < 1, c outside 0 .. 8, slack < 0 or a null array
 * the operation needs. */
enum { KKT_ANDERSON_PUSH = 0, KKT_ANDERSON_GRAM = 1, KKT_ANDERSON_MIX = 2, KKT_ANDERSON_READ = 3 };
typedef struct kkt_anderson_op {
    int32_t op, c, alias, which, slot, inputs_changed;
    int64_t n, slack;
    double beta;
    double gamma[KKT_ANDERSON_MAX_DEPTH];
    const double *f, *dF, *dX;
    double *f_prev, *out, *out2, *G, *r;
    int32_t ring[4];
} kkt_anderson_op;
int kkt_debug_anderson_op(kkt_handle h, kkt_anderson_op *op);

/* `reps` back-to-back kkt_apply_device / kkt_pc_apply_device launches timed with HIP
 * events on the library's own stream; *ms = total elapsed milliseconds. */
int kkt_time_apply(kkt_handle h, const double *d_x, double *d_y, int reps, float *ms);
int kkt_time_pc_apply(kkt_handle h, const double *d_x, double *d_y, int reps, float *ms);
/* One preconditioner application with HIP events around every persistent sweep program of the
 * built-in preconditioner: *ms = their summed duration, *launches / *phases = how many programs
 * and dependent phases ran (0 when the preconditioner has no such programs).  Measurement only. */
int kkt_time_pc_sweeps(kkt_handle h, const double *d_x, double *d_y, float *ms, int *launches,
                       int64_t *phases);

/* Per-stage GPU time of the last kkt_solve* with gmres / fgmres (option "stage_timers" = "1"):
 * HIP events on the library's stream between the stages of every iteration, summed over the
 * solve.  operator = kkt_apply incl. its halo exchange; pc = Preconditioner.apply; orth =
 * classical Gram-Schmidt (dots, updates, norm) without its all-reduces; allreduce = the
 * all-reduces of the inner products (time-sharded handles; includes the wait for the slowest
 * rank); other = residual set-up, normalisation, solution update, host round trips. */
typedef struct kkt_stage_times {
    double operator_ms, pc_ms, orth_ms, allreduce_ms, other_ms, total_ms;
    int64_t iterations, operator_applies, pc_applies;
} kkt_stage_times;
int kkt_get_stage_times(kkt_handle h, kkt_stage_times *out);
/* One application of the built-in block-Schur preconditioner replayed step by step with HIP
 * events: sweeps = the persistent sweep programs (or, without them, the single-block steps of
 * the time sweeps), batched = the steps over all time levels at once (mass solves, products,
 * time transforms), comm = the hand-offs between ranks (time-sharded handles: includes the
 * wait for the neighbour's pipeline stage).  Works on time-sharded handles (collective: every
 * rank calls it).  Measurement only. */
typedef struct kkt_pc_stage_times {
    double sweeps_ms, batched_ms, comm_ms, total_ms;
    int64_t sweep_launches, sweep_phases, batched_launches, comm_steps;
} kkt_pc_stage_times;
int kkt_time_pc_stages(kkt_handle h, const double *d_x, double *d_y, kkt_pc_stage_times *out);

/* The last coarse set-up of the two-grid sub-solves built on this handle (kkt_set_pc_schur, every
 * rebuild after kkt_update_block_values; kkt_set_pc_stokes: the K_p solve -- the velocity
 * sub-solves report on the inner handle): Galerkin matrices P^T A P formed and inverted, kernel
 * launches issued, wall time between two synchronisations of the library's stream, and the
 * coarse dimension.  All zero before any set-up.  Option "coarse_setup" = "columns" selects the
 * previous column-by-column path (3 launches per coarse function, 4 per pivot) for A/B runs. */
typedef struct kkt_coarse_stats {
    int64_t matrices, launches, n_coarse;
    double ms;
    /* diagonal blocks of P^T A P inverted as matrices of their own (the components of a
     * vector-valued space, equal contiguous index ranges) and their size; 1 and n_coarse: the
     * whole matrix (a scalar space, the deflated K_p solve, or option "coarse_blocks" = "0") */
    int64_t blocks, block_n;
} kkt_coarse_stats;
int kkt_coarse_setup_stats(kkt_handle h, kkt_coarse_stats *out);

/* The spectrum estimates of the last preconditioner build on this handle (kkt_set_pc_schur, every
 * rebuild after kkt_update_block_values; kkt_set_pc_stokes: the velocity sub-solves report on the
 * inner handle).  matrices: distinct value sets estimated (twins share); batches: lock-step
 * batches (0 with option "spectrum_batch" = "0"); lanczos_steps / power_steps: summed over the
 * matrices; launches: kernel launches of the estimates and of the twin search; syncs: blocking
 * host round trips of all of it, of which twin_syncs belong to the twin search and lanczos_syncs_max
 * is the largest count one batched Lanczos run took; fallbacks: matrices a batched build estimated
 * or compared one at a time because its collection pass had not covered them (0 expected); ms:
 * wall time of the estimates and the twin search between two synchronisations of the stream;
 * batch_bytes: device memory the largest batch held.  Option "pc_alias": alias_blocks: stored
 * blocks the preconditioner multiplies with that rode the twin search (its launches and
 * synchronisations, not counted in matrices or fallbacks); aliased: arrays, formed or stored, that
 * the build reads from an equal earlier array instead. */
typedef struct kkt_spectrum_stats {
    int64_t matrices, batches, lanczos_steps, power_steps, launches, syncs, twin_syncs,
        lanczos_syncs_max, fallbacks, batch_bytes;
    double ms;
    int64_t alias_blocks, aliased;
} kkt_spectrum_stats;
int kkt_spectrum_stats_get(kkt_handle h, kkt_spectrum_stats *out);
/* Test hooks of the coarse set-up.  With option "coarse_keep" = "1" every set-up keeps its Galerkin
 * matrices P^T A P (before any deflation) on the host: kkt_debug_coarse_matrices copies them,
 * matrices x n_coarse^2 doubles row-major in set-up order (cap: doubles available at out).
 * kkt_debug_dense_inverse inverts nmat host matrices (n x n, row-major, contiguous) with the
 * batched device inverse; bad[b] = first column with a pivot below 1e-13 max|diag| or with a
 * non-finite entry (n: none). */
int kkt_debug_coarse_matrices(kkt_handle h, double *out, int64_t cap);
/* ... and the inverses of the same set-up, in the same layout (the rows as the solves read them:
 * full n_coarse columns, zeros outside the diagonal blocks on the block path) */
int kkt_debug_coarse_inverses(kkt_handle h, double *out, int64_t cap);
int kkt_debug_dense_inverse(kkt_handle h, int n, int nmat, const double *a, double *inv, int *bad);
/* Test hook of the plain coarse correction x_out = x_in + P E^-1 P^T r, on the coarse space of the
 * two-grid preconditioner last built on this handle (kkt_set_pc_schur with a coarse space; with
 * kkt_set_pc_stokes the space of the K_p solve), through the launchers the solves call: the
 * one-vector launches (batched = 0, nb = 1) or the batched ones (batched = 1: nb vectors vstride
 * doubles apart, vstride >= the rows n of P).  All arrays are host memory.  r and x_in (NULL: none)
 * hold nb * vstride doubles; einv is the n_c x n_c row-major matrix to apply -- any matrix, not
 * only an inverse the handle formed.  x_out (nb * vstride doubles) is read and written: entries the
 * kernels do not write come back as given.  The hook owns its coarse scratch and returns it: rc =
 * P^T r and ec = einv rc, nb * n_c doubles each.  shape (NULL, or KKT_COARSE_SHAPE_INTS values)
 * receives the launch constants: rows n of P, n_c, then of the Galerkin set-up on that space R,
 * uniform_w (-1: ragged slices), row-sorted storage (0 | 1), masked rows (0 | 1), block_n of the
 * structure of P^T A P (0: one block), and the longest row of P^T.  nb = 0 fills shape and
 * launches nothing.  KKT_ERR_STATE without such a preconditioner; KKT_ERR_ARG for nb < 0, nb != 1
 * with batched = 0, vstride < n or a null array. */
#define KKT_COARSE_SHAPE_INTS 8
int kkt_debug_coarse_correction(kkt_handle h, int batched, int nb, int64_t vstride, const double *r,
                                const double *x_in, const double *einv, double *rc, double *ec,
                                double *x_out, int32_t *shape);

/* Test hook of the Krylov vector kernels: one operation of the GMRES / MINRES loops on host data,
 * through the members and launchers the solves call.  Independent of the handle's layout: works
 * on a created handle, before or after kkt_finalize (not on a time-sharded one).  w: n doubles;
 * V: nv vectors of n doubles, contiguous; coef: nv doubles (BUILD_SOLUTION, MAXPY).  On the
 * device the vectors sit as the solves keep them, in one allocation at a stride of (n + 31) & ~31
 * doubles: w in slot 0, V_i in slot 1 + i, the padding of every slot set to KKT_KRYLOV_PAD.
 * w_out (n doubles) receives slot 0 after the operation, scalars_out (nv + 2 doubles, zero where
 * the operation writes nothing) its scalar results, arena_out (NULL, or (nv + 1) * stride
 * doubles) the whole allocation.
 *   MDOT            scalars[i] = <w, V_i>
 *   ORTHOGONALISE   the classical Gram-Schmidt step (nv >= 1): scalars[i] = h_i = <w, V_i>,
 *                   w -= sum h_i V_i, scalars[nv] = ||w||, scalars[nv + 1] = ||w||^2
 *   BUILD_SOLUTION  w += sum coef_i V_i, grouped as KSPGMRESBuildSoln
 *   SCALE_INV       w = w * (1 / a)
 *   AXPBY           w = a V_0 + b w (nv >= 1)
 *   COPY            w = V_0; nv == 0: w = w, which launches nothing
 *   FILL            w = a
 *   NORM2           scalars[0] = ||w||, scalars[1] = ||w||^2
 *   MAXPY           w += a sum coef_i V_i by the plain grouped passes alone (a = -1: the update of
 *                   ORTHOGONALISE without the fused norm)
 * KKT_ERR_ARG for n < 1, nv < 0, an unknown op or a null array the operation reads or writes. */
enum { KKT_KRYLOV_MDOT = 0, KKT_KRYLOV_ORTHOGONALISE = 1, KKT_KRYLOV_BUILD_SOLUTION = 2,
       KKT_KRYLOV_SCALE_INV = 3, KKT_KRYLOV_AXPBY = 4, KKT_KRYLOV_COPY = 5, KKT_KRYLOV_FILL = 6,
       KKT_KRYLOV_NORM2 = 7, KKT_KRYLOV_MAXPY = 8 };
#define KKT_KRYLOV_PAD (-6.02214076e23)
int kkt_debug_krylov_op(kkt_handle h, int op, int64_t n, int nv, const double *w, const double *V,
                        const double *coef, double a, double b, double *w_out,
                        double *scalars_out, double *arena_out);

/* Test hook of the time-transform, nullspace and value set-up kernels: one launcher of
 * csrc/kernels.hpp on host data, once, on the handle's stream.  Independent of the handle's layout:
 * works on a created handle.  Every pointer is host memory; the hook uploads, launches, synchronises,
 * downloads and releases.  What each operation reads (others ignored; "opt": may be NULL):
 *   TIME_TRANSFORM       kind 1..4 (T_1, T_2, T_1^-1, T_2^-1), n levels of nx; x (n nx; in_place:
 *                        ignored, the levels are taken from y and y is both operands of the launch);
 *                        lo_halo, hi_halo (opt, nx: the level before the first / after the last); y
 *   TIME_TRANSFORM_MASK  kind 1 | 2, n, nx; x = the raw rows t (n nx), x2 = xin (n nx; opt when no
 *                        level has a mask); mask, has_mask, alpha; lo_halo, hi_halo (opt); y
 *   MASK_BLOCKS          n blocks of nx; x (n nx; in_place as above), x2 = mx (opt); mask, has_mask,
 *                        alpha; y
 *   CONST_CORRECT        kind = second (0, 1, 2), n jobs on a vector of len; y (len, read and
 *                        written), x2 = b (len; second != 0), job_*; y2 = sums (2 n)
 *   CONST_CENTER         n jobs, len; x (len); job_*; y = xc (len), y2 = sums (n)
 *   CSR_TO_SELL          nx padded entries; x = CSR values (len), idx = map (nx, -1 | < len); y
 *   MASK_COLUMNS         nx; idx = col (nx, in [0, len)), mask = column mask (len bytes); y (nx,
 *                        read and written)
 *   VALS_AXPY            nx; x = a (opt), c, x2 = b; y
 *   VALS_DIFFER          nx; x = a, x2 = b; flag
 *   VALS_SYM_SKEW        nx; x = a, idx = tpos (nx, -1 | < nx); y = h, y2 = sk; flag
 *   EXTRACT_DINV         kind = R (1 | 2), n slices of C = 64 R positions, len rows (without idx3:
 *                        len <= n C); idx2 = slice_off (n + 1, from 0, ascending), nx =
 *                        slice_off[n] C; idx = col (nx), x = vals (nx), idx3 = perm (opt, n C
 *                        entries, -1 | < len), mask = row mask (opt, len bytes); y = dinv (len)
 * mask: n * nx bytes, level i at i * nx (NULL: no level has a mask); has_mask (opt, n): 0 gives
 * level i a null mask; alpha: n doubles (required with mask).  job_off, job_nx, job_c1,
 * job_c2_one, job_c2_alpha: n entries each, the fields of the launch's job list (the launch's
 * max_nx is the largest job_nx).
 * Written arrays are guarded.  y and y2 hold KKT_BLOCK_GUARD doubles, the array, KKT_BLOCK_GUARD
 * doubles; flag holds KKT_BLOCK_GUARD words, the flag, KKT_BLOCK_GUARD words.  The hook sets the
 * guards to KKT_KRYLOV_PAD (flag: KKT_BLOCK_FLAG_PAD), uploads the whole allocation -- the array
 * part as the caller filled it, so that elements a kernel must not touch can be recognised -- and
 * returns the whole allocation.  Every array the launch only reads is downloaded again and
 * compared with what went up: inputs_changed receives the number of arrays that differ.
 * KKT_ERR_ARG (nothing launched) for an unknown op or kind, a null array the operation needs,
 * in_place on another operation, sizes < 1, an index outside its array, a job that is not inside
 * [0, len). */
enum { KKT_BLOCK_TIME_TRANSFORM = 0, KKT_BLOCK_TIME_TRANSFORM_MASK = 1, KKT_BLOCK_MASK_BLOCKS = 2,
       KKT_BLOCK_CONST_CORRECT = 3, KKT_BLOCK_CONST_CENTER = 4, KKT_BLOCK_CSR_TO_SELL = 5,
       KKT_BLOCK_MASK_COLUMNS = 6, KKT_BLOCK_VALS_AXPY = 7, KKT_BLOCK_VALS_DIFFER = 8,
       KKT_BLOCK_VALS_SYM_SKEW = 9, KKT_BLOCK_EXTRACT_DINV = 10 };
#define KKT_BLOCK_GUARD 64
#define KKT_BLOCK_FLAG_PAD 0xA5A5A5A5u
typedef struct kkt_block_op {
    int op, kind, in_place, n;
    int64_t nx, len;
    double c;
    const double *x, *x2, *lo_halo, *hi_halo;
    const uint8_t *mask;
    const int32_t *has_mask;
    const double *alpha;
    const int64_t *job_off, *job_nx;
    const double *job_c1, *job_c2_one, *job_c2_alpha;
    const int32_t *idx, *idx2, *idx3;
    double *y, *y2;
    uint32_t *flag;
    int32_t inputs_changed;
} kkt_block_op;
int kkt_debug_block_op(kkt_handle h, kkt_block_op *op);

/* Test hook of the kernels of the batched spectrum estimates and the twin search
 * (csrc/spectrum_kernels.hip): one launch_spec_* of csrc/kernels.hpp on host data, once, on the
 * handle's stream, with the launcher's own grid.  Works on a created handle; every pointer is host
 * memory; the hook uploads, launches, synchronises, downloads and releases.
 *   DOT           launch_spec_dot (both stages), mode KKT_SPECTRUM_DOT_*, k (NORM: the power step),
 *                 nmat matrices of n rows, max_steps >= 1; x, y: the two vector families, nmat
 *                 vectors at a spacing of `stride` doubles each (even, >= n; y may be x), read only;
 *                 the scalar state, all read and written: active, na, nb, rz, coef, last, mu2 (nmat
 *                 each), alpha, beta (max_steps * nmat, step-major), part (1024 nmat partial sums)
 *   UPDATE        launch_spec_update, mode KKT_SPECTRUM_UPD_*: v is the family written (R, SCALE: r;
 *                 P, COPY: p), x the family read (R: w; P, SCALE, COPY: z), both nmat * stride;
 *                 active and coef, read only here
 *   SYM_SKEW      launch_spec_sym_skew over nmat arrays of n values: a (nmat * n, contiguous), tpos
 *                 (n, -1 | < n); h, sk (nmat * n), flag (nmat words)
 *   FINGERPRINT   launch_spec_fingerprint: a (nmat * n); words receives the nwords =
 *                 max(1, min(64, ceil(n / 2048))) words of each array (nmat * nwords), fold (nmat,
 *                 not guarded) the host's fold of them, the value the twin search groups by
 *   PAIRS_DIFFER  launch_spec_pairs_differ: a (nmat * n); pair q compares arrays pair_a[q] and
 *                 pair_b[q] (npairs entries in [0, nmat) each; an array may stand on both sides and
 *                 in several pairs); flag (npairs words, read and written)
 * Every array but x, y, a, tpos, pair_a, pair_b and fold is guarded as those of kkt_debug_block_op
 * are: KKT_BLOCK_GUARD elements, the array, KKT_BLOCK_GUARD elements.  The hook sets the guards --
 * doubles to KKT_KRYLOV_PAD, 64-bit words to its bit pattern, 32-bit words to KKT_BLOCK_FLAG_PAD --
 * uploads the whole allocation, the array part as the caller filled it, and returns the whole
 * allocation.  Arrays the launch only reads (active and coef of UPDATE, with their guards, among
 * them) are downloaded again and compared with what went up: inputs_changed receives the number of
 * arrays that differ.  batch_stride receives the spacing the estimates themselves use for n rows
 * (DOT, UPDATE).
 * KKT_ERR_ARG (nothing launched, no array touched) for an unknown op or mode, a null array the
 * operation needs, nmat, n, npairs or max_steps < 1, nmat or npairs > 65535, more than 2^31
 * elements in an array, an odd stride or one below n, k < 0, a negative na or nb, a tpos entry or
 * pair index outside its range. */
enum { KKT_SPECTRUM_DOT = 0, KKT_SPECTRUM_UPDATE = 1, KKT_SPECTRUM_SYM_SKEW = 2,
       KKT_SPECTRUM_FINGERPRINT = 3, KKT_SPECTRUM_PAIRS_DIFFER = 4 };
enum { KKT_SPECTRUM_DOT_START = 0, KKT_SPECTRUM_DOT_PAP = 1, KKT_SPECTRUM_DOT_RZ = 2,
       KKT_SPECTRUM_DOT_NORM0 = 3, KKT_SPECTRUM_DOT_NORM = 4 };
enum { KKT_SPECTRUM_UPD_R = 0, KKT_SPECTRUM_UPD_P = 1, KKT_SPECTRUM_UPD_SCALE = 2,
       KKT_SPECTRUM_UPD_COPY = 3 };
typedef struct kkt_spectrum_op {
    int op, mode, k, nmat, max_steps, npairs;
    int64_t n, stride;
    const double *x, *y;
    double *v;
    uint32_t *active;
    int32_t *na, *nb;
    double *rz, *coef, *last, *mu2, *alpha, *beta, *part;
    const double *a;
    const int32_t *tpos;
    double *h, *sk;
    const int32_t *pair_a, *pair_b;
    uint32_t *flag;
    uint64_t *words, *fold;
    int64_t batch_stride;
    int32_t inputs_changed;
} kkt_spectrum_op;
int kkt_debug_spectrum_op(kkt_handle h, kkt_spectrum_op *op);

/* Test hook of the preconditioner's row steps: ONE launch of a launcher SchurPC::replay calls
 * (csrc/kernels.hpp) on host data, on the handle's stream.  Needs a finalized handle: block
 * (q, i, j) names the SELL pattern of every op of the call, and every term matrix is a stored block
 * of that pattern (square: the vectors of a call all have its `nrows` elements).
 *   form ROWS         launch_rowops, tag 1, nops >= 1 ops from device memory       (pc_rows)
 *        SINGLE       the same with one op handed over by value (h_single)         (pc_row_step)
 *        SHARED       launch_rowops_shared: every op has one term, all the same block; `launched`
 *                     receives the launcher's return value (0: it declined, nothing ran)
 *        INTERLEAVED  launch_rowops_il: nops time LEVELS in groups of four, as
 *                     SchurPC::emit_solves_interleaved builds them.  ops[l] gives the level's b,
 *                     post1, post2 and, on the last step, its output y; ops[0] the matrix (its
 *                     one term's block, in every step; term_x is not read) and c1, c2, c3.  il_x / il_pkm1 (NULL: first / second step) hold the
 *                     interleaved iterates, ceil(nops / 4) * 4 * nrows doubles, element (group g,
 *                     row r, level l) at 4 (g nrows + r) + l; il_y (guarded like a vector of that
 *                     length) receives the interleaved output, NULL: the last step, which writes
 *                     the levels' y.
 * Vectors are named by their index into `vecs` (-1: absent): nvec slots of KKT_BLOCK_GUARD + nrows
 * + KKT_BLOCK_GUARD doubles.  The hook sets every guard to KKT_KRYLOV_PAD, uploads the whole table,
 * and afterwards returns the slots the launch may write (y, y2) whole; every other slot, the mask,
 * dinv, il_x and il_pkm1 are downloaded again and compared (inputs_changed: how many differ).
 * An op reads term_x[t] through block (term_q[t], term_i[t], term_j[t]); mode KKT_ROWSTEP_LIN:
 * y = ca acc + cy yin + cz z (masked rows: malpha mx, 0 without mx) and y2 = c3 dinv y;
 * KKT_ROWSTEP_CHEB: y = post2 (post1 (c1 pkm1 + c2 pk + c3 dinv (b - acc))) (masked rows: 0).  An op
 * without terms is given the all-zero slice offsets and uniform_w 0, as the emitters do.
 * The one aliasing the emitters produce is allowed -- LIN with yin == y (the level update in place);
 * KKT_ERR_ARG for any other vector that one op writes and the same or another op of the launch
 * reads or writes, for a term block of another pattern, an index outside the table, a missing
 * operand (CHEB: b, dinv; y2: dinv), SINGLE with nops != 1, SHARED or INTERLEAVED on R != 2 or with
 * ops the production planner would not batch.  Nothing is launched then.
 * Out: family (KKT_ROWSTEP_PC_*) and width -- the template instantiation the launcher's dispatch
 * picks for this pattern (pc_rows / pc_row_step: WFIX; pc_rows_shared: W; pc_rows_shared_g and
 * pc_rows_il: KC) -- and the pattern's R, uniform_w (-1: ragged), sorted (row-sorted storage) and
 * nslices.  The launchers themselves report nothing: family and width are the hook's restatement
 * of their dispatch (csrc/rowstep.cpp), not an observation of the kernel that ran; `launched` is
 * the launcher's own return value. */
enum { KKT_ROWSTEP_ROWS = 0, KKT_ROWSTEP_SINGLE = 1, KKT_ROWSTEP_SHARED = 2,
       KKT_ROWSTEP_INTERLEAVED = 3 };
enum { KKT_ROWSTEP_LIN = 0, KKT_ROWSTEP_CHEB = 1 };
enum { KKT_ROWSTEP_PC_ROWS = 0, KKT_ROWSTEP_PC_ROW_STEP = 1, KKT_ROWSTEP_PC_ROWS_SHARED = 2,
       KKT_ROWSTEP_PC_ROWS_SHARED_G = 3, KKT_ROWSTEP_PC_ROWS_IL = 4 };
#define KKT_ROWSTEP_MAX_TERMS 8
typedef struct kkt_row_step_op {
    int32_t mode, nterms;
    int32_t term_q[KKT_ROWSTEP_MAX_TERMS], term_i[KKT_ROWSTEP_MAX_TERMS],
        term_j[KKT_ROWSTEP_MAX_TERMS], term_x[KKT_ROWSTEP_MAX_TERMS];
    int32_t y, y2, yin, z, mx, b, pkm1, pk;
    double ca, cy, cz, malpha, c1, c2, c3, post1, post2;
} kkt_row_step_op;
typedef struct kkt_row_step {
    int32_t form, q, i, j, nops, pc_xcd, nvec, pad_;
    const kkt_row_step_op *ops;
    double *vecs;
    const uint8_t *rowmask;     /* nrows bytes, or NULL */
    const double *dinv;         /* nrows doubles, or NULL */
    const double *il_x, *il_pkm1;
    double *il_y;
    /* out */
    int32_t family, width, launched, inputs_changed, R, uniform_w, sorted, nslices;
} kkt_row_step;
int kkt_debug_row_step(kkt_handle h, kkt_row_step *step);

/* Test hook of the tile program's two-grid levels: ONE call of launch_tile_sweep (csrc/kernels.hpp,
 * the variant with coarse corrections) on host data, on the handle's stream, with the tile plan,
 * the coarse tables, the row mask and the error words of the two-grid block Schur preconditioner
 * last built on this handle (kkt_set_pc_schur with a coarse space, after its first application) --
 * so with what the options "tile_coarse_cache", "tile_coarse_rows", "coarse_rings", "tile_depth"
 * and "tile_waves" made of them.  The launch runs `nlevels` levels of `cycles` x [coarse correction
 * of the iterate, `its` sweeps] from a zero guess each.  Per level:
 *   (q, i, j)   a stored block on the preconditioner's level pattern: the level's matrix
 *   dinv        nrows doubles; coef: `its` triples c1, c2, c3 (sweep s: p+ = c1 p- + c2 p + c3 dinv
 *               (b - A p), without the p- term in the first sweep after a correction); post1,
 *               post2: the factors of the last sweep of the last cycle; p1_scale: the first step
 *               p_1 = p1_scale dinv b, which a two-grid level computes and then overwrites
 *   einv        n_coarse x n_coarse doubles, row-major, applied as (P^T A P)^-1: any matrix (with
 *               "block" rows: zero outside the column range the tables give its rows).  Levels
 *               that name the same array share one device copy, as levels with one matrix do.
 *   n_upd = 0   a solo level: the right-hand side is bin
 *   n_upd = 1   a chained level (not the first): b = ca U x_prev + cy bin with U the stored block
 *               (uq, ui, uj) and x_prev the previous level's result, handed over inside the launch;
 *               bout (may be NULL) receives b on the rows some tile owns
 *   bin, out, bout   KKT_BLOCK_GUARD + nrows + KKT_BLOCK_GUARD doubles each.  The hook sets the
 *               guards to KKT_KRYLOV_PAD and the nrows elements of out to +0.0 (the rows of the
 *               mask belong to no tile and are never written); out and bout come back whole.
 * What the launch only reads (bin, dinv) is downloaded again and compared: inputs_changed is the
 * number of arrays that differ.  own_ptr (own_cap >= tiles + 1 entries) and own_rows (nrows
 * entries) receive, tile by tile, the global rows a tile owns in its local order: tile t owns
 * own_rows[own_ptr[t] .. own_ptr[t + 1]); unused entries are -1.  Further out: tiles, threads,
 * row_slots, depth, W and nk_pad of the plan; cache (2 | 1 | 0), rings and ew of the coarse tables;
 * n_coarse; nrows.  nlevels = 0 fills these and launches nothing (own_ptr, own_rows may be NULL).
 * The workgroups of the program wait for one another: the hook launches only after the residency
 * check of the production path for the LDS bytes of this `its`, zeroes the granule buffers as the
 * first launch of an application does, and launches once.  A bounded-spin time-out comes back as
 * KKT_ERR_STATE with the diagnostic record in kkt_last_error.  KKT_ERR_STATE also without a
 * two-grid tile program on the handle.  KKT_ERR_ARG, nothing launched: nlevels < 0 or > 64, its or
 * cycles < 1, a plan that is not resident with this `its`, a null operand, a block that is not
 * stored or has another pattern, n_upd other than 0 | 1 or 1 on the first level, bout on a solo
 * level, own_cap too small, "block" rows with a matrix that is non-zero outside its ranges. */
typedef struct kkt_tile_level {
    int32_t q, i, j, n_upd, uq, ui, uj, pad_;
    double ca, cy, p1_scale, post1, post2;
    const double *dinv, *coef, *einv;
    double *bin, *out, *bout;
} kkt_tile_level;
typedef struct kkt_tile_levels {
    int32_t nlevels, its, cycles, own_cap;
    kkt_tile_level *levels;
    int32_t *own_ptr, *own_rows;
    /* out */
    int32_t inputs_changed, tiles, threads, row_slots, depth, W, nk_pad, cache, rings, ew,
        n_coarse, nrows;
} kkt_tile_levels;
int kkt_debug_tile_levels(kkt_handle h, kkt_tile_levels *run);

/* Step-locked parity hook (tests): while set, kkt_solve / kkt_solve_device with gmres or
 * fgmres replace their Krylov basis v_0 .. v_it by the caller's vectors before inner step `it`
 * of global step s (s < n_steps), and record what the step produced from them: the classical
 * Gram-Schmidt coefficients h_0 .. h_it and ||w|| after the projection (h + s * (restart + 2)),
 * and the normalised new basis vector (v_next + s * n_local).  Two implementations of GMRES
 * separate exponentially along a trajectory; single steps from identical inputs do not
 * (preconditioner.py:732-759 is third-party PETSc code: this pins the restatement step by step
 * against the CPU oracle).  V holds n_steps * (restart + 1) * n_local doubles; all arrays are
 * host memory owned by the caller and must stay valid through the NEXT solve, which consumes
 * the hook: it is cleared when that solve returns (or by passing NULL). */
typedef struct kkt_steplock {
    int n_steps;
    int restart;
    const double *V;
    double *h;
    double *v_next;
} kkt_steplock;
int kkt_debug_set_steplock(kkt_handle h, const kkt_steplock *lock);

/* Test hooks: which kernel form each planned launch runs (read-only; they change no launch).
 * Both return the number of records (>= 0) or a negative KKT_ERR_*; out == NULL asks for the count,
 * otherwise `cap` (int32 values available at out) must hold every record.
 * kkt_debug_apply_forms: one record of KKT_APPLY_FORM_INTS per kkt_apply launch, in launch order:
 *   R (rows per lane of the SELL-64R storage); uniform_w: 1..16 the fixed-width kernel of that
 *   width, 0 rows without blocks, -1 or a uniform width above 16 the slot loop, -2 / -3 / -4 the
 *   width-switched kernel (four
 *   waves / one wave per workgroup / narrow slices); groups of equal structure served by the
 *   shared-values kernel (0: none); 1 when the storage is row-sorted (SELL-C-sigma), else 0.
 * kkt_debug_pc_forms: one record of KKT_PC_FORM_INTS per row step, sweep program and tile launch
 *   of the built-in preconditioner, in replay order: form (KKT_PC_*); width; slots; stream (0 the
 *   handle's, 1 the side lane); count; variant.
 *     row steps (PLAIN, SHARED matrix, KERNARG single op, INTERLEAVED levels): width = uniform_w
 *       of the level pattern (as above), slots = R, count = row ops (interleaved: groups of four
 *       time levels), variant 0;
 *     PROGRAM (a persistent row program): width = uniform_w, slots = R, count = phases, variant
 *       0 counters ("flags"), 1 data-flow fixed width, 2 data-flow any width ("w");
 *     TILE: width = W of the tile kernel, slots = row slots per thread, count = threads per
 *       workgroup, variant = 1 (level update fused) | 2 (coarse corrections);
 *     TILE_CHEB (several steps of a batched one-matrix solve out of LDS): width = W of the form's
 *       tile plan, slots = row slots per thread, count = Chebyshev steps in this launch, variant =
 *       threads per workgroup.
 *   0 records before kkt_set_pc_schur. */
enum { KKT_APPLY_FORM_INTS = 4, KKT_PC_FORM_INTS = 6 };
enum { KKT_PC_ROWS_PLAIN = 0, KKT_PC_ROWS_SHARED = 1, KKT_PC_ROWS_KERNARG = 2,
       KKT_PC_ROWS_INTERLEAVED = 3, KKT_PC_PROGRAM = 4, KKT_PC_TILE = 5, KKT_PC_TILE_CHEB = 6 };
int kkt_debug_apply_forms(kkt_handle h, int32_t *out, int cap);
int kkt_debug_pc_forms(kkt_handle h, int32_t *out, int cap);

/* Test hooks: the Chebyshev intervals the built-in preconditioner runs with (read-only; they
 * change no launch).  Same calling convention as kkt_debug_pc_forms, in doubles: the return value
 * is the number of records, `cap` counts doubles.  0 records before the preconditioner is built.
 * kkt_debug_pc_solves: one record of KKT_PC_SOLVE_VALS per Schur sub-solve of the block Schur
 *   preconditioner, in emission order: sweep (KKT_PC_SWEEP_*); time level; index of the matrix
 *   (a kkt_debug_pc_matrices record); shift c of the matrix blk + c M~; emin; emax; eimag; degree
 *   its (two-grid: sweeps per cycle); estimate (KKT_PC_EST_* of the matrix).
 *   On a handle with the Stokes preconditioner: one record, sweep KKT_PC_SWEEP_KP, for the K_p
 *   solve -- level and matrix -1, c 0, emin / emax / its of K_p, eimag 0, estimate
 *   KKT_PC_EST_ZERO_MEAN (both ends by Lanczos on the range), KKT_PC_EST_UPPER (upper end only,
 *   emin from the velocity sub-solves) or KKT_PC_EST_GIVEN; the velocity sub-solves are reported
 *   by the inner handle.
 * kkt_debug_pc_matrices: one record of KKT_PC_MATRIX_VALS per distinct matrix blk + c M~ the
 *   Schur preconditioner formed, in creation order: c; estimate (KKT_PC_EST_GIVEN, _LANCZOS,
 *   _SHARED with an earlier matrix of equal values, _NONE: only multiplied with); Lanczos steps;
 *   power-iteration steps (skew part); 1 if it has a coarse inverse, else 0; number of sub-solves
 *   that use it. */
enum { KKT_PC_SOLVE_VALS = 9, KKT_PC_MATRIX_VALS = 6 };
enum { KKT_PC_SWEEP_FIRST = 0, KKT_PC_SWEEP_SECOND = 1, KKT_PC_SWEEP_FORWARD = 2,
       KKT_PC_SWEEP_BACKWARD = 3, KKT_PC_SWEEP_KP = 4 };
enum { KKT_PC_EST_GIVEN = 0, KKT_PC_EST_LANCZOS = 1, KKT_PC_EST_SHARED = 2, KKT_PC_EST_NONE = 3,
       KKT_PC_EST_ZERO_MEAN = 4, KKT_PC_EST_UPPER = 5 };
int kkt_debug_pc_solves(kkt_handle h, double *out, int cap);
int kkt_debug_pc_matrices(kkt_handle h, double *out, int cap);
/* Test hook of option "pc_alias" (read-only; same calling convention as kkt_debug_pc_forms): one
 * record of KKT_PC_ALIAS_INTS per Schur sub-solve, in the order of kkt_debug_pc_solves, naming the
 * device arrays the level reads -- its matrix, its Jacobi diagonal, the first term of its update
 * (-1: a level without update).  Arrays are numbered in order of first appearance; equal numbers
 * mean the same device array. */
enum { KKT_PC_ALIAS_INTS = 3 };
int kkt_debug_pc_alias(kkt_handle h, int32_t *out, int cap);

/* Test hook of the batched mass solves on tiles (form KKT_PC_TILE_CHEB; read-only): the mass
 * matrix's values as the tile kernels read them -- n_entries doubles in the layout of the plan's
 * column table, [tile][row slot][entry][thread] -- into `copy`; the plan's position table (index
 * into the value array, -1: padding) into `gpos`; the value array itself (n_vals doubles) into
 * `vals`.  copy[i] is vals[gpos[i]], and +0.0 where gpos[i] < 0.  Null pointers are skipped: call
 * once with the three arrays null for the two lengths.  KKT_ERR_STATE where no mass solve runs on
 * tiles. */
int kkt_debug_mass_tile_values(kkt_handle h, int64_t *n_entries, int64_t *n_vals, double *copy,
                               int32_t *gpos, double *vals);

/* Byte accounting of the stored operator ("algorithmic bytes"). */
typedef struct kkt_info {
    int64_t n_local;            /* local KKT vector length */
    int64_t n_blocks_stored;    /* (i,j) blocks held by this handle */
    int64_t n_value_arrays;     /* distinct value arrays (== blocks in mode G) */
    int64_t n_patterns;         /* distinct sparsity structures */
    int64_t nnz_blocks;         /* sum of nnz over stored blocks */
    int64_t rows_blocks;        /* sum of rows over stored blocks */
    int64_t bytes_algorithmic;  /* sum_unique[12 nnz + 4(rows+1)] + 16 N */
    int64_t bytes_device_values;/* padded value bytes actually resident */
    int64_t bytes_device_index; /* padded index bytes actually resident */
    int64_t bytes_streamed;     /* bytes one kkt_apply must move with what is stored once read
                                   once: sum over value arrays 8 nnz + sum over sparsity
                                   structures [4 nnz + 4 (rows + 1)] + 16 N */
    double last_solve_ms;       /* wall time of the last kkt_solve* Krylov loop */
    int64_t last_pc_applies;    /* preconditioner applications in the last solve */
    int64_t last_op_applies;    /* operator applications in the last solve */
    int64_t program_fallbacks;  /* times a persistent sweep program timed out waiting for a
                                   neighbour workgroup and the preconditioner was rebuilt as
                                   plain launches (kkt_last_error holds the diagnostic record) */
    /* how the time sweeps of the built-in preconditioner run (0 everywhere: none built yet) */
    int64_t sweep_form;         /* 0 plain launches, 1 counter row program, 2 data-flow row
                                   program, 3 tile program */
    int64_t sweep_tiles, sweep_threads, sweep_depth, sweep_row_slots;   /* tile program plan */
    int64_t sweep_its;          /* Chebyshev degree of the sub-solves (given or derived) */
    int64_t apply_launches;     /* kernel launches of one kkt_apply (block rows only) */
    int64_t apply_switched;     /* ... of which run the width-switched kernel for ragged
                                   structures (P2 / Stokes blocks; option "ragged_switch") */
    int64_t blocks_unset;       /* blocks added by kkt_add_block_structure that no composition or
                                   update has written yet */
    int64_t sweep_coarse_rings; /* 1: the tile program that was built prolongs coarse corrections
                                   onto the tiles' rings (option "coarse_rings", where the lists
                                   fit on chip); 0: it fetches them in a hand-off, or no two-grid
                                   tile program was built */
    int64_t sweep_coarse_cache; /* where sweep_form == 3 and a two-grid tile program was built: 2 a
                                   tile's coarse lists and its rows of the coarse inverse are in
                                   LDS, 1 the lists only, 0 neither (option "tile_coarse_cache");
                                   otherwise 0 */
    int64_t sweep_coarse_ew;    /* ... and the row length of the coarse inverse in use: the widest
                                   diagonal block of P^T A P (from a multiple of 64), or n_coarse
                                   for full rows (option "tile_coarse_rows"); otherwise 0 */
} kkt_info;
int kkt_get_info(kkt_handle h, kkt_info *info);

/* ------------------------------------------------------------------ multi-GPU */

/* Transport for time-sharded handles.  RCCL: `unique_id` is the 128-byte ncclUniqueId
 * from kkt_comm_unique_id() on rank 0, distributed by the launcher. */
int kkt_comm_unique_id(void *id_out_128);
int kkt_comm_init_rccl(kkt_handle h, const void *unique_id_128);
/* Host-staged transport through caller functions (tests; any launcher without RCCL).
 * allreduce: in-place reduction over ranks of n doubles, op = KKT_OP_SUM or KKT_OP_MAX;
 * sendrecv: send `n_send` doubles to `dst` (or -1: nothing) and receive `n_recv` from
 * `src` (or -1).  Return 0 on success. */
enum { KKT_OP_SUM = 0, KKT_OP_MAX = 1 };
typedef int (*kkt_allreduce_fn)(void *user, double *buf, int n, int op);
typedef int (*kkt_sendrecv_fn)(void *user, const double *send, int64_t n_send, int dst,
                               double *recv, int64_t n_recv, int src);
int kkt_comm_init_callbacks(kkt_handle h, kkt_allreduce_fn ar, kkt_sendrecv_fn sr,
                            void *user);
/* Barrier and max over ranks of a scalar (timing bracket of bench.py). */
int kkt_comm_barrier(kkt_handle h);
int kkt_comm_max(kkt_handle h, double *value_inout);

#ifdef __cplusplus
}
#endif
#endif /* KKT_H */
