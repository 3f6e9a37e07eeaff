// Built-in block Schur-complement preconditioner on the GPU: the `pc_linear` closures of
// Control.Stationary.construct_pc (reference control/control.py:351-450) and
// Control.Instationary.construct_pc (control.py:1943-2440).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "comm.hpp"
#include "rowlaunch.hpp"
#include "spectrum_host.hpp"
#include "system.hpp"
#include "tiles.hpp"

namespace kkt {

// (Spectrum: spectrum_host.hpp)
Spectrum jacobi_spectrum(System &S, int pattern, const double *vals, const double *dinv,
                         const uint8_t *rowmask, int max_steps,
                         bool zero_mean = false);
// spectral radius of D^-1 S for the values `skew_vals` of a skew-symmetric matrix on `pattern`
// (power iteration on -(D^-1 S)^2; an estimate from below)
double jacobi_skew_radius(System &S, int pattern, const double *skew_vals, const double *dinv,
                          const uint8_t *rowmask, int max_steps, int *steps_out);

// The same for a batch of matrices on one pattern in lock-step (spectrum.cpp): results equal the
// one-matrix functions' bit for bit.  Counters add up over calls; bytes and lanczos_syncs_max keep
// the largest.
struct SpectrumCounters {
    int64_t launches = 0, syncs = 0, lanczos_syncs_max = 0, bytes = 0;
};
std::vector<Spectrum> jacobi_spectrum_batch(System &S, int pattern, const std::vector<const double *> &vals,
                                            const std::vector<const double *> &dinv, const uint8_t *rowmask,
                                            int max_steps, SpectrumCounters *cnt);
std::vector<double> jacobi_skew_radius_batch(System &S, int pattern,
                                             const std::vector<const double *> &skew_vals,
                                             const std::vector<const double *> &dinv,
                                             const uint8_t *rowmask, int max_steps,
                                             std::vector<int> *steps_out, SpectrumCounters *cnt);

struct PcStep {
    enum Kind { ROWS, TIME, COPY, COMM, PROG, TILE, EV_RECORD, EV_WAIT, COARSE, ROWS_IL, TILE_CHEB } kind;
    int mt = -1;                    // TILE_CHEB: index into the mass tile launches (K steps of a batched solve)
    IlOp *d_il = nullptr;           // ROWS_IL: one IlOp per group of four time levels
    int il_groups = 0, il_slices = 0, il_w = 0;
    const double *einv = nullptr;   // COARSE: y = (x or 0) + P E^-1 P^T cr
    const double *cr = nullptr;     // COARSE: the residual that is restricted
    int lane = 0;                   // 0: the system's stream; 1: the side stream
    int level = -1;                 // the sweep level this step belongs to (index into sweep_levels_)
    int solve = -1;                 // the batched mass solve it belongs to (index into mass_solves_)
    int ev = -1;                    // EV_RECORD / EV_WAIT: event index
    RowLaunch rows;                 // ROWS
    double *y = nullptr;            // TIME / COPY
    const double *x = nullptr;
    int tkind = 0, n = 0;
    int64_t nx = 0;                 // TIME: block length; COPY / COMM: element count
    const double *lo_halo = nullptr, *hi_halo = nullptr;   // TIME on a time shard
    int dst = -1, src = -1;         // COMM: send x to dst, receive y from src
    int nphases = 0;                // PROG: rows.d_ops holds nphases single-block RowOps
    bool granule = false;           // PROG: data-flow form (tagged granules)
    PhaseLite *d_lite = nullptr;    // PROG: compact per-phase records (data-flow form)
    int gmode = 0;                  // PROG: 0 counters, 1 data-flow fixed width, 2 data-flow any width
    TileLevel *d_levels = nullptr;  // TILE: nlevels time levels of `its` steps each
    int nlevels = 0, its = 0;
    uint32_t epoch0 = 0;            // TILE: first hand-off tag of this launch minus one
    bool fused = true;              // TILE: kernel variant with the level update
    bool clear = false;             // TILE: zero the granule buffers first
    bool clear_coarse = false;      // TILE, coarse: zero the coarse exchanges' granule buffers first
    bool coarse = false;            // TILE: two-grid levels
    const double **d_einv = nullptr;   // TILE, coarse: per level (P^T A P)^-1
    uint32_t cepoch0 = 0;           // TILE, coarse: first coarse-exchange tag of this launch minus one
};

// Coarse set-up of the two-grid solves, shared by the Schur sub-solves and the K_p solve.
// Structure of E = P^T A P (rows of P^T, rows of A, rows of P in CSR): row i holds every k whose
// coarse function meets the rows that A couples to coarse function i, ascending.
void galerkin_structure(int nc, const std::vector<int32_t> &pt_ip, const std::vector<int32_t> &pt_ix,
                        const std::vector<int32_t> &a_ip, const std::vector<int32_t> &a_ix,
                        const std::vector<int32_t> &p_ip, const std::vector<int32_t> &p_ix,
                        std::vector<int32_t> &e_ip, std::vector<int32_t> &e_ix);
// Size b of the diagonal blocks of E = P^T A P on the structure e_ip / e_ix when its coupled coarse
// functions form nc / b >= 2 contiguous index ranges of equal size (the components of a
// vector-valued space: one copy of the coarse functions per component), else 0.
int coarse_block_size(int nc, const std::vector<int32_t> &e_ip, const std::vector<int32_t> &e_ix);
// einv[b] = (P^T A_b P + shift_b 1 1^T)^-1 for a batch of level matrices (SELL values vals[b] on
// the pattern `pat` of S): one Galerkin launch, a blocked Gauss-Jordan over the batch, or -- option
// "coarse_setup" = "columns" -- the column path per matrix.  deflate: shift_b = trace(E_b) / nc^2
// (the K_p solve: E inherits the constants as its kernel).  Fills S.coarse_stats; fails with
// KKT_ERR_STATE naming the matrix and column of a (relatively) zero pivot.  Without deflation and
// with g.block_n > 0 (option "coarse_blocks" = "0" turns it off) the batched path inverts the
// diagonal blocks of every E_b as matrices of size block_n and scatters them into einv's full
// rows, exact zeros outside the blocks; the singularity test then scales by each block's max|diag|.
void coarse_setup(System &S, int pat, const CoarseDev &c, const GalerkinDev &g,
                  const std::vector<const double *> &vals, const std::vector<double *> &einv,
                  bool deflate, const char *what);

// inv[b] = a_b^-1 for nmat host matrices through the batched device inverse (test hook)
void dense_inverse_host(System &S, int n, int nmat, const double *a, double *inv, int *bad);
// kkt_debug_coarse_correction (include/kkt.h)
void coarse_correction_host(System &S, int batched, int nb, int64_t vstride, const double *r,
                            const double *x_in, const double *einv, double *rc, double *ec,
                            double *x_out, int32_t *shape);

// A device-resident pc_fn: reads the nullspace-corrected right-hand side from in(), leaves
// pc_fn(b) in out() (both n_local doubles, fixed buffers).
class PcBase {
   public:
    virtual ~PcBase() {}
    virtual void run() = 0;
    virtual double *in() = 0;
    virtual double *out() = 0;
    virtual void values_changed() {}
    virtual void check() {}
    // A persistent sweep program gave up waiting for a neighbour (bounded spins): true once,
    // with the diagnostic record in *why.  fallback_plain() then rebuilds the preconditioner as
    // plain launches (same arithmetic), so the caller can redo the work instead of failing.
    virtual bool timed_out(std::string *) { return false; }
    virtual bool fallback_plain() { return false; }
    // device word that is non-zero after a time-out (null: this preconditioner has no programs)
    virtual const unsigned *err_word() const { return nullptr; }
    // one application replayed step by step with events (kkt_time_pc_stages)
    virtual void time_stages(kkt_pc_stage_times *out);
    virtual void debug_read(unsigned long long *, int) {}
    // kkt_debug_pc_forms: KKT_PC_FORM_INTS values per row step or sweep program, replay order
    virtual void plain_forms(std::vector<int32_t> &) const {}
    // kkt_debug_mass_tile_values (include/kkt.h)
    virtual void mass_tile_debug(int64_t *, int64_t *, double *, int32_t *, double *) {
        fail(KKT_ERR_STATE, "kkt_debug_mass_tile_values: no mass solves on tiles on this handle");
    }
    // kkt_debug_pc_solves / kkt_debug_pc_matrices: KKT_PC_SOLVE_VALS values per sub-solve,
    // KKT_PC_MATRIX_VALS per distinct sub-solve matrix (include/kkt.h)
    virtual void solve_records(std::vector<double> &) const {}
    virtual void matrix_records(std::vector<double> &) const {}
    // kkt_debug_pc_alias: KKT_PC_ALIAS_INTS values per sub-solve (include/kkt.h)
    virtual void alias_records(std::vector<int32_t> &) const {}
    // kkt_debug_coarse_correction: the coarse space of the two-grid sub-solves, the Galerkin
    // launch constants of its set-up and the rows of P (false: built without a coarse space)
    virtual bool coarse_space(CoarseDev *, GalerkinDev *, int64_t *) const { return false; }
    // kkt_debug_tile_levels: one launch of the tile program's two-grid levels on host data
    virtual void debug_tile_levels(kkt_tile_levels *) {
        fail(KKT_ERR_STATE, "kkt_debug_tile_levels: no two-grid tile program on this handle");
    }
    // measurement: time the persistent programs of the next run() with events
    virtual void time_programs(float *ms, int *launches, int64_t *phases) {
        *ms = 0.f;
        *launches = 0;
        *phases = 0;
    }
};

class SchurPC : public PcBase {
   public:
    SchurPC(System &S, const kkt_pc_desc &d);
    // u = pc_fn(b) on the fixed internal vectors in_ / out_ (bc-corrected by the caller)
    void run() override;
    double *in() override { return in_; }
    double *out() override { return out_; }
    void values_changed() override;
    void check() override;   // throws if a persistent row program reported a time-out
    bool timed_out(std::string *why) override;
    bool fallback_plain() override;
    const unsigned *err_word() const override { return d_err_; }
    void time_stages(kkt_pc_stage_times *out) override;
    void debug_read(unsigned long long *out, int n) override;   // diagnostic builds (KKT_STAMPS)
    void plain_forms(std::vector<int32_t> &out) const override;
    void mass_tile_debug(int64_t *n_entries, int64_t *n_vals, double *copy, int32_t *gpos,
                         double *vals) override;
    void solve_records(std::vector<double> &out) const override;
    bool coarse_space(CoarseDev *c, GalerkinDev *g, int64_t *n) const override;
    void debug_tile_levels(kkt_tile_levels *run) override;
    void matrix_records(std::vector<double> &out) const override;
    void alias_records(std::vector<int32_t> &out) const override;
    void time_programs(float *ms, int *launches, int64_t *phases) override;
    int bc_set() const { return bc_set_; }
    // degree and interval the sub-solves of a typical time level run with (given or derived)
    int schur_its() const { return schur_its_; }
    int coarse_cycles() const { return coarse_cycles_; }
    double typical_emin() const { return typical_emin_; }
    double typical_emax() const { return typical_emax_; }
    int64_t n_launches() const { return (int64_t)steps_.size(); }

   private:
    System &S_;
    kkt_pc_desc d_;
    // Lifetimes go by declaration order (members are destroyed in reverse): the side stream, then
    // the events, then the device memory, and segments_' graphs after all of them, so that the
    // graphs go first and what their nodes name -- buffers, events, the stream -- goes after.
    // Side lane: work that does not depend on the sweep in flight (the mass solves and the
    // right-hand-side products of later time levels) runs on a second stream while the
    // latency-bound sweep program occupies a quarter of the wave slots.
    Stream side_;                 // made by the first replay() of a program with events
    std::vector<Event> events_;
    // Device memory by lifetime: the handle's; the current values' (mats_ and the coarse
    // inverses: values_changed() releases it); the current program's (steps_, tile tables, the
    // interleaved iterates: clear_program() releases it).
    DevPool handle_mem_, values_mem_, program_mem_;
    std::vector<int32_t> m_indptr_, m_indices_, bc_idx_;
    std::vector<double> m_values_;
    int n_ = 1;                // blocks per variable (global)
    int lo_ = 0, hi_ = 1;      // owned block range
    int64_t nx_ = 0;
    int bc_set_ = -1;
    const uint8_t *mask_ = nullptr;
    int m_pat_ = -1;
    double *m_vals_ = nullptr;           // bc-assembled M (cols masked)
    double *m_dinv_ = nullptr;
    double *in_ = nullptr, *out_ = nullptr;
    double *B_ = nullptr, *T_ = nullptr;             // n_ blocks each
    double *P_[3] = {nullptr, nullptr, nullptr};     // Chebyshev rotation, n_ blocks each
    struct Mat {
        double *vals;
        double *dinv;
        double emin = 0.0, emax = 0.0;   // Chebyshev interval of this matrix (given or estimated)
        double eimag = 0.0;              // > 0: imaginary semi-axis of the spectrum's ellipse
        double *einv = nullptr;          // two-grid form: (P^T A P)^-1, nc x nc row-major (shared
                                         // by matrices with equal values)
        int index = -1;                  // position in mat_recs_ (creation order)
        int est = KKT_PC_EST_NONE;       // KKT_PC_EST_*: where emin / emax come from
    };
    // what kkt_debug_pc_matrices reports per matrix, and one record per sub-solve emitted
    struct MatRec {
        double c = 0.0;
        int est = KKT_PC_EST_NONE, lanczos = 0, power = 0, solves = 0;
        bool coarse = false;
    };
    std::vector<MatRec> mat_recs_;
    std::vector<double> solve_recs_;
    std::vector<const double *> alias_recs_;   // per sub-solve: matrix, diagonal, first update term
    void note_solve(int sweep, int level, const Mat &m, const double *upd_vals = nullptr);
    int schur_its_ = 0;                  // degree of the sub-solves (given or derived)
    double typical_emin_ = 0.0, typical_emax_ = 0.0;
    int resolve_its(const Mat &typical);
    int64_t spectrum_steps_ = 0;         // Lanczos steps spent on estimates (reported when verbose)
    // two-grid form of the sub-solves (kkt_pc_desc.coarse_*)
    int coarse_cycles_ = 0;
    std::vector<int32_t> p_indptr_, p_indices_;
    std::vector<double> p_values_;
    std::vector<int32_t> pt_indptr_, pt_indices_;      // P^T (host copies: tile plan)
    std::vector<double> pt_values_;
    CoarseDev coarse_;
    std::vector<const double *> einvs_;   // every coarse inverse of the current values
    double *R_ = nullptr;                // residual of a cycle (one block)
    void build_coarse();
    GalerkinDev galerkin_{};                          // structure of P^T A P on the device
    // (P^T A P)^-1 on the device: allocated here, formed for all matrices of a build at once by
    // flush_coarse (the pointer is recorded by the steps emitted before that)
    double *coarse_inverse(const double *vals);
    std::vector<std::pair<const double *, double *>> pending_coarse_;
    void flush_coarse();
    void emit_coarse(const double *r, const double *x_in, double *x_out, const double *einv);
    std::map<std::pair<const double *, uint64_t>, Mat> mats_;
    double *h_u0_ = nullptr, *h_u1_ = nullptr, *h_t_ = nullptr;   // one-block halos
    std::vector<PcStep> steps_;
    struct Segment : GraphExec {
        size_t first = 0, last = 0;
        bool comm = false;
    };
    std::vector<Segment> segments_;
    bool use_graph_ = true;
    bool use_lanes_ = false;      // side lane (side_, events_)
    int cur_lane_ = 0;
    int n_events_ = 0;
    int emit_record(int lane);          // returns the event index
    void emit_wait(int lane, int ev);
    // the arguments of the op builders (rowlaunch.hpp)
    using Term = RowTerm;
    using Lin = LinStep;
    using Cheb = ChebStep;
    void build();
    void clear_program();
    const double *block_vals(int q, int i, int j) const;
    // `solved`: false for matrices only multiplied with (CN: c M~ and the upper blocks): no
    // interval, no coarse inverse (formed later if the same matrix is solved with after all)
    Mat schur_matrix(const double *base_vals, double c, bool solved = true);
    // Collection pass of a build (option "spectrum_batch" >= 1): the matrices the build will
    // solve with, in the order of its schur_matrix calls, formed at once; their twins found with
    // one fingerprint launch and one comparison launch; the distinct ones estimated in lock-step
    // batches.  schur_matrix then takes values, twin and interval from here -- and still forms,
    // compares and estimates by itself whatever the pass did not cover (counted as a fall-back).
    using MatKey = std::pair<const double *, uint64_t>;
    struct Pre {
        double *vals = nullptr, *dinv = nullptr;
        int cls = -1;                    // index into pre_cls_: equal values, equal shift (-1: not compared)
    };
    struct PreCls {
        bool estimated = false;
        Spectrum sp{0.0, 0.0, 0};
        bool nonsym = false;
        double radius = 0.0;
        int power = 0;
    };
    std::map<MatKey, Pre> pre_;
    std::vector<PreCls> pre_cls_;
    // Option "pc_alias": the twins the pass proves are read from one array.  A formed twin takes its
    // class representative's vals / dinv (its own are not kept); the stored blocks the program
    // multiplies with join the same search under a tag of their own, and shared_block() names the
    // representative of a block's class -- an array of the system's, as the block itself.
    // Matrices the pass does not cover (those only multiplied with) are formed once per (class of
    // the base block, shift): form_matrix is a function of the bits of its inputs.
    std::map<const double *, const double *> block_rep_;
    std::map<MatKey, std::pair<double *, double *>> formed_;
    const double *shared_block(const double *vals) const;
    std::vector<const double *> multiplied_blocks() const;
    // the array a product with block (i, j) of quadrant q reads
    const double *mult_vals(int q, int i, int j) const { return shared_block(block_vals(q, i, j)); }
    void form_matrix(const double *base_vals, double c, double *vals, double *dinv);
    std::vector<std::pair<const double *, double>> solved_matrices() const;
    void collect_matrices();
    void emit_lin(const std::vector<Lin> &ops);
    void emit_cheb(const std::vector<Cheb> &ops);
    double *il_P_[3] = {nullptr, nullptr, nullptr};
    size_t il_cap_ = 0;
    void emit_time(double *y, const double *x, int kind, int n, const double *lo_halo = nullptr,
                   const double *hi_halo = nullptr);
    void emit_comm(const double *send, int dst, double *recv, int src);
    // its-step Jacobi-Chebyshev solves of `count` independent systems in lock step
    struct Solve {
        const double *vals, *dinv, *b;
        double *out;
        double post1 = 1.0, post2 = 1.0;
    };
    // The levels of the sweeps as the emit functions record them.  A level's steps carry its index
    // (PcStep::level): they are the maximal stretch of consecutive steps with that tag.
    struct SweepLevel {
        TileLevel lev{};
        std::vector<TileCoef> coef;     // steps 2 .. its
        int its = 0;
        bool eligible = false;
        const double *b_after = nullptr;   // the right-hand side after the update (B_i)
        bool coarse = false;               // two-grid level: coef holds sweeps 1 .. its
        const double *einv = nullptr;      // its (P^T A P)^-1
    };
    std::vector<SweepLevel> sweep_levels_;
    int cur_level_ = -1;                // the level being emitted: push_rows / emit_coarse stamp it
    size_t level_first_ = 0;
    void begin_level();
    void end_level(SweepLevel lv);      // fails unless exactly the steps since begin_level() carry the tag
    // what the tile form runs as the level "[update;] solve" (ok: it can express the update)
    struct LevelForm {
        TileLevel lev{};
        const double *b_after = nullptr;
        bool ok = true;
    };
    static LevelForm level_form(const Lin *upd, const Solve &sv, double p1_scale);
    // batched solves on one matrix with the iterates of four levels interleaved (kernels.hpp IlOp);
    // the ROWS_IL steps of a solve carry its index (PcStep::solve)
    struct MassSolve {
        int its = 0;
        std::vector<Solve> sv;
        std::vector<TileCoef> coef;     // steps 1 .. its
    };
    std::vector<MassSolve> mass_solves_;
    bool emit_solves_interleaved(const std::vector<Solve> &sv, int its, double emin, double emax);
    void emit_solves(const std::vector<Solve> &sv, int its, double emin, double emax,
                     double *const P[3], int64_t pstride, bool first_done = false,
                     std::vector<TileCoef> *coef_out = nullptr, double eimag = 0.0,
                     const Mat *mat = nullptr);
    // the sweep step "b -= A u_prev (masked), then solve": the update and the first
    // Chebyshev step share one launch
    void emit_update_and_solve(Lin upd, const Solve &sv, int its, double emin, double emax,
                               double eimag = 0.0, const Mat *mat = nullptr);
    void emit_coarse_solve(const Lin *upd, const Solve &sv, const Mat &F);
    // position of the transposed entry of every stored entry of the preconditioner's sparsity
    // structure (device array, built on first use; null when the structure is not symmetric)
    const int32_t *transpose_positions();
    int32_t *d_tpos_ = nullptr;
    bool tpos_tried_ = false;
    void push_rows(std::vector<RowOp> &r);
    void build_stationary();
    void build_BE();
    void build_CN();
    void replay(size_t first, size_t last);

    // ---- lowering (pc_lower.cpp): runs of steps_ become tile launches, batched mass-tile launches
    // or row programs
    bool use_programs_ = true;
    void fuse_programs();
    // the row programs' tables (kernels.hip, pc_row_program)
    int prog_wpw_ = 0, prog_nwg_ = 0;
    int32_t *d_dep_ = nullptr;
    unsigned *d_flags_ = nullptr, *d_err_ = nullptr;
    bool prog_granule_ = false;
    bool prog_lowreg_ = false;   // counter form at three waves per SIMD (> 2 048 slices)
    int prog_mode_ = 0;   // 0 counter form, 1 pc_row_program_g, 2 pc_row_program_gw
    unsigned long long *d_g0_ = nullptr, *d_g1_ = nullptr;
    size_t granule_words_ = 0;
    bool setup_row_programs();
    bool legacy_tried_ = false, legacy_ok_ = false;
    // the tile plan of the sweeps (tile_kernels.hip), its coarse tables (kernels.hpp,
    // TileCoarseDev) and the cursors of one application's hand-off tags
    TilePlan tile_plan_;
    bool tile_tried_ = false, tile_ok_ = false;
    size_t tile_lds_checked_ = 0;       // dynamic LDS bytes residency was checked for
    TileCoarseDev h_tile_coarse_{};     // host copy (device pointers inside)
    TileCoarseDev *d_tile_coarse_ = nullptr;
    bool tile_coarse_ok_ = false;
    bool tile_coarse_rings_built_ = false;   // the lists hold the ring rows' entries
    std::vector<int32_t> tile_e_lo_, tile_e_hi_;   // host copies of TileCoarseDev::e_lo / e_hi
    unsigned long long *d_tg_[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t tile_epoch_cursor_ = 0;    // hand-off tags handed out to the launches of one application
    uint32_t tile_cepoch_cursor_ = 0;
    bool tile_cleared_ = false;
    bool tile_coarse_cleared_ = false;  // (the first tile launch of an application may have no coarse levels)
    bool prepare_tiles();
    bool build_tile_coarse();
    // the plan holds `need` bytes of dynamic LDS per tile on the chip at once (and notes the bytes)
    bool tile_resident(size_t need, bool coarse);
    bool fuse_tile_run(size_t k, size_t e, std::vector<PcStep> &out);
    // what a TILE step launches, options as they are now (replay() and debug_tile_levels)
    TileArgs tile_args(const PcStep &s) const;
    // the mass-tile plan (mass_tile_kernels.hip) and its buffers: the runs of ROWS_IL steps of a
    // batched solve are replaced by ceil(its / K) TILE_CHEB steps on a tile plan of the form's own
    // (depth K)
    struct MassLaunch {
        MassTileArgs a;
        int grid_y = 1;
    };
    std::vector<MassLaunch> mass_launches_;
    TilePlan mass_plan_;
    bool mass_tried_ = false, mass_ok_ = false;
    int mass_per_cu_ = 0, mass_cus_ = 0;
    int32_t *d_masked_ = nullptr;
    double *mt_P_[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t mt_cap_ = 0;
    // a value array in the layout of the plan's lcol (launch_mass_tile_gather), one copy per array:
    // that of m_vals_ lives as long as the handle, as m_vals_ does; any other goes with the program
    struct MassTileValues {
        const double *vals;
        double *copy;
    };
    std::vector<MassTileValues> mass_vals_;
    const double *mass_tile_values(const double *vals);
    bool prepare_mass_tiles();
    void fuse_mass_tiles();
};

// Preconditioner of the incompressible (Stokes / Navier-Stokes) control systems:
// the pc_fn closures of Stationary.incompressible_linear_solve (reference
// control/control.py:986-1085) and Instationary.incompressible_linear_solve, BE branch
// (control.py:4515-4687).  u_0 = `inner_its` GMRES iterations on the velocity KKT system
// (a second handle with its own block-Schur preconditioner); then per pressure block
// h = s2 (sB B u_0 - b_1), m = K_p^-1 h (Jacobi-Chebyshev in place of one BoomerAMG cycle),
// g = C m with C the pressure-space commutator block system (a third handle), and
// u_1 = M_p^-1 g (20 Jacobi-Chebyshev steps, control.py:957-971).
class StokesPC : public PcBase {
   public:
    StokesPC(System &outer, System &inner, System &commutator, const kkt_pc_stokes_desc &d);
    void run() override;
    double *in() override { return in_; }
    double *out() override { return out_; }
    void check() override;
    bool timed_out(std::string *why) override { return inner_.pc && inner_.pc->timed_out(why); }
    void solve_records(std::vector<double> &out) const override;
    bool coarse_space(CoarseDev *c, GalerkinDev *g, int64_t *n) const override;
    bool fallback_plain() override { return inner_.pc && inner_.pc->fallback_plain(); }
    const unsigned *err_word() const override { return inner_.pc ? inner_.pc->err_word() : nullptr; }

   private:
    System &S_, &inner_, &comm_;
    int n_ = 1;   // pressure blocks per variable
    bool cn_ = false;
    int64_t nv_ = 0, np_ = 0;
    double sB_ = 1.0, s2_ = 1.0;
    int kp_its_ = 0, mp_its_ = 0;
    double kp_emin_ = 0, kp_emax_ = 0, mp_emin_ = 0, mp_emax_ = 0;
    int kp_est_ = KKT_PC_EST_GIVEN;    // where kp_emin_ / kp_emax_ come from (KKT_PC_EST_*)
    struct DevMat {
        int pat = -1;
        double *vals = nullptr, *dinv = nullptr;
    } B_, Kp_, Mp_;
    double *in_ = nullptr, *out_ = nullptr, *h_ = nullptr, *m_ = nullptr, *g_ = nullptr;
    double *P_[3] = {nullptr, nullptr, nullptr};
    double *halo_a_ = nullptr, *halo_b_ = nullptr;   // CN on time shards: neighbour blocks of the T scans
    // Lifetimes go by declaration order (members are destroyed in reverse): the device memory
    // before the chains, so that their graphs go first and the buffers their nodes name after.
    DevPool mem_;
    // a step of a pressure-space chain: a batched row launch, or -- two-grid K_p solve -- the
    // Galerkin correction x_out = x_in + P E^-1 P^T r of every block
    struct ChainStep {
        RowLaunch L;
        bool coarse = false;
        const double *r = nullptr, *x_in = nullptr;
        double *x_out = nullptr;
    };
    std::vector<RowLaunch> lin_;
    std::vector<ChainStep> kp_steps_, mp_steps_;
    // the two Chebyshev chains (hundreds of small launches on fixed buffers) replayed as graphs
    struct Chain : GraphExec {
        bool usable = true;   // false once a capture failed: plain launches from then on
    } kp_chain_, mp_chain_;
    void run_chain(Chain &c, const std::vector<ChainStep> &steps);
    // two-grid K_p solve
    CoarseDev kp_coarse_;
    GalerkinDev kp_galerkin_{};
    double *kp_einv_ = nullptr, *kp_r_ = nullptr, *kp_x0_ = nullptr;
    int kp_cycles_ = 0;
    void build_kp_coarse(const kkt_pc_stokes_desc &d);
    void emit_kp_two_grid(int its, double emin, double emax, const double *b, double *out);
    DevMat upload(int64_t nrows, int64_t ncols, const int32_t *ip, const int32_t *ix,
                  const double *v, bool want_dinv);
    void emit_cheb(std::vector<ChainStep> &dst, const DevMat &A, int its, double emin, double emax,
                   const double *b, double *out);
};

}  // namespace kkt
