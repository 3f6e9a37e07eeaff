#include "pc.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace kkt {

SchurPC::SchurPC(System &S, const kkt_pc_desc &d) : S_(S), d_(d) {
    if (!S.finalized) fail(KKT_ERR_STATE, "kkt_set_pc_schur needs a finalized system");
    if (d.kind < KKT_PC_STATIONARY || d.kind > KKT_PC_INSTATIONARY_CN)
        fail(KKT_ERR_ARG, "unknown preconditioner kind");
    if (!d.m_indptr || !d.m_indices || !d.m_values) fail(KKT_ERR_ARG, "mass matrix missing");
    if (S.nx0 != S.nx1 || d.nx != S.nx0)
        fail(KKT_ERR_ARG, "built-in preconditioner needs equal spatial spaces of size nx");
    nx_ = d.nx;
    if (d.kind == KKT_PC_STATIONARY)
        n_ = 1;
    else
        n_ = d.kind == KKT_PC_INSTATIONARY_BE ? d.n_t : d.n_t - 1;
    if (n_ != S.n0 || n_ != S.n1 || n_ < 1)
        fail(KKT_ERR_ARG, "n_t does not match the block counts of the system");
    lo_ = S.sharded ? S.lo : 0;
    hi_ = S.sharded ? S.hi : n_;
    if (d.kind != KKT_PC_STATIONARY && n_ < 2) fail(KKT_ERR_ARG, "need at least two blocks");
    // schur_its == -1: degree from the spectrum; schur_emin <= 0: interval from the spectrum
    if (d.mass_its < 0 || d.schur_its < -1) fail(KKT_ERR_ARG, "negative Chebyshev degree");
    if ((d.mass_its > 0 && !(d.mass_emax > d.mass_emin && d.mass_emin > 0)) ||
        (d.schur_emin > 0 && !(d.schur_emax > d.schur_emin)) || d.schur_eimag < 0)
        fail(KKT_ERR_ARG, "Chebyshev bounds must satisfy 0 < emin < emax, eimag >= 0");
    // deep copies: the caller's arrays are not kept (kkt.h conventions)
    m_indptr_.assign(d.m_indptr, d.m_indptr + nx_ + 1);
    m_indices_.assign(d.m_indices, d.m_indices + m_indptr_[nx_]);
    m_values_.assign(d.m_values, d.m_values + m_indptr_[nx_]);
    if (d.n_bc > 0) bc_idx_.assign(d.bc_idx, d.bc_idx + d.n_bc);
    if (d.coarse_cycles < 0) fail(KKT_ERR_ARG, "negative number of coarse cycles");
    if (d.coarse_cycles > 0) {
        if (!d.p_indptr || !d.p_indices || !d.p_values || d.n_coarse < 1)
            fail(KKT_ERR_ARG, "coarse_cycles > 0 needs the prolongation matrix P");
        if (d.n_coarse > 4096) fail(KKT_ERR_ARG, "coarse space too large (dense inverse): n_coarse <= 4096");
        coarse_cycles_ = d.coarse_cycles;
        p_indptr_.assign(d.p_indptr, d.p_indptr + nx_ + 1);
        const int64_t pn = p_indptr_[nx_];
        if (p_indptr_[0] != 0 || pn < 0) fail(KKT_ERR_ARG, "bad P indptr");
        p_indices_.assign(d.p_indices, d.p_indices + pn);
        p_values_.assign(d.p_values, d.p_values + pn);
        for (int64_t r = 0; r < nx_; ++r)
            if (p_indptr_[r + 1] < p_indptr_[r]) fail(KKT_ERR_ARG, "P indptr not monotone");
        for (int32_t c : p_indices_)
            if (c < 0 || c >= d.n_coarse) fail(KKT_ERR_ARG, "P column index out of range");
    }
    d_.p_indptr = d_.p_indices = nullptr;
    d_.p_values = nullptr;
    d_.m_indptr = d_.m_indices = nullptr;
    d_.m_values = nullptr;
    d_.bc_idx = nullptr;
    use_graph_ = !S_.opts.no_graph;
    use_programs_ = S_.opts.persistent;
    // opt-in: measured 0-3 % on cfg 2 (both lanes slow down when they share the chip, and the
    // smaller batches of a chunk are less efficient), DESIGN.md section 6
    use_lanes_ = S_.opts.lanes;
    build();
}

void SchurPC::clear_program() {
    segments_.clear();   // the graphs first: their nodes point into the program's memory
    program_mem_.release();
    il_cap_ = 0;
    mt_cap_ = 0;
    // (the copies of arrays other than m_vals_ were the program's memory)
    mass_vals_.erase(std::remove_if(mass_vals_.begin(), mass_vals_.end(),
                                    [&](const MassTileValues &c) { return c.vals != m_vals_; }),
                     mass_vals_.end());
    mass_solves_.clear();
    mass_launches_.clear();
    sweep_levels_.clear();
    steps_.clear();
    n_events_ = 0;
    cur_lane_ = 0;
    cur_level_ = -1;
}

int SchurPC::emit_record(int lane) {
    PcStep s;
    s.kind = PcStep::EV_RECORD;
    s.lane = lane;
    s.ev = n_events_++;
    steps_.push_back(s);
    return s.ev;
}

void SchurPC::emit_wait(int lane, int ev) {
    PcStep s;
    s.kind = PcStep::EV_WAIT;
    s.lane = lane;
    s.ev = ev;
    steps_.push_back(s);
}

void SchurPC::values_changed() {
    // Schur matrices are sums with block values: rebuild them and the program
    clear_program();
    values_mem_.release();
    mats_.clear();
    mat_recs_.clear();
    solve_recs_.clear();
    alias_recs_.clear();
    einvs_.clear();
    pending_coarse_.clear();
    S_.spectrum_stats = kkt_spectrum_stats{};
    collect_matrices();
    if (d_.kind == KKT_PC_STATIONARY)
        build_stationary();
    else if (d_.kind == KKT_PC_INSTATIONARY_BE)
        build_BE();
    else
        build_CN();
    pre_.clear();
    pre_cls_.clear();
    flush_coarse();
    if (S_.opts.verbose && d_.schur_emin <= 0) {
        std::fprintf(stderr, "[kkt] Chebyshev sub-solves: degree %d; %lld Lanczos steps spent on "
                     "%zu matrices\n", schur_its_, (long long)spectrum_steps_, mats_.size());
        const kkt_spectrum_stats &t = S_.spectrum_stats;
        std::fprintf(stderr, "[kkt] spectrum estimates: %lld matrices in %lld batches (at most %lld "
                     "bytes each), %lld launches, %lld synchronisations, %lld fall-backs, %.1f ms\n",
                     (long long)t.matrices, (long long)t.batches, (long long)t.batch_bytes,
                     (long long)t.launches, (long long)t.syncs, (long long)t.fallbacks, t.ms);
    }
    S_.info.sweep_form = 0;
    S_.info.sweep_coarse_rings = 0;
    S_.info.sweep_coarse_cache = S_.info.sweep_coarse_ew = 0;
    S_.info.sweep_tiles = S_.info.sweep_threads = S_.info.sweep_depth = S_.info.sweep_row_slots = 0;
    S_.info.sweep_its = schur_its_;
    fuse_programs();
}

void SchurPC::mass_tile_debug(int64_t *n_entries, int64_t *n_vals, double *copy, int32_t *gpos,
                              double *vals) {
    const double *d_copy = nullptr;
    for (const MassTileValues &c : mass_vals_)
        if (c.vals == m_vals_) d_copy = c.copy;
    if (!mass_ok_ || !d_copy)
        fail(KKT_ERR_STATE, "kkt_debug_mass_tile_values: no mass solves on tiles on this handle");
    const size_t n = mass_plan_.gpos.size(), nv = (size_t)S_.patterns[m_pat_].npadded;
    if (n_entries) *n_entries = (int64_t)n;
    if (n_vals) *n_vals = (int64_t)nv;
    HIPCHK(hipStreamSynchronize(S_.stream));
    if (copy) HIPCHK(hipMemcpy(copy, d_copy, n * sizeof(double), hipMemcpyDeviceToHost));
    if (gpos) HIPCHK(hipMemcpy(gpos, mass_plan_.d_gpos, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vals) HIPCHK(hipMemcpy(vals, m_vals_, nv * sizeof(double), hipMemcpyDeviceToHost));
}

void SchurPC::debug_read(unsigned long long *out, int n) {
    if (!d_err_) return;
    HIPCHK(hipStreamSynchronize(S_.stream));
    HIPCHK(hipMemcpy(out, d_err_ + 64, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(d_err_ + 64, 0, (size_t)n * 8));
}

// One application as plain launches with an event pair around every persistent program.
void SchurPC::time_programs(float *ms, int *launches, int64_t *phases) {
    hipStream_t st = S_.stream;
    *ms = 0.f;
    *launches = 0;
    *phases = 0;
    std::vector<std::pair<Event, Event>> evs;
    size_t k = 0;
    while (k < steps_.size()) {
        if (steps_[k].kind == PcStep::PROG || steps_[k].kind == PcStep::TILE) {
            evs.emplace_back(Event::create(true), Event::create(true));
            HIPCHK(hipEventRecord(evs.back().first, st));
            replay(k, k + 1);
            HIPCHK(hipEventRecord(evs.back().second, st));
            *launches += 1;
            *phases += steps_[k].nphases;
        } else {
            replay(k, k + 1);
        }
        ++k;
    }
    HIPCHK(hipStreamSynchronize(st));
    for (auto &e : evs) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e.first, e.second));
        *ms += t;
    }
}

void PcBase::time_stages(kkt_pc_stage_times *out) {
    // no itemisation: the whole application between two events
    *out = kkt_pc_stage_times{};
    fail(KKT_ERR_STATE, "kkt_time_pc_stages needs the built-in block-Schur preconditioner");
}

// One application step by step, an event after every step; a step's time goes to the sweeps
// (persistent programs, or the single-block steps they replace), to the hand-offs between ranks,
// or to the batched steps over all time levels.
void SchurPC::time_stages(kkt_pc_stage_times *out) {
    hipStream_t st = S_.stream;
    *out = kkt_pc_stage_times{};
    std::vector<Event> ev(steps_.size() + 1);
    for (Event &e : ev) e = Event::create(true);
    HIPCHK(hipEventRecord(ev[0], st));
    for (size_t k = 0; k < steps_.size(); ++k) {
        replay(k, k + 1);
        // (side-lane steps are rare -- option "lanes" -- and are charged to the step that waits)
        HIPCHK(hipEventRecord(ev[k + 1], st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < steps_.size(); ++k) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        const PcStep &s = steps_[k];
        out->total_ms += ms;
        if (s.kind == PcStep::PROG || s.kind == PcStep::TILE) {
            out->sweeps_ms += ms;
            out->sweep_launches += 1;
            out->sweep_phases += s.nphases;
        } else if (s.kind == PcStep::ROWS && s.rows.nops == 1 && n_ > 1) {
            out->sweeps_ms += ms;          // a sweep step as a plain launch
            out->sweep_launches += 1;
            out->sweep_phases += 1;
        } else if (s.kind == PcStep::COMM) {
            out->comm_ms += ms;
            out->comm_steps += 1;
        } else {
            out->batched_ms += ms;
            if (s.kind == PcStep::ROWS || s.kind == PcStep::TIME || s.kind == PcStep::ROWS_IL ||
                s.kind == PcStep::TILE_CHEB)
                out->batched_launches += 1;
        }
    }
}

bool SchurPC::timed_out(std::string *why) {
    if (!d_err_) return false;
    unsigned e = 0;
    HIPCHK(hipMemcpyAsync(&e, d_err_, sizeof e, hipMemcpyDeviceToHost, S_.stream));
    HIPCHK(hipStreamSynchronize(S_.stream));
    if (!e) return false;
    unsigned rec[40] = {0};
    HIPCHK(hipMemcpy(rec, d_err_, sizeof rec, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(d_err_, 0, sizeof rec));
    std::string msg = "persistent sweep kernel timed out waiting for a neighbour workgroup";
    if (e & 4u)
        msg += " (tile form: tile " + std::to_string(rec[8]) + ", hand-off " +
               std::to_string(rec[9]) + ", local row " + std::to_string(rec[10]) +
               ", global row " + std::to_string(rec[11]) + ", tags seen new " +
               std::to_string(rec[12]) + "/" + std::to_string(rec[13]) + " old " +
               std::to_string(rec[14]) + "/" + std::to_string(rec[15]) +
               (rec[16] ? ", both iterates)" : ", newest iterate only)");
    if (e & 8u)
        msg = "persistent sweep kernel abandoned at entry: its workgroups are not co-resident (" +
              std::to_string(rec[17]) + " of " + std::to_string(rec[18]) +
              " tiles checked in within the bounded wait; tile form)";
    if (e & 2u)
        msg += " (data-flow form: workgroup " + std::to_string(rec[24]) + " wave " +
               std::to_string(rec[25]) + " lane " + std::to_string(rec[26]) + ", phase " +
               std::to_string(rec[27]) + ", expected tag " + std::to_string(rec[28]) +
               ", seen " + std::to_string(rec[29]) + "/" + std::to_string(rec[30]) +
               " at column " + std::to_string(rec[31]) + " of slice " + std::to_string(rec[32]) + ")";
    if (e & 1u) msg += " (counter form)";
    if (why) *why = msg;
    return true;
}

void SchurPC::check() {
    std::string why;
    if (timed_out(&why)) fail(KKT_ERR_HIP, why);
}

// The same steps as plain launches (bit-identical arithmetic, tests/test_gpu_parity.py).
bool SchurPC::fallback_plain() {
    if (!use_programs_) return false;
    use_programs_ = false;
    values_changed();
    return true;
}

const double *SchurPC::block_vals(int q, int i, int j) const {
    auto it = S_.blocks.find(std::make_tuple(q, i, j));
    if (it == S_.blocks.end())
        fail(KKT_ERR_STATE, "preconditioner needs block (" + std::to_string(q) + "," +
                                std::to_string(i) + "," + std::to_string(j) + ")");
    const ValueArray &va = S_.values[it->second.va];
    if (va.pattern != m_pat_)
        fail(KKT_ERR_STATE, "preconditioner blocks must share the mass matrix's sparsity");
    return va.d_vals;
}

void SchurPC::build() {
    hipStream_t st = S_.stream;
    bc_set_ = bc_idx_.empty() ? -1 : S_.add_bc_set(nx_, (int64_t)bc_idx_.size(), bc_idx_.data());
    mask_ = bc_set_ >= 0 ? S_.bc_sets[bc_set_].d_mask : nullptr;
    m_pat_ = S_.find_or_add_pattern(nx_, nx_, m_indptr_.data(), m_indices_.data());
    const Pattern &P = S_.patterns[m_pat_];
    {
        auto d_csr = DevBuf<double>::upload(m_values_.data(), m_values_.size());
        m_vals_ = handle_mem_.alloc<double>(P.npadded);
        launch_csr_to_sell(st, d_csr.get(), P.d_sell2csr, m_vals_, P.npadded);
        if (mask_) launch_mask_columns(st, m_vals_, P.d_col, mask_, P.npadded);
        HIPCHK(hipStreamSynchronize(st));
    }
    m_dinv_ = handle_mem_.alloc<double>(nx_);
    launch_extract_dinv(st, P.d_col, P.d_slice_off, m_vals_, mask_, m_dinv_, (int)nx_, P.nslices,
                        P.R, P.d_perm);
    auto vec = [&](int64_t blocks) {
        double *p = handle_mem_.alloc<double>(blocks * nx_ + 32);
        HIPCHK(hipMemsetAsync(p, 0, (blocks * nx_ + 32) * sizeof(double), st));
        return p;
    };
    const int nl = hi_ - lo_;
    in_ = vec(2 * nl);
    out_ = vec(2 * nl);
    B_ = vec(nl);
    T_ = vec(nl);
    for (int k = 0; k < 3; ++k) P_[k] = vec(nl);
    h_u0_ = vec(1);
    h_u1_ = vec(1);
    h_t_ = vec(1);
    if (coarse_cycles_ > 0) {
        R_ = vec(1);
        build_coarse();
    }
    values_changed();
}

// tpos[position of (r, c)] = position of (c, r) in the SELL value arrays of the preconditioner's
// structure; null when some entry has no transposed partner (not a finite-element structure)
const int32_t *SchurPC::transpose_positions() {
    if (tpos_tried_) return d_tpos_;
    tpos_tried_ = true;
    const Pattern &P = S_.patterns[m_pat_];
    if (P.nrows != P.ncols) return nullptr;
    std::vector<int32_t> t((size_t)P.npadded, -1);
    for (int64_t r = 0; r < P.nrows; ++r)
        for (int32_t q = P.h_indptr[r]; q < P.h_indptr[r + 1]; ++q) {
            const int32_t c = P.h_indices[q];
            const int32_t *b = P.h_indices.data() + P.h_indptr[c];
            const int32_t *e = P.h_indices.data() + P.h_indptr[c + 1];
            const int32_t *hit = std::lower_bound(b, e, (int32_t)r);
            if (hit == e || *hit != (int32_t)r) return nullptr;
            t[(size_t)P.sell_index(r, q - P.h_indptr[r])] =
                (int32_t)P.sell_index(c, (int)(hit - b));
        }
    d_tpos_ = handle_mem_.upload(t.data(), t.size());   // built once per handle (tpos_tried_)
    return d_tpos_;
}

// ---- two-grid form of the sub-solves: coarse space on the device, Galerkin inverses
void SchurPC::build_coarse() {
    const int nc = (int)d_.n_coarse;
    // P^T by a counting sort over the columns (entries of a column in ascending row order: the
    // restriction sums them in that order)
    pt_indptr_.assign(nc + 1, 0);
    for (int32_t c : p_indices_) pt_indptr_[c + 1]++;
    for (int j = 0; j < nc; ++j) pt_indptr_[j + 1] += pt_indptr_[j];
    pt_indices_.resize(p_indices_.size());
    pt_values_.resize(p_indices_.size());
    std::vector<int32_t> cur(pt_indptr_.begin(), pt_indptr_.end() - 1);
    for (int64_t r = 0; r < nx_; ++r)
        for (int32_t q = p_indptr_[r]; q < p_indptr_[r + 1]; ++q) {
            const int32_t at = cur[p_indices_[q]]++;
            pt_indices_[at] = (int32_t)r;
            pt_values_[at] = p_values_[q];
        }
    auto up = [&](const auto &v) { return handle_mem_.upload(v.data(), v.size()); };
    coarse_.nc = nc;
    coarse_.p_ip = up(p_indptr_);
    coarse_.p_ix = up(p_indices_);
    coarse_.p_v = up(p_values_);
    coarse_.pt_ip = up(pt_indptr_);
    coarse_.pt_ix = up(pt_indices_);
    coarse_.pt_v = up(pt_values_);
    {
        const Pattern &P = S_.patterns[m_pat_];
        std::vector<int32_t> e_ip, e_ix;
        galerkin_structure(nc, pt_indptr_, pt_indices_, P.h_indptr, P.h_indices, p_indptr_,
                           p_indices_, e_ip, e_ix);
        galerkin_.e_ip = up(e_ip);
        galerkin_.e_ix = up(e_ix);
        galerkin_.col = P.d_col;
        galerkin_.slice_off = P.d_slice_off;
        galerkin_.pos = P.h_pos_of.empty() ? nullptr : up(P.h_pos_of);
        galerkin_.mask = mask_;
        galerkin_.R = P.R;
        galerkin_.uniform_w = P.uniform_w;
        galerkin_.block_n = coarse_block_size(nc, e_ip, e_ix);
    }
    coarse_.rc = handle_mem_.alloc<double>(nc);
    coarse_.ec = handle_mem_.alloc<double>(nc);
}

double *SchurPC::coarse_inverse(const double *vals) {
    const int nc = coarse_.nc;
    double *d_inv = values_mem_.alloc<double>((size_t)nc * nc);
    einvs_.push_back(d_inv);
    pending_coarse_.emplace_back(vals, d_inv);
    return d_inv;
}

// every coarse inverse of this build in one batch (before the programs are fused: the tile plan
// reads the inverses)
void SchurPC::flush_coarse() {
    if (pending_coarse_.empty()) return;
    std::vector<const double *> vals;
    std::vector<double *> inv;
    for (auto &pr : pending_coarse_) {
        vals.push_back(pr.first);
        inv.push_back(pr.second);
    }
    pending_coarse_.clear();
    coarse_setup(S_, m_pat_, coarse_, galerkin_, vals, inv, false, "Schur sub-solves");
}

void SchurPC::emit_coarse(const double *r, const double *x_in, double *x_out, const double *einv) {
    PcStep s;
    s.kind = PcStep::COARSE;
    s.cr = r;
    s.x = x_in;
    s.y = x_out;
    s.einv = einv;
    s.nx = nx_;
    s.lane = cur_lane_;
    s.level = cur_level_;
    steps_.push_back(s);
}

// The steps emitted between begin_level() and end_level() are one sweep level: push_rows and
// emit_coarse stamp them with its index.
void SchurPC::begin_level() {
    cur_level_ = (int)sweep_levels_.size();
    level_first_ = steps_.size();
}

// A level's steps are one stretch by construction (also with option "lanes": the side lane's
// steps are emitted between the levels): a step without the tag inside it fails the build.
void SchurPC::end_level(SweepLevel lv) {
    for (size_t i = level_first_; i < steps_.size(); ++i)
        if (steps_[i].level != cur_level_)
            fail(KKT_ERR_STATE, "preconditioner program: the steps of a sweep level are not contiguous");
    sweep_levels_.push_back(std::move(lv));
    cur_level_ = -1;
}

// What the tile form runs as one level: the solve `sv`, after the update `upd` of its right-hand
// side if there is one.  The form can express b = ca * sum_t U_t x + cy * b_in with one x.
SchurPC::LevelForm SchurPC::level_form(const Lin *upd, const Solve &sv, double p1_scale) {
    LevelForm f;
    TileLevel &L = f.lev;
    L.vals = sv.vals;
    L.dinv = sv.dinv;
    L.out = sv.out;
    L.p1_scale = p1_scale;
    L.post1 = sv.post1;
    L.post2 = sv.post2;
    if (!upd) {
        L.bin = sv.b;
        L.bout = nullptr;
        L.n_upd = 0;
        return f;
    }
    f.ok = !upd->terms.empty() && upd->terms.size() <= 2 && upd->cz == 0.0 && !upd->z &&
           upd->yin != nullptr;
    for (const Term &t : upd->terms) f.ok = f.ok && t.x == upd->terms[0].x;
    if (!f.ok) return f;
    L.bin = upd->yin;
    // The plain steps update the right-hand side in place.  A tile re-computes the rows of
    // its rings from b_in, so an in-place store by the owner would race with its neighbours'
    // reads: the updated right-hand side stays on chip (nothing reads B_i after a sweep: the
    // next batched step overwrites it).
    L.bout = upd->y == upd->yin ? nullptr : upd->y;
    f.b_after = upd->y;
    L.x_prev = upd->terms[0].x;
    L.n_upd = (int32_t)upd->terms.size();
    for (size_t t = 0; t < upd->terms.size(); ++t) L.upd_vals[t] = upd->terms[t].vals;
    L.ca = upd->ca;
    L.cy = upd->cy;
    return f;
}

// One sub-solve in its two-grid form: [update of the right-hand side;] cycles x [Galerkin
// correction of the current iterate; `its` smoothing sweeps from it].
void SchurPC::emit_coarse_solve(const Lin *upd, const Solve &sv, const Mat &F) {
    const int its = std::max(1, schur_its_);
    SweepLevel lv;
    begin_level();
    if (upd) {
        Lin u = *upd;
        u.y2 = nullptr;
        emit_lin({u});
    }
    const ChebCoefficients cheb = cheb_coefficients(its, F.emin, F.emax, F.eimag);
    const double scale = cheb.scale;
    {
        // what the tile form runs as one two-grid level
        lv.its = its;
        lv.coarse = true;
        lv.einv = F.einv;
        lv.coef.push_back(TileCoef{0.0, 1.0, scale});
        lv.coef.insert(lv.coef.end(), cheb.steps.begin(), cheb.steps.end());
        const LevelForm f = level_form(upd, sv, scale);
        lv.lev = f.lev;
        lv.b_after = f.b_after;
        lv.eligible = f.ok;
    }
    double *p0 = P_[2];
    const double *xcur = nullptr;
    for (int c = 0; c < coarse_cycles_; ++c) {
        const bool last_cycle = c + 1 == coarse_cycles_;
        const double *r = sv.b;
        if (c > 0) {
            // r = b - F x
            emit_lin({Lin{{Term{F.vals, xcur}}, R_, -1.0, 0.0, 1.0, nullptr, sv.b}});
            r = R_;
        }
        emit_coarse(r, xcur, p0, F.einv);
        auto target = [&](int step) -> double * {
            return (last_cycle && step == its) ? sv.out : P_[(step - 1) % 3];
        };
        for (int step = 1; step <= its; ++step) {
            const bool last = last_cycle && step == its;
            const double *pk = step == 1 ? p0 : target(step - 1);
            const double *pkm1 = step == 1 ? nullptr : (step == 2 ? p0 : target(step - 2));
            const TileCoef k = step == 1 ? TileCoef{0.0, 1.0, scale} : cheb.step(step);
            emit_cheb({Cheb{F.vals, F.dinv, sv.b, pk, pkm1, target(step), k.c1, k.c2, k.c3,
                            last ? sv.post1 : 1.0, last ? sv.post2 : 1.0}});
        }
        xcur = target(its);
    }
    end_level(std::move(lv));
}

// the values of base + c * M~ and the Jacobi diagonal, into arrays of the current values' lifetime
void SchurPC::form_matrix(const double *base_vals, double c, double *vals, double *dinv) {
    const Pattern &P = S_.patterns[m_pat_];
    hipStream_t st = S_.stream;
    launch_vals_axpy(st, vals, base_vals, c, m_vals_, P.npadded);
    if (mask_) launch_mask_columns(st, vals, P.d_col, mask_, P.npadded);
    launch_extract_dinv(st, P.d_col, P.d_slice_off, vals, mask_, dinv, (int)nx_, P.nslices, P.R,
                        P.d_perm);
}

// (base, shift) of every matrix the build of this kind solves with on this rank, in the order of
// build_*'s schur_matrix(..., solved = true) calls.  What this list misses, schur_matrix handles
// alone; what it has too much only costs an estimate.
std::vector<std::pair<const double *, double>> SchurPC::solved_matrices() const {
    std::vector<std::pair<const double *, double>> out;
    const int n = n_, lo = lo_, hi = hi_;
    if (d_.kind == KKT_PC_STATIONARY) {
        const double c = 1.0 / std::sqrt(d_.beta);
        out.emplace_back(block_vals(KKT_Q10, 0, 0), c);
        out.emplace_back(block_vals(KKT_Q01, 0, 0), c);
        return out;
    }
    const bool be = d_.kind == KKT_PC_INSTATIONARY_BE;
    const double shift = d_.tau / std::sqrt(d_.beta);
    auto coef = [&](int i) {
        if (!be) return 0.5 * d_.tau / std::sqrt(d_.beta);
        return i == 0 ? 0.0 : (i == n - 1 ? std::sqrt(d_.epsilon) * shift : shift);
    };
    const int imid = (lo + hi) / 2;
    out.emplace_back(block_vals(KKT_Q10, imid, imid), coef(imid));
    for (int i = lo; i < hi; ++i) out.emplace_back(block_vals(KKT_Q10, i, i), coef(i));
    for (int i = hi - 1; i >= lo; --i) out.emplace_back(block_vals(KKT_Q01, i, i), coef(i));
    return out;
}

// The stored blocks the program multiplies with (the right-hand-side products and the updates of
// the sweeps), in emission order.
std::vector<const double *> SchurPC::multiplied_blocks() const {
    std::vector<const double *> out;
    if (d_.kind == KKT_PC_STATIONARY) {
        out.push_back(block_vals(KKT_Q10, 0, 0));
        return out;
    }
    for (int i = lo_; i < hi_; ++i) {
        out.push_back(block_vals(KKT_Q10, i, i));
        if (i >= 1) out.push_back(block_vals(KKT_Q10, i, i - 1));
    }
    for (int i = hi_ - 1; i >= lo_; --i)
        if (i <= n_ - 2) out.push_back(block_vals(KKT_Q01, i, i + 1));
    return out;
}

const double *SchurPC::shared_block(const double *vals) const {
    const auto it = block_rep_.find(vals);
    return it == block_rep_.end() ? vals : it->second;
}

void SchurPC::collect_matrices() {
    pre_.clear();
    pre_cls_.clear();
    block_rep_.clear();
    formed_.clear();
    const int nbatch = S_.opts.spectrum_batch;
    const bool estimates = d_.schur_emin <= 0;
    const bool alias = S_.opts.pc_alias;
    if (nbatch <= 0 || !(estimates || coarse_cycles_ > 0)) return;
    const Pattern &P = S_.patterns[m_pat_];
    hipStream_t st = S_.stream;
    kkt_spectrum_stats &stats = S_.spectrum_stats;
    SpectrumCounters cnt;
    HIPCHK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    // the candidates in creation order, each formed once (owned here until their classes are known)
    std::vector<MatKey> keys;
    std::vector<DevBuf<double>> own_vals, own_dinv;
    for (const auto &bc : solved_matrices()) {
        uint64_t bits;
        std::memcpy(&bits, &bc.second, sizeof bits);
        const MatKey key(bc.first, bits);
        if (pre_.count(key)) continue;
        own_vals.push_back(DevBuf<double>::alloc(P.npadded));
        own_dinv.push_back(DevBuf<double>::alloc(nx_));
        Pre pr;
        pr.vals = own_vals.back().get();
        pr.dinv = own_dinv.back().get();
        form_matrix(bc.first, bc.second, pr.vals, pr.dinv);
        cnt.launches += mask_ ? 3 : 2;
        pre_[key] = pr;
        keys.push_back(key);
    }
    const int C = (int)keys.size();
    if (C == 0) return;
    // "pc_alias": the stored blocks the program multiplies with ride the same search, behind the
    // formed candidates and under a tag of their own (no shift)
    std::vector<const double *> h_vals(C);
    for (int i = 0; i < C; ++i) h_vals[i] = pre_[keys[i]].vals;
    if (alias)
        for (const double *b : multiplied_blocks())
            if (std::find(h_vals.begin() + C, h_vals.end(), b) == h_vals.end()) h_vals.push_back(b);
    const int N = (int)h_vals.size();
    stats.alias_blocks += N - C;
    // twins: a fingerprint per candidate, then the candidates of a (tag, shift, fingerprint) group
    // bit for bit against the group's first
    spec::TwinGroups twins;
    twins.first_of.resize(N);
    for (int i = 0; i < N; ++i) twins.first_of[i] = i;
    twins.pair_of.assign(N, -1);
    std::vector<unsigned> h_flag;
    DevPool tmp;
    if (N > 1) {
        const double *const *d_vals = tmp.upload(h_vals.data(), h_vals.size());
        const int nw = spec_fingerprint_blocks(P.npadded);
        unsigned long long *d_fp = tmp.alloc<unsigned long long>((size_t)N * nw);
        std::vector<unsigned long long> h_fp((size_t)N * nw);
        launch_spec_fingerprint(st, d_vals, N, P.npadded, d_fp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_fp.data(), d_fp, h_fp.size() * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        cnt.launches++;
        cnt.syncs++;
        stats.twin_syncs++;
        std::vector<uint64_t> shifts(N, 0), folded(N);
        std::vector<int> tag(N, 1);
        for (int i = 0; i < N; ++i) {
            if (i < C) shifts[i] = keys[i].second, tag[i] = 0;
            folded[i] = spec_fingerprint_fold(&h_fp[(size_t)i * nw], nw);
        }
        twins = spec::group_twins(shifts, folded, tag);
        std::vector<SpecPair> pairs;
        for (const auto &pr : twins.pairs) pairs.push_back(SpecPair{h_vals[pr.first], h_vals[pr.second]});
        if (!pairs.empty()) {
            const SpecPair *d_pairs = tmp.upload(pairs.data(), pairs.size());
            unsigned *d_flag = tmp.alloc<unsigned>(pairs.size());
            h_flag.assign(pairs.size(), 1u);
            HIPCHK(hipMemsetAsync(d_flag, 0, pairs.size() * sizeof(unsigned), st));
            launch_spec_pairs_differ(st, d_pairs, (int)pairs.size(), P.npadded, d_flag);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_flag.data(), d_flag, h_flag.size() * sizeof(unsigned),
                                  hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            cnt.launches++;
            cnt.syncs++;
            stats.twin_syncs++;
        }
    }
    // equal fingerprints, different bits: no class, left to schur_matrix's own comparison
    std::vector<int> all_reps;      // the first candidate of every class
    const std::vector<int> cls = spec::twin_classes(twins, h_flag, &all_reps);
    for (int i = 0; i < C; ++i) pre_[keys[i]].cls = cls[i];
    pre_cls_.assign(all_reps.size(), PreCls{});
    // a twin reads its class's first array: the formed ones give theirs up, the stored blocks get
    // a representative.  (Every comparison was synchronised above: nothing in flight reads them.)
    for (int i = 0; i < N; ++i) {
        const int first = alias && cls[i] >= 0 ? all_reps[cls[i]] : i;
        if (first != i) stats.aliased++;
        if (i >= C) {
            if (first != i) block_rep_[h_vals[i]] = h_vals[first];
            continue;
        }
        Pre &pr = pre_[keys[i]];
        if (first != i) {
            pr.vals = pre_[keys[first]].vals;
            pr.dinv = pre_[keys[first]].dinv;
            own_vals[i].reset();
            own_dinv[i].reset();
        } else {
            values_mem_.adopt(std::move(own_vals[i]));
            values_mem_.adopt(std::move(own_dinv[i]));
        }
    }
    std::vector<int> reps;          // ... of the formed matrices: the ones to estimate
    for (int r : all_reps)
        if (r < C) reps.push_back(r);
    // the distinct matrices' intervals, nbatch at a time: symmetric / skew split, Lanczos on the
    // symmetric parts, power iteration on the skew parts of those that have one
    const int32_t *tpos = estimates ? transpose_positions() : nullptr;
    for (size_t r0 = 0; estimates && r0 < reps.size(); r0 += (size_t)nbatch) {
        const int B = (int)std::min<size_t>((size_t)nbatch, reps.size() - r0);
        DevPool bmem;      // the batch's split values: gone before the next batch
        std::vector<const double *> lv(B), dv(B);
        std::vector<SpecSplit> split(B);
        std::vector<unsigned> nonsym(B, 0u);
        for (int b = 0; b < B; ++b) {
            const Pre &pr = pre_[keys[reps[r0 + b]]];
            lv[b] = pr.vals;
            dv[b] = pr.dinv;
        }
        size_t split_bytes = 0;
        if (tpos) {
            for (int b = 0; b < B; ++b)
                split[b] = SpecSplit{lv[b], bmem.alloc<double>(P.npadded), bmem.alloc<double>(P.npadded)};
            split_bytes = 2 * (size_t)B * P.npadded * sizeof(double);
            const SpecSplit *d_split = bmem.upload(split.data(), split.size());
            unsigned *d_flag = bmem.alloc<unsigned>(B);
            HIPCHK(hipMemsetAsync(d_flag, 0, (size_t)B * sizeof(unsigned), st));
            launch_spec_sym_skew(st, d_split, B, tpos, P.npadded, d_flag);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(nonsym.data(), d_flag, (size_t)B * sizeof(unsigned),
                                  hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            cnt.launches++;
            cnt.syncs++;
            for (int b = 0; b < B; ++b)
                if (nonsym[b]) lv[b] = split[b].h;
        }
        SpectrumCounters bc;
        const std::vector<Spectrum> sp = jacobi_spectrum_batch(S_, m_pat_, lv, dv, mask_, 400, &bc);
        // (a matrix without an interval fails the build in schur_matrix: no radius for it, as there)
        std::vector<const double *> sk, sd;
        std::vector<int> who;
        for (int b = 0; b < B; ++b)
            if (nonsym[b] && sp[b].emin > 0.0 && sp[b].emax > sp[b].emin) {
                sk.push_back(split[b].sk);
                sd.push_back(dv[b]);
                who.push_back(b);
            }
        std::vector<int> psteps;
        const std::vector<double> radius =
            jacobi_skew_radius_batch(S_, m_pat_, sk, sd, mask_, 40, &psteps, &bc);
        HIPCHK(hipGetLastError());
        for (int b = 0; b < B; ++b) {
            PreCls &pc = pre_cls_[pre_[keys[reps[r0 + b]]].cls];
            pc.estimated = true;
            pc.sp = sp[b];
            pc.nonsym = nonsym[b] != 0;
        }
        for (size_t q = 0; q < who.size(); ++q) {
            PreCls &pc = pre_cls_[pre_[keys[reps[r0 + who[q]]]].cls];
            pc.radius = radius[q];
            pc.power = psteps[q];
        }
        cnt.launches += bc.launches;
        cnt.syncs += bc.syncs;
        cnt.lanczos_syncs_max = std::max(cnt.lanczos_syncs_max, bc.lanczos_syncs_max);
        cnt.bytes = std::max<int64_t>(cnt.bytes, bc.bytes + (int64_t)split_bytes);
        stats.batches++;
        stats.matrices += B;
        if (S_.opts.verbose)
            std::fprintf(stderr, "[kkt] spectrum batch of %d matrices holds %lld bytes\n", B,
                         (long long)(bc.bytes + (int64_t)split_bytes));
    }
    stats.launches += cnt.launches;
    stats.syncs += cnt.syncs;
    stats.lanczos_syncs_max = cnt.lanczos_syncs_max;
    stats.batch_bytes = cnt.bytes;
    stats.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// base + c * M with bc rows/cols of `assemble(form, bcs=...)`, and its Jacobi diagonal
SchurPC::Mat SchurPC::schur_matrix(const double *base_vals, double c, bool solved) {
    uint64_t bits;
    std::memcpy(&bits, &c, sizeof bits);
    auto key = std::make_pair(base_vals, bits);
    auto it = mats_.find(key);
    if (it != mats_.end() && (!solved || it->second.est != KKT_PC_EST_NONE)) return it->second;
    const Pattern &P = S_.patterns[m_pat_];
    hipStream_t st = S_.stream;
    Mat m;
    if (it != mats_.end()) {
        m = it->second;      // formed for products only, now solved with: interval and inverse below
    } else {
        const auto pre = pre_.find(key);
        if (pre != pre_.end()) {
            m.vals = pre->second.vals;      // formed by the collection pass
            m.dinv = pre->second.dinv;
        } else {
            // formed here, once per (class of the base block, shift)
            auto &f = formed_[MatKey(shared_block(base_vals), bits)];
            if (!f.first) {
                f.first = values_mem_.alloc<double>(P.npadded);
                f.second = values_mem_.alloc<double>(nx_);
                form_matrix(base_vals, c, f.first, f.second);
            } else {
                S_.spectrum_stats.aliased++;
            }
            m.vals = f.first;
            m.dinv = f.second;
        }
        m.index = (int)mat_recs_.size();
        MatRec r;
        r.c = c;
        mat_recs_.push_back(r);
    }
    if (!solved) {
        mats_[key] = m;
        return m;
    }
    MatRec &rec = mat_recs_[m.index];
    // an earlier matrix with the same shift and the same values (mode G stores one copy per time
    // level of a time-invariant operator) shares its spectrum estimate and its coarse inverse
    // (matrices only multiplied with carry neither: emax == 0)
    const Mat *twin = nullptr;
    kkt_spectrum_stats &stats = S_.spectrum_stats;
    const bool batched = S_.opts.spectrum_batch > 0;
    auto cls_of = [&](const MatKey &k) {
        const auto pre = pre_.find(k);
        return pre == pre_.end() ? -1 : pre->second.cls;
    };
    const int cls = cls_of(key);
    bool fell_back = false;
    const auto t0 = std::chrono::steady_clock::now();
    if (d_.schur_emin <= 0 || coarse_cycles_ > 0) {
        for (auto &kv : mats_) {
            if (kv.first.second != bits || kv.second.emax <= 0.0) continue;
            // both compared by the collection pass: equal values have one class
            const int other = cls_of(kv.first);
            if (cls >= 0 && other >= 0) {
                if (cls != other) continue;
                twin = &kv.second;
                break;
            }
            fell_back = batched;
            stats.launches++;
            stats.syncs++;
            stats.twin_syncs++;
            auto d_flag = DevBuf<unsigned>::alloc(1);
            HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(unsigned), st));
            launch_vals_differ(st, m.vals, kv.second.vals, P.npadded, d_flag.get());
            unsigned differ = 1;
            HIPCHK(hipMemcpyAsync(&differ, d_flag.get(), sizeof differ, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!differ) {
                twin = &kv.second;
                break;
            }
        }
    }
    if (twin && S_.opts.pc_alias && m.vals != twin->vals) {
        // found equal here and not by the collection pass: read the twin's arrays from now on
        // (this one's stay allocated until the values change)
        m.vals = twin->vals;
        m.dinv = twin->dinv;
        stats.aliased++;
    }
    if (d_.schur_emin > 0) {
        m.emin = d_.schur_emin;
        m.emax = d_.schur_emax;
        m.eimag = d_.schur_eimag > 0 ? d_.schur_eimag : 0.0;
        m.est = KKT_PC_EST_GIVEN;
    } else if (twin) {
        // Interval from the matrix itself; the first and last levels carry other shifts
        // (control.py:2241-2327) and get their own, wider, intervals.
        m.emin = twin->emin;
        m.emax = twin->emax;
        m.eimag = twin->eimag;
        m.est = KKT_PC_EST_SHARED;
    } else {
        // Blocks with a convection term are not symmetric: the interval comes from the
        // symmetric part H = (A + A^T) / 2 (Bendixson: Re lambda lies in the spectrum of
        // D^-1/2 H D^-1/2) and the ellipse's imaginary semi-axis from the spectral radius of
        // the skew part (|Im lambda| <= rho(D^-1/2 (A - A^T) / 2 D^-1/2)).
        DevBuf<double> hv, sv2;
        unsigned nonsym = 0;
        Spectrum sp{0.0, 0.0, 0};
        double radius = 0.0;
        int power = 0;
        const bool have = cls >= 0 && pre_cls_[cls].estimated;
        if (have) {
            const PreCls &pc = pre_cls_[cls];      // estimated in a batch, on equal values
            sp = pc.sp;
            nonsym = pc.nonsym;
            radius = pc.radius;
            power = pc.power;
        } else {
            fell_back = batched;
            stats.matrices++;
            const int32_t *tpos = transpose_positions();
            if (tpos) {
                hv = DevBuf<double>::alloc(P.npadded);
                sv2 = DevBuf<double>::alloc(P.npadded);
                auto d_flag = DevBuf<unsigned>::alloc(1);
                HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(unsigned), st));
                launch_vals_sym_skew(st, m.vals, tpos, hv.get(), sv2.get(), P.npadded, d_flag.get());
                HIPCHK(hipMemcpyAsync(&nonsym, d_flag.get(), sizeof nonsym, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            }
            sp = jacobi_spectrum(S_, m_pat_, nonsym ? hv.get() : m.vals, m.dinv, mask_, 400);
            if (nonsym && sp.emin > 0.0 && sp.emax > sp.emin)
                radius = jacobi_skew_radius(S_, m_pat_, sv2.get(), m.dinv, mask_, 40, &power);
            hv.reset(), sv2.reset();   // before the coarse inverse below is allocated
        }
        stats.lanczos_steps += sp.steps;
        spectrum_steps_ += sp.steps;
        rec.lanczos = sp.steps;
        if (!(sp.emin > 0.0) || !(sp.emax > sp.emin))
            fail(KKT_ERR_STATE, "sub-solve matrix is not positive definite: no Chebyshev interval");
        m.emin = 0.85 * sp.emin;      // Ritz values lie inside the spectrum
        m.emax = 1.05 * sp.emax;
        if (nonsym) {
            m.eimag = 1.1 * radius;
            spectrum_steps_ += 2 * power;
            stats.power_steps += power;
            rec.power = power;
        }
        // two-grid form: the sweeps smooth -- they cover the upper part of the spectrum, the
        // coarse space the rest (emax / 30: measured optimum for 8 sweeps at coarse cells of 8
        // to 16 mesh widths, scripts/proto_subsolve.py)
        if (coarse_cycles_ > 0) m.emin = std::max(m.emin, m.emax / 30.0);
        m.est = KKT_PC_EST_LANCZOS;
    }
    if (fell_back) stats.fallbacks++;
    if (!batched || fell_back)      // (the host's clock: every branch taken here ends in a synchronisation)
        stats.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (coarse_cycles_ > 0) m.einv = twin && twin->einv ? twin->einv : coarse_inverse(m.vals);
    rec.est = m.est;
    rec.coarse = m.einv != nullptr;
    mats_[key] = m;
    return m;
}

void SchurPC::alias_records(std::vector<int32_t> &out) const {
    out.clear();
    std::map<const double *, int32_t> number;      // arrays in order of first appearance
    for (const double *p : alias_recs_) {
        if (p && !number.count(p)) {
            const int32_t k = (int32_t)number.size();
            number[p] = k;
        }
        out.push_back(p ? number[p] : -1);
    }
}

void SchurPC::note_solve(int sweep, int level, const Mat &m, const double *upd_vals) {
    alias_recs_.insert(alias_recs_.end(), {m.vals, m.dinv, upd_vals});
    mat_recs_[m.index].solves++;
    solve_recs_.insert(solve_recs_.end(),
                       {(double)sweep, (double)level, (double)m.index, mat_recs_[m.index].c, m.emin,
                        m.emax, m.eimag, (double)schur_its_, (double)m.est});
}

void SchurPC::solve_records(std::vector<double> &out) const { out = solve_recs_; }
bool SchurPC::coarse_space(CoarseDev *c, GalerkinDev *g, int64_t *n) const {
    if (coarse_.nc <= 0) return false;
    *c = coarse_;
    *g = galerkin_;
    *n = nx_;
    return true;
}

void SchurPC::matrix_records(std::vector<double> &out) const {
    out.clear();
    for (const MatRec &r : mat_recs_)
        out.insert(out.end(), {r.c, (double)r.est, (double)r.lanczos, (double)r.power,
                               r.coarse ? 1.0 : 0.0, (double)r.solves});
}

// Degree of the sub-solves: as given, or 1.6 sqrt(kappa) of a typical (interior-level) matrix --
// the measured minimum for GMRES(10) to converge on 256^2 P1 is 1.46 sqrt(kappa).
// Crank-Nicolson: 2.6 sqrt(kappa) -- its preconditioner wraps the sweeps in the running sums
// T_2^-1 / T_2 over all time levels (control.py:2053, 2118), which accumulate the error of the
// inexact sub-solves: with 1.6 sqrt(kappa) GMRES(10) stalls on 256^2 x 64, with 2.5 it needs 15
// iterations.
int SchurPC::resolve_its(const Mat &typical) {
    typical_emin_ = typical.emin;
    typical_emax_ = typical.emax;
    if (d_.schur_its >= 0) return d_.schur_its;
    if (coarse_cycles_ > 0) return 8;      // smoothing sweeps per cycle
    const double factor = d_.kind == KKT_PC_INSTATIONARY_CN ? 2.6 : 1.6;
    int its = (int)std::ceil(factor * std::sqrt(typical.emax / typical.emin));
    its = std::max(4, std::min(600, its));
    if (S_.sharded && S_.comm) its = (int)S_.comm->max_host((double)its, S_.stream);
    return its;
}

void SchurPC::push_rows(std::vector<RowOp> &r) {
    PcStep s;
    s.kind = PcStep::ROWS;
    s.rows = make_row_launch(program_mem_, S_.patterns[m_pat_], r, S_.opts.kernarg_ops,
                             S_.opts.shared_rows);
    s.lane = cur_lane_;
    s.level = cur_level_;
    steps_.push_back(s);
}

void SchurPC::emit_lin(const std::vector<Lin> &ops) {
    std::vector<RowOp> r;
    for (const Lin &l : ops) r.push_back(lin_op(S_.patterns[m_pat_], nx_, mask_, l));
    push_rows(r);
}

void SchurPC::emit_cheb(const std::vector<Cheb> &ops) {
    std::vector<RowOp> r;
    for (const Cheb &c : ops) r.push_back(cheb_op(S_.patterns[m_pat_], nx_, mask_, c));
    push_rows(r);
}

void SchurPC::emit_time(double *y, const double *x, int kind, int n, const double *lo_halo,
                        const double *hi_halo) {
    PcStep s;
    s.kind = PcStep::TIME;
    s.y = y;
    s.x = x;
    s.tkind = kind;
    s.n = n;
    s.nx = nx_;
    s.lo_halo = lo_halo;
    s.hi_halo = hi_halo;
    s.lane = cur_lane_;
    steps_.push_back(s);
}

// KSPSolve_Chebyshev (first kind) + PCJACOBI, zero initial guess, exactly `its` steps
// (options of control.py:1973-1982); its == 0: one Jacobi application (control.py:1984-1991).
void SchurPC::emit_update_and_solve(Lin upd, const Solve &sv, int its, double emin, double emax,
                                    double eimag, const Mat *mat) {
    if (coarse_cycles_ > 0 && mat && mat->einv) {
        emit_coarse_solve(&upd, sv, *mat);
        return;
    }
    if (its == 0) {
        upd.y2 = sv.out;        // Jacobi: u = D^-1 b
        upd.dinv = sv.dinv;
        upd.c3 = 1.0;
        emit_lin({upd});
        return;
    }
    upd.y2 = its == 1 ? sv.out : P_[0];
    upd.dinv = sv.dinv;
    upd.c3 = 2.0 / (emax + emin);
    SweepLevel lv;
    begin_level();
    emit_lin({upd});
    emit_solves({sv}, its, emin, emax, P_, nx_, true, &lv.coef, eimag);
    lv.its = its;
    const LevelForm f = level_form(&upd, sv, upd.c3);
    if (its >= 2 && f.ok) {
        lv.lev = f.lev;
        lv.b_after = f.b_after;
        lv.eligible = true;
    }
    end_level(std::move(lv));
}

// Batched solves with ONE matrix (the mass solves: every time level the same M): the Chebyshev
// iterates of four levels interleaved, one IlOp per group and step (kernels.hpp).  Same
// coefficients and the same fma chain per row and level as emit_solves below.
bool SchurPC::emit_solves_interleaved(const std::vector<Solve> &sv, int its, double emin,
                                      double emax) {
    // (lanes: chunks on two streams would share the buffers)
    if (!S_.opts.interleave || S_.opts.lanes) return false;
    const size_t m = sv.size();
    for (const Solve &q : sv)
        if (q.vals != sv[0].vals || q.dinv != sv[0].dinv) return false;
    const Pattern &P = S_.patterns[m_pat_];
    // pc_rows_il reads the SELL-128 layout (R = 2): with sell_r = 1 its slice count and offsets
    // would address 64-row slices as 128-row ones, past the end of the index and value arrays
    if (P.R != 2) return false;
    const int ng = (int)((m + 3) / 4);
    const size_t need = (size_t)ng * 4 * (size_t)nx_;
    if (need > il_cap_) {
        for (int k = 0; k < 3; ++k) {
            // program memory: steps emitted before a regrow keep the smaller buffers
            il_P_[k] = program_mem_.alloc<double>(need + 32);
            HIPCHK(hipMemsetAsync(il_P_[k], 0, (need + 32) * sizeof(double), S_.stream));
        }
        il_cap_ = need;
    }
    const ChebCoefficients cheb = cheb_coefficients(its, emin, emax);
    auto buf = [&](int step, int g) -> double * {
        return il_P_[(step - 1) % 3] + (size_t)g * 4 * (size_t)nx_;
    };
    MassSolve rec;      // for fuse_mass_tiles()
    rec.its = its;
    rec.sv = sv;
    for (int step = 1; step <= its; ++step) {
        const TileCoef k = step >= 2 ? cheb.step(step) : TileCoef{0.0, 0.0, cheb.scale};
        rec.coef.push_back(k);
        const bool last = step == its;
        std::vector<IlOp> ops(ng);
        for (int g = 0; g < ng; ++g) {
            const int nlev = (int)std::min<size_t>(4, m - (size_t)g * 4);
            IlLevel lev[4];
            for (int l = 0; l < nlev; ++l) {
                const Solve &q = sv[(size_t)g * 4 + l];
                lev[l] = IlLevel{q.b, last ? q.out : nullptr, last ? q.post1 : 1.0,
                                 last ? q.post2 : 1.0};
            }
            ops[g] = il_op(P, nx_, mask_, sv[0].vals, sv[0].dinv, lev, nlev,
                           step >= 2 ? buf(step - 1, g) : nullptr,
                           step >= 3 ? buf(step - 2, g) : nullptr, last ? nullptr : buf(step, g), k);
        }
        PcStep s;
        s.kind = PcStep::ROWS_IL;
        s.d_il = program_mem_.upload(ops.data(), ops.size());
        s.il_groups = ng;
        s.il_slices = P.nslices;
        s.il_w = P.uniform_w;
        s.lane = cur_lane_;
        s.solve = (int)mass_solves_.size();
        steps_.push_back(s);
    }
    mass_solves_.push_back(std::move(rec));
    return true;
}

void SchurPC::emit_solves(const std::vector<Solve> &sv, int its, double emin, double emax,
                          double *const P[3], int64_t pstride, bool first_done,
                          std::vector<TileCoef> *coef_out, double eimag, const Mat *mat) {
    if (coarse_cycles_ > 0 && mat && mat->einv && sv.size() == 1 && !first_done) {
        emit_coarse_solve(nullptr, sv[0], *mat);
        return;
    }
    const size_t m = sv.size();
    if (m >= 4 && !first_done && its >= 2 && eimag == 0.0 && pstride == nx_ &&
        emit_solves_interleaved(sv, its, emin, emax))
        return;
    // a single solve on a final right-hand side is a sweep level without update (the first
    // level of a sweep, the sub-solves of the stationary preconditioner)
    SweepLevel solo;
    const bool record_solo = m == 1 && !first_done && its >= 2;
    if (record_solo) {
        begin_level();
        coef_out = &solo.coef;
    }
    std::vector<Cheb> ops(m);
    if (its == 0) {
        for (size_t q = 0; q < m; ++q)
            ops[q] = Cheb{nullptr, sv[q].dinv, sv[q].b, nullptr, nullptr, sv[q].out,
                          0.0, 0.0, 1.0, sv[q].post1, sv[q].post2};
        emit_cheb(ops);
        return;
    }
    // (eimag > 0: the coefficients of the ellipse, chebyshev.hpp)
    const ChebCoefficients cheb = cheb_coefficients(its, emin, emax, eimag);
    const double scale = cheb.scale;
    // step 1: p_1 = scale * D^-1 b
    auto target = [&](int step, size_t q) -> double * {
        return step == its ? sv[q].out : P[(step - 1) % 3] + (int64_t)q * pstride;
    };
    if (!first_done) {
        for (size_t q = 0; q < m; ++q) {
            const bool last = its == 1;
            ops[q] = Cheb{nullptr, sv[q].dinv, sv[q].b, nullptr, nullptr, target(1, q),
                          0.0, 0.0, scale, last ? sv[q].post1 : 1.0, last ? sv[q].post2 : 1.0};
        }
        emit_cheb(ops);
    }
    for (int step = 2; step <= its; ++step) {
        const TileCoef &k = cheb.step(step);
        const bool last = step == its;
        for (size_t q = 0; q < m; ++q) {
            const double *pk = target(step - 1, q);
            const double *pkm1 = step >= 3 ? target(step - 2, q) : nullptr;
            ops[q] = Cheb{sv[q].vals, sv[q].dinv, sv[q].b, pk, pkm1, target(step, q),
                          k.c1, k.c2, k.c3,
                          last ? sv[q].post1 : 1.0, last ? sv[q].post2 : 1.0};
        }
        if (coef_out) coef_out->push_back(k);
        emit_cheb(ops);
    }
    if (record_solo) {
        solo.its = its;
        solo.lev = level_form(nullptr, sv[0], scale).lev;
        solo.eligible = true;
        end_level(std::move(solo));
    }
}

// ---- Control.Stationary.construct_pc, control.py:356-448
void SchurPC::build_stationary() {
    const double c = 1.0 / std::sqrt(d_.beta);
    const double *Dv = block_vals(KKT_Q10, 0, 0);
    const double *Dz = block_vals(KKT_Q01, 0, 0);
    double *b0 = in_, *b1 = in_ + nx_;
    double *u0 = out_, *u1 = out_ + nx_;
    emit_solves({Solve{m_vals_, m_dinv_, b0, u0}}, d_.mass_its, d_.mass_emin, d_.mass_emax, P_, nx_);
    emit_lin({Lin{{Term{shared_block(Dv), u0}}, B_, 1.0, 0.0, -1.0, nullptr, b1}});
    Mat S1 = schur_matrix(Dv, c), S2 = schur_matrix(Dz, c);
    schur_its_ = resolve_its(S1);
    note_solve(KKT_PC_SWEEP_FIRST, 0, S1);
    emit_solves({Solve{S1.vals, S1.dinv, B_, u1}}, schur_its_, S1.emin, S1.emax, P_, nx_, false, nullptr, S1.eimag, &S1);
    emit_lin({Lin{{Term{m_vals_, u1}}, B_, 1.0}});
    note_solve(KKT_PC_SWEEP_SECOND, 0, S2);
    emit_solves({Solve{S2.vals, S2.dinv, B_, u1}}, schur_its_, S2.emin, S2.emax, P_, nx_, false, nullptr, S2.eimag, &S2);
}

// Time sharding: a rank owns blocks [lo, hi).  Everything that is independent
// per time level (mass solves, residual products) runs on the local blocks; the sweeps and
// the CN scans are serial in time, so ranks hand one N_x vector to the next rank and form a
// pipeline -- COMM steps between graph-captured segments of the program.

// ---- Control.Instationary.construct_pc, BE branch, control.py:2191-2438
void SchurPC::build_BE() {
    const int n = n_, lo = lo_, hi = hi_;
    const double tau = d_.tau, eps = d_.epsilon;
    const double shift = tau / std::sqrt(d_.beta);
    const int64_t nl = hi - lo;
    double *b0 = in_, *b1 = in_ + nl * nx_;
    double *u0 = out_, *u1 = out_ + nl * nx_;
    auto blk = [&](double *base, int i) { return base + (int64_t)(i - lo) * nx_; };
    const int up = hi < n ? S_.rank + 1 : -1, dn = lo > 0 ? S_.rank - 1 : -1;
    // Unsharded handles split the level range into chunks: the mass solves and the
    // right-hand-side products of chunk c run on the side lane while the forward sweep works
    // through chunk c - 1 on the main lane.
    const bool lanes = use_lanes_ && !S_.sharded && (hi - lo) >= 16;
    int n_chunks = 1;
    if (lanes) n_chunks = std::max(2, std::min((hi - lo) / 4, S_.opts.lane_chunks));
    std::vector<int> cfirst(n_chunks + 1);
    for (int c = 0; c <= n_chunks; ++c) cfirst[c] = lo + (int)((int64_t)(hi - lo) * c / n_chunks);
    std::vector<int> chunk_done(n_chunks, -1);
    auto coef = [&](int i) { return i == 0 ? 0.0 : (i == n - 1 ? std::sqrt(eps) * shift : shift); };
    {
        const int imid = (lo + hi) / 2;      // a typical level: decides the degree when it is derived
        schur_its_ = resolve_its(schur_matrix(block_vals(KKT_Q10, imid, imid), coef(imid)));
    }
    auto side_chunk = [&](int c) {
        const int c0 = cfirst[c], c1 = cfirst[c + 1];
        cur_lane_ = lanes ? 1 : 0;
        // (1,1)-block: u0_i = (1/tau) M~^-1 b0_i, last one also / epsilon   (2193-2206)
        {
            std::vector<Solve> sv;
            for (int i = c0; i < c1; ++i)
                sv.push_back(Solve{m_vals_, m_dinv_, blk(b0, i), blk(u0, i), 1.0 / tau,
                                   i == n - 1 ? 1.0 / eps : 1.0});
            double *const Pc[3] = {blk(P_[0], c0), blk(P_[1], c0), blk(P_[2], c0)};
            emit_solves(sv, d_.mass_its, d_.mass_emin, d_.mass_emax, Pc, nx_);
        }
        if (c == n_chunks - 1 && (up >= 0 || dn >= 0)) emit_comm(blk(u0, hi - 1), up, h_u0_, dn);
        // b_i = block_10(i,i) u0_i + block_10(i,i-1) u0_{i-1} - b1_i   (2208-2237)
        {
            std::vector<Lin> ops;
            for (int i = c0; i < c1; ++i) {
                Lin l;
                l.terms.push_back(Term{mult_vals(KKT_Q10, i, i), blk(u0, i)});
                if (i >= 1)
                    l.terms.push_back(Term{mult_vals(KKT_Q10, i, i - 1),
                                           i - 1 >= lo ? blk(u0, i - 1) : h_u0_});
                l.y = blk(B_, i);
                l.cz = -1.0;
                l.z = blk(b1, i);
                ops.push_back(l);
            }
            emit_lin(ops);
        }
        if (lanes) chunk_done[c] = emit_record(1);
        cur_lane_ = 0;
    };
    // forward sweep (2241-2327)
    auto sweep_chunk = [&](int c) {
        if (lanes) emit_wait(0, chunk_done[c]);
        for (int i = cfirst[c]; i < cfirst[c + 1]; ++i) {
            Mat F = schur_matrix(block_vals(KKT_Q10, i, i), coef(i));
            const double *upd = i >= 1 ? mult_vals(KKT_Q10, i, i - 1) : nullptr;
            note_solve(KKT_PC_SWEEP_FORWARD, i, F, upd);
            const Solve sv{F.vals, F.dinv, blk(B_, i), blk(u1, i)};
            if (i >= 1)
                emit_update_and_solve(Lin{{Term{upd, i - 1 >= lo ? blk(u1, i - 1) : h_u1_}},
                                          blk(B_, i), -1.0, 1.0, 0.0, blk(B_, i), nullptr},
                                      sv, schur_its_, F.emin, F.emax, F.eimag, &F);
            else
                emit_solves({sv}, schur_its_, F.emin, F.emax, P_, nx_, false, nullptr, F.eimag, &F);
        }
    };
    if (lanes) {
        // host submission order interleaves the lanes: the sweep of chunk c (three calls) is
        // queued before the ~20 launches of chunk c + 1, so neither stream waits for the host
        const int e_start = emit_record(0);
        emit_wait(1, e_start);
        side_chunk(0);
        for (int c = 0; c < n_chunks; ++c) {
            sweep_chunk(c);
            if (c + 1 < n_chunks) side_chunk(c + 1);
        }
    } else {
        side_chunk(0);
        if (dn >= 0) emit_comm(nullptr, -1, h_u1_, dn);
        sweep_chunk(0);
    }
    if (up >= 0) emit_comm(blk(u1, hi - 1), up, nullptr, -1);
    // b_i = tau M u1_i (epsilon tau for the last)   (2330-2350)
    {
        std::vector<Lin> ops;
        for (int i = lo; i < hi; ++i)
            ops.push_back(Lin{{Term{m_vals_, blk(u1, i)}}, blk(B_, i),
                              i == n - 1 ? eps * tau : tau});
        emit_lin(ops);
    }
    // backward sweep (2353-2437)
    if (up >= 0) emit_comm(nullptr, -1, h_u1_, up);
    for (int i = hi - 1; i >= lo; --i) {
        Mat G = schur_matrix(block_vals(KKT_Q01, i, i), coef(i));
        const double *upd = i <= n - 2 ? mult_vals(KKT_Q01, i, i + 1) : nullptr;
        note_solve(KKT_PC_SWEEP_BACKWARD, i, G, upd);
        const Solve sv{G.vals, G.dinv, blk(B_, i), blk(u1, i)};
        if (i <= n - 2)
            emit_update_and_solve(Lin{{Term{upd, i + 1 < hi ? blk(u1, i + 1) : h_u1_}},
                                      blk(B_, i), -1.0, 1.0, 0.0, blk(B_, i), nullptr},
                                  sv, schur_its_, G.emin, G.emax, G.eimag, &G);
        else
            emit_solves({sv}, schur_its_, G.emin, G.emax, P_, nx_, false, nullptr, G.eimag, &G);
    }
    if (dn >= 0) emit_comm(blk(u1, lo), dn, nullptr, -1);
}

// ---- Control.Instationary.construct_pc, CN branch, control.py:1995-2189
void SchurPC::build_CN() {
    const int n = n_, lo = lo_, hi = hi_;
    const double tau = d_.tau;
    const double c = 0.5 * tau / std::sqrt(d_.beta);   // my_const, control.py:2051
    const int64_t nl = hi - lo;
    const int nloc = (int)nl;
    double *b0 = in_, *b1 = in_ + nl * nx_;
    double *u0 = out_, *u1 = out_ + nl * nx_;
    auto blk = [&](double *base, int i) { return base + (int64_t)(i - lo) * nx_; };
    const int up = hi < n ? S_.rank + 1 : -1, dn = lo > 0 ? S_.rank - 1 : -1;
    Mat cM = schur_matrix(nullptr, c, false);   // c * M~ (base absent): products with my_const * M
    {
        const int imid = (lo + hi) / 2;
        schur_its_ = resolve_its(schur_matrix(block_vals(KKT_Q10, imid, imid), c));
    }
    // (1,1)-block (1997-2014): T_1^-1 is a scan from the last block down
    if (up >= 0) emit_comm(nullptr, -1, h_t_, up);
    emit_time(T_, b0, 3, nloc, nullptr, up >= 0 ? h_t_ : nullptr);
    if (dn >= 0) emit_comm(blk(T_, lo), dn, nullptr, -1);
    {
        std::vector<Solve> sv;
        for (int i = lo; i < hi; ++i)
            sv.push_back(Solve{m_vals_, m_dinv_, blk(T_, i), blk(u0, i), 2.0 / tau, 1.0});
        emit_solves(sv, d_.mass_its, d_.mass_emin, d_.mass_emax, P_, nx_);
    }
    // T_2^-1: scan from the first block up; afterwards h_u0_ holds the final u0_{lo-1}
    if (dn >= 0) emit_comm(nullptr, -1, h_u0_, dn);
    emit_time(u0, u0, 4, nloc, dn >= 0 ? h_u0_ : nullptr, nullptr);
    if (up >= 0) emit_comm(blk(u0, hi - 1), up, nullptr, -1);
    // b = T_2 (D_v u0) - b1 (2016-2048)
    {
        std::vector<Lin> ops;
        for (int i = lo; i < hi; ++i) {
            Lin l;
            l.terms.push_back(Term{mult_vals(KKT_Q10, i, i), blk(u0, i)});
            if (i >= 1)
                l.terms.push_back(Term{mult_vals(KKT_Q10, i, i - 1),
                                       i - 1 >= lo ? blk(u0, i - 1) : h_u0_});
            l.y = blk(B_, i);
            ops.push_back(l);
        }
        emit_lin(ops);
    }
    if (up >= 0 || dn >= 0) emit_comm(blk(B_, hi - 1), up, h_t_, dn);   // old values
    emit_time(B_, B_, 2, nloc, dn >= 0 ? h_t_ : nullptr, nullptr);
    {
        std::vector<Lin> ops;
        for (int i = lo; i < hi; ++i)
            ops.push_back(Lin{{}, blk(B_, i), 0.0, 1.0, -1.0, blk(B_, i), blk(b1, i)});
        emit_lin(ops);
    }
    // forward sweep (2050-2116)
    if (dn >= 0) emit_comm(nullptr, -1, h_t_, dn);
    emit_time(B_, B_, 4, nloc, dn >= 0 ? h_t_ : nullptr, nullptr);
    if (up >= 0) emit_comm(blk(B_, hi - 1), up, nullptr, -1);
    if (dn >= 0) emit_comm(nullptr, -1, h_u1_, dn);
    for (int i = lo; i < hi; ++i) {
        Mat F = schur_matrix(block_vals(KKT_Q10, i, i), c);
        const double *upd = i >= 1 ? mult_vals(KKT_Q10, i, i - 1) : nullptr;
        note_solve(KKT_PC_SWEEP_FORWARD, i, F, upd);
        const Solve sv{F.vals, F.dinv, blk(B_, i), blk(u1, i)};
        if (i >= 1) {
            const double *prev = i - 1 >= lo ? blk(u1, i - 1) : h_u1_;
            emit_update_and_solve(Lin{{Term{upd, prev},
                                       Term{cM.vals, prev}},
                                      blk(B_, i), -1.0, 1.0, 0.0, blk(B_, i), nullptr},
                                  sv, schur_its_, F.emin, F.emax, F.eimag, &F);
        } else {
            emit_solves({sv}, schur_its_, F.emin, F.emax, P_, nx_, false, nullptr, F.eimag, &F);
        }
    }
    if (up >= 0) emit_comm(blk(u1, hi - 1), up, nullptr, -1);
    // u1 = T_2 u1 (h_u1_ still holds the untransformed u1_{lo-1}); b_i = (tau/2) M u1_i
    emit_time(u1, u1, 2, nloc, dn >= 0 ? h_u1_ : nullptr, nullptr);
    {
        std::vector<Lin> ops;
        for (int i = lo; i < hi; ++i)
            ops.push_back(Lin{{Term{m_vals_, blk(u1, i)}}, blk(B_, i), 0.5 * tau});
        emit_lin(ops);
    }
    // backward sweep (2135-2189)
    if (up >= 0) emit_comm(nullptr, -1, h_u1_, up);
    for (int i = hi - 1; i >= lo; --i) {
        Mat G = schur_matrix(block_vals(KKT_Q01, i, i), c);
        // the update's matrix h K^T + (c - 1) M: only multiplied with (indefinite for c < 1)
        Mat H{};
        if (i <= n - 2) H = schur_matrix(block_vals(KKT_Q01, i, i + 1), c, false);
        note_solve(KKT_PC_SWEEP_BACKWARD, i, G, H.vals);
        const Solve sv{G.vals, G.dinv, blk(B_, i), blk(u1, i)};
        if (i <= n - 2) {
            emit_update_and_solve(Lin{{Term{H.vals, i + 1 < hi ? blk(u1, i + 1) : h_u1_}},
                                      blk(B_, i), -1.0, 1.0, 0.0, blk(B_, i), nullptr},
                                  sv, schur_its_, G.emin, G.emax, G.eimag, &G);
        } else {
            emit_solves({sv}, schur_its_, G.emin, G.emax, P_, nx_, false, nullptr, G.eimag, &G);
        }
    }
    if (dn >= 0) emit_comm(blk(u1, lo), dn, nullptr, -1);
}

void SchurPC::emit_comm(const double *send, int dst, double *recv, int src) {
    PcStep s;
    s.kind = PcStep::COMM;
    s.x = send;
    s.y = recv;
    s.dst = dst;
    s.src = src;
    s.nx = nx_;
    s.lane = cur_lane_;
    steps_.push_back(s);
}

// What a TILE step launches.  Options are read here, when it is launched: kkt_set_option may
// change "stamps", "tile_poll_delay" and "debug_drop_handoff" after the build.
TileArgs SchurPC::tile_args(const PcStep &s) const {
    const TilePlan &tp = tile_plan_;
    TileArgs a{};
    a.coarse = s.coarse ? d_tile_coarse_ : nullptr;
    a.einv = s.d_einv;
    a.cycles = s.coarse ? coarse_cycles_ : 0;
    a.cepoch0 = s.cepoch0;
    a.nlevels = s.nlevels;
    a.its = s.its;
    a.depth = tp.depth;
    a.nk_pad = tp.nk_pad;
    a.rpt = tp.rpt;
    a.W = tp.W;
    a.gnew[0] = d_tg_[0];
    a.gnew[1] = d_tg_[1];
    a.gold[0] = d_tg_[2];
    a.gold[1] = d_tg_[3];
    const size_t words = 2 * (size_t)S_.patterns[m_pat_].nrows;
    a.granule_bytes = (unsigned)(words * sizeof(unsigned long long));
    a.err = d_err_;
    a.epoch0 = s.epoch0;
    a.clear = (s.clear ? 1 : 0) | (s.clear_coarse ? 2 : 0);
    a.fused_update = s.fused ? 1 : 0;
    a.hslots = tp.hslots;
    a.stamps = S_.opts.stamps;
    a.debug_drop = S_.opts.debug_drop_handoff;
    // s_sleep units before the first poll (default 24: ~0.7 us; ~1.4 us for the big
    // rings of 3-D tiles -- measured optima: 256^2 P1 24, 64^3 P1 48)
    a.poll_delay = S_.opts.tile_poll_delay;
    return a;
}

void SchurPC::replay(size_t first, size_t last) {
    const bool xcd = S_.opts.pc_xcd;
    if (n_events_ > 0 && !side_) side_ = Stream::create();
    while ((int)events_.size() < n_events_) events_.push_back(Event::create(false));
    for (size_t k = first; k < last; ++k) {
        const PcStep &s = steps_[k];
        hipStream_t st = s.lane == 0 ? S_.stream : side_;
        switch (s.kind) {
            case PcStep::EV_RECORD:
                HIPCHK(hipEventRecord(events_[s.ev], st));
                break;
            case PcStep::EV_WAIT:
                HIPCHK(hipStreamWaitEvent(st, events_[s.ev], 0));
                break;
            case PcStep::ROWS:
                run_row_launch(st, s.rows, xcd);
                break;
            case PcStep::ROWS_IL:
                launch_rowops_il(st, s.d_il, s.il_groups, s.il_slices, s.il_w, xcd);
                break;
            case PcStep::TILE_CHEB: {
                const MassLaunch &ml = mass_launches_[s.mt];
                try {
                    launch_mass_tile(st, ml.a, mass_plan_.ntiles, ml.grid_y, mass_plan_.rpt,
                                     mass_plan_.threads);
                } catch (const TileLaunchError &e) {
                    fail(KKT_ERR_HIP, e.msg);
                }
                break;
            }
            case PcStep::TIME:
                launch_time_transform(st, s.y, s.x, s.tkind, s.n, s.nx, s.lo_halo, s.hi_halo);
                break;
            case PcStep::COPY:
                launch_copy(st, s.y, s.x, s.nx);
                break;
            case PcStep::COARSE:
                launch_coarse_correction(st, coarse_, s.einv, s.cr, s.x, s.y, s.nx);
                break;
            case PcStep::PROG: {
                const Pattern &P = S_.patterns[m_pat_];
                if (s.gmode == 2)
                    launch_row_program_gw(st, s.rows.d_ops, s.nphases, prog_nwg_, prog_wpw_, d_g0_,
                                          d_g1_, granule_words_, d_err_);
                else if (s.granule)
                    launch_row_program_g(st, s.rows.d_ops, s.d_lite, s.nphases, prog_nwg_, prog_wpw_,
                                         P.uniform_w, d_g0_, d_g1_, granule_words_, d_err_);
                else
                    launch_row_program(st, s.rows.d_ops, s.nphases, prog_nwg_, prog_wpw_, P.R,
                                       P.uniform_w, d_dep_, d_flags_, d_err_, prog_lowreg_);
                break;
            }
            case PcStep::TILE: {
                const TilePlan &tp = tile_plan_;
                const TileArgs a = tile_args(s);
                const size_t words = 2 * (size_t)S_.patterns[m_pat_].nrows;
                try {
                    launch_tile_sweep(st, a, s.d_levels, tp.d_n, tp.d_grow, tp.d_lcol, tp.d_gpos,
                                      mask_, tp.ntiles, tp.threads, words,
                                      s.coarse ? &h_tile_coarse_ : nullptr);
                } catch (const TileLaunchError &e) {
                    fail(KKT_ERR_HIP, e.msg);
                }
                break;
            }
            case PcStep::COMM:
                if (!S_.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
                S_.comm->sendrecv(s.x, s.nx, s.dst, s.y, s.nx, s.src, st);
                break;
        }
    }
}

// The program is a fixed launch sequence on fixed buffers: every maximal run of kernel
// steps between two COMM steps is captured once into a hipGraph and replayed.
void SchurPC::run() {
    hipStream_t st = S_.stream;
    if (segments_.empty()) {
        size_t k = 0;
        while (k < steps_.size()) {
            Segment g;
            g.first = k;
            if (steps_[k].kind == PcStep::COMM) {
                g.last = k + 1;
                g.comm = true;
            } else {
                size_t e = k;
                while (e < steps_.size() && steps_[e].kind != PcStep::COMM) ++e;
                g.last = e;
            }
            k = g.last;
            segments_.push_back(std::move(g));
        }
    }
    for (Segment &g : segments_) {
        if (g.comm || !use_graph_ || g.last - g.first < 4) {
            replay(g.first, g.last);
            continue;
        }
        run_captured(st, g, use_graph_, [&] { replay(g.first, g.last); });
    }
}

}  // namespace kkt
