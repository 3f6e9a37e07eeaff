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

// Shape and dependency tables of the row programs (counter and data-flow forms).
bool SchurPC::setup_row_programs() {
    const Pattern &P = S_.patterns[m_pat_];
    {
        int wpw = 0, nwg = 0;
        const ProgMode pm = S_.opts.prog_mode;
        const bool try_g0 = pm != ProgMode::Flags && row_program_g_available(P.R, P.uniform_w);
        // the data-flow form for any width (matrix re-read from L2 every phase) is opt-in
        // (prog_mode "w"): re-polling whole chunks of granules costs more fabric traffic
        // than the counter form's single gather round once rows are wide or row-sorted
        // (measured: Stokes P2 47 -> 121 ms, 3-D P1 3.3 -> 4.8 ms per application)
        const bool try_gw = pm == ProgMode::W && P.R == 2;
        const bool try_g = !try_gw && try_g0;
        // data-flow form: one wave per workgroup (no workgroup barrier on the critical path)
        // while all of them are co-resident; else 4 / 8 waves per workgroup
        const int pw = S_.opts.prog_waves;      // 0: not chosen
        const int first = pw ? pw : (try_g ? 1 : 4);
        int n_cus = 0, dev_id = 0;
        if (hipGetDevice(&dev_id) != hipSuccess ||
            hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev_id) != hipSuccess)
            n_cus = 0;
        // Multi-wave workgroups: one per CU is the shape preferred (pass 0).  Two 4-wave
        // workgroups of the data-flow form on a CU did not stay co-resident reliably (below);
        // the counter form has run that way (P2 Stokes: 259 workgroups) without a failure, so it
        // remains the fallback (pass 1) when no one-per-CU shape fits.
        for (int pass = 0; pass < 2 && !wpw; ++pass)
        for (int cand : {first, 4, 8}) {
            if (cand < 1 || cand > 8) continue;
            if (pass == 0 && cand > 1 && cand != pw &&
                (P.nslices + cand - 1) / cand > n_cus)
                continue;
            // (Round 1 fenced the data-flow form with two 4-wave workgroups on a CU off: programs
            // of about 1 000 phases on 401^2 -- 315 workgroups -- ran into the bounded spin.  Its
            // poll loop spun at full rate; an older wave that spins takes the issue slots and the
            // memory queue of the CU whose younger waves must produce what it waits for.  With
            // the back-off in the poll loop the same shape reproduces the plain launches bit
            // for bit (scripts/dbg_midsize.py 400 12 80, KKT_PROG_WAVES=4); a time-out is no
            // longer fatal either -- the step falls back to plain launches.)
            const int n = (P.nslices + cand - 1) / cand;
            int cap = row_program_max_wgs(P.R, P.uniform_w, cand);
            if (try_g) cap = std::min(cap, row_program_g_max_wgs(P.uniform_w, cand));
            if (try_gw) cap = std::min(cap, row_program_gw_max_wgs(cand));
            if (n <= cap) {
                wpw = cand;
                nwg = n;
                break;
            }
        }
        if (!wpw) {
            // more than 2 048 slices: the counter form held to 168 registers keeps three waves
            // per SIMD resident (kernels.hip, pc_row_program_lo)
            // (rows of up to 8 entries only: wider ones spill at 168 registers and run slower than
            // the plain launches -- 26.8 against 20 us per step on 64^3 P1)
            for (int cand : {4, 8}) {
                if (P.uniform_w < 1 || P.uniform_w > 8) break;
                const int n = (P.nslices + cand - 1) / cand;
                if (n <= row_program_max_wgs(P.R, P.uniform_w, cand, true)) {
                    wpw = cand;
                    nwg = n;
                    prog_lowreg_ = true;
                    break;
                }
            }
        }
        if (!wpw) return false;
        // workgroup j must wait for every workgroup whose rows it gathers from, and for
        // every workgroup that gathers from its rows (write-after-read on rotating buffers)
        const int64_t rpw = (int64_t)wpw * 64 * P.R;
        std::vector<int32_t> lo(nwg), hi(nwg);
        const int64_t npos = (int64_t)P.nslices * 64 * P.R;
        for (int j = 0; j < nwg; ++j) {
            // producers of the columns this workgroup gathers, as workgroup indices (positions
            // of the rows in the SELL storage: row-sorted structures permute them)
            int64_t wmin = j, wmax = j;
            const int64_t p1 = std::min<int64_t>(npos, (j + 1) * rpw);
            for (int64_t p = j * rpw; p < p1; ++p) {
                const int64_t r = P.row_of(p);
                if (r < 0) continue;
                for (int32_t q = P.h_indptr[r]; q < P.h_indptr[r + 1]; ++q) {
                    const int64_t w = P.pos_of(P.h_indices[q]) / rpw;
                    wmin = std::min(wmin, w);
                    wmax = std::max(wmax, w);
                }
            }
            lo[j] = (int32_t)wmin;
            hi[j] = (int32_t)std::min<int64_t>(nwg - 1, wmax);
        }
        std::vector<int32_t> slo = lo, shi = hi;
        for (int j = 0; j < nwg; ++j)
            for (int k = lo[j]; k <= hi[j]; ++k) {
                slo[k] = std::min(slo[k], (int32_t)j);
                shi[k] = std::max(shi[k], (int32_t)j);
            }
        std::vector<int32_t> dep(2 * (size_t)nwg);
        for (int j = 0; j < nwg; ++j) {
            if (shi[j] - slo[j] + 1 > 64) return false;   // one polling wave covers at most 64 neighbours
            dep[2 * j] = slo[j];
            dep[2 * j + 1] = shi[j];
        }
        // data-flow form: needs the exact gather relation between workgroups to be symmetric
        {
            const bool gw_ok = pm == ProgMode::W && P.R == 2 && nwg <= row_program_gw_max_wgs(wpw);
            const bool g_ok = !gw_ok && row_program_g_available(P.R, P.uniform_w) &&
                              nwg <= row_program_g_max_wgs(P.uniform_w, wpw);
            bool want = pm != ProgMode::Flags && (g_ok || gw_ok) && !prog_lowreg_;
            if (want) {
                // between waves (the unit that publishes and polls), in storage positions
                const int64_t rw = 64 * P.R;
                const int nw = P.nslices;
                std::vector<std::vector<int32_t>> reads(nw);
                for (int j = 0; j < nw; ++j) {
                    std::vector<char> seen(nw, 0);
                    for (int64_t p = j * rw; p < (j + 1) * rw; ++p) {
                        const int64_t r = P.row_of(p);
                        if (r < 0) continue;
                        for (int32_t q = P.h_indptr[r]; q < P.h_indptr[r + 1]; ++q)
                            seen[P.pos_of(P.h_indices[q]) / rw] = 1;
                    }
                    for (int k = 0; k < nw; ++k)
                        if (seen[k]) reads[j].push_back(k);
                }
                for (int j = 0; j < nw && want; ++j)
                    for (int32_t k : reads[j])
                        if (!std::binary_search(reads[k].begin(), reads[k].end(), (int32_t)j))
                            want = false;
            }
            prog_mode_ = want ? (g_ok ? 1 : 2) : 0;
            prog_granule_ = want;
            if (want) {
                granule_words_ = 2 * (size_t)P.nslices * 64 * P.R;
                d_g0_ = handle_mem_.alloc<unsigned long long>(granule_words_);
                d_g1_ = handle_mem_.alloc<unsigned long long>(granule_words_);
            }
        }
        prog_wpw_ = wpw;
        prog_nwg_ = nwg;
        if (S_.opts.verbose)
            std::fprintf(stderr, "[kkt] sweep program: mode %d (0 counters, 1 data-flow, 2 data-flow "
                         "any width), %d workgroups x %d waves, %d slices\n",
                         prog_mode_, nwg, wpw, P.nslices);
        d_dep_ = handle_mem_.upload(dep.data(), dep.size());
        d_flags_ = handle_mem_.alloc<unsigned>(prog_flag_words(nwg));
    }
    return true;
}

// Tile plan and granule buffers of the tile sweep program (tile_kernels.hip), once per
// preconditioner.  False when the structure does not fit (then the other forms run).
bool SchurPC::prepare_tiles() {
    if (tile_tried_) return tile_ok_;
    tile_tried_ = true;
    const Pattern &P = S_.patterns[m_pat_];
    int n_cus = 0, dev_id = 0;
    if (hipGetDevice(&dev_id) != hipSuccess ||
        hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev_id) != hipSuccess ||
        n_cus < 1)
        return false;
    const int depth = S_.opts.tile_depth;      // 0: modelled
    // one workgroup per CU; tiny meshes get fewer tiles (at least 32 own rows each)
    const int ntiles = (int)std::max<int64_t>(1, std::min<int64_t>(n_cus, P.nrows / 32));
    // workgroup size: 1 024 threads (one row slot per thread, 128 registers) or 512 (up to three
    // row slots, 256 registers) -- whichever the model prefers, unless the caller chose
    int threads = 0;
    // Dirichlet rows belong to no tile (their iterates are exactly zero)
    std::vector<uint8_t> hmask;
    if (!bc_idx_.empty()) {
        hmask.assign(P.nrows, 0);
        for (int32_t k : bc_idx_) hmask[k] = 1;
    }
    const uint8_t *hm = hmask.empty() ? nullptr : hmask.data();
    // coordinates of the rows, if the caller gave them (kkt_set_tile_coordinates)
    const double *tc = (S_.tile_dim > 0 && (int64_t)S_.tile_coords.size() == P.nrows * S_.tile_dim)
                           ? S_.tile_coords.data() : nullptr;
    const int xh = coarse_cycles_ > 0 ? 2 : 0;     // extra hand-offs per cycle of a two-grid level
    if (S_.opts.tile_waves) {
        threads = 64 * S_.opts.tile_waves;
        // (the depth model must only consider what a kernel variant exists for: wide rows have
        // one or two row slots, and a deeper plan that needs more would lose the tile form)
        if (!build_tile_plan(P, ntiles, depth, threads,
                             std::max(1, tile_sweep_max_rpt(P.max_width, threads)), tile_plan_, hm,
                             schur_its_, tc, S_.tile_dim, tile_sweep_max_hslots, xh))
            return false;
    } else {
        TilePlan big;
        const bool ok_big = tile_sweep_max_rpt(P.max_width, 1024) >= 1 &&
                            build_tile_plan(P, ntiles, depth, 1024, 1, big, hm, schur_its_, tc, S_.tile_dim,
                                            tile_sweep_max_hslots, xh) &&
                            tile_sweep_available(big.W, big.rpt, 1024, big.hslots);
        const bool ok_small = tile_sweep_max_rpt(P.max_width, 512) >= 1 &&
                              build_tile_plan(P, ntiles, depth, 512,
                                              tile_sweep_max_rpt(P.max_width, 512), tile_plan_, hm,
                                              schur_its_, tc, S_.tile_dim, tile_sweep_max_hslots, xh) &&
                              tile_sweep_available(tile_plan_.W, tile_plan_.rpt, 512, tile_plan_.hslots);
        // wide rows (P2: 19 entries) have no 1 024-thread variant -- 128 registers do not hold a
        // row -- but a 768-thread one: 12 waves with one row each instead of 8 with two
        TilePlan mid;
        const bool ok_mid = !ok_big && tile_sweep_max_rpt(P.max_width, 768) >= 1 &&
                            build_tile_plan(P, ntiles, depth, 768, 1, mid, hm, schur_its_, tc, S_.tile_dim,
                                            tile_sweep_max_hslots, xh) &&
                            tile_sweep_available(mid.W, mid.rpt, 768, mid.hslots);
        if (!ok_big && !ok_small && !ok_mid) return false;
        if (ok_mid && (!ok_small || (mid.max_rows > 512 && mid.model_us <= tile_plan_.model_us) ||
                       (coarse_cycles_ > 0 && mid.max_own > 128)))
            tile_plan_ = mid;
        // (1 024 threads only where more than 512 rows are computed: with fewer, half of the 16
        // waves never have a live row -- 32^3: 293 its/s with 512 threads, 283 with 1 024)
        // (two-grid levels: 16 waves also share the coarse exchange's work -- measured on cfg 2:
        // 1 024 threads at depth 5 118 its/s, 512 threads at depth 4 103)
        if (ok_big && (!ok_small || (big.max_rows > 512 && big.model_us <= tile_plan_.model_us) ||
                       (coarse_cycles_ > 0 && big.max_own > 128)))
            tile_plan_ = big;
        threads = tile_plan_.threads;
    }
    TilePlan &tp = tile_plan_;
    if (!tp.symmetric || !tile_sweep_available(tp.W, tp.rpt, threads, tp.hslots)) return false;
    // (solo levels of the stationary preconditioner run with mass_its, which may exceed schur_its_)
    int max_its = std::max(schur_its_, 2);
    for (const SweepLevel &lv : sweep_levels_) max_its = std::max(max_its, lv.its);
    size_t lds = tile_sweep_lds_bytes(tp.nk_pad, max_its);
    if (tp.ntiles > tile_sweep_max_tiles(tp.W, tp.rpt, threads, lds, tp.hslots)) return false;
    tile_lds_checked_ = lds;
    // two-grid levels: the variant with coarse corrections and its larger LDS footprint
    tile_coarse_ok_ = false;
    if (coarse_cycles_ > 0 && tile_sweep_coarse_available(tp.W, tp.rpt, threads, tp.hslots) &&
        build_tile_coarse()) {
        // the tiles' P entries go into LDS when everything fits in 150 KB, else they stay in memory
        // (and, room permitting, its rows of the coarse inverse: cache = 2; and the ring rows'
        // entries: the ring form).  Short of room the rings are given up before the rows of the
        // inverse (those save 6 us of an exchange, tile_kernels.hip; a hand-off costs 2-3.4) --
        // but where the rows do not fit anyway, the rings are taken if they do.
        for (int pick = 0; pick < 5 && !tile_coarse_ok_; ++pick) {
            const int cache = pick < 2 ? 2 : pick < 4 ? 1 : 0;
            const bool rings = pick == 0 || pick == 2;
            if (rings && !tile_coarse_rings_built_) continue;
            // (option "tile_coarse_cache": that level or none)
            if (S_.opts.tile_coarse_cache >= 0 && cache != S_.opts.tile_coarse_cache) continue;
            const size_t lds_c = tile_sweep_lds_bytes(tp.nk_pad, max_its, h_tile_coarse_, cache, rings);
            if (lds_c <= 150 * 1024 &&
                tp.ntiles <= tile_sweep_max_tiles(tp.W, tp.rpt, threads, lds_c, tp.hslots, true)) {
                tile_coarse_ok_ = true;
                h_tile_coarse_.cache_lists = cache >= 1;
                h_tile_coarse_.cache_einv = cache == 2;
                h_tile_coarse_.ring_prolong = rings;
                HIPCHK(hipMemcpy(d_tile_coarse_, &h_tile_coarse_, sizeof h_tile_coarse_,
                                 hipMemcpyHostToDevice));
                if (S_.opts.verbose)
                    std::fprintf(stderr, "[kkt] tile sweep program, coarse corrections: %zu bytes of "
                                 "LDS for %d sweeps (lists %s, coarse inverse rows %s), "
                                 "sweep_coarse_rings %d\n", lds_c, max_its, cache >= 1 ? "cached" : "in memory",
                                 cache == 2 ? "cached" : "in memory", (int)rings);
            }
        }
    }
    tp.upload(handle_mem_);   // once per handle (tile_tried_)
    const size_t words = 2 * (size_t)P.nrows;
    for (int i = 0; i < 4; ++i)
        d_tg_[i] = handle_mem_.alloc<unsigned long long>(words);
    if (S_.opts.verbose)
        std::fprintf(stderr, "[kkt] tile sweep program: %d tiles x %d threads, depth %d, W %d, "
                     "%d row slots per thread; largest tile: %lld own rows, %lld computed rows, "
                     "%lld ring rows; mean redundancy %.2f; modelled %.2f us per step\n", tp.ntiles,
                     threads, tp.depth, tp.W, tp.rpt, (long long)tp.max_own, (long long)tp.max_rows,
                     (long long)tp.max_halo, tp.mean_redundancy, tp.model_us);
    tile_ok_ = true;
    return true;
}

// Coarse corrections inside the tile program: the lists of tiles.cpp (build_tile_coarse_lists)
// on the device, the granule buffers of the exchanges, the column ranges of the coarse inverse.
bool SchurPC::build_tile_coarse() {
    const TilePlan &tp = tile_plan_;
    const int nt = tp.ntiles, nc = coarse_.nc;
    TileCoarseLists L;
    if (!build_tile_coarse_lists(tp, nc, p_indptr_.data(), p_indices_.data(), p_values_.data(),
                                 S_.opts.coarse_rings, L))
        return false;
    const int jmax = L.jmax, nslots = L.nslots;
    std::vector<int32_t> &nj = L.nj, &njx = L.njx, &slot0 = L.slot0, &jglob = L.jglob, &r_ip = L.r_ip,
                         &p_ip = L.p_ip, &c_ip = L.c_ip, &c_slot = L.c_slot;
    std::vector<uint16_t> &r_row = L.r_row, &p_k = L.p_k;
    std::vector<double> &r_w = L.r_w, &p_w = L.p_w;
    // handle memory: prepare_tiles() runs once per handle, and so does this
    auto up = [&](const auto &v) {
        return handle_mem_.upload(v.data(), std::max<size_t>(1, v.size()));
    };
    TileCoarseDev &D = h_tile_coarse_;
    D.nc = nc;
    D.jmax = jmax;
    D.pstride = L.pstride;
    D.nslots = nslots;
    D.nr_max = L.nr_max;
    D.jxmax = L.jxmax;
    D.np_max = L.np_max;
    D.ring_prolong = 0;           // prepare_tiles(): where the longer lists fit on chip
    tile_coarse_rings_built_ = L.rings;
    D.nj = up(nj);
    D.njx = up(njx);
    D.jglob = up(jglob);
    D.slot0 = up(slot0);
    D.r_ip = up(r_ip);
    if (r_row.empty()) r_row.push_back(0), r_w.push_back(0.0);
    D.r_row = up(r_row);
    D.r_w = up(r_w);
    D.p_ip = up(p_ip);
    if (p_k.empty()) p_k.push_back(0), p_w.push_back(0.0);
    D.p_k = up(p_k);
    D.p_w = up(p_w);
    D.c_ip = up(c_ip);
    D.c_slot = up(c_slot);
    D.cg_bytes = (uint32_t)((size_t)nslots * 16);
    D.eg_bytes = (uint32_t)((size_t)nc * 16);
    D.nown = (nc + nt - 1) / nt;
    {
        // Diagonal blocks of P^T A P (kernels.hpp, TileCoarseDev): coarse functions i and j are
        // coupled when P[r, i], A[r, s] and P[s, j] are stored entries for some rows r, s --
        // structure only, so the blocks hold for every matrix on this pattern (the Dirichlet
        // rows and columns only remove couplings).  Union-find over the coarse functions.
        const Pattern &P = S_.patterns[m_pat_];
        std::vector<int32_t> uf(nc);
        for (int j = 0; j < nc; ++j) uf[j] = j;
        auto find = [&](int32_t a) {
            while (uf[a] != a) a = uf[a] = uf[uf[a]];
            return a;
        };
        for (int64_t r = 0; r < P.nrows; ++r) {
            if (p_indptr_[r + 1] == p_indptr_[r]) continue;
            const int32_t a = find(p_indices_[p_indptr_[r]]);
            auto join = [&](int64_t row) {
                for (int32_t q = p_indptr_[row]; q < p_indptr_[row + 1]; ++q) {
                    const int32_t b = find(p_indices_[q]);
                    if (b != a) uf[b] = a;
                }
            };
            join(r);
            for (int32_t q = P.h_indptr[r]; q < P.h_indptr[r + 1]; ++q) join(P.h_indices[q]);
        }
        std::vector<int32_t> cmin(nc, nc), cmax(nc, -1), e_lo(nc), e_hi(nc);
        for (int j = 0; j < nc; ++j) {
            const int32_t c = find(j);
            cmin[c] = std::min(cmin[c], (int32_t)j);
            cmax[c] = std::max(cmax[c], (int32_t)j);
        }
        int ew = 64;
        for (int j = 0; j < nc; ++j) {
            const int32_t c = find(j);
            e_lo[j] = cmin[c] & ~63;
            e_hi[j] = cmax[c] + 1;
            ew = std::max(ew, e_hi[j] - e_lo[j]);
        }
        D.e_lo = up(e_lo);
        D.e_hi = up(e_hi);
        D.ew = ew;
        // (narrower than the whole row for some j -- also where ew, which starts at 64, is not
        // below a small nc)
        bool narrow = false;
        for (int j = 0; j < nc; ++j) narrow = narrow || e_lo[j] > 0 || e_hi[j] < nc;
        auto full_rows = [&] {
            std::fill(e_lo.begin(), e_lo.end(), 0);
            std::fill(e_hi.begin(), e_hi.end(), nc);
            D.e_lo = up(e_lo);
            D.e_hi = up(e_hi);
            D.ew = nc;
        };
        if (S_.opts.tile_coarse_full) {
            full_rows();      // option "tile_coarse_rows" = "full"
        } else if (narrow) {
            // The ranges are structure (the graph of P and the level pattern), made once per handle
            // (prepare_tiles); the inverses are formed again with every values_changed().  What
            // the block rows rely on for those later inverses is the structural argument, not a
            // check: every set-up eliminates with partial pivoting inside a matrix that is block
            // diagonal over these components -- a pivot column holds exact zeros outside its block,
            // so no row outside the block is swapped in or updated (its multiplier is an exact
            // zero, and a singular or non-finite block is refused by the set-up) -- and the
            // component-block path writes exact zeros outside each block by construction
            // (launch_coarse_block_scatter).  tests/test_gpu_tile_levels.py holds rebuilt block
            // rows to full rows and to a fresh handle bit for bit.
            // Belt and braces for the first build: every inverse formed so far is looked at, and
            // the program applies full rows if one has an entry outside its ranges.
            auto d_flag = DevBuf<unsigned>::alloc(1);
            HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(unsigned), S_.stream));
            for (const double *inv : einvs_)
                launch_einv_outside(S_.stream, inv, nc, D.e_lo, D.e_hi, d_flag.get());
            unsigned bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, d_flag.get(), sizeof bad, hipMemcpyDeviceToHost, S_.stream));
            HIPCHK(hipStreamSynchronize(S_.stream));
            if (bad) {
                std::fprintf(stderr, "[kkt] coarse inverse: entries outside the diagonal blocks of its "
                             "structure -- the tile program applies full rows\n");
                full_rows();
            }
        }
        tile_e_lo_ = e_lo;
        tile_e_hi_ = e_hi;
        if (S_.opts.verbose)
            std::fprintf(stderr, "[kkt] coarse inverse: rows of at most %d of %d columns (diagonal "
                         "blocks of P^T A P)\n", D.ew, nc);
    }
    for (int i = 0; i < 2; ++i) {
        D.cg[i] = handle_mem_.alloc<unsigned long long>((size_t)nslots * 2);
        HIPCHK(hipMemset(D.cg[i], 0, D.cg_bytes));
        D.eg[i] = handle_mem_.alloc<unsigned long long>((size_t)nc * 2);
        HIPCHK(hipMemset(D.eg[i], 0, D.eg_bytes));
    }
    d_tile_coarse_ = handle_mem_.upload(&D, 1);
    if (S_.opts.verbose)
        std::fprintf(stderr, "[kkt] tile sweep program, coarse corrections: %d coarse functions, at most "
                     "%d per tile (%d with the rings'), %d partial-sum slots; prolongation entries of a "
                     "tile: at most %d on own rows, %d with the rings (%s)\n", nc, jmax, L.jxmax,
                     nslots, L.nr_max, L.np_max,
                     L.rings ? "lists with rings" : S_.opts.coarse_rings ? "no rings: long rows of P"
                                                                         : "no rings: coarse_rings = 0");
    return true;
}

// Steps [k, e) are single-block steps: if they are exactly a run of recorded sweep levels the
// tile form can express, replace them by one TILE step.
bool SchurPC::fuse_tile_run(size_t k, size_t e, std::vector<PcStep> &out) {
    std::vector<const SweepLevel *> run;
    size_t cursor = k;
    while (cursor < e) {
        const SweepLevel *hit = nullptr;
        for (const SweepLevel &lv : sweep_levels_)
            if (lv.first == cursor) hit = &lv;
        if (!hit || !hit->eligible || hit->last > e) return false;
        run.push_back(hit);
        cursor = hit->last;
    }
    if (run.empty()) return false;
    const int its = run[0]->its;
    const bool coarse = run[0]->coarse;
    if (coarse && !tile_coarse_ok_) return false;
    {
        // residency and the dynamic-LDS attribute were checked for tile_lds_checked_ bytes
        const size_t need = coarse ? tile_sweep_lds_bytes(tile_plan_.nk_pad, its, h_tile_coarse_)
                                   : tile_sweep_lds_bytes(tile_plan_.nk_pad, its);
        if (need > tile_lds_checked_) {
            if (need > 150 * 1024 ||
                tile_plan_.ntiles > tile_sweep_max_tiles(tile_plan_.W, tile_plan_.rpt,
                                                         tile_plan_.threads, need, tile_plan_.hslots,
                                                         coarse))
                return false;
            tile_lds_checked_ = need;
        }
    }
    std::vector<TileLevel> levels;
    for (size_t i = 0; i < run.size(); ++i) {
        const SweepLevel &lv = *run[i];
        if (lv.its != its || lv.coarse != coarse ||
            (int)lv.coef.size() != (coarse ? its : its - 1))
            return false;
        TileLevel L = lv.lev;
        L.prev_in_lds = 0;
        // operands read from plain memory must not be produced inside this launch
        for (size_t j = 0; j < run.size(); ++j) {
            const TileLevel &o = run[j]->lev;
            if (L.bin == o.out || L.dinv == o.out) return false;
            if (j != i && o.bout && (L.bin == o.bout)) return false;
            if (L.n_upd > 0 && L.x_prev == o.out) {
                if (j + 1 != i) return false;       // only the previous level's result is on chip
                L.prev_in_lds = 1;
            }
            if (L.n_upd > 0 && o.bout && L.x_prev == o.bout) return false;
        }
        // identical coefficient tables share one device copy
        TileCoef *d_coef = nullptr;
        for (size_t j = 0; j < i && !d_coef; ++j)
            if (run[j]->coef.size() == lv.coef.size() &&
                std::memcmp(run[j]->coef.data(), lv.coef.data(), lv.coef.size() * sizeof(TileCoef)) == 0)
                d_coef = const_cast<TileCoef *>(levels[j].coef);
        if (!d_coef) d_coef = program_mem_.upload(lv.coef.data(), lv.coef.size());
        L.coef = d_coef;
        levels.push_back(L);
    }
    // hand-offs of a level, at most (two-grid levels: per cycle one after the correction, one in
    // front of the residual, those of the sweeps; one at the level's end)
    const int per_launch = coarse ? coarse_cycles_ * (its / std::max(1, tile_plan_.depth) + 3) + 2
                                  : its / std::max(1, tile_plan_.depth) + 2;
    std::vector<const double *> einvs;
    for (const SweepLevel *lv : run) einvs.push_back(lv->einv);
    auto tile_step = [&](const TileLevel *lv, int n, int nphases, bool fused) {
        PcStep s;
        s.kind = PcStep::TILE;
        s.fused = fused;
        s.coarse = coarse;
        if (coarse) {
            s.d_einv = program_mem_.upload(einvs.data(), einvs.size());
            s.cepoch0 = tile_cepoch_cursor_;
            tile_cepoch_cursor_ += (uint32_t)(n * coarse_cycles_);
        }
        s.d_levels = program_mem_.upload(lv, (size_t)n);
        s.nlevels = n;
        s.its = its;
        s.nphases = nphases;
        s.epoch0 = tile_epoch_cursor_;
        s.clear = !tile_cleared_;
        tile_cleared_ = true;
        // the coarse exchanges' buffers with the first launch that uses them: on a one-level time
        // shard the first tile launch of an application is the mass solve, without coarse levels
        s.clear_coarse = coarse && !tile_coarse_cleared_;
        tile_coarse_cleared_ = tile_coarse_cleared_ || coarse;
        tile_epoch_cursor_ += (uint32_t)(n * per_launch);
        out.push_back(s);
    };
    int max_terms = 0;
    for (const TileLevel &L : levels) max_terms = std::max(max_terms, (int)L.n_upd);
    if (coarse && !tile_sweep_fuses_update(tile_plan_.W, max_terms)) return false;
    if (tile_sweep_fuses_update(tile_plan_.W, max_terms) &&
        !(tile_plan_.W > 9 && S_.opts.tile_unfused && !coarse)) {
        // the RowOp arrays of the steps this launch replaces (a few hundred bytes per step) stay
        // in the program's memory until the next clear_program()
        tile_step(levels.data(), (int)levels.size(), (int)(e - k), true);
        return true;
    }
    // Wide rows: the kernel has no registers for the level update.  It stays the plain launch it
    // was (it also leaves p_1, which the tile launch recomputes from the same right-hand side),
    // and every level's Chebyshev steps become a tile launch of their own; the hand-off tags
    // keep counting through the launches of an application.
    for (size_t i = 0; i < run.size(); ++i) {
        const SweepLevel &lv = *run[i];
        TileLevel L = levels[i];
        size_t first_cheb = lv.first;
        if (L.n_upd > 0) {
            out.push_back(steps_[lv.first]);         // the update, as a plain single-block step
            first_cheb = lv.first + 1;
            L.n_upd = 0;
            L.prev_in_lds = 0;
            L.bin = lv.b_after;
            L.bout = nullptr;
        }
        tile_step(&L, 1, (int)(lv.last - first_cheb), false);
    }
    return true;
}

// Replace every run of >= 4 consecutive single-block steps (the time sweeps) by one
// persistent launch: the tile form (tile_kernels.hip: `depth` steps per hand-off) where it
// fits, else a row program with neighbour synchronisation (kernels.hip, pc_row_program*).
// Tile plan of the batched one-matrix solves (mass_tile_kernels.hip): once per handle.  Its own
// tile count and depth K -- the sweeps' plan (one tile per CU, a few hundred rows) computes 2.25 x
// the rows at depth 4 and is the wrong shape here.
bool SchurPC::prepare_mass_tiles() {
    if (mass_tried_) return mass_ok_;
    mass_tried_ = true;
    const Pattern &P = S_.patterns[m_pat_];
    if (P.R != 2 || mass_tile_kernel_width(P.max_width) == 0) return false;
    int dev_id = 0;
    if (hipGetDevice(&dev_id) != hipSuccess ||
        hipDeviceGetAttribute(&mass_cus_, hipDeviceAttributeMultiprocessorCount, dev_id) != hipSuccess ||
        mass_cus_ < 1)
        return false;
    std::vector<uint8_t> hmask;
    if (!bc_idx_.empty()) {
        hmask.assign(P.nrows, 0);
        for (int32_t k : bc_idx_) hmask[k] = 1;
    }
    int64_t live = 0;
    for (int64_t r = 0; r < P.nrows; ++r) live += hmask.empty() || !hmask[r];
    if (live < 1) return false;
    const double *tc = (S_.tile_dim > 0 && (int64_t)S_.tile_coords.size() == P.nrows * S_.tile_dim)
                           ? S_.tile_coords.data() : nullptr;
    // defaults: what won on 256^2 P1 x 64 levels among K = 2 .. 6 and 192 .. 1 024 own rows
    // (profiles/mass_tiles.md): 5 steps on tiles of 512 rows, 256 threads with four row slots, two
    // workgroups per CU
    const bool chosen = S_.opts.mass_tile_depth > 0 || S_.opts.mass_tile_rows > 0;
    const int K = S_.opts.mass_tile_depth > 0 ? S_.opts.mass_tile_depth : 5;
    const int rows = S_.opts.mass_tile_rows > 0 ? S_.opts.mass_tile_rows : 512;
    const int ntiles = (int)std::max<int64_t>(1, (live + rows - 1) / rows);
    // the rings are loaded by a loop, not by slots per thread: no limit on their size
    auto any_halo = [](int, int, int) { return 1 << 20; };
    bool ok = false;
    for (int threads : {256, 512}) {
        if (S_.opts.mass_tile_waves && threads != 64 * S_.opts.mass_tile_waves) continue;
        if (build_tile_plan(P, ntiles, K, threads, mass_tile_max_rpt(threads), mass_plan_,
                            hmask.empty() ? nullptr : hmask.data(), 0, tc, S_.tile_dim, any_halo)) {
            ok = true;
            break;
        }
    }
    if (!ok) return false;
    const TilePlan &tp = mass_plan_;
    const size_t lds = mass_tile_lds_bytes(tp.nk_pad);
    mass_per_cu_ = mass_tile_prepare(tp.W, tp.rpt, tp.threads, lds);
    if (mass_per_cu_ < 1) return false;
    // Cost rule: bytes a launch of K steps moves per tile and level group -- two iterates on
    // n[K] rows in, the right-hand sides on n[K-1] rows, two iterates on the own rows out, 32 bytes
    // per row and group each -- against K plain steps at 40 bytes per unknown.  The form also pays
    // the redundant rows' LDS gathers, so it must move less than 0.6 of the plain bytes.
    // (a caller who sets the depth or the tile size has chosen: the rule is not asked)
    double tile_bytes = 0.0, plain_bytes = 0.0;
    for (int t = 0; t < tp.ntiles; ++t) {
        const int32_t *nt = &tp.n[(size_t)t * (TILE_MAX_DEPTH + 1)];
        tile_bytes += 64.0 * nt[K] + 32.0 * nt[K - 1] + 64.0 * nt[0];
        plain_bytes += 160.0 * K * nt[0];
    }
    const double ratio = tile_bytes / std::max(1.0, plain_bytes);
    const bool pays = ratio < 0.6;
    if (S_.opts.verbose)
        std::fprintf(stderr, "[kkt] mass tile form: %d tiles x %d threads, K %d, W %d, %d row slots; "
                     "largest tile: %lld own rows, %lld computed rows; redundancy %.2f; %zu bytes of "
                     "LDS, %d workgroups per CU; modelled bytes %.2f of the plain steps'%s\n",
                     tp.ntiles, tp.threads, K, tp.W, tp.rpt, (long long)tp.max_own,
                     (long long)tp.max_rows, tp.mean_redundancy, lds, mass_per_cu_, ratio,
                     pays || chosen ? "" : ": off");
    if (!pays && !chosen) return false;
    mass_plan_.upload(handle_mem_);
    if (!bc_idx_.empty()) d_masked_ = handle_mem_.upload(bc_idx_.data(), bc_idx_.size());
    mass_ok_ = true;
    return true;
}

// The values of a matrix in the order the tile kernels read them: gathered once per value array.
const double *SchurPC::mass_tile_values(const double *vals) {
    for (const MassTileValues &c : mass_vals_)
        if (c.vals == vals) return c.copy;
    const TilePlan &tp = mass_plan_;
    const size_t n = tp.gpos.size();
    double *copy = (vals == m_vals_ ? handle_mem_ : program_mem_).alloc<double>(n);
    launch_mass_tile_gather(S_.stream, vals, tp.d_gpos, copy, (int64_t)n);
    mass_vals_.push_back(MassTileValues{vals, copy});
    return copy;
}

// Replace every run of ROWS_IL steps of one batched solve by ceil(its / K) TILE_CHEB steps.
void SchurPC::fuse_mass_tiles() {
    if (!S_.opts.mass_tiles || S_.opts.lanes || mass_solves_.empty()) return;
    bool any = false;
    for (const MassSolve &ms : mass_solves_) any = any || ms.its >= 2;
    if (!any || !prepare_mass_tiles()) return;
    const TilePlan &tp = mass_plan_;
    const int K = tp.depth;
    std::vector<PcStep> out;
    std::vector<size_t> new_index(steps_.size() + 1, 0);
    size_t k = 0, q = 0;
    while (k < steps_.size()) {
        while (q < mass_solves_.size() && mass_solves_[q].first < k) ++q;
        const MassSolve *ms = q < mass_solves_.size() && mass_solves_[q].first == k ? &mass_solves_[q] : nullptr;
        bool run = ms && ms->its >= 2 && k + ms->its <= steps_.size();
        for (int i = 0; run && i < ms->its; ++i) run = steps_[k + i].kind == PcStep::ROWS_IL;
        if (!run) {
            new_index[k] = out.size();
            out.push_back(steps_[k++]);
            continue;
        }
        const size_t m = ms->sv.size();
        const int ng = (int)((m + 3) / 4);
        const size_t need = (size_t)ng * 4 * (size_t)nx_;
        if (need > mt_cap_) {
            for (int i = 0; i < 4; ++i) {
                mt_P_[i] = program_mem_.alloc<double>(need + 32);
                HIPCHK(hipMemsetAsync(mt_P_[i], 0, (need + 32) * sizeof(double), S_.stream));
            }
            mt_cap_ = need;
        }
        std::vector<MassTileGroup> groups(ng);
        for (int g = 0; g < ng; ++g) {
            MassTileGroup G{};
            G.nlev = (int32_t)std::min<size_t>(4, m - (size_t)g * 4);
            for (int l = 0; l < 4; ++l) {
                const bool live = l < G.nlev;
                const Solve *sv = live ? &ms->sv[(size_t)g * 4 + l] : nullptr;
                G.b[l] = live ? sv->b : nullptr;
                G.out[l] = live ? sv->out : nullptr;
                G.post1[l] = live ? sv->post1 : 1.0;
                G.post2[l] = live ? sv->post2 : 1.0;
            }
            groups[g] = G;
        }
        const MassTileGroup *d_groups = program_mem_.upload(groups.data(), groups.size());
        // level groups per workgroup: as many workgroups as the chip holds at once, unless chosen
        int gpw = S_.opts.mass_tile_levels > 0 ? (S_.opts.mass_tile_levels + 3) / 4 : 0;
        if (gpw <= 0) {
            const int64_t slots = (int64_t)mass_per_cu_ * mass_cus_;
            const int gy = (int)std::max<int64_t>(1, std::min<int64_t>(ng, slots / tp.ntiles));
            gpw = (ng + gy - 1) / gy;
        }
        const double *tvals = mass_tile_values(ms->sv[0].vals);
        const int grid_y = (ng + gpw - 1) / gpw;
        const int nl = (ms->its + K - 1) / K;
        for (int i = 0; i < ms->its; ++i) new_index[k + i] = out.size();
        for (int j = 0; j < nl; ++j) {
            MassLaunch ml;
            MassTileArgs &a = ml.a;
            a = MassTileArgs{};
            a.n = tp.d_n;
            a.grow = tp.d_grow;
            a.lcol = tp.d_lcol;
            a.masked = d_masked_;
            a.nmasked = (int32_t)bc_idx_.size();
            a.tvals = tvals;
            a.dinv = ms->sv[0].dinv;
            a.groups = d_groups;
            const int wr = j & 1, rd = wr ^ 1;
            a.in_new = mt_P_[2 * rd];
            a.in_old = mt_P_[2 * rd + 1];
            a.out_new = mt_P_[2 * wr];
            a.out_old = mt_P_[2 * wr + 1];
            a.nx = nx_;
            a.ngroups = ng;
            a.nk_pad = tp.nk_pad;
            a.W = tp.W;
            a.s0 = j * K;
            a.k = std::min(K, ms->its - a.s0);
            a.last = j + 1 == nl ? 1 : 0;
            for (int i = 0; i < a.k; ++i) {
                const TileCoef &c = ms->coef[a.s0 + i];
                a.coef[i][0] = c.c1;
                a.coef[i][1] = c.c2;
                a.coef[i][2] = c.c3;
            }
            ml.grid_y = grid_y;
            PcStep s;
            s.kind = PcStep::TILE_CHEB;
            s.mt = (int)mass_launches_.size();
            s.lane = steps_[k].lane;
            mass_launches_.push_back(ml);
            out.push_back(s);
        }
        if (S_.opts.verbose)
            std::fprintf(stderr, "[kkt] mass tile form: a solve of %d steps on %zu levels as %d "
                         "launches of %d x %d workgroups (%d level groups each)\n", ms->its, m, nl,
                         tp.ntiles, grid_y, gpw);
        k += ms->its;
    }
    new_index[steps_.size()] = out.size();
    // (the sweep levels name their steps by index)
    for (SweepLevel &lv : sweep_levels_) {
        lv.first = new_index[lv.first];
        lv.last = new_index[lv.last];
    }
    steps_.swap(out);
}

void SchurPC::fuse_programs() {
    if (!use_programs_) return;
    fuse_mass_tiles();
    if (!d_err_) {
        d_err_ = handle_mem_.alloc<unsigned>(64 + 16 * 1024);   // word 0: error bits; rest: diagnostics
        HIPCHK(hipMemset(d_err_, 0, (64 + 16 * 1024) * sizeof(unsigned)));
    }
    const bool tile_wanted = S_.opts.prog_mode == ProgMode::Auto || S_.opts.prog_mode == ProgMode::Tile;
    const bool use_tiles = tile_wanted && prepare_tiles();
    tile_epoch_cursor_ = 0;
    tile_cepoch_cursor_ = 0;
    tile_cleared_ = false;
    tile_coarse_cleared_ = false;
    if (!legacy_tried_) {
        legacy_tried_ = true;
        legacy_ok_ = setup_row_programs();
    }
    if (!use_tiles && !legacy_ok_) {
        use_programs_ = false;
        return;
    }
    // output pointer the next phase may gather from
    auto gather_out = [](const RowOp &op) -> int64_t {
        return (op.mode == EPI_LIN && op.y2.base >= 0) ? op.y2.off : op.y.off;
    };
    std::vector<PcStep> out;
    // one row program for the single-block steps [q0, q1)
    auto emit_prog = [&](size_t q0, size_t q1) {
        std::vector<RowOp> ops;
        // (the replaced steps' own RowOp arrays stay in the program's memory, as above)
        for (size_t q = q0; q < q1; ++q) ops.push_back(steps_[q].rows.h_op);
        PcStep s;
        s.kind = PcStep::PROG;
        s.rows.d_ops = program_mem_.upload(ops.data(), ops.size());
        s.nphases = (int)ops.size();
        {
            // compact records: Chebyshev steps that only continue the previous phase's
            // solve are marked STEP (kernels.hpp, PhaseLite)
            std::vector<PhaseLite> lite(ops.size());
            const bool use_steps = S_.opts.prog_steps;
            auto same = [](const VRef &a, const VRef &b) {
                return a.base == b.base && (a.base < 0 || a.off == b.off);
            };
            for (size_t e2 = 0; e2 < ops.size(); ++e2) {
                const RowOp &op = ops[e2];
                PhaseLite L{};
                L.kind = 0;
                if (use_steps && e2 >= 1) {
                    const RowOp &pv = ops[e2 - 1];
                    const bool has_pkm1 = op.pkm1.base >= 0;
                    bool stepk = op.mode == EPI_CHEB && pv.mode == EPI_CHEB &&
                                 op.nterms == 1 && pv.nterms == 1 &&
                                 op.t[0].vals == pv.t[0].vals && op.col == pv.col &&
                                 op.rowmask == pv.rowmask && op.dinv == pv.dinv &&
                                 op.nslices == pv.nslices && op.nrows == pv.nrows &&
                                 same(op.b, pv.b) && op.b.base == 0 && op.y.base == 0 &&
                                 op.pk.base == 0 && same(op.pk, pv.y) &&
                                 same(op.t[0].x, pv.y) &&
                                 (!has_pkm1 || (pv.pk.base == 0 && same(op.pkm1, pv.pk)));
                    if (stepk) {
                        L.kind = 1;
                        L.flags = has_pkm1 ? 1u : 0u;
                        L.y = (uint64_t)op.y.off;
                        L.c1 = op.c1;
                        L.c2 = op.c2;
                        L.c3 = op.c3;
                        L.post1 = op.post1;
                        L.post2 = op.post2;
                    }
                }
                lite[e2] = L;
            }
            s.d_lite = program_mem_.upload(lite.data(), lite.size());
        }
        s.granule = prog_granule_;
        s.gmode = prog_mode_;
        out.push_back(s);
    };
    // single-block steps [a, b) outside the tile form: two-grid levels stay plain launches, the
    // rest becomes row programs
    auto emit_rest = [&](size_t a, size_t b) {
        if (a >= b) return;
        bool has_coarse = false;
        for (size_t i = a; i < b; ++i) has_coarse = has_coarse || steps_[i].kind == PcStep::COARSE;
        if (has_coarse) {
            for (size_t i = a; i < b; ++i) out.push_back(steps_[i]);
            return;
        }
        // the data-flow form needs phase ph >= 1 to gather exactly what phase ph - 1 produced,
        // so a run is cut where that chain breaks
        size_t q = a;
        while (q < b) {
            size_t q1 = q + 1;
            while (q1 < b) {
                if (prog_granule_ && legacy_ok_) {
                    const RowOp &op = steps_[q1].rows.h_op, &prev = steps_[q1 - 1].rows.h_op;
                    bool chain = op.nterms > 0;
                    for (int t = 0; t < op.nterms; ++t)
                        chain &= op.t[t].x.base == 0 && op.t[t].x.off == gather_out(prev);
                    if (!chain) break;
                }
                ++q1;
            }
            if (q1 - q >= 4 && legacy_ok_)
                emit_prog(q, q1);
            else
                for (size_t i = q; i < q1; ++i) out.push_back(steps_[i]);
            q = q1;
        }
    };
    // the recorded sweep level that starts at step c and ends inside the run, if the tile form takes it
    auto level_at = [&](size_t c, size_t e) -> const SweepLevel * {
        for (const SweepLevel &lv : sweep_levels_)
            if (lv.first == c && lv.eligible && lv.last > c && lv.last <= e) return &lv;
        return nullptr;
    };
    size_t k = 0;
    while (k < steps_.size()) {
        size_t e = k;
        // (the coarse corrections of two-grid levels sit between the single-block steps)
        while (e < steps_.size() && ((steps_[e].kind == PcStep::ROWS && steps_[e].rows.nops == 1) ||
                                     steps_[e].kind == PcStep::COARSE))
            ++e;
        if (e == k) {
            out.push_back(steps_[k++]);
            continue;
        }
        if (e - k >= 4 && use_tiles && fuse_tile_run(k, e, out)) {
            k = e;
            continue;
        }
        if (use_tiles && S_.sharded) {
            // A rank with ONE level: the products between the sweeps have one op, so they are
            // single-block steps of the same run as a sweep level wherever no hand-off separates
            // them (rank 0 in front of the forward level, the last rank between the sweeps).  Every
            // stretch of levels inside the run still becomes a tile launch, the steps between them
            // stay what they were.
            size_t pend = k, c = k;
            while (c < e) {
                size_t c2 = c;
                while (const SweepLevel *lv = level_at(c2, e)) c2 = lv->last;
                std::vector<PcStep> tiles;
                if (c2 - c >= 4 && fuse_tile_run(c, c2, tiles)) {
                    emit_rest(pend, c);
                    out.insert(out.end(), tiles.begin(), tiles.end());
                    pend = c = c2;
                } else {
                    c = std::max(c2, c + 1);
                }
            }
            emit_rest(pend, e);
        } else {
            emit_rest(k, e);
        }
        k = e;
    }
    steps_.swap(out);
    // what runs, for the caller's records (kkt_info)
    int form = 0;
    for (const PcStep &s : steps_) {
        if (s.kind == PcStep::TILE) form = 3;
        if (s.kind == PcStep::PROG && form < 3) form = std::max(form, s.granule ? 2 : 1);
    }
    S_.info.sweep_form = form;
    S_.info.sweep_tiles = form == 3 ? tile_plan_.ntiles : 0;
    S_.info.sweep_threads = form == 3 ? tile_plan_.threads : 0;
    S_.info.sweep_depth = form == 3 ? tile_plan_.depth : 0;
    S_.info.sweep_row_slots = form == 3 ? tile_plan_.rpt : 0;
    bool rings = false, two_grid = false;
    for (const PcStep &s : steps_)
        if (s.kind == PcStep::TILE && s.coarse) {
            two_grid = true;
            rings = h_tile_coarse_.ring_prolong != 0;
        }
    S_.info.sweep_coarse_rings = rings ? 1 : 0;
    S_.info.sweep_coarse_cache =
        !two_grid ? 0 : h_tile_coarse_.cache_einv ? 2 : h_tile_coarse_.cache_lists ? 1 : 0;
    S_.info.sweep_coarse_ew = two_grid ? h_tile_coarse_.ew : 0;
}

// The form replay() gives each row step, sweep program and tile launch (kkt_debug_pc_forms)
void SchurPC::plain_forms(std::vector<int32_t> &out) const {
    const Pattern &P = S_.patterns[m_pat_];
    for (const PcStep &s : steps_) {
        if (s.kind == PcStep::ROWS) {
            const RowFamily f = row_launch_kernel(s.rows).family;
            const int form = f == ROW_PC_ROWS       ? KKT_PC_ROWS_PLAIN
                             : f == ROW_PC_ROW_STEP ? KKT_PC_ROWS_KERNARG
                                                    : KKT_PC_ROWS_SHARED;
            out.insert(out.end(), {form, s.rows.uniform_w, s.rows.R, s.lane, s.rows.nops, 0});
        } else if (s.kind == PcStep::ROWS_IL) {
            out.insert(out.end(), {KKT_PC_ROWS_INTERLEAVED, s.il_w, 2, s.lane, s.il_groups, 0});
        } else if (s.kind == PcStep::TILE_CHEB) {
            out.insert(out.end(), {KKT_PC_TILE_CHEB, mass_plan_.W, mass_plan_.rpt, s.lane,
                                   mass_launches_[s.mt].a.k, mass_plan_.threads});
        } else if (s.kind == PcStep::PROG) {
            out.insert(out.end(), {KKT_PC_PROGRAM, P.uniform_w, P.R, s.lane, s.nphases,
                                   s.gmode == 2 ? 2 : s.granule ? 1 : 0});
        } else if (s.kind == PcStep::TILE) {
            out.insert(out.end(), {KKT_PC_TILE, tile_plan_.W, tile_plan_.rpt, s.lane,
                                   tile_plan_.threads, (s.fused ? 1 : 0) | (s.coarse ? 2 : 0)});
        }
    }
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

int coarse_block_size(int nc, const std::vector<int32_t> &e_ip, const std::vector<int32_t> &e_ix) {
    std::vector<int32_t> uf(nc);
    for (int j = 0; j < nc; ++j) uf[j] = j;
    auto find = [&](int32_t a) {
        while (uf[a] != a) a = uf[a] = uf[uf[a]];
        return a;
    };
    for (int i = 0; i < nc; ++i)
        for (int32_t e = e_ip[i]; e < e_ip[i + 1]; ++e) {
            const int32_t a = find(i), b = find(e_ix[e]);
            if (a != b) uf[std::max(a, b)] = std::min(a, b);
        }
    int b = 1;
    while (b < nc && find(b) == find(0)) ++b;
    if (b >= nc || nc % b != 0) return 0;
    // every block one component of its own: [k b, (k+1) b) all joined to k b, the k b distinct
    std::vector<int32_t> root(nc / b);
    for (int k = 0; k < nc / b; ++k) root[k] = find(k * b);
    for (int i = 0; i < nc; ++i)
        if (find(i) != root[i / b]) return 0;
    std::sort(root.begin(), root.end());
    if (std::adjacent_find(root.begin(), root.end()) != root.end()) return 0;
    return b;
}

void galerkin_structure(int nc, const std::vector<int32_t> &pt_ip, const std::vector<int32_t> &pt_ix,
                        const std::vector<int32_t> &a_ip, const std::vector<int32_t> &a_ix,
                        const std::vector<int32_t> &p_ip, const std::vector<int32_t> &p_ix,
                        std::vector<int32_t> &e_ip, std::vector<int32_t> &e_ix) {
    std::vector<int32_t> seen(nc, -1), row;
    e_ip.assign(1, 0);
    e_ix.clear();
    for (int i = 0; i < nc; ++i) {
        row.clear();
        for (int32_t q = pt_ip[i]; q < pt_ip[i + 1]; ++q) {
            const int32_t r = pt_ix[q];
            for (int32_t t = a_ip[r]; t < a_ip[r + 1]; ++t) {
                const int32_t c = a_ix[t];
                for (int32_t u = p_ip[c]; u < p_ip[c + 1]; ++u) {
                    const int32_t k = p_ix[u];
                    if (seen[k] != i) {
                        seen[k] = i;
                        row.push_back(k);
                    }
                }
            }
        }
        std::sort(row.begin(), row.end());
        e_ix.insert(e_ix.end(), row.begin(), row.end());
        e_ip.push_back((int32_t)e_ix.size());
    }
}

// The column path (option "coarse_setup" = "columns"): E = P^T A P column by column with the
// kernels the sweeps use (x = column k of P, y = A x with the masked rows zero, E(:, k) = P^T y),
// inverted by Gauss-Jordan with partial pivoting, four launches per pivot.  Returns the launches.
static int64_t coarse_columns(System &S, const Pattern &P, const CoarseDev &c, const uint8_t *mask,
                              const double *vals, double *E, double *einv, unsigned *d_flag,
                              bool deflate, double *h_keep) {
    hipStream_t st = S.stream;
    const int nc = c.nc;
    const int64_t n = P.nrows;
    DevPool tmp;   // released on every way out
    double *x = tmp.alloc<double>(n + 32), *y = tmp.alloc<double>(n + 32);
    const RowOp op = lin_op(P, n, mask, LinStep{{RowTerm{vals, x}}, y});
    RowOp *d_op = tmp.upload(&op, 1);
    const Bases B{{nullptr, nullptr, nullptr, nullptr}};
    for (int k = 0; k < nc; ++k) {
        launch_coarse_column(st, c, k, x, n);
        launch_rowops(st, d_op, 1, P.nslices, P.R, B, 1, P.uniform_w);
        launch_coarse_restrict(st, c, y, E + k, nc);     // column k of the row-major E
    }
    int64_t launches = 4 * (int64_t)nc;     // launch_coarse_column: a zero fill and a scatter
    if (h_keep)
        HIPCHK(hipMemcpyAsync(h_keep, E, (size_t)nc * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (deflate) {
        std::vector<double> diag(nc);
        HIPCHK(hipMemcpy2DAsync(diag.data(), sizeof(double), E, ((size_t)nc + 1) * sizeof(double),
                                sizeof(double), nc, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double tr = 0.0;
        for (double v : diag) tr += v;
        launch_add_constant(st, E, tr / ((double)nc * (double)nc), (int64_t)nc * nc);
        launches += 1;
    }
    int *d_piv = tmp.alloc<int>(1);
    double *d_colbuf = tmp.alloc<double>(nc + 1);     // multipliers; slot nc: the pivot
    launch_dense_inverse(st, E, einv, nc, d_piv, d_colbuf, d_flag);
    launches += 1 + 4 * (int64_t)nc;
    HIPCHK(hipStreamSynchronize(st));
    return launches;
}

void coarse_setup(System &S, int pat, const CoarseDev &c, const GalerkinDev &g,
                  const std::vector<const double *> &vals, const std::vector<double *> &einv,
                  bool deflate, const char *what) {
    const Pattern &P = S.patterns[pat];
    hipStream_t st = S.stream;
    const int nc = c.nc, nmat = (int)vals.size();
    const size_t n2 = (size_t)nc * nc;
    S.coarse_stats = kkt_coarse_stats{};
    const bool keep = S.opts.coarse_keep;
    S.coarse_E.clear();
    S.coarse_Einv.clear();
    if (nmat == 0) return;
    if (keep) S.coarse_E.resize(n2 * nmat);
    const bool columns = S.opts.coarse_columns;
    HIPCHK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    int64_t launches = 0;
    std::vector<int> bad(nmat, nc);
    if (columns) {
        DevPool tmp;
        double *E = tmp.alloc<double>(n2);
        unsigned *d_flag = tmp.alloc<unsigned>(1);
        for (int b = 0; b < nmat; ++b) {
            HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
            launches += coarse_columns(S, P, c, g.mask, vals[b], E, einv[b], d_flag, deflate,
                                       keep ? S.coarse_E.data() + b * n2 : nullptr);
            unsigned singular = 0;
            HIPCHK(hipMemcpyAsync(&singular, d_flag, sizeof singular, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (singular) bad[b] = -1;      // this path does not know the column
        }
    } else {
        // component blocks: the Galerkin launch writes the nblk diagonal blocks of size bn as
        // matrices of their own (E: nmat * nblk of them), the inverses go to Ib and are scattered
        // into einv's full rows
        const bool blocked = !deflate && g.block_n > 0 && g.block_n < nc && nc % g.block_n == 0 &&
                             S.opts.coarse_blocks;
        const int bn = blocked ? g.block_n : nc, nblk = nc / bn;
        const size_t b2 = (size_t)bn * bn, ne = nblk * b2;     // doubles of E per level matrix
        GalerkinDev gb = g;
        gb.block_n = blocked ? bn : 0;
        // chunks of at most ~1 GiB of Galerkin matrices and scratch (Picard: one matrix per level)
        const size_t per = (blocked ? 2 : 1) * ne * sizeof(double) +
                           dense_inverse_batched_scratch(bn, nblk);
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>(nmat, ((size_t)1 << 30) / per));
        DevPool tmp;
        double *E = tmp.alloc<double>(ne * chunk);
        const double **d_vals = tmp.alloc<const double *>(chunk);
        double **d_inv = tmp.alloc<double *>(chunk);
        void *scratch = tmp.alloc<char>(dense_inverse_batched_scratch(bn, nblk * chunk));
        int *d_bad = tmp.alloc<int>((size_t)nblk * chunk);
        double *Ib = nullptr, **d_binv = nullptr;
        std::vector<int> bad_blk;
        std::vector<double> h_blocks;
        if (blocked) {
            Ib = tmp.alloc<double>(ne * chunk);
            std::vector<double *> ptr((size_t)nblk * chunk);
            for (size_t q = 0; q < ptr.size(); ++q) ptr[q] = Ib + q * b2;
            d_binv = tmp.upload(ptr.data(), ptr.size());
            bad_blk.resize((size_t)nblk * chunk);
            if (keep) h_blocks.resize(ne * chunk);
        }
        for (int b0 = 0; b0 < nmat; b0 += chunk) {
            const int nb = std::min(chunk, nmat - b0);
            HIPCHK(hipMemcpyAsync(d_vals, vals.data() + b0, nb * sizeof(double *),
                                  hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_inv, einv.data() + b0, nb * sizeof(double *),
                                  hipMemcpyHostToDevice, st));
            launch_zero_bytes(st, E, ne * nb * sizeof(double));
            launch_galerkin_batched(st, c, gb, d_vals, E, nb);
            launches += 2;
            if (keep && !blocked)
                HIPCHK(hipMemcpyAsync(S.coarse_E.data() + b0 * n2, E, n2 * nb * sizeof(double),
                                      hipMemcpyDeviceToHost, st));
            if (keep && blocked) {      // the full matrices, zeros outside the blocks
                HIPCHK(hipMemcpyAsync(h_blocks.data(), E, ne * nb * sizeof(double),
                                      hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b)
                    for (int k = 0; k < nblk; ++k)
                        for (int r = 0; r < bn; ++r)
                            std::copy_n(h_blocks.data() + ((size_t)b * nblk + k) * b2 + (size_t)r * bn,
                                        bn, S.coarse_E.data() + (b0 + b) * n2 +
                                                (size_t)(k * bn + r) * nc + (size_t)k * bn);
            }
            if (deflate) {
                // every entry + trace(E) / n_c^2, the diagonal summed on the host in index order
                std::vector<double> diag((size_t)nc * nb);
                for (int b = 0; b < nb; ++b)
                    HIPCHK(hipMemcpy2DAsync(diag.data() + (size_t)b * nc, sizeof(double), E + b * n2,
                                            ((size_t)nc + 1) * sizeof(double), sizeof(double), nc,
                                            hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b) {
                    double tr = 0.0;
                    for (int i = 0; i < nc; ++i) tr += diag[(size_t)b * nc + i];
                    launch_add_constant(st, E + b * n2, tr / ((double)nc * (double)nc), (int64_t)n2);
                    launches += 1;
                }
            }
            if (blocked) {
                launches += launch_dense_inverse_batched(st, E, d_binv, bn, nblk * nb, scratch, d_bad);
                launch_coarse_block_scatter(st, Ib, d_inv, nc, bn, nb);
                launches += 1;
                HIPCHK(hipMemcpyAsync(bad_blk.data(), d_bad, (size_t)nblk * nb * sizeof(int),
                                      hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b)        // first singular column of the whole E_b
                    for (int k = nblk - 1; k >= 0; --k)
                        if (bad_blk[(size_t)b * nblk + k] < bn)
                            bad[b0 + b] = k * bn + bad_blk[(size_t)b * nblk + k];
            } else {
                launches += launch_dense_inverse_batched(st, E, d_inv, nc, nb, scratch, d_bad);
                HIPCHK(hipMemcpyAsync(bad.data() + b0, d_bad, nb * sizeof(int), hipMemcpyDeviceToHost,
                                      st));
                HIPCHK(hipStreamSynchronize(st));
            }
        }
        S.coarse_stats.blocks = nblk;
        S.coarse_stats.block_n = bn;
    }
    if (columns) {
        S.coarse_stats.blocks = 1;
        S.coarse_stats.block_n = nc;
    }
    if (keep) {
        S.coarse_Einv.resize(n2 * nmat);
        for (int b = 0; b < nmat; ++b)
            HIPCHK(hipMemcpyAsync(S.coarse_Einv.data() + b * n2, einv[b], n2 * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    S.coarse_stats.matrices = nmat;
    S.coarse_stats.launches = launches;
    S.coarse_stats.n_coarse = nc;
    S.coarse_stats.ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int b = 0; b < nmat; ++b) {
        if (bad[b] == nc) continue;
        char msg[320];
        if (bad[b] < 0)
            std::snprintf(msg, sizeof msg, "%s: coarse matrix P^T A P of level matrix %d is singular "
                          "(a coarse function without support on free rows, or dependent coarse "
                          "functions)", what, b);
        else
            std::snprintf(msg, sizeof msg, "%s: coarse matrix P^T A P of level matrix %d is singular "
                          "at column %d (pivot below 1e-13 max|diag|: a coarse function without "
                          "support on free rows, or dependent coarse functions)", what, b, bad[b]);
        fail(KKT_ERR_STATE, msg);
    }
}

void dense_inverse_host(System &S, int n, int nmat, const double *a, double *inv, int *bad) {
    hipStream_t st = S.stream;
    const size_t n2 = (size_t)n * n;
    DevPool tmp;
    double *E = tmp.upload(a, n2 * nmat);
    double *I = tmp.alloc<double>(n2 * nmat);
    std::vector<double *> ptr(nmat);
    for (int b = 0; b < nmat; ++b) ptr[b] = I + b * n2;
    double **d_inv = tmp.upload(ptr.data(), ptr.size());
    void *scratch = tmp.alloc<char>(dense_inverse_batched_scratch(n, nmat));
    int *d_bad = tmp.alloc<int>(nmat);
    launch_dense_inverse_batched(st, E, d_inv, n, nmat, scratch, d_bad);
    HIPCHK(hipMemcpyAsync(inv, I, n2 * nmat * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bad, d_bad, nmat * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

void coarse_correction_host(System &S, int batched, int nb, int64_t vstride, const double *r,
                            const double *x_in, const double *einv, double *rc, double *ec,
                            double *x_out, int32_t *shape) {
    CoarseDev c;
    GalerkinDev g;
    int64_t n = 0;
    if (!S.pc || !S.pc->coarse_space(&c, &g, &n))
        fail(KKT_ERR_STATE,
             "kkt_debug_coarse_correction: no two-grid preconditioner built on this handle");
    hipStream_t st = S.stream;
    const int nc = c.nc;
    if (shape) {
        std::vector<int32_t> pt_ip((size_t)nc + 1);
        HIPCHK(hipMemcpyAsync(pt_ip.data(), c.pt_ip, pt_ip.size() * sizeof(int32_t),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int32_t longest = 0;
        for (int j = 0; j < nc; ++j) longest = std::max(longest, pt_ip[j + 1] - pt_ip[j]);
        const int32_t v[KKT_COARSE_SHAPE_INTS] = {(int32_t)n, nc, g.R, g.uniform_w, g.pos != nullptr,
                                                  g.mask != nullptr, g.block_n, longest};
        std::copy(v, v + KKT_COARSE_SHAPE_INTS, shape);
    }
    if (nb == 0) return;
    if (nb < 1 || (!batched && nb != 1) || vstride < n || !r || !einv || !rc || !ec || !x_out)
        fail(KKT_ERR_ARG, "bad coarse correction arguments");
    const size_t len = (size_t)nb * vstride;
    DevPool tmp;
    const double *d_r = tmp.upload(r, len);
    const double *d_xin = x_in ? tmp.upload(x_in, len) : nullptr;
    double *d_xout = tmp.upload(x_out, len);
    const double *d_einv = tmp.upload(einv, (size_t)nc * nc);
    c.rc = tmp.alloc<double>((size_t)nb * nc);      // its own scratch, nb vectors wide
    c.ec = tmp.alloc<double>((size_t)nb * nc);
    if (batched)
        launch_coarse_correction_batched(st, c, d_einv, d_r, d_xin, d_xout, n, nb, vstride);
    else
        launch_coarse_correction(st, c, d_einv, d_r, d_xin, d_xout, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rc, c.rc, (size_t)nb * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ec, c.ec, (size_t)nb * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(x_out, d_xout, len * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
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
    steps_.push_back(s);
}

// One sub-solve in its two-grid form: [update of the right-hand side;] cycles x [Galerkin
// correction of the current iterate; `its` smoothing sweeps from it].
void SchurPC::emit_coarse_solve(const Lin *upd, const Solve &sv, const Mat &F) {
    const int its = std::max(1, schur_its_);
    SweepLevel lv;
    lv.first = steps_.size();
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
        TileLevel &L = lv.lev;
        L.vals = F.vals;
        L.dinv = F.dinv;
        L.out = sv.out;
        L.p1_scale = scale;
        L.post1 = sv.post1;
        L.post2 = sv.post2;
        bool ok = true;
        if (upd) {
            ok = !upd->terms.empty() && upd->terms.size() <= 2 && upd->cz == 0.0 && !upd->z &&
                 upd->yin != nullptr;
            for (const Term &t : upd->terms) ok = ok && t.x == upd->terms[0].x;
            if (ok) {
                L.bin = upd->yin;
                L.bout = upd->y == upd->yin ? nullptr : upd->y;
                lv.b_after = upd->y;
                L.x_prev = upd->terms[0].x;
                L.n_upd = (int32_t)upd->terms.size();
                for (size_t t = 0; t < upd->terms.size(); ++t) L.upd_vals[t] = upd->terms[t].vals;
                L.ca = upd->ca;
                L.cy = upd->cy;
            }
        } else {
            L.bin = sv.b;
            L.bout = nullptr;
            L.n_upd = 0;
        }
        lv.eligible = ok;
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
    lv.last = steps_.size();
    sweep_levels_.push_back(lv);
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

void SchurPC::collect_matrices() {
    pre_.clear();
    pre_cls_.clear();
    const int nbatch = S_.opts.spectrum_batch;
    const bool estimates = d_.schur_emin <= 0;
    if (nbatch <= 0 || !(estimates || coarse_cycles_ > 0)) return;
    const Pattern &P = S_.patterns[m_pat_];
    hipStream_t st = S_.stream;
    kkt_spectrum_stats &stats = S_.spectrum_stats;
    SpectrumCounters cnt;
    HIPCHK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    // the candidates in creation order, each formed once
    std::vector<MatKey> keys;
    for (const auto &bc : solved_matrices()) {
        uint64_t bits;
        std::memcpy(&bits, &bc.second, sizeof bits);
        const MatKey key(bc.first, bits);
        if (pre_.count(key)) continue;
        Pre pr;
        pr.vals = values_mem_.alloc<double>(P.npadded);
        pr.dinv = values_mem_.alloc<double>(nx_);
        form_matrix(bc.first, bc.second, pr.vals, pr.dinv);
        cnt.launches += mask_ ? 3 : 2;
        pre_[key] = pr;
        keys.push_back(key);
    }
    const int C = (int)keys.size();
    if (C == 0) return;
    // twins: a fingerprint per candidate, then the candidates of a (shift, fingerprint) group bit
    // for bit against the group's first
    spec::TwinGroups twins;
    twins.first_of.resize(C);
    for (int i = 0; i < C; ++i) twins.first_of[i] = i;
    twins.pair_of.assign(C, -1);
    std::vector<unsigned> h_flag;
    DevPool tmp;
    if (C > 1) {
        std::vector<const double *> h_vals(C);
        for (int i = 0; i < C; ++i) h_vals[i] = pre_[keys[i]].vals;
        const double *const *d_vals = tmp.upload(h_vals.data(), h_vals.size());
        const int nw = spec_fingerprint_blocks(P.npadded);
        unsigned long long *d_fp = tmp.alloc<unsigned long long>((size_t)C * nw);
        std::vector<unsigned long long> h_fp((size_t)C * nw);
        launch_spec_fingerprint(st, d_vals, C, P.npadded, d_fp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_fp.data(), d_fp, h_fp.size() * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        cnt.launches++;
        cnt.syncs++;
        stats.twin_syncs++;
        std::vector<uint64_t> shifts(C), folded(C);
        for (int i = 0; i < C; ++i) {
            shifts[i] = keys[i].second;
            folded[i] = spec_fingerprint_fold(&h_fp[(size_t)i * nw], nw);
        }
        twins = spec::group_twins(shifts, folded);
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
    std::vector<int> reps;      // the first candidate of every class
    const std::vector<int> cls = spec::twin_classes(twins, h_flag, &reps);
    for (int i = 0; i < C; ++i) pre_[keys[i]].cls = cls[i];
    pre_cls_.assign(reps.size(), PreCls{});
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
            m.vals = values_mem_.alloc<double>(P.npadded);
            m.dinv = values_mem_.alloc<double>(nx_);
            form_matrix(base_vals, c, m.vals, m.dinv);
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

void SchurPC::note_solve(int sweep, int level, const Mat &m) {
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
    lv.first = steps_.size();
    emit_lin({upd});
    emit_solves({sv}, its, emin, emax, P_, nx_, true, &lv.coef, eimag);
    lv.last = steps_.size();
    lv.its = its;
    // what the tile form can express: b = ca * sum_t U_t x + cy * b_in with one x
    bool ok = its >= 2 && !upd.terms.empty() && upd.terms.size() <= 2 && upd.cz == 0.0 && !upd.z &&
              upd.yin != nullptr;
    for (const Term &t : upd.terms) ok = ok && t.x == upd.terms[0].x;
    if (ok) {
        TileLevel &L = lv.lev;
        L.vals = sv.vals;
        L.dinv = sv.dinv;
        L.bin = upd.yin;
        // The plain steps update the right-hand side in place.  A tile re-computes the rows of
        // its rings from b_in, so an in-place store by the owner would race with its neighbours'
        // reads: the updated right-hand side stays on chip (nothing reads B_i after a sweep: the
        // next batched step overwrites it).
        L.bout = upd.y == upd.yin ? nullptr : upd.y;
        lv.b_after = upd.y;
        L.out = sv.out;
        L.x_prev = upd.terms[0].x;
        L.n_upd = (int32_t)upd.terms.size();
        for (size_t t = 0; t < upd.terms.size(); ++t) L.upd_vals[t] = upd.terms[t].vals;
        L.ca = upd.ca;
        L.cy = upd.cy;
        L.p1_scale = upd.c3;
        L.post1 = sv.post1;
        L.post2 = sv.post2;
        lv.eligible = true;
    }
    sweep_levels_.push_back(lv);
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
    rec.first = steps_.size();
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
        solo.first = steps_.size();
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
        solo.last = steps_.size();
        solo.its = its;
        TileLevel &L = solo.lev;
        L.vals = sv[0].vals;
        L.dinv = sv[0].dinv;
        L.bin = sv[0].b;
        L.bout = nullptr;
        L.out = sv[0].out;
        L.n_upd = 0;
        L.p1_scale = scale;
        L.post1 = sv[0].post1;
        L.post2 = sv[0].post2;
        solo.eligible = true;
        sweep_levels_.push_back(solo);
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
    emit_lin({Lin{{Term{Dv, u0}}, B_, 1.0, 0.0, -1.0, nullptr, b1}});
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
                l.terms.push_back(Term{block_vals(KKT_Q10, i, i), blk(u0, i)});
                if (i >= 1)
                    l.terms.push_back(Term{block_vals(KKT_Q10, i, i - 1),
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
            note_solve(KKT_PC_SWEEP_FORWARD, i, F);
            const Solve sv{F.vals, F.dinv, blk(B_, i), blk(u1, i)};
            if (i >= 1)
                emit_update_and_solve(Lin{{Term{block_vals(KKT_Q10, i, i - 1),
                                                i - 1 >= lo ? blk(u1, i - 1) : h_u1_}},
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
        note_solve(KKT_PC_SWEEP_BACKWARD, i, G);
        const Solve sv{G.vals, G.dinv, blk(B_, i), blk(u1, i)};
        if (i <= n - 2)
            emit_update_and_solve(Lin{{Term{block_vals(KKT_Q01, i, i + 1),
                                            i + 1 < hi ? blk(u1, i + 1) : h_u1_}},
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
            l.terms.push_back(Term{block_vals(KKT_Q10, i, i), blk(u0, i)});
            if (i >= 1)
                l.terms.push_back(Term{block_vals(KKT_Q10, i, i - 1),
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
        note_solve(KKT_PC_SWEEP_FORWARD, i, F);
        const Solve sv{F.vals, F.dinv, blk(B_, i), blk(u1, i)};
        if (i >= 1) {
            const double *prev = i - 1 >= lo ? blk(u1, i - 1) : h_u1_;
            emit_update_and_solve(Lin{{Term{block_vals(KKT_Q10, i, i - 1), prev},
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
        note_solve(KKT_PC_SWEEP_BACKWARD, i, G);
        const Solve sv{G.vals, G.dinv, blk(B_, i), blk(u1, i)};
        if (i <= n - 2) {
            // h K^T + (c - 1) M: only multiplied with (indefinite for c < 1)
            Mat H = schur_matrix(block_vals(KKT_Q01, i, i + 1), c, false);
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
