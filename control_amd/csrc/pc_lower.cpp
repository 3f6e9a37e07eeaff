// Lowering of the preconditioner program (SchurPC, pc.hpp): the steps the builds emitted become
// tile launches, batched mass-tile launches or row programs -- the plans and tables of the three
// forms, and the passes that rewrite steps_.
#include "pc.hpp"
#include "program_partition.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace kkt {

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

// Residency of the plan with `need` bytes of dynamic LDS per tile (the kernel's dynamic-LDS limit
// is set to the bytes of the last check).
bool SchurPC::tile_resident(size_t need, bool coarse) {
    const TilePlan &tp = tile_plan_;
    if (need > 150 * 1024 ||
        tp.ntiles > tile_sweep_max_tiles(tp.W, tp.rpt, tp.threads, need, tp.hslots, coarse))
        return false;
    tile_lds_checked_ = need;
    return true;
}

// Steps [k, e) are single-block steps: if they are exactly a run of recorded sweep levels the
// tile form can express (a level's steps: the stretch that carries its tag), replace them by one
// TILE step.
bool SchurPC::fuse_tile_run(size_t k, size_t e, std::vector<PcStep> &out) {
    std::vector<const SweepLevel *> run;
    std::vector<size_t> first;          // where each level's stretch starts; the run ends at e
    for (size_t i = k; i < e; ++i) {
        const int tag = steps_[i].level;
        if (tag < 0 || !sweep_levels_[tag].eligible) return false;
        if (i > k && tag == steps_[i - 1].level) continue;
        run.push_back(&sweep_levels_[tag]);
        first.push_back(i);
    }
    if (run.empty()) return false;
    first.push_back(e);
    const int its = run[0]->its;
    const bool coarse = run[0]->coarse;
    if (coarse && !tile_coarse_ok_) return false;
    {
        // residency and the dynamic-LDS attribute were checked for tile_lds_checked_ bytes
        const size_t need = coarse ? tile_sweep_lds_bytes(tile_plan_.nk_pad, its, h_tile_coarse_)
                                   : tile_sweep_lds_bytes(tile_plan_.nk_pad, its);
        if (need > tile_lds_checked_ && !tile_resident(need, coarse)) return false;
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
        size_t first_cheb = first[i];
        if (L.n_upd > 0) {
            out.push_back(steps_[first[i]]);         // the update, as a plain single-block step
            first_cheb = first[i] + 1;
            L.n_upd = 0;
            L.prev_in_lds = 0;
            L.bin = lv.b_after;
            L.bout = nullptr;
        }
        tile_step(&L, 1, (int)(first[i + 1] - first_cheb), false);
    }
    return true;
}

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

// Replace the ROWS_IL steps of every batched solve -- the stretch of steps that carries the solve's
// tag -- by ceil(its / K) TILE_CHEB steps with the same tag.  Every other step is copied as it is,
// its level tag with it: nothing names a step by its index.
void SchurPC::fuse_mass_tiles() {
    if (!S_.opts.mass_tiles || S_.opts.lanes || mass_solves_.empty()) return;
    bool any = false;
    for (const MassSolve &ms : mass_solves_) any = any || ms.its >= 2;
    if (!any || !prepare_mass_tiles()) return;
    const TilePlan &tp = mass_plan_;
    const int K = tp.depth;
    std::vector<PcStep> out;
    size_t k = 0;
    while (k < steps_.size()) {
        const int tag = steps_[k].solve;
        size_t e = k + 1;
        while (tag >= 0 && e < steps_.size() && steps_[e].solve == tag) ++e;
        const MassSolve *ms = tag >= 0 ? &mass_solves_[tag] : nullptr;
        if (!ms || ms->its < 2 || e - k != (size_t)ms->its) {
            out.insert(out.end(), steps_.begin() + k, steps_.begin() + e);
            k = e;
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
            s.solve = tag;
            mass_launches_.push_back(ml);
            out.push_back(s);
        }
        if (S_.opts.verbose)
            std::fprintf(stderr, "[kkt] mass tile form: a solve of %d steps on %zu levels as %d "
                         "launches of %d x %d workgroups (%d level groups each)\n", ms->its, m, nl,
                         tp.ntiles, grid_y, gpw);
        k = e;
    }
    steps_.swap(out);
}

// Replace every run of >= 4 consecutive single-block steps (the time sweeps) by one
// persistent launch: the tile form (tile_kernels.hip: `depth` steps per hand-off) where it
// fits, else a row program with neighbour synchronisation (kernels.hip, pc_row_program*).
// Which steps form a run and what becomes of it is partition_program's (program_partition.hpp);
// here the steps are described to it and each piece it returns is emitted.
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
    // describe the steps, let partition_program cut them, emit each piece
    std::vector<StepDesc> desc(steps_.size());
    for (size_t i = 0; i < steps_.size(); ++i) {
        const PcStep &st = steps_[i];
        StepDesc &d = desc[i];
        d.kind = st.kind == PcStep::ROWS ? StepDesc::ROWS
                 : st.kind == PcStep::COARSE ? StepDesc::COARSE : StepDesc::OTHER;
        d.single = (st.kind == PcStep::ROWS && st.rows.nops == 1) || st.kind == PcStep::COARSE;
        d.level = st.level;
        d.eligible = st.level >= 0 && sweep_levels_[st.level].eligible;
    }
    std::vector<std::vector<PcStep>> tile_runs;     // what fuse_tile_run made of the runs it took
    auto tiles_take = [&](size_t a, size_t b) {
        std::vector<PcStep> tiles;
        if (!fuse_tile_run(a, b, tiles)) return false;
        tile_runs.push_back(std::move(tiles));
        return true;
    };
    // step q gathers exactly what step q - 1 produced
    auto chains = [&](size_t q) {
        const RowOp &op = steps_[q].rows.h_op, &prev = steps_[q - 1].rows.h_op;
        bool chain = op.nterms > 0;
        for (int t = 0; t < op.nterms; ++t)
            chain &= op.t[t].x.base == 0 && op.t[t].x.off == gather_out(prev);
        return chain;
    };
    size_t next_tiles = 0;
    for (const Piece &pc : partition_program(desc, use_tiles, S_.sharded, legacy_ok_, prog_granule_,
                                             tiles_take, chains)) {
        if (pc.kind == Piece::PROGRAM) {
            emit_prog(pc.first, pc.last);
        } else if (pc.kind == Piece::TILES) {
            const std::vector<PcStep> &tiles = tile_runs[next_tiles++];
            out.insert(out.end(), tiles.begin(), tiles.end());
        } else {
            out.insert(out.end(), steps_.begin() + pc.first, steps_.begin() + pc.last);
        }
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

}  // namespace kkt
