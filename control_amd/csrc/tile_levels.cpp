// kkt_debug_tile_levels: one launch of the tile program's two-grid levels on host data
// (include/kkt.h documents the arguments).  As rowstep.cpp, nothing here computes and there is no
// second path: the vectors go up, the TileLevel records are filled as fuse_tile_run fills them and
// launch_tile_sweep runs once on the handle's stream with the arguments replay() passes for a TILE
// step (SchurPC::tile_args: the preconditioner's own plan, coarse tables, granule buffers and
// error words) after the residency check fuse_tile_run makes (SchurPC::tile_resident).
// Every vector sits between guards; what the launch only reads is downloaded again and compared
// with what went up.
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "pc.hpp"

namespace kkt {

namespace {

constexpr size_t G = KKT_BLOCK_GUARD;

[[noreturn]] void bad(const char *what) {
    fail(KKT_ERR_ARG, std::string("kkt_debug_tile_levels: ") + what);
}

}  // namespace

void SchurPC::debug_tile_levels(kkt_tile_levels *pa) {
    kkt_tile_levels &a = *pa;
    if (!use_programs_ || !tile_ok_ || !tile_coarse_ok_ || coarse_cycles_ <= 0 || !d_tile_coarse_)
        fail(KKT_ERR_STATE, "kkt_debug_tile_levels: no two-grid tile program on this handle");
    const TilePlan &tp = tile_plan_;
    const TileCoarseDev &D = h_tile_coarse_;
    const Pattern &P = S_.patterns[m_pat_];
    const size_t n = (size_t)P.nrows, slot = n + 2 * G;
    const int nc = D.nc;
    a.inputs_changed = 0;
    a.tiles = tp.ntiles;
    a.threads = tp.threads;
    a.row_slots = tp.rpt;
    a.depth = tp.depth;
    a.W = tp.W;
    a.nk_pad = tp.nk_pad;
    a.cache = D.cache_einv ? 2 : D.cache_lists ? 1 : 0;
    a.rings = D.ring_prolong != 0;
    a.ew = D.ew;
    a.n_coarse = nc;
    a.nrows = (int32_t)n;
    if (a.own_ptr || a.own_rows) {
        if (!a.own_ptr || !a.own_rows) bad("own_ptr and own_rows come together");
        if (a.own_cap < tp.ntiles + 1) bad("own_cap is smaller than tiles + 1");
        std::fill(a.own_ptr, a.own_ptr + a.own_cap, -1);
        std::fill(a.own_rows, a.own_rows + n, -1);
        int32_t at = 0;
        for (int t = 0; t < tp.ntiles; ++t) {
            a.own_ptr[t] = at;
            const int32_t n0 = tp.n[(size_t)t * (TILE_MAX_DEPTH + 1)];
            if ((size_t)at + n0 > n) fail(KKT_ERR_STATE, "kkt_debug_tile_levels: the tiles own more rows than there are");
            for (int32_t l = 0; l < n0; ++l) a.own_rows[at++] = tp.grow[(size_t)t * tp.nk_pad + l];
        }
        a.own_ptr[tp.ntiles] = at;
    }
    if (a.nlevels == 0) return;

    // ---- checks
    if (a.nlevels < 0 || a.nlevels > 64 || !a.levels) bad("nlevels must be 0..64");
    if (a.its < 1 || a.cycles < 1) bad("its and cycles must be at least 1");
    if (!a.own_ptr) bad("a launch reports the tiles' own rows: own_ptr and own_rows are needed");
    auto block = [&](int q, int i, int j) -> const double * {
        const auto it = S_.blocks.find({q, i, j});
        if (it == S_.blocks.end()) bad("a level names a block that is not stored");
        const ValueArray &va = S_.values[it->second.va];
        if (va.pattern != m_pat_) bad("a level names a block of another pattern than the preconditioner's");
        return va.d_vals;
    };
    for (int l = 0; l < a.nlevels; ++l) {
        const kkt_tile_level &L = a.levels[l];
        if (!L.dinv || !L.coef || !L.einv || !L.bin || !L.out) bad("a level lacks an operand");
        if (L.n_upd != 0 && L.n_upd != 1) bad("n_upd must be 0 or 1");
        if (L.n_upd == 1 && l == 0) bad("the first level has no previous level to be chained to");
        if (L.n_upd == 0 && L.bout) bad("a solo level does not write bout");
        (void)block(L.q, L.i, L.j);
        if (L.n_upd) (void)block(L.uq, L.ui, L.uj);
        for (int m = 0; m < l; ++m) {
            const kkt_tile_level &O = a.levels[m];
            if (L.out == O.out || L.out == O.bout || L.out == O.bin || L.bin == O.out ||
                L.bin == O.bout || (L.bout && (L.bout == O.out || L.bout == O.bout || L.bout == O.bin)))
                bad("two levels share a vector");
        }
        if (L.out == L.bin || L.out == L.bout || L.bin == L.bout) bad("a level's vectors must differ");
        // "block" rows: the products leave out what lies outside [e_lo, e_hi) of a row
        bool seen = false;
        for (int m = 0; m < l; ++m) seen = seen || a.levels[m].einv == L.einv;
        if (!seen)
            for (int j = 0; j < nc; ++j)
                for (int q = 0; q < nc; ++q)
                    if ((q < tile_e_lo_[j] || q >= tile_e_hi_[j]) && L.einv[(size_t)j * nc + q] != 0.0)
                        bad("block rows: the matrix is non-zero outside the column range of a row");
    }
    // residency, as fuse_tile_run checks it: for the bytes of this `its`, and never below what was
    // checked before (the kernel's dynamic-LDS limit is set to the bytes of the last check)
    if (!tile_resident(std::max(tile_sweep_lds_bytes(tp.nk_pad, a.its, D), tile_lds_checked_), true))
        bad("the plan is not resident with this number of sweeps");
    if (!tile_sweep_fuses_update(tp.W, 1)) bad("no kernel variant with the level update for this width");

    // ---- upload
    hipStream_t st = S_.stream;
    DevPool pool;
    struct Watch {
        const void *dev;
        const void *host;
        size_t bytes;
    };
    std::vector<Watch> watched;
    auto guard = [&](double *h) {
        std::fill(h, h + G, KKT_KRYLOV_PAD);
        std::fill(h + G + n, h + slot, KKT_KRYLOV_PAD);
    };
    std::vector<TileLevel> levels((size_t)a.nlevels);
    std::vector<const double *> einvs((size_t)a.nlevels);
    std::vector<double *> d_out((size_t)a.nlevels), d_bout((size_t)a.nlevels, nullptr);
    std::map<const double *, const double *> einv_dev;
    std::vector<std::pair<const double *, const TileCoef *>> coef_dev;
    static_assert(sizeof(TileCoef) == 3 * sizeof(double), "a coefficient table is triples of doubles");
    for (int l = 0; l < a.nlevels; ++l) {
        const kkt_tile_level &L = a.levels[l];
        guard(L.bin);
        guard(L.out);
        std::fill(L.out + G, L.out + G + n, 0.0);
        const double *d_bin = pool.upload(L.bin, slot);
        watched.push_back({d_bin, L.bin, slot * sizeof(double)});
        const double *d_dinv = pool.upload(L.dinv, n);
        watched.push_back({d_dinv, L.dinv, n * sizeof(double)});
        d_out[l] = pool.upload(L.out, slot);
        if (L.bout) {
            guard(L.bout);
            d_bout[l] = pool.upload(L.bout, slot);
        }
        if (!einv_dev.count(L.einv)) einv_dev[L.einv] = pool.upload(L.einv, (size_t)nc * nc);
        einvs[l] = einv_dev[L.einv];
        // identical coefficient tables share one device copy (fuse_tile_run)
        const TileCoef *d_coef = nullptr;
        for (const auto &c : coef_dev)
            if (std::memcmp(c.first, L.coef, 3 * (size_t)a.its * sizeof(double)) == 0) d_coef = c.second;
        if (!d_coef) {
            d_coef = reinterpret_cast<const TileCoef *>(pool.upload(L.coef, 3 * (size_t)a.its));
            coef_dev.push_back({L.coef, d_coef});
        }
        TileLevel &T = levels[l];
        T = TileLevel{};
        T.vals = block(L.q, L.i, L.j);
        T.dinv = d_dinv;
        T.bin = d_bin + G;
        T.bout = d_bout[l] ? d_bout[l] + G : nullptr;
        T.out = d_out[l] + G;
        T.n_upd = L.n_upd;
        if (L.n_upd) {
            T.x_prev = d_out[l - 1] + G;
            T.upd_vals[0] = block(L.uq, L.ui, L.uj);
            T.prev_in_lds = 1;
        }
        T.ca = L.ca;
        T.cy = L.cy;
        T.p1_scale = L.p1_scale;
        T.post1 = L.post1;
        T.post2 = L.post2;
        T.coef = d_coef;
    }
    const TileLevel *d_levels = pool.upload(levels.data(), levels.size());
    const double **d_einvs = pool.upload(einvs.data(), einvs.size());

    // ---- the launch replay() makes for a TILE step, as the first one of an application
    PcStep step;
    step.kind = PcStep::TILE;
    step.coarse = true;
    step.d_einv = d_einvs;
    step.nlevels = a.nlevels;
    step.its = a.its;
    step.clear = step.clear_coarse = true;
    TileArgs t = tile_args(step);
    t.cycles = a.cycles;
    t.stamps = 0;
    t.debug_drop = 0;
    const size_t words = 2 * n;
    HIPCHK(hipStreamSynchronize(st));
    try {
        launch_tile_sweep(st, t, d_levels, tp.d_n, tp.d_grow, tp.d_lcol, tp.d_gpos, mask_, tp.ntiles,
                          tp.threads, words, &h_tile_coarse_);
    } catch (const TileLaunchError &e) {
        fail(KKT_ERR_HIP, e.msg);
    }
    HIPCHK(hipStreamSynchronize(st));
    // a bounded spin that ran out: the record, once, and no second launch
    std::string why;
    if (timed_out(&why)) fail(KKT_ERR_STATE, "kkt_debug_tile_levels: " + why);

    // ---- download
    int32_t changed = 0;
    for (int l = 0; l < a.nlevels; ++l) {
        const kkt_tile_level &L = a.levels[l];
        HIPCHK(hipMemcpy(L.out, d_out[l], slot * sizeof(double), hipMemcpyDeviceToHost));
        if (L.bout) HIPCHK(hipMemcpy(L.bout, d_bout[l], slot * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<char> buf;
    for (const Watch &w : watched) {
        buf.resize(w.bytes);
        HIPCHK(hipMemcpy(buf.data(), w.dev, w.bytes, hipMemcpyDeviceToHost));
        changed += std::memcmp(buf.data(), w.host, w.bytes) != 0;
    }
    a.inputs_changed = changed;
}

}  // namespace kkt
