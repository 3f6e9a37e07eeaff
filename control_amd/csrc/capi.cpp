// extern "C" boundary of libkkt (include/kkt.h).  No C++ exception leaves this file.
#include <algorithm>
#include <charconv>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "anderson.hpp"
#include "comm.hpp"
#include "pc.hpp"
#include "reaction.hpp"
#include "relin.hpp"
#include "system.hpp"
#include "tiles.hpp"

using namespace kkt;

struct kkt_system {
    System S;
};

static std::string g_create_error;

#define KKT_TRY(h, ...)                                   \
    if (!(h)) return KKT_ERR_ARG;                         \
    System &S = (h)->S;                                   \
    try {                                                 \
        if (hipSetDevice(S.device) != hipSuccess)         \
            fail(KKT_ERR_HIP, "hipSetDevice failed");     \
        __VA_ARGS__;                                      \
        return KKT_OK;                                    \
    } catch (const Error &e) {                            \
        S.err = e.msg;                                    \
        return e.code;                                    \
    } catch (const std::exception &e) {                   \
        S.err = e.what();                                 \
        return KKT_ERR_STATE;                             \
    }

// ---- execution options: one row per key (include/kkt.h documents them)
template <bool Options::*F>
static bool set_switch(Options &o, const char *v) {
    if (std::strcmp(v, "0") != 0 && std::strcmp(v, "1") != 0) return false;
    o.*F = v[0] == '1';
    return true;
}
// a decimal integer, the whole string, in [LO, HI]
template <int Options::*F, int LO = INT_MIN, int HI = INT_MAX>
static bool set_int(Options &o, const char *v) {
    int x = 0;
    const auto r = std::from_chars(v, v + std::strlen(v), x);
    if (r.ec != std::errc() || *r.ptr || x < LO || x > HI) return false;
    o.*F = x;
    return true;
}
static bool set_prog_mode(Options &o, const char *v) {
    static const char *names[] = {"auto", "tile", "dataflow", "flags", "w"};   // ProgMode order
    for (int k = 0; k < 5; ++k)
        if (std::strcmp(v, names[k]) == 0) {
            o.prog_mode = (ProgMode)k;
            return true;
        }
    return false;
}
static bool set_coarse_setup(Options &o, const char *v) {
    o.coarse_columns = std::strcmp(v, "columns") == 0;
    return o.coarse_columns || std::strcmp(v, "batched") == 0;
}

static bool set_tile_coarse_cache(Options &o, const char *v) {
    if (std::strcmp(v, "auto") == 0) {
        o.tile_coarse_cache = -1;
        return true;
    }
    return set_int<&Options::tile_coarse_cache, 0, 2>(o, v);
}
static bool set_tile_coarse_rows(Options &o, const char *v) {
    o.tile_coarse_full = std::strcmp(v, "full") == 0;
    return o.tile_coarse_full || std::strcmp(v, "block") == 0;
}

static bool set_mass_tile_waves(Options &o, const char *v) {
    if (std::strcmp(v, "0") != 0 && std::strcmp(v, "4") != 0 && std::strcmp(v, "8") != 0) return false;
    o.mass_tile_waves = v[0] - '0';
    return true;
}

struct OptionKey {
    const char *key, *accepted;
    bool (*set)(Options &, const char *);
};
static const OptionKey option_keys[] = {
    {"sell_r", "1 | 2", set_int<&Options::sell_r, 1, 2>},
    {"sell_sort", "0 | 1", set_switch<&Options::sell_sort>},
    {"sell_sigma", "1..64", set_int<&Options::sell_sigma, 1, 64>},
    {"shared_rows", "0 | 1", set_switch<&Options::shared_rows>},
    {"ragged_switch", "0 | 1", set_switch<&Options::ragged_switch>},
    {"ragged_xcd", "0 | 1", set_switch<&Options::ragged_xcd>},
    {"apply_xcd", "0 | 1", set_switch<&Options::apply_xcd>},
    {"pc_xcd", "0 | 1", set_switch<&Options::pc_xcd>},
    {"interleave", "0 | 1", set_switch<&Options::interleave>},
    {"kernarg_ops", "0 | 1", set_switch<&Options::kernarg_ops>},
    {"no_graph", "0 | 1", set_switch<&Options::no_graph>},
    {"persistent", "0 | 1", set_switch<&Options::persistent>},
    {"prog_mode", "auto | tile | dataflow | flags | w", set_prog_mode},
    {"prog_waves", "1..8", set_int<&Options::prog_waves, 1, 8>},
    {"prog_steps", "0 | 1", set_switch<&Options::prog_steps>},
    {"tile_depth", "1..16", set_int<&Options::tile_depth, 1, TILE_MAX_DEPTH>},
    {"tile_waves", "1..16", set_int<&Options::tile_waves, 1, 16>},
    {"tile_unfused", "0 | 1", set_switch<&Options::tile_unfused>},
    {"tile_poll_delay", "an integer", set_int<&Options::tile_poll_delay>},
    {"lanes", "0 | 1", set_switch<&Options::lanes>},
    {"lane_chunks", "an integer", set_int<&Options::lane_chunks>},
    {"coarse_setup", "batched | columns", set_coarse_setup},
    {"coarse_keep", "0 | 1", set_switch<&Options::coarse_keep>},
    {"coarse_blocks", "0 | 1", set_switch<&Options::coarse_blocks>},
    {"spectrum_batch", "0..4096", set_int<&Options::spectrum_batch, 0, 4096>},
    {"pc_alias", "0 | 1", set_switch<&Options::pc_alias>},
    {"coarse_rings", "0 | 1", set_switch<&Options::coarse_rings>},
    {"tile_coarse_cache", "auto | 0 | 1 | 2", set_tile_coarse_cache},
    {"tile_coarse_rows", "block | full", set_tile_coarse_rows},
    {"mass_tiles", "0 | 1", set_switch<&Options::mass_tiles>},
    {"mass_tile_depth", "0..8", set_int<&Options::mass_tile_depth, 0, MASS_TILE_MAX_DEPTH>},
    {"mass_tile_rows", "0..65536", set_int<&Options::mass_tile_rows, 0, 65536>},
    {"mass_tile_levels", "0..4096", set_int<&Options::mass_tile_levels, 0, 4096>},
    {"mass_tile_waves", "0 | 4 | 8", set_mass_tile_waves},
    {"stage_timers", "0 | 1", set_switch<&Options::stage_timers>},
    {"verbose", "0 | 1", set_switch<&Options::verbose>},
    {"stamps", "0 | 1", set_switch<&Options::stamps>},
    {"debug_drop_handoff", "an integer", set_int<&Options::debug_drop_handoff>},
};

extern "C" {

int kkt_create(kkt_handle *out, int device_id) {
    if (!out) return KKT_ERR_ARG;
    *out = nullptr;
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
            fail(KKT_ERR_HIP, "no HIP device available: libkkt has no CPU path");
        if (device_id < 0 || device_id >= ndev) fail(KKT_ERR_ARG, "device id out of range");
        HIPCHK(hipSetDevice(device_id));
        auto h = std::make_unique<kkt_system>();
        h->S.device = device_id;
        h->S.own_stream = Stream::create();
        h->S.stream = h->S.own_stream;
        *out = h.release();
        return KKT_OK;
    } catch (const Error &e) {
        g_create_error = e.msg;
        return e.code;
    } catch (const std::exception &e) {
        g_create_error = e.what();
        return KKT_ERR_STATE;
    }
}

int kkt_destroy(kkt_handle h) {
    if (!h) return KKT_OK;
    delete h;
    return KKT_OK;
}

const char *kkt_last_error(kkt_handle h) { return h ? h->S.err.c_str() : g_create_error.c_str(); }

int kkt_set_option(kkt_handle h, const char *key, const char *value) {
    KKT_TRY(h, {
        if (!key || !value) fail(KKT_ERR_ARG, "null option");
        for (const OptionKey &k : option_keys) {
            if (std::strcmp(k.key, key) != 0) continue;
            Options o = S.opts;      // a rejected value leaves the options as they were
            if (!k.set(o, value))
                fail(KKT_ERR_ARG, std::string("option ") + key + ": \"" + value +
                                      "\" is not accepted (" + k.accepted + ")");
            S.opts = o;
            return KKT_OK;
        }
        fail(KKT_ERR_ARG, std::string("unknown option: ") + key);
    });
}

int kkt_set_tile_coordinates(kkt_handle h, int dim, int64_t n, const double *coords) {
    KKT_TRY(h, {
        if (dim < 1 || dim > 3 || n < 1 || !coords) fail(KKT_ERR_ARG, "bad tile coordinates");
        for (size_t i = 0; i < (size_t)n * dim; ++i)      // (they are sorted: no NaN)
            if (!std::isfinite(coords[i])) fail(KKT_ERR_ARG, "tile coordinates must be finite");
        S.tile_coords.assign(coords, coords + (size_t)n * dim);
        S.tile_dim = dim;
    });
}

int kkt_set_layout(kkt_handle h, int n00, int n11, int64_t nx0, int64_t nx1, int CN, int s00,
                   int s11) {
    KKT_TRY(h, S.set_layout(n00, n11, nx0, nx1, CN, s00, s11));
}

int kkt_shard_range(int m, int rank, int world, int *lo, int *hi) {
    if (m < 1 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return KKT_ERR_ARG;
    // contiguous, as even as possible, earlier ranks take the remainder
    const int q = m / world, r = m % world;
    *lo = rank * q + (rank < r ? rank : r);
    *hi = *lo + q + (rank < r ? 1 : 0);
    return KKT_OK;
}

int kkt_set_shard(kkt_handle h, int rank, int world) { KKT_TRY(h, S.set_shard(rank, world)); }
int kkt_set_shard_families(kkt_handle h, int rank, int world, int families) {
    KKT_TRY(h, S.set_shard(rank, world, families));
}

int kkt_add_block(kkt_handle h, int q, int i, int j, int64_t nrows, int64_t ncols,
                  const int32_t *indptr, const int32_t *indices, const double *values,
                  int64_t share_id) {
    KKT_TRY(h, {
        if (!values) fail(KKT_ERR_ARG, "bad block args");
        S.add_block(q, i, j, nrows, ncols, indptr, indices, values, share_id);
    });
}

int kkt_add_block_structure(kkt_handle h, int q, int i, int j, int64_t nrows, int64_t ncols,
                            const int32_t *indptr, const int32_t *indices) {
    KKT_TRY(h, S.add_block(q, i, j, nrows, ncols, indptr, indices, nullptr, -1));
}

int kkt_update_block_values(kkt_handle h, int q, int i, int j, const double *values) {
    KKT_TRY(h, S.update_block_values(q, i, j, values));
}

int kkt_set_bc(kkt_handle h, int k, int64_t n, const int32_t *idx, double alpha) {
    KKT_TRY(h, S.set_bc(k, n, idx, alpha));
}

int kkt_set_const_nullspace(kkt_handle h, int k, double alpha) {
    KKT_TRY(h, S.set_const_ns(k, alpha));
}

int kkt_finalize(kkt_handle h) { KKT_TRY(h, S.finalize()); }

int kkt_set_pc_schur(kkt_handle h, const kkt_pc_desc *desc) {
    KKT_TRY(h, {
        if (!desc) fail(KKT_ERR_ARG, "null descriptor");
        S.require_values("kkt_set_pc_schur");
        S.pc.reset();
        S.pc_cb = nullptr;
        S.pc = std::make_unique<SchurPC>(S, *desc);
        S.pc_stale = false;
    });
}

int kkt_set_pc_stokes(kkt_handle h, kkt_handle inner, kkt_handle commutator,
                      const kkt_pc_stokes_desc *desc) {
    KKT_TRY(h, {
        if (!desc || !inner || !commutator) fail(KKT_ERR_ARG, "null argument");
        S.require_values("kkt_set_pc_stokes");
        inner->S.require_values("kkt_set_pc_stokes (inner handle)");
        commutator->S.require_values("kkt_set_pc_stokes (commutator handle)");
        S.pc.reset();
        S.pc_cb = nullptr;
        S.pc = std::make_unique<StokesPC>(S, inner->S, commutator->S, *desc);
    });
}

int kkt_set_pc_callback(kkt_handle h, kkt_pc_callback fn, void *user) {
    KKT_TRY(h, {
        if (!fn) fail(KKT_ERR_ARG, "null callback");
        S.pc.reset();
        S.pc_cb = fn;
        S.pc_cb_user = user;
    });
}

int kkt_set_pc_identity(kkt_handle h) {
    KKT_TRY(h, {
        S.pc.reset();
        S.pc_cb = nullptr;
    });
}

int kkt_set_krylov(kkt_handle h, int type, int pc_side, int restart, double rtol, double atol,
                   double divtol, int max_it) {
    KKT_TRY(h, {
        if (type != KKT_KSP_GMRES && type != KKT_KSP_FGMRES && type != KKT_KSP_MINRES)
            fail(KKT_ERR_ARG, "linear_solver must be gmres, fgmres or minres");
        if (restart < 1 || max_it < 0 || rtol < 0 || atol < 0) fail(KKT_ERR_ARG, "bad KSP options");
        S.ksp.type = type;
        S.ksp.pc_side = pc_side;
        S.ksp.restart = restart;
        S.ksp.rtol = rtol;
        S.ksp.atol = atol;
        S.ksp.divtol = divtol > 0 ? divtol : 1.0e4;
        S.ksp.max_it = max_it;
    });
}

// ---- host-array variants: stage through temporary device vectors
namespace {
void up(System &S, double *d, const double *h) {
    HIPCHK(hipMemcpyAsync(d, h, S.n_local * 8, hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
}
void down(System &S, const double *d, double *h) {
    HIPCHK(hipMemcpyAsync(h, d, S.n_local * 8, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
}
}  // namespace

int kkt_apply(kkt_handle h, const double *x, double *y) {
    KKT_TRY(h, {
        if (!x || !y) fail(KKT_ERR_ARG, "null vector");
        if (!S.finalized) fail(KKT_ERR_STATE, "system not finalized");
        S.require_values("kkt_apply");   // before anything is staged
        DevBuf<double> dx = S.new_vec(), dy = S.new_vec();
        up(S, dx.get(), x);
        S.apply(dx.get(), dy.get());
        down(S, dy.get(), y);
    });
}

int kkt_pc_apply(kkt_handle h, const double *x, double *y) {
    KKT_TRY(h, {
        if (!x || !y) fail(KKT_ERR_ARG, "null vector");
        if (!S.finalized) fail(KKT_ERR_STATE, "system not finalized");
        S.require_values("kkt_pc_apply");   // before anything is staged
        DevBuf<double> dx = S.new_vec(), dy = S.new_vec();
        up(S, dx.get(), x);
        S.pc_apply(dx.get(), dy.get());
        if (S.pc) {
            // a sweep program that timed out (on any rank of a time shard: the decision is
            // collective) is replaced by plain launches and the application redone (same
            // arithmetic)
            std::string why;
            if (S.pc_timed_out_agreed(&why)) {
                if (!S.pc_fallback_plain(why)) fail(KKT_ERR_HIP, why);
                S.pc_apply(dx.get(), dy.get());
                if (S.pc_timed_out_agreed(&why)) fail(KKT_ERR_HIP, why);
            }
        }
        down(S, dy.get(), y);
        if (S.pc_cb_failed) {
            S.pc_cb_failed = false;
            fail(KKT_ERR_CALLBACK, "Error encountered in preconditioner callback");
        }
    });
}

int kkt_solve(kkt_handle h, const double *b, double *u, int *its, int *reason, double *rnorm,
              double *hist, int hist_cap, int *hist_len) {
    KKT_TRY(h, {
        if (!b || !u) fail(KKT_ERR_ARG, "null vector");
        if (!S.finalized) fail(KKT_ERR_STATE, "system not finalized");
        S.require_values("kkt_solve");   // before anything is staged
        DevBuf<double> db = S.new_vec(), du = S.new_vec();
        up(S, db.get(), b);
        up(S, du.get(), u);
        S.solve(db.get(), du.get(), its, reason, rnorm, hist, hist_cap, hist_len);
        down(S, du.get(), u);
    });
}

// ---- device-resident variants
int64_t kkt_local_size(kkt_handle h) { return h ? h->S.n_local : -1; }

int kkt_vec_alloc(kkt_handle h, double **d_vec) {
    KKT_TRY(h, {
        if (!d_vec) fail(KKT_ERR_ARG, "null out pointer");
        if (!S.finalized) fail(KKT_ERR_STATE, "system not finalized");
        *d_vec = S.new_vec().release();   // the caller owns it (kkt_vec_free)
        S.sync();
    });
}
int kkt_vec_free(kkt_handle h, double *d_vec) {
    KKT_TRY(h, {
        if (d_vec) HIPCHK(hipFree(d_vec));
    });
}
int kkt_vec_upload(kkt_handle h, double *d_vec, const double *host) {
    KKT_TRY(h, up(S, d_vec, host));
}
int kkt_vec_download(kkt_handle h, const double *d_vec, double *host) {
    KKT_TRY(h, down(S, d_vec, host));
}
int kkt_apply_device(kkt_handle h, const double *d_x, double *d_y) {
    KKT_TRY(h, S.apply(d_x, d_y));
}
int kkt_pc_apply_device(kkt_handle h, const double *d_x, double *d_y) {
    KKT_TRY(h, S.pc_apply(d_x, d_y));
}
int kkt_solve_device(kkt_handle h, const double *d_b, double *d_u, int *its, int *reason,
                     double *rnorm, double *hist, int hist_cap, int *hist_len) {
    KKT_TRY(h, S.solve(d_b, d_u, its, reason, rnorm, hist, hist_cap, hist_len));
}
int kkt_sync(kkt_handle h) { KKT_TRY(h, S.sync()); }

int kkt_set_relinearisation(kkt_handle h, const kkt_relin_desc *desc) {
    KKT_TRY(h, relin_set(S, desc));
}
int kkt_relinearise_device(kkt_handle h, kkt_handle plan, const double *d_v, int n,
                           const kkt_relin_recipe *recipes) {
    KKT_TRY(h, {
        if (!plan) fail(KKT_ERR_ARG, "kkt_relinearise_device: null plan handle");
        relin_apply(S, plan->S, d_v, n, recipes);
    });
}
int kkt_picard_state(kkt_handle plan, int download, double *v, double *zeta, double *p,
                     double *mu) {
    KKT_TRY(plan, relin_state(S, download, v, zeta, p, mu));
}
int kkt_picard_window(kkt_handle plan, int out[8]) {
    KKT_TRY(plan, relin_window(S, out));
}
int kkt_picard_iterate(kkt_handle plan, double **d_v, double **d_zeta, double **d_p,
                       double **d_mu) {
    KKT_TRY(plan, relin_iterate(S, d_v, d_zeta, d_p, d_mu));
}
int kkt_picard_residual_device(kkt_handle plan, double *d_out, int rhs, double *norm) {
    KKT_TRY(plan, relin_residual(S, d_out, rhs, norm));
}
int kkt_picard_update_device(kkt_handle plan, double *d_u) {
    KKT_TRY(plan, relin_update(S, d_u));
}
int kkt_debug_relin_array(kkt_handle plan, int which, double *out, int64_t cap) {
    KKT_TRY(plan, relin_debug_array(S, which, out, cap));
}
int kkt_set_reaction_relinearisation(kkt_handle h, const kkt_reaction_desc *desc) {
    KKT_TRY(h, reaction_set(S, desc));
}
int kkt_reaction_relinearise(kkt_handle h, kkt_handle plan, int assemble, int n,
                             const kkt_relin_recipe *recipes) {
    KKT_TRY(h, {
        if (!plan) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: null plan handle");
        reaction_apply(S, plan->S, assemble, n, recipes);
    });
}
int kkt_reaction_state(kkt_handle plan, int download, double *v, double *zeta) {
    KKT_TRY(plan, reaction_state(S, download, v, zeta));
}
int kkt_reaction_window(kkt_handle plan, int out[8]) {
    KKT_TRY(plan, reaction_window(S, out));
}
int kkt_reaction_iterate(kkt_handle plan, double **d_v, double **d_zeta) {
    KKT_TRY(plan, reaction_iterate(S, d_v, d_zeta));
}
int kkt_reaction_residual_device(kkt_handle plan, double *d_out, int rhs, double *norm) {
    KKT_TRY(plan, reaction_residual(S, d_out, rhs, norm));
}
int kkt_reaction_update_device(kkt_handle plan, double *d_u) {
    KKT_TRY(plan, reaction_update(S, d_u));
}
int kkt_debug_reaction_array(kkt_handle plan, int which, double *out, int64_t cap) {
    KKT_TRY(plan, reaction_debug_array(S, which, out, cap));
}
int kkt_anderson_set(kkt_handle h, int depth, double beta, double cond_max) {
    KKT_TRY(h, anderson_set(S, depth, beta, cond_max));
}
int kkt_anderson_step(kkt_handle h, double *d_u, kkt_anderson_info *info) {
    KKT_TRY(h, anderson_step(S, d_u, info));
}
int kkt_anderson_reset(kkt_handle h) { KKT_TRY(h, anderson_reset(S)); }
int kkt_debug_anderson_op(kkt_handle h, kkt_anderson_op *op) {
    KKT_TRY(h, debug_anderson_op(S, op));
}
int kkt_debug_block_values(kkt_handle h, int quadrant, int i, int j, double *out, int64_t cap,
                           int64_t *nnz, int *padding_zero) {
    KKT_TRY(h, {
        if (!nnz || !padding_zero) fail(KKT_ERR_ARG, "kkt_debug_block_values: null argument");
        auto it = S.blocks.find(std::make_tuple(quadrant, i, j));
        if (it == S.blocks.end()) fail(KKT_ERR_ARG, "kkt_debug_block_values: no such block");
        const ValueArray &va = S.values[it->second.va];
        const Pattern &P = S.patterns[va.pattern];
        *nnz = P.nnz;
        if (!out) return KKT_OK;
        if (cap < P.nnz) fail(KKT_ERR_ARG, "kkt_debug_block_values: buffer too small");
        S.sync();
        std::vector<int32_t> map((size_t)P.npadded);
        std::vector<double> vals((size_t)P.npadded);
        HIPCHK(hipMemcpy(map.data(), P.d_sell2csr, P.npadded * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(vals.data(), va.d_vals, P.npadded * 8, hipMemcpyDeviceToHost));
        *padding_zero = 1;
        for (int64_t p = 0; p < P.npadded; ++p) {
            if (map[p] >= 0)
                out[map[p]] = vals[p];
            else if (vals[p] != 0.0 || std::signbit(vals[p]))
                *padding_zero = 0;
        }
    });
}

static void time_loop(System &S, bool pc, const double *d_x, double *d_y, int reps, float *ms) {
    if (reps < 1 || !ms) fail(KKT_ERR_ARG, "bad timing arguments");
    const Event e0 = Event::create(true), e1 = Event::create(true);
    HIPCHK(hipEventRecord(e0, S.stream));
    for (int r = 0; r < reps; ++r) {
        if (pc)
            S.pc_apply(d_x, d_y);
        else
            S.apply(d_x, d_y);
    }
    HIPCHK(hipEventRecord(e1, S.stream));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
}
int kkt_time_apply(kkt_handle h, const double *d_x, double *d_y, int reps, float *ms) {
    KKT_TRY(h, time_loop(S, false, d_x, d_y, reps, ms));
}
int kkt_time_pc_apply(kkt_handle h, const double *d_x, double *d_y, int reps, float *ms) {
    KKT_TRY(h, time_loop(S, true, d_x, d_y, reps, ms));
}

int kkt_time_pc_sweeps(kkt_handle h, const double *d_x, double *d_y, float *ms, int *launches,
                       int64_t *phases) {
    KKT_TRY(h, {
        if (!d_x || !d_y || !ms || !launches || !phases) fail(KKT_ERR_ARG, "null argument");
        S.pc_apply_timed(d_x, d_y, ms, launches, phases);
    });
}

int kkt_get_stage_times(kkt_handle h, kkt_stage_times *out) {
    KKT_TRY(h, {
        if (!out) fail(KKT_ERR_ARG, "null argument");
        *out = S.stage_times;
    });
}

int kkt_time_pc_stages(kkt_handle h, const double *d_x, double *d_y, kkt_pc_stage_times *out) {
    KKT_TRY(h, {
        if (!d_x || !d_y || !out) fail(KKT_ERR_ARG, "null argument");
        S.pc_apply_timed_stages(d_x, d_y, out);
    });
}

int kkt_coarse_setup_stats(kkt_handle h, kkt_coarse_stats *out) {
    KKT_TRY(h, {
        if (!out) fail(KKT_ERR_ARG, "null argument");
        *out = S.coarse_stats;
    });
}

int kkt_spectrum_stats_get(kkt_handle h, kkt_spectrum_stats *out) {
    KKT_TRY(h, {
        if (!out) fail(KKT_ERR_ARG, "null argument");
        *out = S.spectrum_stats;
    });
}

int kkt_debug_coarse_matrices(kkt_handle h, double *out, int64_t cap) {
    KKT_TRY(h, {
        if (!out && cap > 0) fail(KKT_ERR_ARG, "null argument");
        if ((size_t)cap < S.coarse_E.size()) fail(KKT_ERR_ARG, "buffer too small for the coarse matrices");
        std::copy(S.coarse_E.begin(), S.coarse_E.end(), out);
    });
}

int kkt_debug_coarse_inverses(kkt_handle h, double *out, int64_t cap) {
    KKT_TRY(h, {
        if (!out && cap > 0) fail(KKT_ERR_ARG, "null argument");
        if ((size_t)cap < S.coarse_Einv.size()) fail(KKT_ERR_ARG, "buffer too small for the coarse inverses");
        std::copy(S.coarse_Einv.begin(), S.coarse_Einv.end(), out);
    });
}

int kkt_debug_dense_inverse(kkt_handle h, int n, int nmat, const double *a, double *inv, int *bad) {
    KKT_TRY(h, {
        if (n < 1 || nmat < 1 || !a || !inv || !bad) fail(KKT_ERR_ARG, "bad dense inverse arguments");
        kkt::dense_inverse_host(S, n, nmat, a, inv, bad);
    });
}

int kkt_debug_coarse_correction(kkt_handle h, int batched, int nb, int64_t vstride, const double *r,
                                const double *x_in, const double *einv, double *rc, double *ec,
                                double *x_out, int32_t *shape) {
    KKT_TRY(h, kkt::coarse_correction_host(S, batched, nb, vstride, r, x_in, einv, rc, ec, x_out,
                                           shape));
}

int kkt_debug_krylov_op(kkt_handle h, int op, int64_t n, int nv, const double *w, const double *V,
                        const double *coef, double a, double b, double *w_out,
                        double *scalars_out, double *arena_out) {
    KKT_TRY(h, S.debug_krylov_op(op, n, nv, w, V, coef, a, b, w_out, scalars_out, arena_out));
}

int kkt_debug_block_op(kkt_handle h, kkt_block_op *op) {
    KKT_TRY(h, kkt::debug_block_op(S, op));
}

int kkt_debug_spectrum_op(kkt_handle h, kkt_spectrum_op *op) {
    KKT_TRY(h, kkt::debug_spectrum_op(S, op));
}

int kkt_debug_row_step(kkt_handle h, kkt_row_step *step) {
    KKT_TRY(h, kkt::debug_row_step(S, step));
}

int kkt_debug_tile_levels(kkt_handle h, kkt_tile_levels *run) {
    KKT_TRY(h, {
        if (!run) fail(KKT_ERR_ARG, "null argument");
        if (!S.pc) fail(KKT_ERR_STATE, "kkt_debug_tile_levels: no preconditioner built on this handle");
        S.pc->debug_tile_levels(run);
    });
}

int kkt_debug_set_steplock(kkt_handle h, const kkt_steplock *lock) {
    KKT_TRY(h, {
        if (!lock) {
            S.steplock = kkt_steplock{};
        } else {
            if (lock->n_steps < 1 || lock->restart < 1 || !lock->V || !lock->h || !lock->v_next)
                fail(KKT_ERR_ARG, "incomplete step-lock description");
            S.steplock = *lock;
        }
    });
}

// records -> out (NULL: count only); returns the record count
static int put_forms(const std::vector<int32_t> &rec, int per, int32_t *out, int cap) {
    const int n = (int)rec.size() / per;
    if (out) {
        if (cap < (int)rec.size()) fail(KKT_ERR_ARG, "buffer too small for the form records");
        std::copy(rec.begin(), rec.end(), out);
    }
    return n;
}

int kkt_debug_apply_forms(kkt_handle h, int32_t *out, int cap) {
    KKT_TRY(h, {
        if (!S.finalized) fail(KKT_ERR_STATE, "system not finalized");
        std::vector<int32_t> rec;
        for (size_t w = 0; w < S.apply_launches.size(); ++w) {
            const RowLaunch &L = S.apply_launches[w];
            int sorted = 0;
            for (const RowOp &op : S.h_apply_ops[w]) sorted |= op.perm != nullptr;
            // the test launch_rowops_grouped makes (System::apply)
            const bool grouped = L.ngroups > 0 && rowops_grouped_kernel(L.R, L.uniform_w);
            rec.insert(rec.end(), {L.R, L.uniform_w, grouped ? L.ngroups : 0, sorted});
        }
        return put_forms(rec, KKT_APPLY_FORM_INTS, out, cap);
    });
}

int kkt_debug_pc_forms(kkt_handle h, int32_t *out, int cap) {
    KKT_TRY(h, {
        std::vector<int32_t> rec;
        if (S.pc) S.pc->plain_forms(rec);
        return put_forms(rec, KKT_PC_FORM_INTS, out, cap);
    });
}

int kkt_debug_pc_alias(kkt_handle h, int32_t *out, int cap) {
    KKT_TRY(h, {
        std::vector<int32_t> rec;
        if (S.pc) S.pc->alias_records(rec);
        return put_forms(rec, KKT_PC_ALIAS_INTS, out, cap);
    });
}

static int put_records(const std::vector<double> &rec, int per, double *out, int cap) {
    const int n = (int)rec.size() / per;
    if (out) {
        if (cap < (int)rec.size()) fail(KKT_ERR_ARG, "buffer too small for the records");
        std::copy(rec.begin(), rec.end(), out);
    }
    return n;
}

int kkt_debug_pc_solves(kkt_handle h, double *out, int cap) {
    KKT_TRY(h, {
        std::vector<double> rec;
        if (S.pc) S.pc->solve_records(rec);
        return put_records(rec, KKT_PC_SOLVE_VALS, out, cap);
    });
}

int kkt_debug_pc_matrices(kkt_handle h, double *out, int cap) {
    KKT_TRY(h, {
        std::vector<double> rec;
        if (S.pc) S.pc->matrix_records(rec);
        return put_records(rec, KKT_PC_MATRIX_VALS, out, cap);
    });
}

int kkt_debug_mass_tile_values(kkt_handle h, int64_t *n_entries, int64_t *n_vals, double *copy,
                               int32_t *gpos, double *vals) {
    KKT_TRY(h, {
        if (!S.pc) fail(KKT_ERR_STATE, "no built-in preconditioner");
        S.pc->mass_tile_debug(n_entries, n_vals, copy, gpos, vals);
    });
}

int kkt_get_info(kkt_handle h, kkt_info *info) {
    KKT_TRY(h, {
        if (!info) fail(KKT_ERR_ARG, "null info");
        *info = S.info;
    });
}

// diagnostic builds only (make EXTRA=-DKKT_STAMPS): per-workgroup cycle sums of the
// persistent row program; not part of include/kkt.h
int kkt_debug_prog_stats(kkt_handle h, unsigned long long *out, int n) {
    KKT_TRY(h, {
        if (!S.pc) fail(KKT_ERR_STATE, "no built-in preconditioner");
        S.pc->debug_read(out, n);
    });
}

// ---- multi-GPU transport
int kkt_comm_unique_id(void *id_out_128) {
    if (!id_out_128) return KKT_ERR_ARG;
    try {
        rccl_unique_id(id_out_128);
        return KKT_OK;
    } catch (const Error &e) {
        g_create_error = e.msg;
        return e.code;
    }
}
int kkt_comm_init_rccl(kkt_handle h, const void *uid) {
    KKT_TRY(h, {
        if (!uid) fail(KKT_ERR_ARG, "null unique id");
        S.comm.reset(make_rccl_comm(S.rank, S.world, uid));
    });
}
int kkt_comm_init_callbacks(kkt_handle h, kkt_allreduce_fn ar, kkt_sendrecv_fn sr, void *user) {
    KKT_TRY(h, {
        if (!ar || !sr) fail(KKT_ERR_ARG, "null transport callbacks");
        S.comm.reset(make_callback_comm(ar, sr, user));
    });
}
int kkt_comm_barrier(kkt_handle h) {
    KKT_TRY(h, {
        if (S.comm)
            S.comm->barrier(S.stream);
        else
            S.sync();
    });
}
int kkt_comm_max(kkt_handle h, double *v) {
    KKT_TRY(h, {
        if (!v) fail(KKT_ERR_ARG, "null value");
        if (S.comm) *v = S.comm->max_host(*v, S.stream);
    });
}

}  // extern "C"
