// Host side of the Anderson mixer (anderson.hpp): the ring, the condition rule, the C-ABI's work.
#include "anderson.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "system.hpp"

namespace kkt {

// Unpivoted Cholesky of the trailing columns [d, c0) of G (lower triangle, i (i + 1) / 2 + j),
// oldest first; d grows until every pivot is positive and max L_ii / min L_ii <= cond_max.
int anderson_solve(const double *tri, int c0, double cond_max, double *gamma) {
    const double *r = tri + c0 * (c0 + 1) / 2;
    for (int d = 0; d < c0; ++d) {
        const int c = c0 - d;
        double L[ANDERSON_MAX][ANDERSON_MAX];
        double lmin = INFINITY, lmax = 0.0;
        bool ok = true;
        for (int i = 0; i < c && ok; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = tri[(d + i) * (d + i + 1) / 2 + d + j];
                for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
                if (j < i) {
                    L[i][j] = s / L[j][j];
                } else {
                    if (!(s > 0.0) || !std::isfinite(s)) {
                        ok = false;
                        break;
                    }
                    L[i][i] = std::sqrt(s);
                    lmin = std::min(lmin, L[i][i]);
                    lmax = std::max(lmax, L[i][i]);
                }
            }
        if (!ok || !(lmax / lmin <= cond_max)) continue;
        double y[ANDERSON_MAX];
        for (int i = 0; i < c; ++i) {            // L y = r
            double s = r[d + i];
            for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
        for (int i = c - 1; i >= 0; --i) {       // L^T gamma = y
            double s = y[i];
            for (int k = i + 1; k < c; ++k) s -= L[k][i] * gamma[k];
            gamma[i] = s / L[i][i];
        }
        return d;
    }
    return c0;
}

static void check_args(int depth, double beta, double cond_max) {
    if (depth < 1 || depth > ANDERSON_MAX)
        fail(KKT_ERR_ARG, "kkt_anderson_set: depth " + std::to_string(depth) + " is outside 0 .. " +
                              std::to_string(ANDERSON_MAX));
    if (!std::isfinite(beta) || beta == 0.0)
        fail(KKT_ERR_ARG, "kkt_anderson_set: beta must be finite and not zero");
    if (!(cond_max > 1.0)) fail(KKT_ERR_ARG, "kkt_anderson_set: cond_max must be above 1");
}

void anderson_set(System &S, int depth, double beta, double cond_max) {
    if (depth == 0) {
        S.anderson.reset();
        return;
    }
    check_args(depth, beta, cond_max);
    if (S.sharded)
        fail(KKT_ERR_STATE, "kkt_anderson_set: not offered on a time-sharded handle (the Gram sums "
                            "would have to be all-reduced)");
    if (!S.finalized) fail(KKT_ERR_STATE, "kkt_anderson_set: system not finalized");
    S.anderson.reset();
    auto M = std::make_unique<AndersonMixer>();
    M->depth = depth, M->beta = beta, M->cond_max = cond_max, M->n = S.n_local;
    for (int j = 0; j < depth; ++j) M->d_dF[j] = M->mem.adopt(S.new_vec());
    for (int j = 0; j < depth; ++j) M->d_dX[j] = M->mem.adopt(S.new_vec());
    M->d_fprev = M->mem.adopt(S.new_vec());
    M->d_part = M->mem.alloc<double>((size_t)(ANDERSON_BLOCKS + 1) * ANDERSON_DOTS_MAX);
    S.sync();
    S.anderson = std::move(M);
}

void anderson_reset(System &S) {
    if (!S.anderson) fail(KKT_ERR_STATE, "kkt_anderson_reset: no mixer on this handle");
    S.anderson->head = S.anderson->count = 0;
    S.anderson->have_prev = false;
}

namespace {
// HIP events around the three kernels of one step (option "stage_timers")
struct StepClock {
    bool on;
    hipStream_t st;
    Event ev[6];
    StepClock(bool on_, hipStream_t st_) : on(on_), st(st_) {
        if (on)
            for (Event &e : ev) e = Event::create(true);
    }
    void mark(int k) {
        if (on) HIPCHK(hipEventRecord(ev[k], st));
    }
    double ms(int k) {   // between marks 2 k and 2 k + 1 (after a synchronisation)
        float t = 0.0f;
        if (on) HIPCHK(hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]));
        return t;
    }
};

void expand(const double *tri, int c0, int d, double *G, double *r) {
    const int c = c0 - d;
    for (int i = 0; i < c; ++i) {
        for (int j = 0; j <= i; ++j)
            G[i * c + j] = G[j * c + i] = tri[(d + i) * (d + i + 1) / 2 + d + j];
        r[i] = tri[c0 * (c0 + 1) / 2 + d + i];
    }
}
}  // namespace

void anderson_step(System &S, double *d_u, kkt_anderson_info *info) {
    if (!S.anderson) fail(KKT_ERR_STATE, "kkt_anderson_step: no mixer on this handle");
    if (!d_u) fail(KKT_ERR_ARG, "kkt_anderson_step: null vector");
    AndersonMixer &M = *S.anderson;
    const int64_t n = M.n;
    hipStream_t st = S.stream;
    StepClock clk(S.opts.stage_timers && info, st);
    if (info) std::memset(info, 0, sizeof *info);

    const bool pushed = M.have_prev;
    if (pushed) {
        clk.mark(0);
        launch_anderson_push(st, d_u, M.d_fprev, M.d_dF[M.head], n);
        clk.mark(1);
        HIPCHK(hipGetLastError());
        M.head = (M.head + 1) % M.depth;
        M.count = std::min(M.count + 1, M.depth);
    } else {
        HIPCHK(hipMemcpyAsync(M.d_fprev, d_u, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                              st));
    }
    AndersonCols cols{};
    int c0 = M.count, dropped = 0;
    double tri[ANDERSON_DOTS_MAX] = {}, gamma[ANDERSON_MAX] = {};
    if (c0 > 0) {
        for (int j = 0; j < c0; ++j) cols.dF[j] = M.d_dF[M.slot(j)];
        clk.mark(2);
        launch_anderson_gram(st, cols, c0, d_u, n, M.d_part);
        clk.mark(3);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tri, M.d_part + (size_t)ANDERSON_BLOCKS * ANDERSON_DOTS_MAX,
                              (size_t)anderson_dots(c0) * sizeof(double), hipMemcpyDeviceToHost, st));
        S.sync();
        dropped = anderson_solve(tri, c0, M.cond_max, gamma);
        M.count = c0 - dropped;      // the dropped pairs leave the ring for good
    }
    const int c = M.count;
    cols = AndersonCols{};
    for (int j = 0; j < c; ++j) {
        cols.dF[j] = M.d_dF[M.slot(j)];
        cols.dX[j] = M.d_dX[M.slot(j)];
        cols.gamma[j] = gamma[j];
    }
    clk.mark(4);
    launch_anderson_mix(st, cols, c, M.beta, d_u, M.d_dX[M.head], n);
    clk.mark(5);
    HIPCHK(hipGetLastError());
    M.have_prev = true;
    if (info) {
        info->columns = c, info->dropped = dropped;
        std::copy(gamma, gamma + c, info->gamma);
        expand(tri, c0, dropped, info->G, info->r);
        if (clk.on) {
            S.sync();
            info->push_ms = pushed ? clk.ms(0) : 0.0;
            info->gram_ms = c0 > 0 ? clk.ms(1) : 0.0;
            info->mix_ms = clk.ms(2);
        }
    }
}

// ---- kkt_debug_anderson_op
namespace {
// a host array on the device, `slack` caller-filled doubles behind it where it is written
struct Staged {
    DevBuf<double> d;
    const double *src;
    size_t len;
    Staged(const double *h, size_t n) : d(DevBuf<double>::upload(h, n)), src(h), len(n) {}
    bool changed() const {
        std::vector<double> back(len);
        if (len) HIPCHK(hipMemcpy(back.data(), d.get(), len * sizeof(double), hipMemcpyDeviceToHost));
        return len && std::memcmp(back.data(), src, len * sizeof(double)) != 0;
    }
    void download(double *h) const {
        HIPCHK(hipMemcpy(h, d.get(), len * sizeof(double), hipMemcpyDeviceToHost));
    }
};
}  // namespace

void debug_anderson_op(System &S, kkt_anderson_op *op) {
    if (!op) fail(KKT_ERR_ARG, "kkt_debug_anderson_op: null argument");
    op->inputs_changed = 0;
    hipStream_t st = S.stream;
    if (op->op == KKT_ANDERSON_READ) {
        if (!S.anderson) fail(KKT_ERR_STATE, "kkt_debug_anderson_op: no mixer on this handle");
        const AndersonMixer &M = *S.anderson;
        op->ring[0] = M.head, op->ring[1] = M.count, op->ring[2] = M.have_prev, op->ring[3] = M.depth;
        if (!op->out) return;
        if (op->which < 0 || op->which > 2 || (op->which < 2 && (op->slot < 0 || op->slot >= M.depth)))
            fail(KKT_ERR_ARG, "kkt_debug_anderson_op: no such array of the ring");
        const double *src = op->which == 0 ? M.d_dF[op->slot] : op->which == 1 ? M.d_dX[op->slot] : M.d_fprev;
        S.sync();
        HIPCHK(hipMemcpy(op->out, src, (size_t)M.n * sizeof(double), hipMemcpyDeviceToHost));
        return;
    }
    const int c = op->c;
    const int64_t n = op->n, slack = op->slack;
    if (op->op < KKT_ANDERSON_PUSH || op->op > KKT_ANDERSON_MIX || n < 1 || slack < 0 || c < 0 ||
        c > ANDERSON_MAX || !op->f)
        fail(KKT_ERR_ARG, "kkt_debug_anderson_op: bad arguments");
    const size_t N = (size_t)n, W = (size_t)(n + slack);
    Staged f(op->f, N);
    if (op->op == KKT_ANDERSON_PUSH) {
        if (!op->f_prev || !op->out) fail(KKT_ERR_ARG, "kkt_debug_anderson_op: PUSH needs f_prev and out");
        Staged fp(op->f_prev, W), out(op->out, W);
        launch_anderson_push(st, f.d.get(), fp.d.get(), out.d.get(), n);
        HIPCHK(hipGetLastError());
        S.sync();
        op->inputs_changed = f.changed();
        fp.download(op->f_prev);
        out.download(op->out);
        return;
    }
    if (c > 0 && (!op->dF || (op->op == KKT_ANDERSON_MIX && !op->dX)))
        fail(KKT_ERR_ARG, "kkt_debug_anderson_op: null columns");
    std::vector<Staged> dF, dX;
    dF.reserve(c), dX.reserve(c);
    AndersonCols cols{};
    for (int j = 0; j < c; ++j) {
        dF.emplace_back(op->dF + (size_t)j * N, N);
        cols.dF[j] = dF.back().d.get();
    }
    if (op->op == KKT_ANDERSON_GRAM) {
        if (c > 0 && (!op->G || !op->r)) fail(KKT_ERR_ARG, "kkt_debug_anderson_op: GRAM needs G and r");
        if (c == 0) return;
        DevBuf<double> part = DevBuf<double>::alloc((size_t)(ANDERSON_BLOCKS + 1) * ANDERSON_DOTS_MAX);
        launch_anderson_gram(st, cols, c, f.d.get(), n, part.get());
        HIPCHK(hipGetLastError());
        S.sync();
        double tri[ANDERSON_DOTS_MAX];
        HIPCHK(hipMemcpy(tri, part.get() + (size_t)ANDERSON_BLOCKS * ANDERSON_DOTS_MAX,
                         (size_t)anderson_dots(c) * sizeof(double), hipMemcpyDeviceToHost));
        expand(tri, c, 0, op->G, op->r);
        op->inputs_changed = f.changed();
        for (const Staged &s : dF) op->inputs_changed += s.changed();
        return;
    }
    // MIX
    if (!op->out || !op->out2 || (op->alias && c < 1))
        fail(KKT_ERR_ARG, "kkt_debug_anderson_op: MIX needs out and out2 (alias: c >= 1)");
    for (int j = 0; j < c; ++j) {
        // the aliased column is written: it carries the slack and the caller's values behind it
        if (j == 0 && op->alias) {
            std::vector<double> h(op->out2, op->out2 + W);
            std::copy(op->dX, op->dX + N, h.begin());
            dX.emplace_back(h.data(), W);
            dX.back().src = nullptr;
        } else {
            dX.emplace_back(op->dX + (size_t)j * N, N);
        }
        cols.dX[j] = dX.back().d.get();
        cols.gamma[j] = op->gamma[j];
    }
    std::vector<double> hu(op->out, op->out + W);
    std::copy(op->f, op->f + N, hu.begin());
    Staged u(hu.data(), W), slot(op->out2, op->alias ? 0 : W);
    double *d_slot = op->alias ? dX[0].d.get() : slot.d.get();
    launch_anderson_mix(st, cols, c, op->beta, u.d.get(), d_slot, n);
    HIPCHK(hipGetLastError());
    S.sync();
    for (const Staged &s : dF) op->inputs_changed += s.changed();
    for (int j = op->alias ? 1 : 0; j < c; ++j) op->inputs_changed += dX[j].changed();
    u.download(op->out);
    if (op->alias)
        dX[0].download(op->out2);
    else
        slot.download(op->out2);
}

}  // namespace kkt
