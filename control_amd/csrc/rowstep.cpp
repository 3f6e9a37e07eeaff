// kkt_debug_row_step: one launch of the preconditioner's row steps on host data (include/kkt.h
// documents the arguments).  As blockops.cpp, nothing here computes and there is no second path:
// the vectors go up, the ops are filled and the launch is built and run by the functions of
// rowlaunch.hpp that SchurPC and StokesPC use, once on the handle's stream, the vectors come back;
// `family` and `width` are the launcher's own choice (rows_kernel / shared_kernel / il_kernel).
// Every vector sits between guards; what the launch only reads is downloaded again and compared
// with what went up.  The epilogue chain the launches run is the one epilogue.hpp writes (candidate
// "ff" of tests/rowstep_ref.py), which the test asserts.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rowlaunch.hpp"

namespace kkt {

namespace {

constexpr size_t G = KKT_BLOCK_GUARD;
static_assert(KKT_ROWSTEP_MAX_TERMS == MAX_TERMS, "kkt.h restates MAX_TERMS");
static_assert(KKT_ROWSTEP_PC_ROWS == (int)ROW_PC_ROWS && KKT_ROWSTEP_PC_ROW_STEP == (int)ROW_PC_ROW_STEP &&
                  KKT_ROWSTEP_PC_ROWS_SHARED == (int)ROW_PC_ROWS_SHARED &&
                  KKT_ROWSTEP_PC_ROWS_SHARED_G == (int)ROW_PC_ROWS_SHARED_G &&
                  KKT_ROWSTEP_PC_ROWS_IL == (int)ROW_PC_ROWS_IL,
              "kkt.h restates RowFamily");

[[noreturn]] void bad(const char *what) {
    fail(KKT_ERR_ARG, std::string("kkt_debug_row_step: ") + what);
}

struct Watch {   // an array the launch must leave as it is
    const void *dev;
    const void *host;
    size_t bytes;
};

// the value array of a stored block, which must have the pattern `pat`
const double *block_values(const System &S, int q, int i, int j, int pat) {
    const auto it = S.blocks.find({q, i, j});
    if (it == S.blocks.end()) bad("a term names a block that is not stored");
    const ValueArray &va = S.values[it->second.va];
    if (va.pattern != pat) bad("a term block has another pattern than the call's");
    return va.d_vals;
}

}  // namespace

void debug_row_step(System &S, kkt_row_step *pa) {
    if (!pa) bad("null argument");
    kkt_row_step &a = *pa;
    if (!S.finalized) fail(KKT_ERR_STATE, "kkt_debug_row_step: system not finalized");
    if (a.form < KKT_ROWSTEP_ROWS || a.form > KKT_ROWSTEP_INTERLEAVED) bad("unknown form");
    if (a.nops < 1 || a.nops > 64 || !a.ops) bad("nops must be 1..64");
    if (a.nvec < 1 || a.nvec > 1024 || !a.vecs) bad("nvec must be 1..1024");
    const auto bit = S.blocks.find({a.q, a.i, a.j});
    if (bit == S.blocks.end()) bad("the pattern block is not stored");
    const int pat = S.values[bit->second.va].pattern;
    const Pattern &P = S.patterns[pat];
    if (P.nrows != P.ncols) bad("the pattern must be square");
    if (P.nrows < 1 || P.nslices < 1) bad("empty pattern");
    const size_t n = (size_t)P.nrows, slot = n + 2 * G;
    const bool il = a.form == KKT_ROWSTEP_INTERLEAVED;
    if ((a.form == KKT_ROWSTEP_SHARED || il) && P.R != 2) bad("this form needs R = 2");
    if (a.form == KKT_ROWSTEP_SINGLE && a.nops != 1) bad("SINGLE takes one op");

    // ---- checks: operands, aliasing
    auto in_table = [&](int v) { return v >= -1 && v < a.nvec; };
    std::vector<int> writes(a.nvec, 0), reads(a.nvec, 0);
    for (int k = 0; k < a.nops; ++k) {
        const kkt_row_step_op &o = a.ops[k];
        if (o.mode != KKT_ROWSTEP_LIN && o.mode != KKT_ROWSTEP_CHEB) bad("unknown mode");
        if (o.nterms < 0 || o.nterms > MAX_TERMS) bad("nterms must be 0..MAX_TERMS");
        for (int v : {o.y, o.y2, o.yin, o.z, o.mx, o.b, o.pkm1, o.pk})
            if (!in_table(v)) bad("vector index outside the table");
        for (int t = 0; t < o.nterms; ++t)
            if (o.term_x[t] < 0 || o.term_x[t] >= a.nvec) bad("term vector outside the table");
        if (il) {
            if (o.mode != KKT_ROWSTEP_CHEB) bad("interleaved levels are Chebyshev steps");
            if (o.b < 0) bad("a level without right-hand side");
            if (!a.il_y && o.y < 0) bad("the last interleaved step needs every level's output");
            reads[o.b]++;
            if (!a.il_y) writes[o.y]++;
            continue;
        }
        if (o.y < 0) bad("an op without output");
        const bool lin = o.mode == KKT_ROWSTEP_LIN;
        writes[o.y]++;
        if (lin && o.y2 >= 0) writes[o.y2]++;
        if (lin && o.y2 >= 0 && !a.dinv) bad("y2 needs dinv");
        if (!lin && (!a.dinv || o.b < 0)) bad("a Chebyshev step needs b and dinv");
        for (int t = 0; t < o.nterms; ++t) reads[o.term_x[t]]++;
        if (lin) {
            for (int v : {o.z, o.mx})
                if (v >= 0) reads[v]++;
            if (o.yin >= 0 && o.yin != o.y) reads[o.yin]++;   // yin == y: the update in place
        } else {
            for (int v : {o.b, o.pkm1, o.pk})
                if (v >= 0) reads[v]++;
        }
    }
    for (int v = 0; v < a.nvec; ++v) {
        if (writes[v] > 1) bad("two outputs of the launch are the same vector");
        if (writes[v] && reads[v]) bad("aliasing the drivers do not produce");
    }
    if (il) {
        if (!a.dinv) bad("a Chebyshev step needs dinv");
        if (a.il_pkm1 && !a.il_x) bad("p_{k-1} without p_k");
        if (a.ops[0].nterms != 1) bad("ops[0] of an interleaved step names the matrix (one term)");
    }

    // ---- upload
    hipStream_t st = S.stream;
    DevPool pool;
    std::vector<Watch> watched;
    auto input = [&](const auto *h, size_t cnt) {
        const auto *d = h ? pool.upload(h, cnt) : nullptr;
        if (h) watched.push_back({d, h, cnt * sizeof(*h)});
        return d;
    };
    for (int v = 0; v < a.nvec; ++v) {
        double *h = a.vecs + (size_t)v * slot;
        std::fill(h, h + G, KKT_KRYLOV_PAD);
        std::fill(h + G + n, h + slot, KKT_KRYLOV_PAD);
    }
    double *d_vecs = pool.upload(a.vecs, (size_t)a.nvec * slot);
    auto vec = [&](int v) -> double * { return v < 0 ? nullptr : d_vecs + (size_t)v * slot + G; };
    const uint8_t *d_mask = input(a.rowmask, n);
    const double *d_dinv = input(a.dinv, n);

    a.R = P.R;
    a.uniform_w = P.uniform_w;
    a.sorted = P.d_perm != nullptr;
    a.nslices = P.nslices;
    a.launched = 1;
    const size_t n_il = (size_t)((a.nops + 3) / 4) * 4 * n;
    double *d_il_y = nullptr;

    if (il) {
        const double *d_x = input(a.il_x, n_il), *d_pkm1 = input(a.il_pkm1, n_il);
        if (a.il_y) {
            std::fill(a.il_y, a.il_y + G, KKT_KRYLOV_PAD);
            std::fill(a.il_y + G + n_il, a.il_y + n_il + 2 * G, KKT_KRYLOV_PAD);
            d_il_y = pool.upload(a.il_y, n_il + 2 * G) + G;
        }
        // (every step names the matrix, the first one too, which does not read it)
        const double *vals = block_values(S, a.ops[0].term_q[0], a.ops[0].term_i[0],
                                          a.ops[0].term_j[0], pat);
        const int ng = (a.nops + 3) / 4;
        std::vector<IlOp> ops((size_t)ng);
        const TileCoef coef{a.ops[0].c1, a.ops[0].c2, a.ops[0].c3};
        for (int g = 0; g < ng; ++g) {
            const int nlev = std::min(4, a.nops - 4 * g);
            IlLevel lev[4];
            for (int l = 0; l < nlev; ++l) {
                const kkt_row_step_op &o = a.ops[4 * g + l];
                lev[l] = IlLevel{vec(o.b), a.il_y ? nullptr : vec(o.y), o.post1, o.post2};
            }
            ops[(size_t)g] = il_op(P, P.nrows, d_mask, vals, d_dinv, lev, nlev,
                                   d_x ? d_x + (size_t)g * 4 * n : nullptr,
                                   d_pkm1 ? d_pkm1 + (size_t)g * 4 * n : nullptr,
                                   d_il_y ? d_il_y + (size_t)g * 4 * n : nullptr, coef);
        }
        const IlOp *d_ops = pool.upload(ops.data(), ops.size());
        const RowKernel k = il_kernel(P.uniform_w);
        a.family = k.family;
        a.width = k.width;
        launch_rowops_il(st, d_ops, ng, P.nslices, P.uniform_w, a.pc_xcd != 0);
    } else {
        const bool shared = a.form == KKT_ROWSTEP_SHARED;
        std::vector<RowOp> ops((size_t)a.nops);
        for (int k = 0; k < a.nops; ++k) {
            const kkt_row_step_op &o = a.ops[k];
            std::vector<RowTerm> terms((size_t)o.nterms);
            for (int t = 0; t < o.nterms; ++t)
                terms[(size_t)t] = RowTerm{block_values(S, o.term_q[t], o.term_i[t], o.term_j[t], pat),
                                           vec(o.term_x[t])};
            if (o.mode == KKT_ROWSTEP_LIN) {
                ops[(size_t)k] = lin_op(P, P.nrows, d_mask,
                                        LinStep{terms, vec(o.y), o.ca, o.cy, o.cz, vec(o.yin), vec(o.z),
                                                vec(o.y2), d_dinv, o.c3, vec(o.mx), o.malpha});
            } else {
                ops[(size_t)k] = cheb_op(P, P.nrows, d_mask,
                                         ChebStep{nullptr, d_dinv, vec(o.b), vec(o.pk), vec(o.pkm1),
                                                  vec(o.y), o.c1, o.c2, o.c3, o.post1, o.post2});
                set_terms(ops[(size_t)k], P, terms.data(), terms.size());   // any number, any vector
            }
        }
        // SHARED: the launch SchurPC::push_rows flags -- the ops must qualify, and where the
        // launcher declines (fewer than four ops) nothing runs: no fall-back to the plain launch
        const RowLaunch L = make_row_launch(pool, P, ops, a.form == KKT_ROWSTEP_SINGLE, shared);
        const RowKernel k = shared ? shared_kernel(L.R, L.uniform_w, L.nops) : row_launch_kernel(L);
        if (shared && !one_shared_matrix(ops)) bad("SHARED ops have one term each, all the same block");
        // (pc_rows_shared<W> takes position == row; find_or_add_pattern gives row-sorted
        // storage no uniform width)
        if (k.family == ROW_PC_ROWS_SHARED && P.d_perm) bad("row-sorted storage with a fixed width");
        a.family = k.family;
        a.width = k.width;
        a.launched = k.declined ? 0 : 1;
        if (!k.declined) run_row_launch(st, L, a.pc_xcd != 0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));

    // ---- download: written slots come back, the others are compared
    int32_t changed = 0;
    std::vector<double> back((size_t)a.nvec * slot);
    HIPCHK(hipMemcpy(back.data(), d_vecs, back.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int v = 0; v < a.nvec; ++v) {
        double *h = a.vecs + (size_t)v * slot;
        const double *d = back.data() + (size_t)v * slot;
        if (writes[v])
            std::copy(d, d + slot, h);
        else
            changed += std::memcmp(d, h, slot * sizeof(double)) != 0;
    }
    if (d_il_y)
        HIPCHK(hipMemcpy(a.il_y, d_il_y - G, (n_il + 2 * G) * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<char> buf;
    for (const Watch &w : watched) {
        buf.resize(w.bytes);
        HIPCHK(hipMemcpy(buf.data(), w.dev, w.bytes, hipMemcpyDeviceToHost));
        changed += std::memcmp(buf.data(), w.host, w.bytes) != 0;
    }
    a.inputs_changed = changed;
}

}  // namespace kkt
