// The host description of a launch of the preconditioner's row steps, once: how a RowOp / IlOp
// (kernels.hpp) is filled, how RowOps become a RowLaunch, and which launcher runs it.  SchurPC,
// StokesPC, the spectrum estimates, the coarse column path and kkt_debug_row_step all build and run
// their launches through these functions, so the launches the test hook pins are production's.
// Host-only: nothing here calls HIP (uploads go through the caller's DevPool, launches through
// the launchers of kernels.hpp, which kernel they pick through rows_kernel / shared_kernel there).
#pragma once
#include <algorithm>
#include <vector>

#include "system.hpp"

namespace kkt {

// an absolute device pointer as a vector operand (null: the operand is absent)
inline VRef vabs(const double *p) {
    return p ? VRef{(int64_t)(uintptr_t)p, 0, 0} : VRef{0, -1, 0};
}

struct RowTerm {
    const double *vals;
    const double *x;
};
struct LinStep {   // y = mask(ca * sum_t A_t x_t + cy * yin + cz * z)
    std::vector<RowTerm> terms;
    double *y;
    double ca = 1.0, cy = 0.0, cz = 0.0;
    const double *yin = nullptr, *z = nullptr;
    // optional fused first Chebyshev step of the solve that follows: y2 = c3 * dinv * y
    double *y2 = nullptr;
    const double *dinv = nullptr;
    double c3 = 0.0;
    // masked rows: y = malpha * mx (0 without mx)
    const double *mx = nullptr;
    double malpha = 0.0;
};
struct ChebStep {   // y = post2 (post1 (c1 pkm1 + c2 pk + c3 dinv (b - A x))), masked rows 0
    const double *vals;   // nullptr: no matrix term (first step)
    const double *dinv, *b, *pk, *pkm1;
    double *y;
    double c1, c2, c3, post1 = 1.0, post2 = 1.0;
    const double *x = nullptr;   // the vector the term multiplies where that is not pk
};

// The structure fields of an op on pattern P, every vector operand absent, every coefficient 0:
// the builders below set exactly the fields their mode's epilogue reads.
inline RowOp row_op(const Pattern &P, int64_t nrows, const uint8_t *rowmask) {
    RowOp op{};
    op.col = P.d_col;
    op.perm = P.d_perm;
    op.slice_off = P.d_slice_off;
    op.uniform_w = P.uniform_w;
    op.nrows = (int32_t)nrows;
    op.nslices = P.nslices;
    op.rowmask = rowmask;
    op.y = op.y2 = op.yin = op.z = op.mx = op.b = op.pk = op.pkm1 = vabs(nullptr);
    return op;
}
// The terms of an op.  None: width 0 everywhere, so that the slot loop of a kernel that is not
// unrolled for the launch's width runs no slot (with uniform_w >= 0 no kernel reads slice_off).
inline void set_terms(RowOp &op, const Pattern &P, const RowTerm *t, size_t n) {
    if (n > (size_t)MAX_TERMS) fail(KKT_ERR_STATE, "too many terms");
    op.nterms = (int32_t)n;
    op.uniform_w = n ? P.uniform_w : 0;
    for (size_t k = 0; k < n; ++k) op.t[k] = SpmvTerm{t[k].vals, vabs(t[k].x)};
}
inline RowOp lin_op(const Pattern &P, int64_t nrows, const uint8_t *rowmask, const LinStep &l) {
    RowOp op = row_op(P, nrows, rowmask);
    op.mode = EPI_LIN;
    set_terms(op, P, l.terms.data(), l.terms.size());
    op.y = vabs(l.y);
    op.ca = l.ca;
    op.cy = l.cy;
    op.cz = l.cz;
    op.yin = vabs(l.yin);
    op.z = vabs(l.z);
    op.y2 = vabs(l.y2);
    op.dinv = l.dinv;
    op.c3 = l.c3;
    op.mx = vabs(l.mx);
    op.malpha = l.malpha;
    return op;
}
inline RowOp cheb_op(const Pattern &P, int64_t nrows, const uint8_t *rowmask, const ChebStep &c) {
    RowOp op = row_op(P, nrows, rowmask);
    op.mode = EPI_CHEB;
    const RowTerm t{c.vals, c.x ? c.x : c.pk};
    set_terms(op, P, &t, c.vals ? 1 : 0);
    op.y = vabs(c.y);
    op.b = vabs(c.b);
    op.pk = vabs(c.pk);
    op.pkm1 = vabs(c.pkm1);
    op.dinv = c.dinv;
    op.c1 = c.c1;
    op.c2 = c.c2;
    op.c3 = c.c3;
    op.post1 = c.post1;
    op.post2 = c.post2;
    return op;
}

// One time level of an interleaved step: its right-hand side, its output (the last step of a solve;
// else null) and the factors this step applies to it
struct IlLevel {
    const double *b;
    double *out;
    double post1 = 1.0, post2 = 1.0;
};
// One group of nlev <= 4 levels of one interleaved Chebyshev step (x: interleaved p_k, null on
// the first step; y: the interleaved output of a step that is not the last)
inline IlOp il_op(const Pattern &P, int64_t nrows, const uint8_t *rowmask, const double *vals,
                  const double *dinv, const IlLevel *lev, int nlev, const double *x,
                  const double *pkm1, double *y, const TileCoef &k) {
    IlOp op{};
    op.col = P.d_col;
    op.slice_off = P.d_slice_off;
    op.perm = P.d_perm;
    op.vals = vals;
    op.dinv = dinv;
    op.rowmask = rowmask;
    op.nrows = (int32_t)nrows;
    op.nslices = P.nslices;
    op.uniform_w = P.uniform_w;
    op.nlev = nlev;
    op.x = x;
    op.pkm1 = pkm1;
    op.y = y;
    op.c1 = k.c1;
    op.c2 = k.c2;
    op.c3 = k.c3;
    for (int l = 0; l < 4; ++l) {
        const bool live = l < nlev;
        op.b[l] = live ? lev[l].b : nullptr;
        op.out[l] = live ? lev[l].out : nullptr;
        op.post1[l] = live ? lev[l].post1 : 1.0;
        op.post2[l] = live ? lev[l].post2 : 1.0;
    }
    return op;
}

// every op applies one and the same matrix (one term) to a vector given by an absolute pointer
inline bool one_shared_matrix(const std::vector<RowOp> &ops) {
    bool same = true;
    for (const RowOp &op : ops)
        same = same && op.nterms == 1 && op.t[0].vals == ops[0].t[0].vals && op.col == ops[0].col &&
               op.rowmask == ops[0].rowmask && op.t[0].x.base == 0;
    return same;
}
// The ops as one launch on pattern P, uploaded into `mem`.  kernarg: a single op rides in the
// kernel arguments.  shared_rows (option "shared_rows"): four ops per thread share the indices and
// values of one matrix -- launch_rowops_shared declines fewer than four ops, so fewer never raise
// the flag.
inline RowLaunch make_row_launch(DevPool &mem, const Pattern &P, const std::vector<RowOp> &ops,
                                 bool kernarg, bool shared_rows) {
    RowLaunch L;
    L.nops = (int)ops.size();
    L.max_slices = P.nslices;
    L.R = P.R;
    L.uniform_w = P.uniform_w;
    L.d_ops = mem.upload(ops.data(), ops.size());
    if (ops.size() == 1) {
        L.single = kernarg;
        L.h_op = ops[0];
    }
    L.shared_matrix = shared_rows && ops.size() >= 4 && one_shared_matrix(ops);
    return L;
}
// The kernel run_row_launch gives the launch
inline RowKernel row_launch_kernel(const RowLaunch &L) {
    if (L.shared_matrix) {
        const RowKernel k = shared_kernel(L.R, L.uniform_w, L.nops);
        if (!k.declined) return k;
    }
    return rows_kernel(L.R, L.uniform_w, L.nops, L.single);
}
// ... and the launch: the shared form where the ops qualify and the launcher accepts, else the
// plain launch with tag 1 and absolute pointers
inline void run_row_launch(hipStream_t st, const RowLaunch &L, bool pc_xcd) {
    if (L.shared_matrix &&
        launch_rowops_shared(st, L.d_ops, L.nops, L.max_slices, L.R, L.uniform_w, pc_xcd))
        return;
    const Bases B{{nullptr, nullptr, nullptr, nullptr}};
    launch_rowops(st, L.d_ops, L.nops, L.max_slices, L.R, B, 1, L.uniform_w,
                  L.single ? &L.h_op : nullptr);
}

}  // namespace kkt
