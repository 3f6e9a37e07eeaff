// Host side of the scalar reaction re-linearisation (include/kkt.h,
// kkt_set_reaction_relinearisation): plan upload and validation, assembly, residual and update.
// Kernels: reaction_kernels.hip; checks, gather and composition: compose.hpp.
#include "reaction.hpp"

#include <string>

#include "comm.hpp"
#include "system.hpp"

namespace kkt {

static void need(bool ok, const std::string &msg) {
    if (!ok) fail(KKT_ERR_ARG, "kkt_set_reaction_relinearisation: " + msg);
}

void reaction_set(System &S, const kkt_reaction_desc *d) {
    need(d != nullptr, "null descriptor");
    need(S.finalized, "the handle must be finalized");
    if (S.relin)
        fail(KKT_ERR_STATE, "kkt_set_reaction_relinearisation: the handle carries a Navier-Stokes "
                            "plan (kkt_set_relinearisation)");
    need(d->nq == 7 || d->nq == 15 || d->nq == 25,
         "nq must be 7 (P1 triangles, Radon's rule), 15 (P1 tetrahedra, Stroud's T3:5-1) or 25 "
         "(P2 triangles, the 5 x 5 conical rule; with nv = 9 Q2 quadrilaterals, the 5 x 5 "
         "Gauss-Legendre product rule)");
    const int inferred = d->nq == 7 ? 3 : d->nq == 15 ? 4 : 6;
    need(d->nv == 0 || d->nv == 3 || d->nv == 4 || d->nv == 6 || d->nv == 9,
         "nv must be 0 (inferred from nq), 3, 4, 6 or 9 (Q2 quadrilaterals, with nq = 25)");
    need(d->nv == 0 || d->nv == inferred || (d->nv == 9 && d->nq == 25),
         "nv = " + std::to_string(d->nv) + " contradicts nq = " + std::to_string(d->nq) +
             " (nq = 7: nv = 3, nq = 15: nv = 4, nq = 25: nv = 6 or 9)");
    const int nv = d->nv ? d->nv : inferred, ep = nv * nv;
    need(d->n_t >= 1 && d->ne > 0 && d->n1 > 0 && d->nnz > 0, "sizes must be positive");
    need(d->degree >= 0 && d->degree <= REACTION_MAX_DEGREE, "degree must be 0 .. 4");
    // n_t == 1: the stationary system [[M, D^T], [D, -(1/beta) M]] -- one level, no time step
    const bool stationary = d->n_t == 1;
    need(!stationary || d->cn == 0, "n_t == 1 (the stationary system) takes cn == 0");
    const int m = d->cn ? d->n_t - 1 : d->n_t;
    if (stationary) {
        need(S.n0 == 1 && S.n1 == 1,
             "n_t == 1: the handle is not the stationary system (one block per family)");
        need(S.nx0 == d->n1 && S.nx1 == d->n1,
             "n_t == 1: the handle is not the stationary system of this space");
        need(!S.CN, "n_t == 1: the stationary system is not a Crank-Nicolson handle");
        need(!S.sharded, "n_t == 1: the stationary system has one block and cannot be time-sharded");
    }
    need(S.n0 == m && S.n1 == m && S.nx0 == d->n1 && S.nx1 == d->n1 && S.CN == (d->cn != 0),
         "the handle is not the scalar instationary system of this space and these time levels");
    need(!S.sharded || (S.families == 1 && S.mf == m),
         "a time-sharded handle must shard the one block family of the scalar system by level");
    need(d->cells && d->W && d->lam && d->L && d->M && d->data && (d->n_bc == 0 || d->bc_idx),
         "null array");
    const int64_t n1 = d->n1, nnz = d->nnz, ne = d->ne;
    const int64_t n_entries = ne * ep;
    const std::string api = "kkt_set_reaction_relinearisation: ";
    check_range(api + "cells", d->cells, ne * nv, n1);
    check_csr(api + "pattern", d->indptr, d->indices, n1, n1, nnz);
    check_perm(api + "tperm", d->tperm, nnz);
    check_lists(api + "contribution lists", d->cptr, d->clist, nnz, n_entries);
    check_range(api + "bc_idx", d->bc_idx, d->n_bc, n1);

    auto P = std::make_unique<ReactionPlan>();
    // the rank's block rows and the level windows its rows read
    P->w = level_windows(d->n_t, d->cn != 0, S.sharded ? S.lo : 0, S.sharded ? S.hi : m);
    const LevelWindows &w = P->w;
    P->stationary = stationary;
    P->nv = nv;
    P->nq = d->nq;
    P->ep = ep;
    P->ne = ne;
    P->n1 = n1;
    P->nnz = nnz;
    P->tau = d->tau;
    P->beta = d->beta;
    P->coef.degree = d->degree;
    for (int k = 0; k <= REACTION_MAX_DEGREE; ++k) P->coef.c[k] = k <= d->degree ? d->c[k] : 0.0;
    P->d_cells = P->mem.upload(d->cells, ne * nv);
    P->d_W = P->mem.upload(d->W, ne * d->nq);
    P->d_lam = P->mem.upload(d->lam, (int64_t)d->nq * nv);
    P->d_ip = P->mem.upload(d->indptr, n1 + 1);
    P->d_ix = P->mem.upload(d->indices, nnz);
    P->d_tperm = P->mem.upload(d->tperm, nnz);
    P->d_cptr = P->mem.upload(d->cptr, nnz + 1);
    P->d_clist = P->mem.upload(d->clist, n_entries);
    P->d_L = P->mem.upload(d->L, nnz);
    P->d_M = P->mem.upload(d->M, nnz);
    P->d_bc = upload_bc_mask(P->mem, d->bc_idx, d->n_bc, n1);
    P->d_data = upload_data_rows(P->mem, w, d->data, n1);
    if (S.sharded && w.CN) {
        P->d_rhalo = P->mem.alloc<double>(2 * n1);
        HIPCHK(hipMemset(P->d_rhalo, 0, 2 * n1 * 8));
    }
    // E is a hipMalloc of its own, so 256-byte aligned: the 16-byte stores of the
    // tetrahedral and the P2 kernel rely on it (128 and 288 bytes a matrix; a Q2 matrix has
    // 648 bytes, is only 8-byte aligned and is written in runs of 8-byte stores).  n_entries fits an int32 (check_lists:
    // cptr[nnz] == n_entries), so n_entries * D_n * 8 stays far inside int64
    P->d_E = P->mem.alloc<double>(n_entries * w.D_n);
    P->d_D = P->mem.alloc<double>(nnz * w.D_n);
    P->d_v = P->mem.alloc<double>(w.v_n * n1);
    P->d_zeta = P->mem.alloc<double>(w.z_n * n1);
    HIPCHK(hipMemset(P->d_v, 0, w.v_n * n1 * 8));
    HIPCHK(hipMemset(P->d_zeta, 0, w.z_n * n1 * 8));
    P->d_red = P->mem.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX + 2);
    P->compose.n_t = d->n_t;
    P->compose.spaces = {{"scalar", std::vector<int32_t>(d->indptr, d->indptr + n1 + 1),
                          std::vector<int32_t>(d->indices, d->indices + nnz), nnz, 1, P->d_D,
                          w.D_l0, w.D_n, P->d_M, P->d_tperm}};
    S.reaction = std::move(P);
}

static ReactionPlan &plan_of(System &S) {
    if (!S.reaction)
        fail(KKT_ERR_STATE, "no reaction plan on this handle (kkt_set_reaction_relinearisation)");
    return *S.reaction;
}

void reaction_apply(System &T, System &PS, int assemble, int n, const kkt_relin_recipe *rec) {
    ReactionPlan &P = plan_of(PS);
    check_apply_target("kkt_reaction_relinearise", T, PS, n, rec);
    // every recipe is validated before anything is written
    std::vector<ComposeJob> jobs = compose_jobs("kkt_reaction_relinearise", T, P.compose, n, rec);
    if (assemble) {
        exchange_iterate_halos(PS, P.w, P.d_v, P.d_zeta, P.n1);
        launch_reaction_elements(PS.stream, P);
        // D = 1.0 * L[k] + acc: the product is exact, so this is L + C with one rounding
        launch_relin_gather_one(PS.stream, P.d_cptr, P.d_clist, P.d_E, P.ne * P.ep, P.d_L, 1.0,
                                P.nnz, P.w.D_n, P.d_D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(PS.stream));
        P.assembled = true;
    }
    if (n == 0) return;
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_reaction_relinearise: nothing assembled yet");
    compose_run(T, P.compose, jobs, rec);
}

// Host arrays of the global shapes, by iterate_spans.
void reaction_state(System &S, int download, double *v, double *zeta) {
    ReactionPlan &P = plan_of(S);
    copy_spans(S.stream, download != 0,
               iterate_spans(P.w, download != 0, P.d_v, P.d_zeta, v, zeta, P.n1));
}

void reaction_window(System &S, int out[8]) {
    ReactionPlan &P = plan_of(S);
    if (!out) fail(KKT_ERR_ARG, "kkt_reaction_window: null argument");
    P.w.report(out);
}

void reaction_iterate(System &S, double **v, double **zeta) {
    ReactionPlan &P = plan_of(S);
    if (v) *v = P.d_v;
    if (zeta) *zeta = P.d_zeta;
}

void reaction_residual(System &S, double *d_out, int rhs, double *norm) {
    ReactionPlan &P = plan_of(S);
    if (!d_out || !norm) fail(KKT_ERR_ARG, "kkt_reaction_residual_device: null argument");
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_reaction_residual_device: D not assembled yet");
    // backward Euler's right-hand side is the rows themselves, and so is the stationary system's
    const bool transform = rhs && P.w.CN;
    double *r = transform ? raw_rows(S) : d_out;
    if (P.stationary)
        launch_reaction_stationary_residual(S.stream, P, r);
    else
        launch_reaction_residual(S.stream, P, r);
    launch_residual_norm(S, r, P.d_red);
    if (transform && S.sharded) {
        // the raw rows the time transforms read across the shard boundary: the adjoint rows (T_1)
        // send their first row down, the state rows (T_2) their last row up
        const int up = P.w.up(S.rank), dn = P.w.dn(S.rank);
        const int64_t n1 = P.n1, nl = P.w.nl;
        S.comm->sendrecv(r, n1, dn, P.d_rhalo, n1, up, S.stream);
        S.comm->sendrecv(r + (2 * nl - 1) * n1, n1, up, P.d_rhalo + n1, n1, dn, S.stream);
    }
    if (transform) launch_reaction_rhs(S.stream, P, r, d_out);
    read_residual_norm(S, P.d_red, norm);
}

void reaction_update(System &S, double *d_u) {
    ReactionPlan &P = plan_of(S);
    if (!d_u) fail(KKT_ERR_ARG, "kkt_reaction_update_device: null update");
    launch_reaction_update(S.stream, P, d_u);
    HIPCHK(hipGetLastError());
}

void reaction_debug_array(System &S, int which, double *out, int64_t cap) {
    ReactionPlan &P = plan_of(S);
    const std::vector<DebugArray> arrays = {
        {P.d_E, P.ne * P.ep, P.w.D_n, true}, {P.d_D, P.nnz, P.w.D_n, true},
        {P.d_v, P.n1, P.w.v_n, false}, {P.d_zeta, P.n1, P.w.z_n, false}};
    copy_debug_array("kkt_debug_reaction_array", S, arrays, P.assembled, which, out, cap);
}

}  // namespace kkt
