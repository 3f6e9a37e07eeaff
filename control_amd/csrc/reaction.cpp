// Host side of the scalar reaction re-linearisation (include/kkt.h,
// kkt_set_reaction_relinearisation): plan upload and validation, assembly, residual and update.
// Kernels: reaction_kernels.hip; checks, gather and composition: compose.hpp.
#include "reaction.hpp"

#include <algorithm>
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
    need(d->nq == 7 || d->nq == 15,
         "nq must be 7 (P1 triangles, Radon's rule) or 15 (P1 tetrahedra, Stroud's T3:5-1)");
    const int nv = d->nq == 7 ? 3 : 4, ep = nv * nv;
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
    P->n_t = d->n_t;
    P->m = m;
    P->CN = d->cn != 0;
    P->stationary = stationary;
    P->nv = nv;
    P->nq = d->nq;
    P->ep = ep;
    P->ne = ne;
    P->n1 = n1;
    P->nnz = nnz;
    P->tau = d->tau;
    P->beta = d->beta;
    // the rank's block rows and the level windows its rows read (reaction.hpp)
    const int lo = S.sharded ? S.lo : 0, hi = S.sharded ? S.hi : m, nl = hi - lo;
    P->lo = lo;
    P->nl = nl;
    P->v_halo = lo > 0;
    P->z_halo = hi < m;
    if (P->CN) {
        P->v_l0 = P->z_l0 = P->D_l0 = lo;
        P->v_n = P->z_n = P->D_n = nl + 1;
    } else {
        P->v_l0 = lo - (P->v_halo ? 1 : 0);
        P->v_n = hi - P->v_l0;
        P->z_l0 = lo;
        P->z_n = nl + (P->z_halo ? 1 : 0);
        P->D_l0 = lo;
        P->D_n = nl;
    }
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
    std::vector<uint8_t> bc(n1, 0);
    for (int64_t k = 0; k < d->n_bc; ++k) bc[d->bc_idx[k]] = 1;
    P->d_bc = P->mem.upload(bc.data(), n1);
    // the data rows of the owned blocks: lo..hi-1 of the adjoint rows, m+lo..m+hi-1 of the state rows
    P->d_data = P->mem.alloc<double>(2 * (int64_t)nl * n1);
    for (int f = 0; f < 2; ++f)
        HIPCHK(hipMemcpy(P->d_data + (int64_t)f * nl * n1, d->data + ((int64_t)f * m + lo) * n1,
                         (int64_t)nl * n1 * 8, hipMemcpyHostToDevice));
    if (S.sharded && P->CN) {
        P->d_rhalo = P->mem.alloc<double>(2 * n1);
        HIPCHK(hipMemset(P->d_rhalo, 0, 2 * n1 * 8));
    }
    P->d_E = P->mem.alloc<double>(n_entries * P->D_n);
    P->d_D = P->mem.alloc<double>(nnz * P->D_n);
    P->d_v = P->mem.alloc<double>(P->v_n * n1);
    P->d_zeta = P->mem.alloc<double>(P->z_n * n1);
    HIPCHK(hipMemset(P->d_v, 0, P->v_n * n1 * 8));
    HIPCHK(hipMemset(P->d_zeta, 0, P->z_n * n1 * 8));
    P->d_red = P->mem.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX + 2);
    P->compose.n_t = d->n_t;
    P->compose.spaces = {{"scalar", std::vector<int32_t>(d->indptr, d->indptr + n1 + 1),
                          std::vector<int32_t>(d->indices, d->indices + nnz), nnz, 1, P->d_D,
                          P->D_l0, P->D_n, P->d_M, P->d_tperm}};
    S.reaction = std::move(P);
}

static ReactionPlan &plan_of(System &S) {
    if (!S.reaction)
        fail(KKT_ERR_STATE, "no reaction plan on this handle (kkt_set_reaction_relinearisation)");
    return *S.reaction;
}

// One level of v up and one of zeta down, after the update and before the assembly: v of my
// last block (BE level hi - 1, CN level hi) is the first level of the window above, zeta of my
// first block the last level of the window below.  Levels are contiguous: nothing is packed.
void reaction_exchange(System &S) {
    ReactionPlan &P = plan_of(S);
    if (!S.sharded) return;
    if (!S.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
    const int up = P.z_halo ? S.rank + 1 : -1, dn = P.v_halo ? S.rank - 1 : -1;
    const int v_last = P.lo + P.nl - 1 + (P.CN ? 1 : 0);
    S.comm->sendrecv(P.d_v + (int64_t)(v_last - P.v_l0) * P.n1, P.n1, up, P.d_v, P.n1, dn, S.stream);
    S.comm->sendrecv(P.d_zeta, P.n1, dn, P.d_zeta + (int64_t)(P.z_n - 1) * P.n1, P.n1, up,
                     S.stream);
}

void reaction_apply(System &T, System &PS, int assemble, int n, const kkt_relin_recipe *rec) {
    ReactionPlan &P = plan_of(PS);
    if (n < 0 || (n > 0 && !rec)) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: bad recipe list");
    if (T.device != PS.device) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: plan on another device");
    if (!T.finalized) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: the target must be finalized");
    if (T.sharded != PS.sharded || (T.sharded && (T.lo != PS.lo || T.hi != PS.hi)))
        fail(KKT_ERR_ARG, "kkt_reaction_relinearise: the target is not sharded as the plan's handle");
    // every recipe is validated before anything is written
    std::vector<ComposeJob> jobs = compose_jobs("kkt_reaction_relinearise", T, P.compose, n, rec);
    if (assemble) {
        reaction_exchange(PS);
        launch_reaction_elements(PS.stream, P);
        // D = 1.0 * L[k] + acc: the product is exact, so this is L + C with one rounding
        launch_relin_gather_one(PS.stream, P.d_cptr, P.d_clist, P.d_E, P.ne * P.ep, P.d_L, 1.0,
                                P.nnz, P.D_n, P.d_D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(PS.stream));
        P.assembled = true;
    }
    if (n == 0) return;
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_reaction_relinearise: nothing assembled yet");
    compose_run(T, P.compose, jobs, rec);
}

// Host arrays of the global shapes.  Upload: the rank's windows, halo levels included.
// Download: the levels the rank owns (BE: v, zeta of its blocks; CN: v one level up), and the
// fixed levels -- CN's v_0, zeta of the last level -- on the rank whose window holds them; the
// rest of the host arrays is left as it is.  (One rank: every level, both ways.)
void reaction_state(System &S, int download, double *v, double *zeta) {
    ReactionPlan &P = plan_of(S);
    const int hi = P.lo + P.nl;
    int v0 = P.v_l0, v1 = P.v_l0 + P.v_n, z0 = P.z_l0, z1 = P.z_l0 + P.z_n;
    if (download) {
        v0 = P.CN ? (P.lo == 0 ? 0 : P.lo + 1) : P.lo;
        v1 = P.CN ? hi + 1 : hi;
        z1 = P.CN && hi == P.m ? hi + 1 : hi;
    }
    copy_spans(S.stream, download != 0,
               {{P.d_v + (int64_t)(v0 - P.v_l0) * P.n1, v ? v + (int64_t)v0 * P.n1 : nullptr,
                 (v1 - v0) * P.n1},
                {P.d_zeta + (int64_t)(z0 - P.z_l0) * P.n1,
                 zeta ? zeta + (int64_t)z0 * P.n1 : nullptr, (z1 - z0) * P.n1}});
}

void reaction_window(System &S, int out[8]) {
    ReactionPlan &P = plan_of(S);
    if (!out) fail(KKT_ERR_ARG, "kkt_reaction_window: null argument");
    const int w[8] = {P.v_l0, P.v_l0 + P.v_n, P.z_l0, P.z_l0 + P.z_n, P.D_l0, P.D_l0 + P.D_n,
                      P.lo, P.lo + P.nl};
    std::copy(w, w + 8, out);
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
    const bool transform = rhs && P.CN;
    double *r = transform ? raw_rows(S) : d_out;
    if (P.stationary)
        launch_reaction_stationary_residual(S.stream, P, r);
    else
        launch_reaction_residual(S.stream, P, r);
    launch_residual_norm(S, r, P.d_red);
    if (transform && S.sharded) {
        // the raw rows the time transforms read across the shard boundary: the adjoint rows (T_1)
        // send their first row down, the state rows (T_2) their last row up
        const int up = P.z_halo ? S.rank + 1 : -1, dn = P.v_halo ? S.rank - 1 : -1;
        const int64_t n1 = P.n1, nl = P.nl;
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
    if (which < 0 || which > 3) fail(KKT_ERR_ARG, "kkt_debug_reaction_array: no such array");
    if (which < 2 && !P.assembled)
        fail(KKT_ERR_STATE, "kkt_debug_reaction_array: nothing assembled yet");
    const double *src[4] = {P.d_E, P.d_D, P.d_v, P.d_zeta};
    const int64_t per_level[4] = {P.ne * P.ep, P.nnz, P.n1, P.n1};
    const int64_t n = per_level[which] * (which < 2 ? P.D_n : which == 2 ? P.v_n : P.z_n);
    if (!out || cap < n) fail(KKT_ERR_ARG, "kkt_debug_reaction_array: buffer too small");
    HIPCHK(hipStreamSynchronize(S.stream));
    HIPCHK(hipMemcpy(out, src[which], n * 8, hipMemcpyDeviceToHost));
}

}  // namespace kkt
