// Host side of the device re-linearisation (include/kkt.h, kkt_set_relinearisation): plan
// upload and validation, assembly, residual and update.  Kernels: relin_kernels.hip; checks and
// composition: compose.hpp.
#include "relin.hpp"

#include <string>

#include "comm.hpp"
#include "reaction.hpp"
#include "system.hpp"

namespace kkt {

static void need(bool ok, const std::string &msg) {
    if (!ok) fail(KKT_ERR_ARG, "kkt_set_relinearisation: " + msg);
}

void relin_set(System &S, const kkt_relin_desc *d) {
    need(d != nullptr, "null descriptor");
    need(S.finalized, "the handle must be finalized");
    if (S.reaction)
        fail(KKT_ERR_STATE, "kkt_set_relinearisation: the handle carries a reaction plan "
                            "(kkt_set_reaction_relinearisation)");
    // nv == 0: the P2-P1 descriptor; nv == 9 with nq == 16: Q2-Q1 (include/kkt.h)
    const bool q2 = d->nv == 9 && d->nq == 16;
    if (d->nv == 0)
        need(d->nq == RELIN_NQ, "nq must be 7 (Radon's rule)");
    else
        need(q2, "nv = " + std::to_string(d->nv) + " with nq = " + std::to_string(d->nq) +
                     ": nv must be 0 (P2-P1 triangles, nq = 7) or 9 with nq = 16 (Q2-Q1 "
                     "quadrilaterals)");
    need(!q2 || d->jinv, "nv = 9 needs jinv (ne x 2: 1 / hx, 1 / hy per cell)");
    const int kv = q2 ? 9 : 6, kp = q2 ? 4 : 3, ev = kv * kv, ep = kp * kp;
    need(d->n_t >= 1, "n_t must be at least 1 (1: the stationary system)");
    need(d->ne > 0 && d->n2 > 0 && d->n1 > 0, "sizes must be positive");
    // n_t == 1: the stationary outer system, one (v, zeta) block pair and no time step
    const bool stationary = d->n_t == 1;
    need(!stationary || d->cn == 0, "n_t == 1 (the stationary system) takes cn == 0");
    const int m = d->cn ? d->n_t - 1 : d->n_t;
    const int64_t nv = 2 * d->n2;
    if (stationary) {
        need(S.n0 == 2 && S.n1 == 2,
             "n_t == 1: the handle is not the stationary outer system (n_blocks_00 = n_blocks_11 "
             "= 2)");
        need(S.nx0 == nv && S.nx1 == d->n1,
             "n_t == 1: the handle is not the stationary outer system of these spaces");
        need(!S.CN, "n_t == 1: the stationary system is not a Crank-Nicolson handle");
        need(!S.sharded, "n_t == 1: the stationary system has one block per family and cannot be "
                         "time-sharded");
    }
    need(S.n0 == 2 * m && S.n1 == 2 * m && S.nx0 == nv && S.nx1 == d->n1 && S.CN == (d->cn != 0),
         "the handle is not the outer system of these spaces and time levels");
    need(!S.sharded || (S.families == 2 && S.mf == m),
         "a time-sharded handle must shard the two block families of the outer system by level");
    need(d->V && d->W && d->phi && d->gphi && d->lam && d->glam && d->K2 && d->M2 && d->Kp &&
             d->Mp && d->b_values && d->data && (d->n_bc == 0 || d->bc_idx),
         "null array");
    const std::string api = "kkt_set_relinearisation: ";
    check_range(api + "V", d->V, d->ne * kv, d->n2);
    check_csr(api + "P2 pattern", d->v_indptr, d->v_indices, d->n2, d->n2, d->nnz2);
    check_csr(api + "P1 pattern", d->p_indptr, d->p_indices, d->n1, d->n1, d->nnz1);
    check_csr(api + "B", d->b_indptr, d->b_indices, d->n1, nv, d->nnz_b);
    check_perm(api + "P2 pattern", d->v_tperm, d->nnz2);
    check_perm(api + "P1 pattern", d->p_tperm, d->nnz1);
    check_lists(api + "P2", d->v_cptr, d->v_clist, d->nnz2, d->ne * ev);
    check_lists(api + "P1", d->p_cptr, d->p_clist, d->nnz1, d->ne * ep);
    check_range(api + "bc_idx", d->bc_idx, d->n_bc, nv);

    auto P = std::make_unique<RelinPlan>();
    // the rank's block rows and the level windows its rows read
    P->w = level_windows(d->n_t, d->cn != 0, S.sharded ? S.lo : 0, S.sharded ? S.hi : m);
    const LevelWindows &w = P->w;
    P->stationary = stationary;
    P->ne = d->ne;
    P->n2 = d->n2;
    P->n1 = d->n1;
    P->nv = nv;
    P->nnz2 = d->nnz2;
    P->nnz1 = d->nnz1;
    P->nu = d->nu;
    P->tau = d->tau;
    P->beta = d->beta;
    P->kv = kv;
    P->kp = kp;
    P->nq = d->nq;
    P->ev = ev;
    P->ep = ep;
    const int64_t ne = d->ne, nq = d->nq;
    P->d_V = P->mem.upload(d->V, ne * kv);
    P->d_W = P->mem.upload(d->W, ne * nq);
    P->d_phi = P->mem.upload(d->phi, nq * kv);
    P->d_lam = P->mem.upload(d->lam, nq * kp);
    if (q2) {   // reference gradients, one table for all cells, and the cells' 1 / hx, 1 / hy
        P->d_gphi = P->mem.upload(d->gphi, nq * kv * 2);
        P->d_glam = P->mem.upload(d->glam, nq * kp * 2);
        P->d_jinv = P->mem.upload(d->jinv, ne * 2);
    } else {
        P->d_gphi = P->mem.upload(d->gphi, ne * nq * 12);
        P->d_glam = P->mem.upload(d->glam, ne * 6);
    }
    P->d_ip2 = P->mem.upload(d->v_indptr, d->n2 + 1);
    P->d_ix2 = P->mem.upload(d->v_indices, d->nnz2);
    P->d_t2 = P->mem.upload(d->v_tperm, d->nnz2);
    P->d_tp = P->mem.upload(d->p_tperm, d->nnz1);
    P->d_K2 = P->mem.upload(d->K2, d->nnz2);
    P->d_M2 = P->mem.upload(d->M2, d->nnz2);
    P->d_Kp = P->mem.upload(d->Kp, d->nnz1);
    P->d_Mp = P->mem.upload(d->Mp, d->nnz1);
    P->d_cptr2 = P->mem.upload(d->v_cptr, d->nnz2 + 1);
    P->d_clist2 = P->mem.upload(d->v_clist, ne * ev);
    P->d_cptrp = P->mem.upload(d->p_cptr, d->nnz1 + 1);
    P->d_clistp = P->mem.upload(d->p_clist, ne * ep);
    // B and its transpose (rows of B^T in ascending column order of B: sorted)
    const int64_t nb = d->nnz_b;
    std::vector<int32_t> tip(nv + 1, 0), tix(nb);
    std::vector<double> tv(nb);
    for (int64_t k = 0; k < nb; ++k) tip[d->b_indices[k] + 1]++;
    for (int64_t c = 0; c < nv; ++c) tip[c + 1] += tip[c];
    std::vector<int32_t> fillp(tip.begin(), tip.end() - 1);
    for (int64_t r = 0; r < d->n1; ++r)
        for (int32_t k = d->b_indptr[r]; k < d->b_indptr[r + 1]; ++k) {
            const int32_t at = fillp[d->b_indices[k]]++;
            tix[at] = (int32_t)r;
            tv[at] = d->b_values[k];
        }
    P->d_Bip = P->mem.upload(d->b_indptr, d->n1 + 1);
    P->d_Bix = P->mem.upload(d->b_indices, nb);
    P->d_Bv = P->mem.upload(d->b_values, nb);
    P->d_BTip = P->mem.upload(tip.data(), nv + 1);
    P->d_BTix = P->mem.upload(tix.data(), nb);
    P->d_BTv = P->mem.upload(tv.data(), nb);
    P->d_bc = upload_bc_mask(P->mem, d->bc_idx, d->n_bc, nv);
    P->d_data = upload_data_rows(P->mem, w, d->data, nv);
    if (S.sharded && w.CN) {
        P->d_rhalo = P->mem.alloc<double>(2 * nv + 2 * d->n1);
        HIPCHK(hipMemset(P->d_rhalo, 0, (2 * nv + 2 * d->n1) * 8));
    }
    P->d_Ev = P->mem.alloc<double>(ne * ev * w.D_n);
    P->d_Ep = P->mem.alloc<double>(ne * ep * w.D_n);
    P->d_D2 = P->mem.alloc<double>(d->nnz2 * w.D_n);
    P->d_Dp = P->mem.alloc<double>(d->nnz1 * w.D_n);
    P->d_v = P->mem.alloc<double>(w.v_n * nv);
    P->d_zeta = P->mem.alloc<double>(w.z_n * nv);
    P->d_p = P->mem.alloc<double>(w.nl * d->n1);
    P->d_mu = P->mem.alloc<double>(w.nl * d->n1);
    HIPCHK(hipMemset(P->d_v, 0, w.v_n * nv * 8));
    HIPCHK(hipMemset(P->d_zeta, 0, w.z_n * nv * 8));
    HIPCHK(hipMemset(P->d_p, 0, w.nl * d->n1 * 8));
    HIPCHK(hipMemset(P->d_mu, 0, w.nl * d->n1 * 8));
    P->d_red = P->mem.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX + 2);
    P->compose.n_t = d->n_t;
    using I32 = std::vector<int32_t>;
    P->compose.spaces = {
        {"velocity", I32(d->v_indptr, d->v_indptr + d->n2 + 1),
         I32(d->v_indices, d->v_indices + d->nnz2), d->nnz2, 2, P->d_D2, w.D_l0, w.D_n, P->d_M2,
         P->d_t2},
        {"pressure", I32(d->p_indptr, d->p_indptr + d->n1 + 1),
         I32(d->p_indices, d->p_indices + d->nnz1), d->nnz1, 1, P->d_Dp, w.D_l0, w.D_n, P->d_Mp,
         P->d_tp}};
    S.relin = std::move(P);
}

static RelinPlan &plan_of(System &S) {
    if (!S.relin) fail(KKT_ERR_STATE, "no re-linearisation plan on this handle (kkt_set_relinearisation)");
    return *S.relin;
}

void relin_apply(System &T, System &PS, const double *d_v, int n, const kkt_relin_recipe *rec) {
    RelinPlan &P = plan_of(PS);
    check_apply_target("kkt_relinearise_device", T, PS, n, rec);
    if (d_v && PS.sharded && d_v != P.d_v)
        fail(KKT_ERR_ARG, "kkt_relinearise_device: a time shard assembles at the plan's iterate "
                          "(kkt_picard_iterate)");
    // every recipe is validated before anything is written
    std::vector<ComposeJob> jobs = compose_jobs("kkt_relinearise_device", T, P.compose, n, rec);
    if (d_v) {
        exchange_iterate_halos(PS, P.w, P.d_v, P.d_zeta, P.nv);
        launch_relin_elements(PS.stream, P, d_v);
        launch_relin_gather(PS.stream, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(PS.stream));
        P.assembled = true;
    }
    if (n == 0) return;
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_relinearise_device: nothing assembled yet (d_v NULL)");
    compose_run(T, P.compose, jobs, rec);
}

// Host arrays of the global shapes: v and zeta by iterate_spans, p and mu the owned blocks' both
// ways.
void relin_state(System &S, int download, double *v, double *zeta, double *p, double *mu) {
    RelinPlan &P = plan_of(S);
    const int64_t rows = P.w.nl * P.n1, at = P.w.lo * P.n1;
    auto spans = iterate_spans(P.w, download != 0, P.d_v, P.d_zeta, v, zeta, P.nv);
    spans.push_back({P.d_p, p ? p + at : nullptr, rows});
    spans.push_back({P.d_mu, mu ? mu + at : nullptr, rows});
    copy_spans(S.stream, download != 0, spans);
}

void relin_window(System &S, int out[8]) {
    RelinPlan &P = plan_of(S);
    if (!out) fail(KKT_ERR_ARG, "kkt_picard_window: null argument");
    P.w.report(out);
}

void relin_iterate(System &S, double **v, double **zeta, double **p, double **mu) {
    RelinPlan &P = plan_of(S);
    if (v) *v = P.d_v;
    if (zeta) *zeta = P.d_zeta;
    if (p) *p = P.d_p;
    if (mu) *mu = P.d_mu;
}

void relin_residual(System &S, double *d_out, int rhs, double *norm) {
    RelinPlan &P = plan_of(S);
    if (!d_out || !norm) fail(KKT_ERR_ARG, "kkt_picard_residual_device: null argument");
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_picard_residual_device: D not assembled yet");
    // the stationary system's right-hand side is the rows themselves: no tau, no time transform
    const bool transform = rhs && !P.stationary;
    double *r = transform ? raw_rows(S) : d_out;
    if (P.stationary)
        launch_relin_stationary_residual(S.stream, P, r);
    else
        launch_relin_residual(S.stream, P, r);
    launch_residual_norm(S, r, P.d_red);
    if (transform && S.sharded && P.w.CN) {
        // the raw rows the time transforms read across the shard boundary (the pattern of
        // comm_exchange_row_halos): T_1 families send their first row down, T_2 their last up
        const int up = P.w.up(S.rank), dn = P.w.dn(S.rank);
        const int64_t nv = P.nv, n1 = P.n1, nl = P.w.nl;
        double *rp = r + 2 * nl * nv, *h = P.d_rhalo;
        S.comm->sendrecv(r, nv, dn, h, nv, up, S.stream);
        S.comm->sendrecv(r + (2 * nl - 1) * nv, nv, up, h + nv, nv, dn, S.stream);
        S.comm->sendrecv(rp + (nl - 1) * n1, n1, up, h + 2 * nv, n1, dn, S.stream);
        S.comm->sendrecv(rp + nl * n1, n1, dn, h + 2 * nv + n1, n1, up, S.stream);
    }
    if (transform) launch_relin_rhs(S.stream, P, r, d_out);
    read_residual_norm(S, P.d_red, norm);
}

void relin_debug_array(System &S, int which, double *out, int64_t cap) {
    RelinPlan &P = plan_of(S);
    const std::vector<DebugArray> arrays = {
        {P.d_Ev, P.ne * P.ev, P.w.D_n, true}, {P.d_Ep, P.ne * P.ep, P.w.D_n, true},
        {P.d_D2, P.nnz2, P.w.D_n, true}, {P.d_Dp, P.nnz1, P.w.D_n, true},
        {P.d_v, P.nv, P.w.v_n, false}, {P.d_zeta, P.nv, P.w.z_n, false}};
    copy_debug_array("kkt_debug_relin_array", S, arrays, P.assembled, which, out, cap);
}

void relin_update(System &S, double *d_u) {
    RelinPlan &P = plan_of(S);
    if (!d_u) fail(KKT_ERR_ARG, "kkt_picard_update_device: null update");
    launch_relin_update(S.stream, P, d_u);
    HIPCHK(hipGetLastError());
}

}  // namespace kkt
