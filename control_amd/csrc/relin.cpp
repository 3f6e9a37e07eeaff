// Host side of the device re-linearisation (include/kkt.h, kkt_set_relinearisation): plan
// upload and validation, assembly, residual and update.  Kernels: relin_kernels.hip; checks and
// composition: compose.hpp.
#include "relin.hpp"

#include <algorithm>
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
    need(d->nq == RELIN_NQ, "nq must be 7 (Radon's rule)");
    need(d->n_t >= 2 && d->ne > 0 && d->n2 > 0 && d->n1 > 0, "sizes must be positive");
    const int m = d->cn ? d->n_t - 1 : d->n_t;
    const int64_t nv = 2 * d->n2;
    need(S.n0 == 2 * m && S.n1 == 2 * m && S.nx0 == nv && S.nx1 == d->n1 && S.CN == (d->cn != 0),
         "the handle is not the outer system of these spaces and time levels");
    need(!S.sharded || (S.families == 2 && S.mf == m),
         "a time-sharded handle must shard the two block families of the outer system by level");
    need(d->V && d->W && d->phi && d->gphi && d->lam && d->glam && d->K2 && d->M2 && d->Kp &&
             d->Mp && d->b_values && d->data && (d->n_bc == 0 || d->bc_idx),
         "null array");
    const std::string api = "kkt_set_relinearisation: ";
    check_range(api + "V", d->V, d->ne * 6, d->n2);
    check_csr(api + "P2 pattern", d->v_indptr, d->v_indices, d->n2, d->n2, d->nnz2);
    check_csr(api + "P1 pattern", d->p_indptr, d->p_indices, d->n1, d->n1, d->nnz1);
    check_csr(api + "B", d->b_indptr, d->b_indices, d->n1, nv, d->nnz_b);
    check_perm(api + "P2 pattern", d->v_tperm, d->nnz2);
    check_perm(api + "P1 pattern", d->p_tperm, d->nnz1);
    check_lists(api + "P2", d->v_cptr, d->v_clist, d->nnz2, d->ne * RELIN_EV);
    check_lists(api + "P1", d->p_cptr, d->p_clist, d->nnz1, d->ne * RELIN_EP);
    check_range(api + "bc_idx", d->bc_idx, d->n_bc, nv);

    auto P = std::make_unique<RelinPlan>();
    P->n_t = d->n_t;
    P->m = m;
    P->CN = d->cn != 0;
    P->ne = d->ne;
    P->n2 = d->n2;
    P->n1 = d->n1;
    P->nv = nv;
    P->nnz2 = d->nnz2;
    P->nnz1 = d->nnz1;
    P->nu = d->nu;
    P->tau = d->tau;
    P->beta = d->beta;
    // the rank's block rows and the level windows its rows read (relin.hpp)
    const int lo = S.sharded ? S.lo : 0, hi = S.sharded ? S.hi : m, nl = hi - lo;
    P->lo = lo;
    P->nl = nl;
    if (P->CN) {
        P->v_l0 = P->z_l0 = P->D_l0 = lo;
        P->v_n = P->z_n = P->D_n = nl + 1;
        P->v_halo = lo > 0;
        P->z_halo = hi < m;
    } else {
        P->v_halo = lo > 0;
        P->z_halo = hi < m;
        P->v_l0 = lo - (P->v_halo ? 1 : 0);
        P->v_n = hi - P->v_l0;
        P->z_l0 = lo;
        P->z_n = nl + (P->z_halo ? 1 : 0);
        P->D_l0 = lo;
        P->D_n = nl;
    }
    const int64_t ne = d->ne, nq = RELIN_NQ;
    P->d_V = P->mem.upload(d->V, ne * 6);
    P->d_W = P->mem.upload(d->W, ne * nq);
    P->d_phi = P->mem.upload(d->phi, nq * 6);
    P->d_gphi = P->mem.upload(d->gphi, ne * nq * 12);
    P->d_lam = P->mem.upload(d->lam, nq * 3);
    P->d_glam = P->mem.upload(d->glam, ne * 6);
    P->d_ip2 = P->mem.upload(d->v_indptr, d->n2 + 1);
    P->d_ix2 = P->mem.upload(d->v_indices, d->nnz2);
    P->d_t2 = P->mem.upload(d->v_tperm, d->nnz2);
    P->d_tp = P->mem.upload(d->p_tperm, d->nnz1);
    P->d_K2 = P->mem.upload(d->K2, d->nnz2);
    P->d_M2 = P->mem.upload(d->M2, d->nnz2);
    P->d_Kp = P->mem.upload(d->Kp, d->nnz1);
    P->d_Mp = P->mem.upload(d->Mp, d->nnz1);
    P->d_cptr2 = P->mem.upload(d->v_cptr, d->nnz2 + 1);
    P->d_clist2 = P->mem.upload(d->v_clist, ne * RELIN_EV);
    P->d_cptrp = P->mem.upload(d->p_cptr, d->nnz1 + 1);
    P->d_clistp = P->mem.upload(d->p_clist, ne * RELIN_EP);
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
    std::vector<uint8_t> bc(nv, 0);
    for (int64_t k = 0; k < d->n_bc; ++k) bc[d->bc_idx[k]] = 1;
    P->d_bc = P->mem.upload(bc.data(), nv);
    // the data rows of the owned blocks: lo..hi-1 of the adjoint rows, m+lo..m+hi-1 of the state rows
    P->d_data = P->mem.alloc<double>(2 * (int64_t)nl * nv);
    for (int f = 0; f < 2; ++f)
        HIPCHK(hipMemcpy(P->d_data + (int64_t)f * nl * nv, d->data + ((int64_t)f * m + lo) * nv,
                         (int64_t)nl * nv * 8, hipMemcpyHostToDevice));
    if (S.sharded && P->CN) {
        P->d_rhalo = P->mem.alloc<double>(2 * nv + 2 * d->n1);
        HIPCHK(hipMemset(P->d_rhalo, 0, (2 * nv + 2 * d->n1) * 8));
    }
    P->d_Ev = P->mem.alloc<double>(ne * RELIN_EV * P->D_n);
    P->d_Ep = P->mem.alloc<double>(ne * RELIN_EP * P->D_n);
    P->d_D2 = P->mem.alloc<double>(d->nnz2 * P->D_n);
    P->d_Dp = P->mem.alloc<double>(d->nnz1 * P->D_n);
    P->d_v = P->mem.alloc<double>(P->v_n * nv);
    P->d_zeta = P->mem.alloc<double>(P->z_n * nv);
    P->d_p = P->mem.alloc<double>((int64_t)nl * d->n1);
    P->d_mu = P->mem.alloc<double>((int64_t)nl * d->n1);
    HIPCHK(hipMemset(P->d_v, 0, P->v_n * nv * 8));
    HIPCHK(hipMemset(P->d_zeta, 0, P->z_n * nv * 8));
    HIPCHK(hipMemset(P->d_p, 0, nl * d->n1 * 8));
    HIPCHK(hipMemset(P->d_mu, 0, nl * d->n1 * 8));
    P->d_red = P->mem.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX + 2);
    P->compose.n_t = d->n_t;
    using I32 = std::vector<int32_t>;
    P->compose.spaces = {
        {"velocity", I32(d->v_indptr, d->v_indptr + d->n2 + 1),
         I32(d->v_indices, d->v_indices + d->nnz2), d->nnz2, 2, P->d_D2, P->D_l0, P->D_n, P->d_M2,
         P->d_t2},
        {"pressure", I32(d->p_indptr, d->p_indptr + d->n1 + 1),
         I32(d->p_indices, d->p_indices + d->nnz1), d->nnz1, 1, P->d_Dp, P->D_l0, P->D_n, P->d_Mp,
         P->d_tp}};
    S.relin = std::move(P);
}

static RelinPlan &plan_of(System &S) {
    if (!S.relin) fail(KKT_ERR_STATE, "no re-linearisation plan on this handle (kkt_set_relinearisation)");
    return *S.relin;
}

// One level of v up and one of zeta down, after the update and before the assembly: v of my
// last block (BE level hi - 1, CN level hi) is the first level of the window above, zeta of my
// first block the last level of the window below.  Levels are contiguous: nothing is packed.
void relin_exchange(System &S) {
    RelinPlan &P = plan_of(S);
    if (!S.sharded) return;
    if (!S.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
    const int up = P.z_halo ? S.rank + 1 : -1, dn = P.v_halo ? S.rank - 1 : -1;
    const int v_last = P.lo + P.nl - 1 + (P.CN ? 1 : 0);
    S.comm->sendrecv(P.d_v + (int64_t)(v_last - P.v_l0) * P.nv, P.nv, up, P.d_v, P.nv, dn, S.stream);
    S.comm->sendrecv(P.d_zeta, P.nv, dn, P.d_zeta + (int64_t)(P.z_n - 1) * P.nv, P.nv, up,
                     S.stream);
}

void relin_apply(System &T, System &PS, const double *d_v, int n, const kkt_relin_recipe *rec) {
    RelinPlan &P = plan_of(PS);
    if (n < 0 || (n > 0 && !rec)) fail(KKT_ERR_ARG, "kkt_relinearise_device: bad recipe list");
    if (T.device != PS.device) fail(KKT_ERR_ARG, "kkt_relinearise_device: plan on another device");
    if (!T.finalized) fail(KKT_ERR_ARG, "kkt_relinearise_device: the target must be finalized");
    if (T.sharded != PS.sharded || (T.sharded && (T.lo != PS.lo || T.hi != PS.hi)))
        fail(KKT_ERR_ARG, "kkt_relinearise_device: the target is not sharded as the plan's handle");
    if (d_v && PS.sharded && d_v != P.d_v)
        fail(KKT_ERR_ARG, "kkt_relinearise_device: a time shard assembles at the plan's iterate "
                          "(kkt_picard_iterate)");
    // every recipe is validated before anything is written
    std::vector<ComposeJob> jobs = compose_jobs("kkt_relinearise_device", T, P.compose, n, rec);
    if (d_v) {
        relin_exchange(PS);
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

// Host arrays of the global shapes.  Upload: the rank's windows, halo levels included.
// Download: the levels the rank owns (BE: v, zeta of its blocks; CN: v one level up), and the
// fixed levels -- CN's v_0, zeta of the last level -- on the rank whose window holds them; the
// rest of the host arrays is left as it is.
void relin_state(System &S, int download, double *v, double *zeta, double *p, double *mu) {
    RelinPlan &P = plan_of(S);
    const int hi = P.lo + P.nl;
    int v0 = P.v_l0, v1 = P.v_l0 + P.v_n, z0 = P.z_l0, z1 = P.z_l0 + P.z_n;
    if (download) {
        v0 = P.CN ? (P.lo == 0 ? 0 : P.lo + 1) : P.lo;
        v1 = P.CN ? hi + 1 : hi;
        z1 = P.CN && hi == P.m ? hi + 1 : hi;
    }
    const int64_t rows = (int64_t)P.nl * P.n1;
    copy_spans(S.stream, download != 0,
               {{P.d_v + (int64_t)(v0 - P.v_l0) * P.nv, v ? v + (int64_t)v0 * P.nv : nullptr,
                 (v1 - v0) * P.nv},
                {P.d_zeta + (int64_t)(z0 - P.z_l0) * P.nv,
                 zeta ? zeta + (int64_t)z0 * P.nv : nullptr, (z1 - z0) * P.nv},
                {P.d_p, p ? p + (int64_t)P.lo * P.n1 : nullptr, rows},
                {P.d_mu, mu ? mu + (int64_t)P.lo * P.n1 : nullptr, rows}});
}

void relin_window(System &S, int out[8]) {
    RelinPlan &P = plan_of(S);
    if (!out) fail(KKT_ERR_ARG, "kkt_picard_window: null argument");
    const int w[8] = {P.v_l0, P.v_l0 + P.v_n, P.z_l0, P.z_l0 + P.z_n, P.D_l0, P.D_l0 + P.D_n,
                      P.lo, P.lo + P.nl};
    std::copy(w, w + 8, out);
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
    double *r = rhs ? raw_rows(S) : d_out;
    launch_relin_residual(S.stream, P, r);
    launch_residual_norm(S, r, P.d_red);
    if (rhs && S.sharded && P.CN) {
        // the raw rows the time transforms read across the shard boundary (the pattern of
        // comm_exchange_row_halos): T_1 families send their first row down, T_2 their last up
        const int up = P.z_halo ? S.rank + 1 : -1, dn = P.v_halo ? S.rank - 1 : -1;
        const int64_t nv = P.nv, n1 = P.n1, nl = P.nl;
        double *rp = r + 2 * nl * nv, *h = P.d_rhalo;
        S.comm->sendrecv(r, nv, dn, h, nv, up, S.stream);
        S.comm->sendrecv(r + (2 * nl - 1) * nv, nv, up, h + nv, nv, dn, S.stream);
        S.comm->sendrecv(rp + (nl - 1) * n1, n1, up, h + 2 * nv, n1, dn, S.stream);
        S.comm->sendrecv(rp + nl * n1, n1, dn, h + 2 * nv + n1, n1, up, S.stream);
    }
    if (rhs) launch_relin_rhs(S.stream, P, r, d_out);
    read_residual_norm(S, P.d_red, norm);
}

void relin_debug_array(System &S, int which, double *out, int64_t cap) {
    RelinPlan &P = plan_of(S);
    if (which < 0 || which > 5) fail(KKT_ERR_ARG, "kkt_debug_relin_array: no such array");
    if (which < 4 && !P.assembled)
        fail(KKT_ERR_STATE, "kkt_debug_relin_array: nothing assembled yet");
    const double *src[6] = {P.d_Ev, P.d_Ep, P.d_D2, P.d_Dp, P.d_v, P.d_zeta};
    const int64_t per_level[6] = {P.ne * RELIN_EV, P.ne * RELIN_EP, P.nnz2, P.nnz1, P.nv, P.nv};
    const int64_t n = per_level[which] * (which < 4 ? P.D_n : which == 4 ? P.v_n : P.z_n);
    if (!out || cap < n) fail(KKT_ERR_ARG, "kkt_debug_relin_array: buffer too small");
    HIPCHK(hipStreamSynchronize(S.stream));
    HIPCHK(hipMemcpy(out, src[which], n * 8, hipMemcpyDeviceToHost));
}

void relin_update(System &S, double *d_u) {
    RelinPlan &P = plan_of(S);
    if (!d_u) fail(KKT_ERR_ARG, "kkt_picard_update_device: null update");
    launch_relin_update(S.stream, P, d_u);
    HIPCHK(hipGetLastError());
}

}  // namespace kkt
