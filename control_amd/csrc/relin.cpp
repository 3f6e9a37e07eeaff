// Host side of the device re-linearisation (include/kkt.h, kkt_set_relinearisation): plan
// upload and validation, composition jobs, residual and update.  Kernels: relin_kernels.hip.
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

// sorted CSR with nrows rows over ncols columns
static void check_csr(const int32_t *ip, const int32_t *ix, int64_t nrows, int64_t ncols,
                      int64_t nnz, const char *what) {
    need(ip && ix, std::string(what) + ": null pattern");
    need(ip[0] == 0 && ip[nrows] == nnz, std::string(what) + ": indptr does not span nnz");
    for (int64_t r = 0; r < nrows; ++r) {
        need(ip[r] <= ip[r + 1], std::string(what) + ": indptr decreases");
        for (int32_t k = ip[r]; k < ip[r + 1]; ++k) {
            need(ix[k] >= 0 && ix[k] < ncols, std::string(what) + ": column out of range");
            need(k == ip[r] || ix[k - 1] < ix[k], std::string(what) + ": columns not sorted");
        }
    }
}

static void check_lists(const int32_t *cptr, const int32_t *clist, int64_t nnz, int64_t n_entries,
                        const char *what) {
    need(cptr && clist, std::string(what) + ": null contribution list");
    need(cptr[0] == 0 && cptr[nnz] == n_entries,
         std::string(what) + ": the lists must hold every element entry once");
    for (int64_t k = 0; k < nnz; ++k) {
        need(cptr[k] <= cptr[k + 1], std::string(what) + ": list pointer decreases");
        for (int32_t j = cptr[k]; j < cptr[k + 1]; ++j)
            need(clist[j] >= 0 && clist[j] < n_entries &&
                     (j == cptr[k] || clist[j - 1] < clist[j]),
                 std::string(what) + ": list entries out of range or not ascending");
    }
}

static void check_perm(const int32_t *t, int64_t nnz, const char *what) {
    need(t != nullptr, std::string(what) + ": null transpose permutation");
    for (int64_t k = 0; k < nnz; ++k)
        need(t[k] >= 0 && t[k] < nnz && t[t[k]] == k,
             std::string(what) + ": not a transpose permutation");
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
    for (int64_t k = 0; k < d->ne * 6; ++k)
        need(d->V[k] >= 0 && d->V[k] < d->n2, "V: node out of range");
    check_csr(d->v_indptr, d->v_indices, d->n2, d->n2, d->nnz2, "P2 pattern");
    check_csr(d->p_indptr, d->p_indices, d->n1, d->n1, d->nnz1, "P1 pattern");
    check_csr(d->b_indptr, d->b_indices, d->n1, nv, d->nnz_b, "B");
    check_perm(d->v_tperm, d->nnz2, "P2 pattern");
    check_perm(d->p_tperm, d->nnz1, "P1 pattern");
    check_lists(d->v_cptr, d->v_clist, d->nnz2, d->ne * RELIN_EV, "P2");
    check_lists(d->p_cptr, d->p_clist, d->nnz1, d->ne * RELIN_EP, "P1");
    for (int64_t k = 0; k < d->n_bc; ++k)
        need(d->bc_idx[k] >= 0 && d->bc_idx[k] < nv, "bc_idx out of range");

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
    P->h_ip2.assign(d->v_indptr, d->v_indptr + d->n2 + 1);
    P->h_ix2.assign(d->v_indices, d->v_indices + d->nnz2);
    P->h_ipp.assign(d->p_indptr, d->p_indptr + d->n1 + 1);
    P->h_ixp.assign(d->p_indices, d->p_indices + d->nnz1);
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
    // validate every recipe before anything is written
    std::vector<ComposeJob> jobs;
    int64_t max_padded = 0;
    for (int r = 0; r < n; ++r) {
        const kkt_relin_recipe &c = rec[r];
        const std::string at = "kkt_relinearise_device: recipe " + std::to_string(r) + ": ";
        const std::string blk = "block (" + std::to_string(c.quadrant) + "; " +
                                std::to_string(c.i) + ", " + std::to_string(c.j) + ")";
        if (T.sharded && c.i >= 0 && !T.owns(c.i))
            fail(KKT_ERR_ARG, at + blk + ": its block row is not owned by this rank");
        auto it = T.blocks.find(std::make_tuple(c.quadrant, c.i, c.j));
        if (it == T.blocks.end()) fail(KKT_ERR_ARG, at + "no such block");
        if (c.space != 0 && c.space != 1) fail(KKT_ERR_ARG, at + "space must be 0 or 1");
        if (c.level < 0 || c.level >= P.n_t) fail(KKT_ERR_ARG, at + "level out of range");
        if (c.alpha != 0.0 && (c.level < P.D_l0 || c.level >= P.D_l0 + P.D_n))
            fail(KKT_ERR_ARG, at + blk + ": level " + std::to_string(c.level) +
                                  " is outside this rank's window of D");
        const int pat = T.values[it->second.va].pattern;
        const Pattern &Q = T.patterns[pat];
        const auto key = std::make_tuple((const void *)&T, pat, c.space);
        if (!P.checked.count(key)) {
            bool same;
            if (c.space == 0) {
                const int64_t n2 = P.n2, nnz2 = P.nnz2;
                same = Q.nrows == 2 * n2 && Q.ncols == 2 * n2 && Q.nnz == 2 * nnz2;
                for (int64_t row = 0; same && row <= 2 * n2; ++row)
                    same = Q.h_indptr[row] ==
                           (row <= n2 ? P.h_ip2[row] : nnz2 + P.h_ip2[row - n2]);
                for (int64_t k = 0; same && k < 2 * nnz2; ++k)
                    same = Q.h_indices[k] ==
                           (k < nnz2 ? P.h_ix2[k] : n2 + P.h_ix2[k - nnz2]);
            } else {
                same = Q.nrows == P.n1 && Q.ncols == P.n1 && Q.nnz == P.nnz1 &&
                       Q.h_indptr == P.h_ipp && Q.h_indices == P.h_ixp;
            }
            if (!same)
                fail(KKT_ERR_ARG, at + "the block's pattern is not the plan's " +
                                      (c.space == 0 ? "velocity" : "pressure") + " pattern");
            P.checked.insert(key);
        }
        ComposeJob J{};
        J.sell2csr = Q.d_sell2csr;
        J.col = Q.d_col;
        J.npadded = Q.npadded;
        J.alpha = c.alpha;
        J.gamma = c.gamma;
        if (c.space == 0) {
            J.D = P.d_D2 + (int64_t)(c.level - P.D_l0) * P.nnz2;
            J.M = P.d_M2;
            J.tperm = c.transpose ? P.d_t2 : nullptr;
            J.nnz_s = P.nnz2;
        } else {
            J.D = P.d_Dp + (int64_t)(c.level - P.D_l0) * P.nnz1;
            J.M = P.d_Mp;
            J.tperm = c.transpose ? P.d_tp : nullptr;
            J.nnz_s = P.nnz1 + 1;   // no second component
        }
        jobs.push_back(J);
        max_padded = std::max(max_padded, Q.npadded);
    }
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
    // copy on write: a value array shared with another block becomes private first
    for (int r = 0; r < n; ++r) {
        Block &blk = T.blocks.at(std::make_tuple(rec[r].quadrant, rec[r].i, rec[r].j));
        int users = 0;
        for (auto &kv : T.blocks) users += kv.second.va == blk.va;
        if (users > 1) {
            const Pattern &Q = T.patterns[T.values[blk.va].pattern];
            T.give_private_values(rec[r].quadrant, rec[r].i, rec[r].j,
                                  DevBuf<double>::alloc(Q.npadded));
        }
        const ValueArray &va = T.values[blk.va];
        jobs[r].dst = va.d_vals;
        jobs[r].colmask = va.colmask_set >= 0 ? T.bc_sets[va.colmask_set].d_mask : nullptr;
    }
    if (P.jobs_cap < n) {
        P.d_jobs.reset();
        P.d_jobs = DevBuf<ComposeJob>::alloc(n);
        P.jobs_cap = n;
    }
    // the job table is shared by every target of the plan: the copy and the launch run in order
    // on the target's stream, and the host waits before the table is reused
    HIPCHK(hipMemcpyAsync(P.d_jobs.get(), jobs.data(), n * sizeof(ComposeJob), hipMemcpyHostToDevice,
                          T.stream));
    launch_relin_compose(T.stream, P.d_jobs.get(), n, max_padded);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(T.stream));
    for (int r = 0; r < n; ++r) T.mark_set(rec[r].quadrant, rec[r].i, rec[r].j);
    T.pc_stale = true;
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
    double *dev[4] = {P.d_v + (int64_t)(v0 - P.v_l0) * P.nv,
                      P.d_zeta + (int64_t)(z0 - P.z_l0) * P.nv, P.d_p, P.d_mu};
    double *host[4] = {v ? v + (int64_t)v0 * P.nv : nullptr,
                       zeta ? zeta + (int64_t)z0 * P.nv : nullptr,
                       p ? p + (int64_t)P.lo * P.n1 : nullptr,
                       mu ? mu + (int64_t)P.lo * P.n1 : nullptr};
    const int64_t len[4] = {(v1 - v0) * P.nv, (z1 - z0) * P.nv, (int64_t)P.nl * P.n1,
                            (int64_t)P.nl * P.n1};
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        if (download)
            HIPCHK(hipMemcpyAsync(host[k], dev[k], len[k] * 8, hipMemcpyDeviceToHost, S.stream));
        else
            HIPCHK(hipMemcpyAsync(dev[k], host[k], len[k] * 8, hipMemcpyHostToDevice, S.stream));
    }
    HIPCHK(hipStreamSynchronize(S.stream));
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
    double *r = d_out;
    if (rhs) {
        if (!S.d_tmp_y) S.d_tmp_y = S.mem.adopt(S.new_vec());
        r = S.d_tmp_y;
    }
    launch_relin_residual(S.stream, P, r);
    VecList V{};
    V.v[0] = r;
    launch_mdot(S.stream, r, V, 1, S.n_local, P.d_red + 2, P.d_red + 1);
    if (S.sharded) {   // every rank holds the same sum, and so the same norm
        if (!S.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
        S.comm->allreduce_sum(P.d_red + 1, 1, S.stream);
    }
    launch_norm2_finish(S.stream, P.d_red + 1, P.d_red);
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
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(norm, P.d_red, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
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
