// Host side of the scalar reaction re-linearisation (include/kkt.h,
// kkt_set_reaction_relinearisation): plan upload and validation, composition jobs, residual and
// update.  Kernels: reaction_kernels.hip; gather and composition: relin_kernels.hip.
#include "reaction.hpp"

#include <algorithm>
#include <string>

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
    need(d->nq == RELIN_NQ, "nq must be 7 (Radon's rule)");
    need(d->n_t >= 2 && d->ne > 0 && d->n1 > 0 && d->nnz > 0, "sizes must be positive");
    need(d->degree >= 0 && d->degree <= REACTION_MAX_DEGREE, "degree must be 0 .. 4");
    const int m = d->cn ? d->n_t - 1 : d->n_t;
    need(!S.sharded, "time-sharded handles are not supported");
    need(S.n0 == m && S.n1 == m && S.nx0 == d->n1 && S.nx1 == d->n1 && S.CN == (d->cn != 0),
         "the handle is not the scalar instationary system of this space and these time levels");
    need(d->cells && d->W && d->lam && d->L && d->M && d->data && (d->n_bc == 0 || d->bc_idx),
         "null array");
    need(d->indptr && d->indices && d->tperm && d->cptr && d->clist, "null pattern, list or permutation");
    const int64_t n1 = d->n1, nnz = d->nnz, ne = d->ne;
    for (int64_t k = 0; k < ne * 3; ++k)
        need(d->cells[k] >= 0 && d->cells[k] < n1, "cells: node out of range");
    need(d->indptr[0] == 0 && d->indptr[n1] == nnz, "pattern: indptr does not span nnz");
    for (int64_t r = 0; r < n1; ++r) {
        need(d->indptr[r] <= d->indptr[r + 1], "pattern: indptr decreases");
        for (int32_t k = d->indptr[r]; k < d->indptr[r + 1]; ++k) {
            need(d->indices[k] >= 0 && d->indices[k] < n1, "pattern: column out of range");
            need(k == d->indptr[r] || d->indices[k - 1] < d->indices[k],
                 "pattern: columns not sorted");
        }
    }
    for (int64_t k = 0; k < nnz; ++k)
        need(d->tperm[k] >= 0 && d->tperm[k] < nnz && d->tperm[d->tperm[k]] == k,
             "tperm: not a transpose permutation");
    const int64_t n_entries = ne * RELIN_EP;
    need(d->cptr[0] == 0 && d->cptr[nnz] == n_entries,
         "the contribution lists must hold every element entry once");
    for (int64_t k = 0; k < nnz; ++k) {
        need(d->cptr[k] <= d->cptr[k + 1], "contribution lists: pointer decreases");
        for (int32_t j = d->cptr[k]; j < d->cptr[k + 1]; ++j)
            need(d->clist[j] >= 0 && d->clist[j] < n_entries &&
                     (j == d->cptr[k] || d->clist[j - 1] < d->clist[j]),
                 "contribution lists: entries out of range or not ascending");
    }
    for (int64_t k = 0; k < d->n_bc; ++k)
        need(d->bc_idx[k] >= 0 && d->bc_idx[k] < n1, "bc_idx out of range");

    auto P = std::make_unique<ReactionPlan>();
    P->n_t = d->n_t;
    P->m = m;
    P->CN = d->cn != 0;
    P->ne = ne;
    P->n1 = n1;
    P->nnz = nnz;
    P->tau = d->tau;
    P->beta = d->beta;
    P->coef.degree = d->degree;
    for (int k = 0; k <= REACTION_MAX_DEGREE; ++k) P->coef.c[k] = k <= d->degree ? d->c[k] : 0.0;
    P->d_cells = P->mem.upload(d->cells, ne * 3);
    P->d_W = P->mem.upload(d->W, ne * RELIN_NQ);
    P->d_lam = P->mem.upload(d->lam, (int64_t)RELIN_NQ * 3);
    P->h_ip.assign(d->indptr, d->indptr + n1 + 1);
    P->h_ix.assign(d->indices, d->indices + nnz);
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
    P->d_data = P->mem.upload(d->data, 2 * (int64_t)m * n1);
    P->d_E = P->mem.alloc<double>(n_entries * d->n_t);
    P->d_D = P->mem.alloc<double>(nnz * d->n_t);
    P->d_v = P->mem.alloc<double>(d->n_t * n1);
    P->d_zeta = P->mem.alloc<double>(d->n_t * n1);
    HIPCHK(hipMemset(P->d_v, 0, d->n_t * n1 * 8));
    HIPCHK(hipMemset(P->d_zeta, 0, d->n_t * n1 * 8));
    P->d_red = P->mem.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX + 2);
    S.reaction = std::move(P);
}

static ReactionPlan &plan_of(System &S) {
    if (!S.reaction)
        fail(KKT_ERR_STATE, "no reaction plan on this handle (kkt_set_reaction_relinearisation)");
    return *S.reaction;
}

// The composition jobs are those of relin_apply for the one scalar space; what differs is the plan
// they read (one pattern, no level windows, no shards), so the builder is this plan's own.
void reaction_apply(System &T, System &PS, int assemble, int n, const kkt_relin_recipe *rec) {
    ReactionPlan &P = plan_of(PS);
    if (n < 0 || (n > 0 && !rec)) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: bad recipe list");
    if (T.device != PS.device) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: plan on another device");
    if (!T.finalized) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: the target must be finalized");
    if (T.sharded) fail(KKT_ERR_ARG, "kkt_reaction_relinearise: time-sharded targets are not supported");
    // validate every recipe before anything is written
    std::vector<ComposeJob> jobs;
    int64_t max_padded = 0;
    for (int r = 0; r < n; ++r) {
        const kkt_relin_recipe &c = rec[r];
        const std::string at = "kkt_reaction_relinearise: recipe " + std::to_string(r) + ": ";
        auto it = T.blocks.find(std::make_tuple(c.quadrant, c.i, c.j));
        if (it == T.blocks.end())
            fail(KKT_ERR_ARG, at + "no such block (" + std::to_string(c.quadrant) + "; " +
                                  std::to_string(c.i) + ", " + std::to_string(c.j) + ")");
        if (c.space != 0) fail(KKT_ERR_ARG, at + "space must be 0");
        if (c.level < 0 || c.level >= P.n_t) fail(KKT_ERR_ARG, at + "level out of range");
        const int pat = T.values[it->second.va].pattern;
        const Pattern &Q = T.patterns[pat];
        const auto key = std::make_pair((const void *)&T, pat);
        if (!P.checked.count(key)) {
            if (!(Q.nrows == P.n1 && Q.ncols == P.n1 && Q.nnz == P.nnz && Q.h_indptr == P.h_ip &&
                  Q.h_indices == P.h_ix))
                fail(KKT_ERR_ARG, at + "the block's pattern is not the plan's pattern");
            P.checked.insert(key);
        }
        ComposeJob J{};
        J.sell2csr = Q.d_sell2csr;
        J.col = Q.d_col;
        J.npadded = Q.npadded;
        J.alpha = c.alpha;
        J.gamma = c.gamma;
        J.D = P.d_D + (int64_t)c.level * P.nnz;
        J.M = P.d_M;
        J.tperm = c.transpose ? P.d_tperm : nullptr;
        J.nnz_s = P.nnz + 1;   // no second component
        jobs.push_back(J);
        max_padded = std::max(max_padded, Q.npadded);
    }
    if (assemble) {
        launch_reaction_elements(PS.stream, P);
        // D = 1.0 * L[k] + acc: the product is exact, so this is L + C with one rounding
        launch_relin_gather_one(PS.stream, P.d_cptr, P.d_clist, P.d_E, P.ne * RELIN_EP, P.d_L, 1.0,
                                P.nnz, P.n_t, P.d_D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(PS.stream));
        P.assembled = true;
    }
    if (n == 0) return;
    if (!P.assembled) fail(KKT_ERR_STATE, "kkt_reaction_relinearise: nothing assembled yet");
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
    HIPCHK(hipMemcpyAsync(P.d_jobs.get(), jobs.data(), n * sizeof(ComposeJob), hipMemcpyHostToDevice,
                          T.stream));
    launch_relin_compose(T.stream, P.d_jobs.get(), n, max_padded);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(T.stream));
    for (int r = 0; r < n; ++r) T.mark_set(rec[r].quadrant, rec[r].i, rec[r].j);
    T.pc_stale = true;
}

void reaction_state(System &S, int download, double *v, double *zeta) {
    ReactionPlan &P = plan_of(S);
    double *dev[2] = {P.d_v, P.d_zeta}, *host[2] = {v, zeta};
    const int64_t len = (int64_t)P.n_t * P.n1 * 8;
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        if (download)
            HIPCHK(hipMemcpyAsync(host[k], dev[k], len, hipMemcpyDeviceToHost, S.stream));
        else
            HIPCHK(hipMemcpyAsync(dev[k], host[k], len, hipMemcpyHostToDevice, S.stream));
    }
    HIPCHK(hipStreamSynchronize(S.stream));
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
    double *r = d_out;
    const bool transform = rhs && P.CN;   // backward Euler's right-hand side is the rows themselves
    if (transform) {
        if (!S.d_tmp_y) S.d_tmp_y = S.mem.adopt(S.new_vec());
        r = S.d_tmp_y;
    }
    launch_reaction_residual(S.stream, P, r);
    VecList V{};
    V.v[0] = r;
    launch_mdot(S.stream, r, V, 1, S.n_local, P.d_red + 2, P.d_red + 1);
    launch_norm2_finish(S.stream, P.d_red + 1, P.d_red);
    if (transform) launch_reaction_rhs(S.stream, P, r, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(norm, P.d_red, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
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
    const int64_t per_level[4] = {P.ne * RELIN_EP, P.nnz, P.n1, P.n1};
    const int64_t n = per_level[which] * P.n_t;
    if (!out || cap < n) fail(KKT_ERR_ARG, "kkt_debug_reaction_array: buffer too small");
    HIPCHK(hipStreamSynchronize(S.stream));
    HIPCHK(hipMemcpy(out, src[which], n * 8, hipMemcpyDeviceToHost));
}

}  // namespace kkt
