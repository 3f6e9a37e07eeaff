// compose.hpp: the composition jobs of both re-linearisation plans and their shared tails.
// Kernels: relin_kernels.hip.
#include "compose.hpp"

#include <algorithm>
#include <string>

#include "comm.hpp"
#include "system.hpp"

namespace kkt {

std::vector<ComposeJob> compose_jobs(const char *api, System &T, Composer &C, int n,
                                     const kkt_relin_recipe *rec) {
    const int nspaces = (int)C.spaces.size();
    std::vector<ComposeJob> jobs;
    for (int r = 0; r < n; ++r) {
        const kkt_relin_recipe &c = rec[r];
        const std::string at = std::string(api) + ": recipe " + std::to_string(r) + ": ";
        const std::string blk = "block (" + std::to_string(c.quadrant) + "; " +
                                std::to_string(c.i) + ", " + std::to_string(c.j) + ")";
        if (c.i >= 0 && !T.owns(c.i))   // (a time shard; one rank owns every row)
            fail(KKT_ERR_ARG, at + blk + ": its block row is not owned by this rank");
        auto it = T.blocks.find(std::make_tuple(c.quadrant, c.i, c.j));
        if (it == T.blocks.end()) fail(KKT_ERR_ARG, at + "no such " + blk);
        if (c.space < 0 || c.space >= nspaces)
            fail(KKT_ERR_ARG, at + "space must be 0" + (nspaces == 2 ? " or 1" : ""));
        if (c.level < 0 || c.level >= C.n_t) fail(KKT_ERR_ARG, at + "level out of range");
        const ComposeSpace &sp = C.spaces[c.space];
        // (a time shard holds the levels its rows read; one rank: every level)
        if (c.alpha != 0.0 && (c.level < sp.D_l0 || c.level >= sp.D_l0 + sp.D_n))
            fail(KKT_ERR_ARG, at + blk + ": level " + std::to_string(c.level) +
                                  " is outside this rank's window of D");
        const int pat = T.values[it->second.va].pattern;
        const Pattern &Q = T.patterns[pat];
        const auto key = std::make_tuple((const void *)&T, pat, c.space);
        if (!C.checked.count(key)) {
            if (!pattern_is_space(Q, sp))
                fail(KKT_ERR_ARG, at + "the block's pattern is not the plan's " + sp.name +
                                      " pattern");
            C.checked.insert(key);
        }
        ComposeJob J{};
        J.sell2csr = Q.d_sell2csr;
        J.col = Q.d_col;
        J.npadded = Q.npadded;
        J.alpha = c.alpha;
        J.gamma = c.gamma;
        J.D = sp.d_D + (int64_t)(c.level - sp.D_l0) * sp.nnz;
        J.M = sp.d_M;
        J.tperm = c.transpose ? sp.d_tperm : nullptr;
        J.nnz_s = sp.ncomp == 2 ? sp.nnz : sp.nnz + 1;   // (one component: no position folds)
        jobs.push_back(J);
    }
    return jobs;
}

void compose_run(System &T, Composer &C, std::vector<ComposeJob> &jobs,
                 const kkt_relin_recipe *rec) {
    const int n = (int)jobs.size();
    int64_t max_padded = 0;
    // copy on write: a value array shared with another block becomes private first
    for (int r = 0; r < n; ++r) {
        Block &blk = T.blocks.at(std::make_tuple(rec[r].quadrant, rec[r].i, rec[r].j));
        int users = 0;
        for (auto &kv : T.blocks) users += kv.second.va == blk.va;
        if (users > 1)
            T.give_private_values(rec[r].quadrant, rec[r].i, rec[r].j,
                                  DevBuf<double>::alloc(jobs[r].npadded));
        const ValueArray &va = T.values[blk.va];
        jobs[r].dst = va.d_vals;
        jobs[r].colmask = va.colmask_set >= 0 ? T.bc_sets[va.colmask_set].d_mask : nullptr;
        max_padded = std::max(max_padded, jobs[r].npadded);
    }
    if (C.jobs_cap < n) {
        C.d_jobs.reset();
        C.d_jobs = DevBuf<ComposeJob>::alloc(n);
        C.jobs_cap = n;
    }
    // the job table is shared by every target of the plan: the copy and the launch run in order
    // on the target's stream, and the host waits before the table is reused
    HIPCHK(hipMemcpyAsync(C.d_jobs.get(), jobs.data(), n * sizeof(ComposeJob),
                          hipMemcpyHostToDevice, T.stream));
    launch_relin_compose(T.stream, C.d_jobs.get(), n, max_padded);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(T.stream));
    for (int r = 0; r < n; ++r) T.mark_set(rec[r].quadrant, rec[r].i, rec[r].j);
    T.pc_stale = true;
}

void check_apply_target(const char *api, const System &T, const System &PS, int n,
                        const kkt_relin_recipe *rec) {
    const std::string at = std::string(api) + ": ";
    if (n < 0 || (n > 0 && !rec)) fail(KKT_ERR_ARG, at + "bad recipe list");
    if (T.device != PS.device) fail(KKT_ERR_ARG, at + "plan on another device");
    if (!T.finalized) fail(KKT_ERR_ARG, at + "the target must be finalized");
    if (T.sharded != PS.sharded || (T.sharded && (T.lo != PS.lo || T.hi != PS.hi)))
        fail(KKT_ERR_ARG, at + "the target is not sharded as the plan's handle");
}

void exchange_iterate_halos(System &S, const LevelWindows &w, double *d_v, double *d_zeta,
                            int64_t row_len) {
    if (!S.sharded) return;
    if (!S.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
    const int up = w.up(S.rank), dn = w.dn(S.rank);
    S.comm->sendrecv(d_v + w.v_last_slot() * row_len, row_len, up, d_v, row_len, dn, S.stream);
    S.comm->sendrecv(d_zeta, row_len, dn, d_zeta + (w.z_n - 1) * row_len, row_len, up, S.stream);
}

void copy_spans(hipStream_t s, bool download, const std::vector<CopySpan> &spans) {
    for (const CopySpan &c : spans) {
        if (!c.host) continue;
        if (download)
            HIPCHK(hipMemcpyAsync(c.host, c.dev, c.len * 8, hipMemcpyDeviceToHost, s));
        else
            HIPCHK(hipMemcpyAsync(c.dev, c.host, c.len * 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
}

std::vector<CopySpan> iterate_spans(const LevelWindows &w, bool download, double *d_v,
                                    double *d_zeta, double *v, double *zeta, int64_t row_len) {
    const LevelRange lv = w.v_levels(download), lz = w.z_levels(download);
    return {{d_v + (lv.l0 - w.v_l0) * row_len, v ? v + lv.l0 * row_len : nullptr,
             (lv.l1 - lv.l0) * row_len},
            {d_zeta + (lz.l0 - w.z_l0) * row_len, zeta ? zeta + lz.l0 * row_len : nullptr,
             (lz.l1 - lz.l0) * row_len}};
}

uint8_t *upload_bc_mask(DevPool &mem, const int32_t *bc_idx, int64_t n_bc, int64_t n) {
    std::vector<uint8_t> bc(n, 0);
    for (int64_t k = 0; k < n_bc; ++k) bc[bc_idx[k]] = 1;
    return mem.upload(bc.data(), n);
}

double *upload_data_rows(DevPool &mem, const LevelWindows &w, const double *data, int64_t row_len) {
    const int64_t rows = w.nl * row_len;
    double *d = mem.alloc<double>(2 * rows);
    for (int f = 0; f < 2; ++f)
        HIPCHK(hipMemcpy(d + f * rows, data + ((int64_t)f * w.m + w.lo) * row_len, rows * 8,
                         hipMemcpyHostToDevice));
    return d;
}

void copy_debug_array(const char *api, System &S, const std::vector<DebugArray> &arrays,
                      bool assembled, int which, double *out, int64_t cap) {
    const std::string at = std::string(api) + ": ";
    if (which < 0 || which >= (int)arrays.size()) fail(KKT_ERR_ARG, at + "no such array");
    const DebugArray &a = arrays[which];
    if (a.needs_assembly && !assembled) fail(KKT_ERR_STATE, at + "nothing assembled yet");
    const int64_t n = a.per_level * a.levels;
    if (!out || cap < n) fail(KKT_ERR_ARG, at + "buffer too small");
    HIPCHK(hipStreamSynchronize(S.stream));
    HIPCHK(hipMemcpy(out, a.src, n * 8, hipMemcpyDeviceToHost));
}

double *raw_rows(System &S) {
    if (!S.d_tmp_y) S.d_tmp_y = S.mem.adopt(S.new_vec());
    return S.d_tmp_y;
}

void launch_residual_norm(System &S, const double *r, double *d_red) {
    VecList V{};
    V.v[0] = r;
    launch_mdot(S.stream, r, V, 1, S.n_local, d_red + 2, d_red + 1);
    if (S.sharded) {   // every rank holds the same sum, and so the same norm
        if (!S.comm) fail(KKT_ERR_STATE, "time-sharded system without a transport");
        S.comm->allreduce_sum(d_red + 1, 1, S.stream);
    }
    launch_norm2_finish(S.stream, d_red + 1, d_red);
}

void read_residual_norm(System &S, const double *d_red, double *norm) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(norm, d_red, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
}

}  // namespace kkt
