// Coarse set-up of the two-grid solves, shared by the Schur sub-solves (SchurPC) and the K_p solve
// (StokesPC): the structure of E = P^T A P, its inverses for a batch of level matrices, and the
// host entry points of the test hooks (declared in pc.hpp).
#include "pc.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace kkt {

int coarse_block_size(int nc, const std::vector<int32_t> &e_ip, const std::vector<int32_t> &e_ix) {
    std::vector<int32_t> uf(nc);
    for (int j = 0; j < nc; ++j) uf[j] = j;
    auto find = [&](int32_t a) {
        while (uf[a] != a) a = uf[a] = uf[uf[a]];
        return a;
    };
    for (int i = 0; i < nc; ++i)
        for (int32_t e = e_ip[i]; e < e_ip[i + 1]; ++e) {
            const int32_t a = find(i), b = find(e_ix[e]);
            if (a != b) uf[std::max(a, b)] = std::min(a, b);
        }
    int b = 1;
    while (b < nc && find(b) == find(0)) ++b;
    if (b >= nc || nc % b != 0) return 0;
    // every block one component of its own: [k b, (k+1) b) all joined to k b, the k b distinct
    std::vector<int32_t> root(nc / b);
    for (int k = 0; k < nc / b; ++k) root[k] = find(k * b);
    for (int i = 0; i < nc; ++i)
        if (find(i) != root[i / b]) return 0;
    std::sort(root.begin(), root.end());
    if (std::adjacent_find(root.begin(), root.end()) != root.end()) return 0;
    return b;
}

void galerkin_structure(int nc, const std::vector<int32_t> &pt_ip, const std::vector<int32_t> &pt_ix,
                        const std::vector<int32_t> &a_ip, const std::vector<int32_t> &a_ix,
                        const std::vector<int32_t> &p_ip, const std::vector<int32_t> &p_ix,
                        std::vector<int32_t> &e_ip, std::vector<int32_t> &e_ix) {
    std::vector<int32_t> seen(nc, -1), row;
    e_ip.assign(1, 0);
    e_ix.clear();
    for (int i = 0; i < nc; ++i) {
        row.clear();
        for (int32_t q = pt_ip[i]; q < pt_ip[i + 1]; ++q) {
            const int32_t r = pt_ix[q];
            for (int32_t t = a_ip[r]; t < a_ip[r + 1]; ++t) {
                const int32_t c = a_ix[t];
                for (int32_t u = p_ip[c]; u < p_ip[c + 1]; ++u) {
                    const int32_t k = p_ix[u];
                    if (seen[k] != i) {
                        seen[k] = i;
                        row.push_back(k);
                    }
                }
            }
        }
        std::sort(row.begin(), row.end());
        e_ix.insert(e_ix.end(), row.begin(), row.end());
        e_ip.push_back((int32_t)e_ix.size());
    }
}

// The column path (option "coarse_setup" = "columns"): E = P^T A P column by column with the
// kernels the sweeps use (x = column k of P, y = A x with the masked rows zero, E(:, k) = P^T y),
// inverted by Gauss-Jordan with partial pivoting, four launches per pivot.  Returns the launches.
static int64_t coarse_columns(System &S, const Pattern &P, const CoarseDev &c, const uint8_t *mask,
                              const double *vals, double *E, double *einv, unsigned *d_flag,
                              bool deflate, double *h_keep) {
    hipStream_t st = S.stream;
    const int nc = c.nc;
    const int64_t n = P.nrows;
    DevPool tmp;   // released on every way out
    double *x = tmp.alloc<double>(n + 32), *y = tmp.alloc<double>(n + 32);
    const RowOp op = lin_op(P, n, mask, LinStep{{RowTerm{vals, x}}, y});
    RowOp *d_op = tmp.upload(&op, 1);
    const Bases B{{nullptr, nullptr, nullptr, nullptr}};
    for (int k = 0; k < nc; ++k) {
        launch_coarse_column(st, c, k, x, n);
        launch_rowops(st, d_op, 1, P.nslices, P.R, B, 1, P.uniform_w);
        launch_coarse_restrict(st, c, y, E + k, nc);     // column k of the row-major E
    }
    int64_t launches = 4 * (int64_t)nc;     // launch_coarse_column: a zero fill and a scatter
    if (h_keep)
        HIPCHK(hipMemcpyAsync(h_keep, E, (size_t)nc * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (deflate) {
        std::vector<double> diag(nc);
        HIPCHK(hipMemcpy2DAsync(diag.data(), sizeof(double), E, ((size_t)nc + 1) * sizeof(double),
                                sizeof(double), nc, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double tr = 0.0;
        for (double v : diag) tr += v;
        launch_add_constant(st, E, tr / ((double)nc * (double)nc), (int64_t)nc * nc);
        launches += 1;
    }
    int *d_piv = tmp.alloc<int>(1);
    double *d_colbuf = tmp.alloc<double>(nc + 1);     // multipliers; slot nc: the pivot
    launch_dense_inverse(st, E, einv, nc, d_piv, d_colbuf, d_flag);
    launches += 1 + 4 * (int64_t)nc;
    HIPCHK(hipStreamSynchronize(st));
    return launches;
}

void coarse_setup(System &S, int pat, const CoarseDev &c, const GalerkinDev &g,
                  const std::vector<const double *> &vals, const std::vector<double *> &einv,
                  bool deflate, const char *what) {
    const Pattern &P = S.patterns[pat];
    hipStream_t st = S.stream;
    const int nc = c.nc, nmat = (int)vals.size();
    const size_t n2 = (size_t)nc * nc;
    S.coarse_stats = kkt_coarse_stats{};
    const bool keep = S.opts.coarse_keep;
    S.coarse_E.clear();
    S.coarse_Einv.clear();
    if (nmat == 0) return;
    if (keep) S.coarse_E.resize(n2 * nmat);
    const bool columns = S.opts.coarse_columns;
    HIPCHK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    int64_t launches = 0;
    std::vector<int> bad(nmat, nc);
    if (columns) {
        DevPool tmp;
        double *E = tmp.alloc<double>(n2);
        unsigned *d_flag = tmp.alloc<unsigned>(1);
        for (int b = 0; b < nmat; ++b) {
            HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
            launches += coarse_columns(S, P, c, g.mask, vals[b], E, einv[b], d_flag, deflate,
                                       keep ? S.coarse_E.data() + b * n2 : nullptr);
            unsigned singular = 0;
            HIPCHK(hipMemcpyAsync(&singular, d_flag, sizeof singular, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (singular) bad[b] = -1;      // this path does not know the column
        }
    } else {
        // component blocks: the Galerkin launch writes the nblk diagonal blocks of size bn as
        // matrices of their own (E: nmat * nblk of them), the inverses go to Ib and are scattered
        // into einv's full rows
        const bool blocked = !deflate && g.block_n > 0 && g.block_n < nc && nc % g.block_n == 0 &&
                             S.opts.coarse_blocks;
        const int bn = blocked ? g.block_n : nc, nblk = nc / bn;
        const size_t b2 = (size_t)bn * bn, ne = nblk * b2;     // doubles of E per level matrix
        GalerkinDev gb = g;
        gb.block_n = blocked ? bn : 0;
        // chunks of at most ~1 GiB of Galerkin matrices and scratch (Picard: one matrix per level)
        const size_t per = (blocked ? 2 : 1) * ne * sizeof(double) +
                           dense_inverse_batched_scratch(bn, nblk);
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>(nmat, ((size_t)1 << 30) / per));
        DevPool tmp;
        double *E = tmp.alloc<double>(ne * chunk);
        const double **d_vals = tmp.alloc<const double *>(chunk);
        double **d_inv = tmp.alloc<double *>(chunk);
        void *scratch = tmp.alloc<char>(dense_inverse_batched_scratch(bn, nblk * chunk));
        int *d_bad = tmp.alloc<int>((size_t)nblk * chunk);
        double *Ib = nullptr, **d_binv = nullptr;
        std::vector<int> bad_blk;
        std::vector<double> h_blocks;
        if (blocked) {
            Ib = tmp.alloc<double>(ne * chunk);
            std::vector<double *> ptr((size_t)nblk * chunk);
            for (size_t q = 0; q < ptr.size(); ++q) ptr[q] = Ib + q * b2;
            d_binv = tmp.upload(ptr.data(), ptr.size());
            bad_blk.resize((size_t)nblk * chunk);
            if (keep) h_blocks.resize(ne * chunk);
        }
        for (int b0 = 0; b0 < nmat; b0 += chunk) {
            const int nb = std::min(chunk, nmat - b0);
            HIPCHK(hipMemcpyAsync(d_vals, vals.data() + b0, nb * sizeof(double *),
                                  hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_inv, einv.data() + b0, nb * sizeof(double *),
                                  hipMemcpyHostToDevice, st));
            launch_zero_bytes(st, E, ne * nb * sizeof(double));
            launch_galerkin_batched(st, c, gb, d_vals, E, nb);
            launches += 2;
            if (keep && !blocked)
                HIPCHK(hipMemcpyAsync(S.coarse_E.data() + b0 * n2, E, n2 * nb * sizeof(double),
                                      hipMemcpyDeviceToHost, st));
            if (keep && blocked) {      // the full matrices, zeros outside the blocks
                HIPCHK(hipMemcpyAsync(h_blocks.data(), E, ne * nb * sizeof(double),
                                      hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b)
                    for (int k = 0; k < nblk; ++k)
                        for (int r = 0; r < bn; ++r)
                            std::copy_n(h_blocks.data() + ((size_t)b * nblk + k) * b2 + (size_t)r * bn,
                                        bn, S.coarse_E.data() + (b0 + b) * n2 +
                                                (size_t)(k * bn + r) * nc + (size_t)k * bn);
            }
            if (deflate) {
                // every entry + trace(E) / n_c^2, the diagonal summed on the host in index order
                std::vector<double> diag((size_t)nc * nb);
                for (int b = 0; b < nb; ++b)
                    HIPCHK(hipMemcpy2DAsync(diag.data() + (size_t)b * nc, sizeof(double), E + b * n2,
                                            ((size_t)nc + 1) * sizeof(double), sizeof(double), nc,
                                            hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b) {
                    double tr = 0.0;
                    for (int i = 0; i < nc; ++i) tr += diag[(size_t)b * nc + i];
                    launch_add_constant(st, E + b * n2, tr / ((double)nc * (double)nc), (int64_t)n2);
                    launches += 1;
                }
            }
            if (blocked) {
                launches += launch_dense_inverse_batched(st, E, d_binv, bn, nblk * nb, scratch, d_bad);
                launch_coarse_block_scatter(st, Ib, d_inv, nc, bn, nb);
                launches += 1;
                HIPCHK(hipMemcpyAsync(bad_blk.data(), d_bad, (size_t)nblk * nb * sizeof(int),
                                      hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (int b = 0; b < nb; ++b)        // first singular column of the whole E_b
                    for (int k = nblk - 1; k >= 0; --k)
                        if (bad_blk[(size_t)b * nblk + k] < bn)
                            bad[b0 + b] = k * bn + bad_blk[(size_t)b * nblk + k];
            } else {
                launches += launch_dense_inverse_batched(st, E, d_inv, nc, nb, scratch, d_bad);
                HIPCHK(hipMemcpyAsync(bad.data() + b0, d_bad, nb * sizeof(int), hipMemcpyDeviceToHost,
                                      st));
                HIPCHK(hipStreamSynchronize(st));
            }
        }
        S.coarse_stats.blocks = nblk;
        S.coarse_stats.block_n = bn;
    }
    if (columns) {
        S.coarse_stats.blocks = 1;
        S.coarse_stats.block_n = nc;
    }
    if (keep) {
        S.coarse_Einv.resize(n2 * nmat);
        for (int b = 0; b < nmat; ++b)
            HIPCHK(hipMemcpyAsync(S.coarse_Einv.data() + b * n2, einv[b], n2 * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    S.coarse_stats.matrices = nmat;
    S.coarse_stats.launches = launches;
    S.coarse_stats.n_coarse = nc;
    S.coarse_stats.ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int b = 0; b < nmat; ++b) {
        if (bad[b] == nc) continue;
        char msg[320];
        if (bad[b] < 0)
            std::snprintf(msg, sizeof msg, "%s: coarse matrix P^T A P of level matrix %d is singular "
                          "(a coarse function without support on free rows, or dependent coarse "
                          "functions)", what, b);
        else
            std::snprintf(msg, sizeof msg, "%s: coarse matrix P^T A P of level matrix %d is singular "
                          "at column %d (pivot below 1e-13 max|diag|: a coarse function without "
                          "support on free rows, or dependent coarse functions)", what, b, bad[b]);
        fail(KKT_ERR_STATE, msg);
    }
}

void dense_inverse_host(System &S, int n, int nmat, const double *a, double *inv, int *bad) {
    hipStream_t st = S.stream;
    const size_t n2 = (size_t)n * n;
    DevPool tmp;
    double *E = tmp.upload(a, n2 * nmat);
    double *I = tmp.alloc<double>(n2 * nmat);
    std::vector<double *> ptr(nmat);
    for (int b = 0; b < nmat; ++b) ptr[b] = I + b * n2;
    double **d_inv = tmp.upload(ptr.data(), ptr.size());
    void *scratch = tmp.alloc<char>(dense_inverse_batched_scratch(n, nmat));
    int *d_bad = tmp.alloc<int>(nmat);
    launch_dense_inverse_batched(st, E, d_inv, n, nmat, scratch, d_bad);
    HIPCHK(hipMemcpyAsync(inv, I, n2 * nmat * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bad, d_bad, nmat * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

void coarse_correction_host(System &S, int batched, int nb, int64_t vstride, const double *r,
                            const double *x_in, const double *einv, double *rc, double *ec,
                            double *x_out, int32_t *shape) {
    CoarseDev c;
    GalerkinDev g;
    int64_t n = 0;
    if (!S.pc || !S.pc->coarse_space(&c, &g, &n))
        fail(KKT_ERR_STATE,
             "kkt_debug_coarse_correction: no two-grid preconditioner built on this handle");
    hipStream_t st = S.stream;
    const int nc = c.nc;
    if (shape) {
        std::vector<int32_t> pt_ip((size_t)nc + 1);
        HIPCHK(hipMemcpyAsync(pt_ip.data(), c.pt_ip, pt_ip.size() * sizeof(int32_t),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int32_t longest = 0;
        for (int j = 0; j < nc; ++j) longest = std::max(longest, pt_ip[j + 1] - pt_ip[j]);
        const int32_t v[KKT_COARSE_SHAPE_INTS] = {(int32_t)n, nc, g.R, g.uniform_w, g.pos != nullptr,
                                                  g.mask != nullptr, g.block_n, longest};
        std::copy(v, v + KKT_COARSE_SHAPE_INTS, shape);
    }
    if (nb == 0) return;
    if (nb < 1 || (!batched && nb != 1) || vstride < n || !r || !einv || !rc || !ec || !x_out)
        fail(KKT_ERR_ARG, "bad coarse correction arguments");
    const size_t len = (size_t)nb * vstride;
    DevPool tmp;
    const double *d_r = tmp.upload(r, len);
    const double *d_xin = x_in ? tmp.upload(x_in, len) : nullptr;
    double *d_xout = tmp.upload(x_out, len);
    const double *d_einv = tmp.upload(einv, (size_t)nc * nc);
    c.rc = tmp.alloc<double>((size_t)nb * nc);      // its own scratch, nb vectors wide
    c.ec = tmp.alloc<double>((size_t)nb * nc);
    if (batched)
        launch_coarse_correction_batched(st, c, d_einv, d_r, d_xin, d_xout, n, nb, vstride);
    else
        launch_coarse_correction(st, c, d_einv, d_r, d_xin, d_xout, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rc, c.rc, (size_t)nb * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ec, c.ec, (size_t)nb * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(x_out, d_xout, len * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

}  // namespace kkt
