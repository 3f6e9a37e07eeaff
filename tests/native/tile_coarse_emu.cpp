// CPU emulation of the two-grid levels of the tile sweep program (control_amd/csrc/tile_kernels.hip,
// COARSE path) on the plan of control_amd/csrc/tiles.cpp and the lists of build_tile_coarse_lists:
// rings, credit, hand-offs, restriction, slot-ordered coarse residual, owned products,
// prolongation, tiles advanced in lock step.  Three runs -- the hand-off form on lists without
// rings, the hand-off form on lists with rings, the ring form -- are compared bit for bit with
// each other and with the global recurrence; every local entry carries the generation of the
// iterate it holds, and a read of an entry of another generation counts as stale.  Test
// infrastructure: checks the plan, the lists and the scheme, not the GPU kernel.
//   usage: tile_coarse_emu <nx> <ny> <nz> <ntiles> <depth> <its> <cycles> <components> [--dump <file>]
// --dump writes the run's data for tests/tile_level_ref.py, little-endian: the magic "TCEMU01\0", ten
// int32 (n, nc, nnz of the level structure, nnz of P, tiles, levels, its, cycles, depth, W), then
//   int32  indptr[n + 1], indices[nnz] of the level structure; uint8 mask[n]
//   per level, doubles: F[nnz], U[nnz] (CSR order), dinv[n], B[n], E[nc * nc]
//   doubles c1[its], c2[its], c3[its] (sweeps 1 .. its), then ca, cy, post1, post2
//   int32  indptr[n + 1], indices[nnzP] of P, doubles values[nnzP]
//   int32  own_ptr[tiles + 1], own_rows[own_ptr[tiles]]: the rows a tile owns, in local order
//   per level, doubles: out[n], the result of the ring-form run (lists without rings: of the
//   hand-off form -- the runs are equal bit for bit or the program fails)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../../control_amd/csrc/tiles.hpp"

using namespace kkt;
namespace kkt {
void fail(int, const std::string &m) { std::fprintf(stderr, "fail: %s\n", m.c_str()); std::exit(2); }
void hip_check(hipError_t, const char *, const char *, int) {}
}

namespace {

// a wave's sum as the kernel forms it: lanes stride the list, then the xor butterfly
template <typename F>
double wave_sum(int e0, int e1, F term) {
    double a[64];
    for (int lane = 0; lane < 64; ++lane) {
        a[lane] = 0.0;
        for (int e = e0 + lane; e < e1; e += 64) a[lane] = term(e, a[lane]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        double b[64];
        for (int lane = 0; lane < 64; ++lane) b[lane] = a[lane] + a[lane ^ o];
        std::memcpy(a, b, sizeof a);
    }
    return a[0];
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main(int argc, char **argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: tile_coarse_emu nx ny nz ntiles depth its cycles components\n");
        return 2;
    }
    const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::max(1, std::atoi(argv[3]));
    const int ntiles = std::atoi(argv[4]), depth_in = std::atoi(argv[5]), its = std::atoi(argv[6]);
    const int cycles = std::atoi(argv[7]), ncomp = std::max(1, std::atoi(argv[8]));
    const int nlev = 2, T = 256;
    const int dim = nz > 1 ? 3 : 2;
    // ---- the fine structure: 7-point (2-D) or the 15-point structure of Kuhn cubes (3-D),
    // `ncomp` uncoupled copies interleaved node by node; boundary rows masked
    Pattern P;
    const int nnode = nx * ny * nz, n = nnode * ncomp;
    P.nrows = P.ncols = n;
    P.R = 2;
    P.h_indptr.push_back(0);
    const int dx[7] = {-1, 0, -1, 0, 1, 0, 1}, dy[7] = {-1, -1, 0, 0, 0, 1, 1};
    const int ex[7] = {1, 0, 0, 1, 0, 1, 1}, ey[7] = {0, 1, 0, 1, 1, 0, 1}, ez[7] = {0, 0, 1, 0, 1, 1, 1};
    const int WS = nz > 1 ? 15 : 7;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                for (int c = 0; c < ncomp; ++c) {
                    std::vector<int32_t> row;
                    if (nz == 1) {
                        for (int q = 0; q < 7; ++q) {
                            const int ii = i + dx[q], jj = j + dy[q];
                            if (ii >= 0 && ii < nx && jj >= 0 && jj < ny)
                                row.push_back((jj * nx + ii) * ncomp + c);
                        }
                    } else {
                        row.push_back(((k * ny + j) * nx + i) * ncomp + c);
                        for (int q = 0; q < 7; ++q)
                            for (int sg = -1; sg <= 1; sg += 2) {
                                const int ii = i + sg * ex[q], jj = j + sg * ey[q], kk = k + sg * ez[q];
                                if (ii >= 0 && ii < nx && jj >= 0 && jj < ny && kk >= 0 && kk < nz)
                                    row.push_back(((kk * ny + jj) * nx + ii) * ncomp + c);
                            }
                        std::sort(row.begin(), row.end());
                    }
                    P.h_indices.insert(P.h_indices.end(), row.begin(), row.end());
                    P.h_indptr.push_back((int32_t)P.h_indices.size());
                }
    P.nnz = P.h_indices.size();
    P.max_width = WS;
    P.uniform_w = WS;
    P.nslices = (n + 127) / 128;
    for (int s = 0; s <= P.nslices; ++s) P.h_slice_off.push_back(WS * s);
    P.npadded = (int64_t)WS * P.nslices * 128;
    std::vector<uint8_t> mask(n, 0);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                if (i == 0 || j == 0 || i == nx - 1 || j == ny - 1 || (nz > 1 && (k == 0 || k == nz - 1)))
                    for (int c = 0; c < ncomp; ++c) mask[((k * ny + j) * nx + i) * ncomp + c] = 1;
    TilePlan tp;
    if (!build_tile_plan(P, ntiles, depth_in, T, 4, tp, mask.data(), its)) {
        std::printf("plan does not fit\n");
        return 3;
    }
    if (!tp.symmetric) return 4;
    const int depth = tp.depth, W = tp.W, RPT = tp.rpt, nkp = tp.nk_pad, NT = tp.ntiles;
    // ---- multilinear P: coarse nodes every 4 fine cells, a copy of them per component, rows of
    // boundary dofs empty, zero weights dropped, columns ascending
    const int H = 4;
    const int cnx = (nx - 1) / H + 1, cny = (ny - 1) / H + 1, cnz = nz > 1 ? (nz - 1) / H + 1 : 1;
    const int ncn = cnx * cny * cnz, nc = ncn * ncomp;
    std::vector<int32_t> pi(1, 0), pj;
    std::vector<double> pv;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                for (int c = 0; c < ncomp; ++c) {
                    const int row = ((k * ny + j) * nx + i) * ncomp + c;
                    if (!mask[row]) {
                        const int I = std::min(i / H, cnx - 2), J = std::min(j / H, cny - 2);
                        const int K = nz > 1 ? std::min(k / H, cnz - 2) : 0;
                        const double fx = (i - H * I) / (double)H, fy = (j - H * J) / (double)H;
                        const double fz = nz > 1 ? (k - H * K) / (double)H : 0.0;
                        std::map<int32_t, double> ent;
                        for (int cz = 0; cz < (nz > 1 ? 2 : 1); ++cz)
                            for (int cy = 0; cy < 2; ++cy)
                                for (int cx = 0; cx < 2; ++cx) {
                                    const double w = (cx ? fx : 1.0 - fx) * (cy ? fy : 1.0 - fy) *
                                                     (nz > 1 ? (cz ? fz : 1.0 - fz) : 1.0);
                                    if (w > 0.0)
                                        ent[c * ncn + ((K + cz) * cny + (J + cy)) * cnx + (I + cx)] = w;
                                }
                        for (auto &e : ent) {
                            pj.push_back(e.first);
                            pv.push_back(e.second);
                        }
                    }
                    pi.push_back((int32_t)pj.size());
                }
    TileCoarseLists LP, LR;      // without / with the rings asked for
    if (!build_tile_coarse_lists(tp, nc, pi.data(), pj.data(), pv.data(), false, LP) ||
        !build_tile_coarse_lists(tp, nc, pi.data(), pj.data(), pv.data(), true, LR)) {
        std::printf("lists do not fit\n");
        return 3;
    }
    std::printf("plan: %d tiles depth %d rpt %d nk_pad %d; lists: nc %d jmax %d jxmax %d nr_max %d "
                "np_max %d rings %d\n", NT, depth, RPT, nkp, nc, LR.jmax, LR.jxmax, LR.nr_max,
                LR.np_max, (int)LR.rings);
    auto nt = [&](int t, int j) { return tp.n[(size_t)t * (TILE_MAX_DEPTH + 1) + j]; };
    auto grow = [&](int t, int l) { return tp.grow[(size_t)t * nkp + l]; };
    long bad_lists = 0;
    // ---- the lists: what covers own rows and J_t is the same with and without rings
    {
        if (LP.rings) ++bad_lists;
        if (dim == 3 && LR.rings) ++bad_lists;          // long rows of P: today's form
        if (dim == 2 && !LR.rings) ++bad_lists;
        if (LP.nj != LR.nj || LP.slot0 != LR.slot0 || LP.r_ip != LR.r_ip || LP.r_row != LR.r_row ||
            LP.r_w != LR.r_w || LP.c_ip != LR.c_ip || LP.c_slot != LR.c_slot || LP.jmax != LR.jmax ||
            LP.nslots != LR.nslots || LP.nr_max != LR.nr_max || LP.njx != LP.nj || LP.jxmax != LP.jmax)
            ++bad_lists;
        for (int t = 0; t < NT; ++t) {
            if (LR.njx[t] < LR.nj[t]) ++bad_lists;
            for (int k = 0; k < LR.nj[t]; ++k)
                if (LP.jglob[(size_t)t * LP.jxmax + k] != LR.jglob[(size_t)t * LR.jxmax + k]) ++bad_lists;
            for (int k = 1; k < LR.njx[t]; ++k)         // ascending inside J_t and behind it
                if (k != LR.nj[t] &&
                    LR.jglob[(size_t)t * LR.jxmax + k - 1] >= LR.jglob[(size_t)t * LR.jxmax + k])
                    ++bad_lists;
            const int32_t *a = &LP.p_ip[(size_t)t * LP.pstride], *b = &LR.p_ip[(size_t)t * LR.pstride];
            for (int l = 0; l < nt(t, 0); ++l) {
                if (a[l + 1] - a[l] != b[l + 1] - b[l]) { ++bad_lists; continue; }
                for (int e = 0; e < a[l + 1] - a[l]; ++e)
                    if (LP.p_k[a[l] + e] != LR.p_k[b[l] + e] || !same_bits(LP.p_w[a[l] + e], LR.p_w[b[l] + e]))
                        ++bad_lists;
            }
            // every local row's entries are P's row, in its order
            for (int l = 0; l < (LR.rings ? nt(t, depth) : nt(t, 0)); ++l) {
                const int g = grow(t, l);
                if (b[l + 1] - b[l] != pi[g + 1] - pi[g]) { ++bad_lists; continue; }
                for (int e = 0; e < b[l + 1] - b[l]; ++e)
                    if (LR.jglob[(size_t)t * LR.jxmax + LR.p_k[b[l] + e]] != pj[pi[g] + e] ||
                        !same_bits(LR.p_w[b[l] + e], pv[pi[g] + e]))
                        ++bad_lists;
            }
        }
    }
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    auto rand_vals = [&]() {
        std::vector<double> v(P.npadded, 0.0);
        for (int r = 0; r < n; ++r)
            for (int k = 0; k < P.h_indptr[r + 1] - P.h_indptr[r]; ++k) {
                const int c = P.h_indices[P.h_indptr[r] + k];
                v[P.sell_index(r, k)] = mask[c] ? 0.0 : (c == r ? 4.0 + U(rng) : 0.3 * U(rng));
            }
        return v;
    };
    std::vector<std::vector<double>> F(nlev), Um(nlev), dinv(nlev), B(nlev), E(nlev);
    for (int l = 0; l < nlev; ++l) {
        F[l] = rand_vals();
        Um[l] = rand_vals();
        dinv[l].assign(n, 1.0);
        for (int r = 0; r < n; ++r)
            if (!mask[r])
                for (int k = 0; k < P.h_indptr[r + 1] - P.h_indptr[r]; ++k)
                    if (P.h_indices[P.h_indptr[r] + k] == r) dinv[l][r] = 1.0 / F[l][P.sell_index(r, k)];
        B[l].resize(n);
        for (auto &x : B[l]) x = U(rng);
        // (any dense matrix stands in for (P^T A P)^-1: the scheme is checked, not the solve)
        E[l].resize((size_t)nc * nc);
        for (auto &x : E[l]) x = 0.05 * U(rng);
    }
    std::vector<double> c1(its + 1), c2(its + 1), c3(its + 1);
    for (int s = 1; s <= its; ++s) { c1[s] = 0.1 * U(rng); c2[s] = 1.0 + 0.1 * U(rng); c3[s] = 0.4 + 0.1 * U(rng); }
    const double ca = -1.0, cy = 1.0, post1 = 0.9, post2 = 1.1;
    auto spmv_row = [&](const std::vector<double> &vals, const std::vector<double> &x, int r) {
        double acc = 0.0;
        const int len = P.h_indptr[r + 1] - P.h_indptr[r];
        for (int k = 0; k < W; ++k) {
            const double v = k < len ? vals[P.sell_index(r, k)] : 0.0;
            const int c = k < len ? P.h_indices[P.h_indptr[r] + k] : r;
            acc = std::fma(v, x[c], acc);
        }
        return acc;
    };
    auto sweep_out = [&](int s, bool last, double xo, double xc, double di, double b, double acc) {
        double t = s >= 2 ? c1[s] * xo : 0.0;
        t = std::fma(c2[s], xc, t);
        t = std::fma(c3[s], di * (b - acc), t);
        return (last ? post2 : 1.0) * ((last ? post1 : 1.0) * t);
    };
    auto product = [&](const std::vector<double> &Einv, const std::vector<double> &rc, int j) {
        return wave_sum(0, nc, [&](int q, double a) { return std::fma(Einv[(size_t)j * nc + q], rc[q], a); });
    };
    // ---- the global recurrence: same arithmetic per row, lists made here from the partition and
    // P alone (own rows ascending, a row's entries in P's order; tiles ascending per function)
    std::vector<std::vector<double>> out_ref(nlev);
    {
        std::vector<std::map<int32_t, std::vector<std::pair<int32_t, double>>>> RL(NT);
        for (int t = 0; t < NT; ++t)
            for (int l = 0; l < nt(t, 0); ++l) {
                const int g = grow(t, l);
                for (int q = pi[g]; q < pi[g + 1]; ++q) RL[t][pj[q]].push_back({g, pv[q]});
            }
        std::vector<double> prev(n, 0.0), b(n), xc(n, 0.0), xo(n, 0.0), res(n), rc(nc), ec(nc);
        for (int l = 0; l < nlev; ++l) {
            for (int r = 0; r < n; ++r) {
                if (l > 0) {
                    double t = ca * spmv_row(Um[l], prev, r);
                    t = std::fma(cy, B[l][r], t);
                    b[r] = mask[r] ? 0.0 : t;
                } else {
                    b[r] = mask[r] ? 0.0 : B[l][r];
                }
            }
            for (int cyc = 0; cyc < cycles; ++cyc) {
                for (int r = 0; r < n; ++r)
                    res[r] = mask[r] ? 0.0 : (cyc == 0 ? b[r] : b[r] - spmv_row(F[l], xc, r));
                std::fill(rc.begin(), rc.end(), 0.0);
                for (int t = 0; t < NT; ++t)
                    for (auto &kv : RL[t]) {
                        const auto &lst = kv.second;
                        rc[kv.first] += wave_sum(0, (int)lst.size(), [&](int e, double a) {
                            return std::fma(lst[e].second, res[lst[e].first], a);
                        });
                    }
                for (int j = 0; j < nc; ++j) ec[j] = product(E[l], rc, j);
                for (int r = 0; r < n; ++r) {
                    if (mask[r]) continue;
                    double a = 0.0;
                    for (int q = pi[r]; q < pi[r + 1]; ++q) a = std::fma(pv[q], ec[pj[q]], a);
                    xc[r] = cyc == 0 ? a : xc[r] + a;
                }
                for (int s = 1; s <= its; ++s) {
                    const bool last = cyc + 1 == cycles && s == its;
                    std::vector<double> xn(n, 0.0);
                    for (int r = 0; r < n; ++r)
                        if (!mask[r])
                            xn[r] = sweep_out(s, last, xo[r], xc[r], dinv[l][r], b[r], spmv_row(F[l], xc, r));
                    xo.swap(xc);
                    xc.swap(xn);
                }
            }
            out_ref[l] = xc;
            prev = xc;
        }
    }
    // ---- emulation of the kernel, tiles in lock step
    long stale = 0;
    auto run = [&](const TileCoarseLists &L, const bool ring_form, std::vector<std::vector<double>> &out,
                   std::vector<long> &handoffs) {
        std::vector<std::vector<double>> X(NT, std::vector<double>(2 * (size_t)nkp, NAN));
        std::vector<std::vector<long>> G(NT, std::vector<long>(2 * (size_t)nkp, -1));   // generations
        for (int t = 0; t < NT; ++t) X[t][nkp - 1] = X[t][2 * (size_t)nkp - 1] = 0.0;      // zero slot
        std::vector<std::vector<double>> bl(NT, std::vector<double>((size_t)RPT * T, NAN));
        std::vector<double> Gn(n, NAN), Go(n, NAN);
        std::vector<long> Tn(n, -1), To(n, -1);
        int cur = 0;
        long gen_c = 0, gen_o = -1, gen_next = 0;      // generation the newest / previous iterate has
        long nho = 0;
        auto handoff = [&](bool both) {
            ++nho;
            for (int t = 0; t < NT; ++t)
                for (int r = 0; r < nt(t, 0); ++r) {
                    Gn[grow(t, r)] = X[t][cur * nkp + r];
                    Tn[grow(t, r)] = G[t][cur * nkp + r];
                    if (both && depth > 1) {
                        Go[grow(t, r)] = X[t][(cur ^ 1) * nkp + r];
                        To[grow(t, r)] = G[t][(cur ^ 1) * nkp + r];
                    }
                }
            for (int t = 0; t < NT; ++t)
                for (int l = nt(t, 0); l < nt(t, depth); ++l) {
                    X[t][cur * nkp + l] = Gn[grow(t, l)];
                    G[t][cur * nkp + l] = Tn[grow(t, l)];
                    if (both && l < nt(t, depth - 1)) {
                        X[t][(cur ^ 1) * nkp + l] = Go[grow(t, l)];
                        G[t][(cur ^ 1) * nkp + l] = To[grow(t, l)];
                    }
                }
        };
        auto lval = [&](const std::vector<double> &vals, int t, int r, int k) {
            const int sl = r / T, tid = r % T;
            const size_t at = (((size_t)t * RPT + sl) * W + k) * T + tid;
            const int g = tp.gpos[at];
            return std::make_pair(g >= 0 ? vals[g] : 0.0, (int)tp.lcol[at]);
        };
        // A x on local row r of tile t out of the newest iterate; every column must hold `gen_c`
        auto lspmv = [&](const std::vector<double> &vals, int t, int r) {
            double acc = 0.0;
            for (int k = 0; k < W; ++k) {
                auto vc = lval(vals, t, r, k);
                const size_t at = (size_t)cur * nkp + vc.second;
                if (tp.gpos[(((size_t)t * RPT + r / T) * W + k) * T + r % T] >= 0 && vc.second != nkp - 1 &&
                    G[t][at] != gen_c)
                    ++stale;
                acc = std::fma(vc.first, X[t][at], acc);
            }
            return acc;
        };
        out.assign(nlev, std::vector<double>(n, 0.0));
        handoffs.assign(nlev, 0);
        std::vector<double> slots(L.nslots), rc(nc), ec(nc);
        for (int l = 0; l < nlev; ++l) {
            const long nho0 = nho;
            for (int t = 0; t < NT; ++t)
                for (int r = 0; r < nt(t, depth - 1); ++r) {
                    const int g = grow(t, r);
                    if (l > 0) {
                        double tt = ca * lspmv(Um[l], t, r);
                        tt = std::fma(cy, B[l][g], tt);
                        bl[t][r] = tt;
                    } else {
                        bl[t][r] = B[l][g];
                    }
                }
            int cr = depth - 1;
            cur ^= 1;           // (the kernel's first step; a two-grid level starts from zero)
            std::swap(gen_c, gen_o);
            for (int cyc = 0; cyc < cycles; ++cyc) {
                if (cyc > 0 && (cr == 0 || (ring_form && cr < depth))) {
                    handoff(false);
                    cr = depth;
                }
                for (int t = 0; t < NT; ++t)
                    for (int r = 0; r < nt(t, 0); ++r)
                        X[t][(cur ^ 1) * nkp + r] = cyc == 0 ? bl[t][r] : bl[t][r] - lspmv(F[l], t, r);
                // restriction, partial sums into the tile's slots
                for (int t = 0; t < NT; ++t)
                    for (int k = 0; k < L.nj[t]; ++k) {
                        const int32_t *rip = &L.r_ip[(size_t)t * L.jmax];
                        slots[L.slot0[t] + k] = wave_sum(rip[k], rip[k + 1], [&](int e, double a) {
                            return std::fma(L.r_w[e], X[t][(cur ^ 1) * nkp + L.r_row[e]], a);
                        });
                    }
                for (int j = 0; j < nc; ++j) {
                    double a = 0.0;
                    for (int q = L.c_ip[j]; q < L.c_ip[j + 1]; ++q) a += slots[L.c_slot[q]];
                    rc[j] = a;
                }
                for (int j = 0; j < nc; ++j) ec[j] = product(E[l], rc, j);      // by its owner
                // prolongation: own rows, in the ring form every local row
                const long gen_new = ++gen_next;
                for (int t = 0; t < NT; ++t) {
                    const int32_t *pip = &L.p_ip[(size_t)t * L.pstride];
                    const int npoll = ring_form ? L.njx[t] : L.nj[t];
                    for (int r = 0; r < (ring_form ? nt(t, depth) : nt(t, 0)); ++r) {
                        double a = 0.0;
                        for (int e = pip[r]; e < pip[r + 1]; ++e) {
                            if (L.p_k[e] >= npoll) ++stale;       // a product that was not polled
                            a = std::fma(L.p_w[e], ec[L.jglob[(size_t)t * L.jxmax + L.p_k[e]]], a);
                        }
                        const size_t at = (size_t)cur * nkp + r;
                        if (cyc > 0 && G[t][at] != gen_c) ++stale;
                        X[t][at] = cyc == 0 ? a : X[t][at] + a;
                        G[t][at] = gen_new;
                    }
                }
                gen_c = gen_new;
                if (!ring_form) handoff(false);
                cr = depth;
                for (int s = 1; s <= its; ++s) {
                    if (cr == 0) { handoff(s >= 2); cr = depth; }
                    const bool last = cyc + 1 == cycles && s == its;
                    const long gen_s = ++gen_next;
                    for (int t = 0; t < NT; ++t) {
                        double *Xc = &X[t][cur * nkp], *Xo = &X[t][(cur ^ 1) * nkp];
                        long *Gc = &G[t][cur * nkp], *Gold = &G[t][(cur ^ 1) * nkp];
                        const int nv = nt(t, cr - 1);
                        for (int r = 0; r < nv; ++r) {
                            const int g = grow(t, r);
                            if (s >= 2 && Gold[r] != gen_o) ++stale;
                            if (Gc[r] != gen_c) ++stale;
                            Xo[r] = sweep_out(s, last, Xo[r], Xc[r], dinv[l][g], bl[t][r], lspmv(F[l], t, r));
                            Gold[r] = gen_s;
                        }
                        // rows beyond the valid region are stale: poisoned, so a wrong read shows
                        for (int r = nv; r < nt(t, depth); ++r) { Xo[r] = NAN; Gold[r] = -1; }
                        Xo[nkp - 1] = 0.0;
                    }
                    cur ^= 1;
                    gen_o = gen_c;
                    gen_c = gen_s;
                    --cr;
                }
            }
            for (int t = 0; t < NT; ++t)
                for (int r = 0; r < nt(t, 0); ++r) out[l][grow(t, r)] = X[t][cur * nkp + r];
            handoffs[l] = nho - nho0;               // (without the one that ends the level)
            if (l + 1 < nlev) handoff(false);
        }
    };
    std::vector<std::vector<double>> o_plain, o_long, o_ring;
    std::vector<long> h_plain, h_long, h_ring;
    run(LP, false, o_plain, h_plain);
    const long stale_plain = stale;
    run(LR, false, o_long, h_long);
    const long stale_long = stale - stale_plain;
    long stale_ring = 0;
    if (LR.rings) {
        const long s0 = stale;
        run(LR, true, o_ring, h_ring);
        stale_ring = stale - s0;
    }
    long bad = 0, bad_counts = 0;
    for (int l = 0; l < nlev; ++l) {
        for (int r = 0; r < n; ++r) {
            if (!same_bits(out_ref[l][r], o_plain[l][r]) || !same_bits(out_ref[l][r], o_long[l][r])) ++bad;
            if (LR.rings && !same_bits(out_ref[l][r], o_ring[l][r])) ++bad;
            if (!mask[r] && !std::isfinite(out_ref[l][r])) ++bad;
        }
        if (h_plain[l] != h_long[l]) ++bad_counts;
        // per cycle the hand-off after the correction goes; the one in front of a later cycle's
        // residual is today's where `depth` divides `its`, else it is new
        const long saved = cycles - (its % depth != 0 ? cycles - 1 : 0);
        if (LR.rings && h_plain[l] - h_ring[l] != saved) ++bad_counts;
    }
    if (argc >= 11 && std::strcmp(argv[9], "--dump") == 0) {
        std::FILE *f = std::fopen(argv[10], "wb");
        if (!f) return 5;
        auto put = [&](const void *p, size_t bytes) {
            if (bytes && std::fwrite(p, 1, bytes, f) != bytes) std::exit(5);
        };
        auto put_i = [&](const std::vector<int32_t> &v) { put(v.data(), v.size() * sizeof(int32_t)); };
        auto put_d = [&](const std::vector<double> &v) { put(v.data(), v.size() * sizeof(double)); };
        auto csr_vals = [&](const std::vector<double> &vals) {
            std::vector<double> c;
            for (int r = 0; r < n; ++r)
                for (int k = 0; k < P.h_indptr[r + 1] - P.h_indptr[r]; ++k)
                    c.push_back(vals[P.sell_index(r, k)]);
            return c;
        };
        put("TCEMU01", 8);
        const std::vector<int32_t> head = {n, nc, (int32_t)P.nnz, (int32_t)pj.size(), NT, nlev, its,
                                           cycles, depth, W};
        put_i(head);
        put_i(P.h_indptr);
        put_i(P.h_indices);
        put(mask.data(), mask.size());
        for (int l = 0; l < nlev; ++l) {
            put_d(csr_vals(F[l]));
            put_d(csr_vals(Um[l]));
            put_d(dinv[l]);
            put_d(B[l]);
            put_d(E[l]);
        }
        put(c1.data() + 1, its * sizeof(double));
        put(c2.data() + 1, its * sizeof(double));
        put(c3.data() + 1, its * sizeof(double));
        const std::vector<double> scal = {ca, cy, post1, post2};
        put_d(scal);
        put_i(pi);
        put_i(pj);
        put_d(pv);
        std::vector<int32_t> own_ptr(1, 0), own_rows;
        for (int t = 0; t < NT; ++t) {
            for (int r = 0; r < nt(t, 0); ++r) own_rows.push_back(grow(t, r));
            own_ptr.push_back((int32_t)own_rows.size());
        }
        put_i(own_ptr);
        put_i(own_rows);
        for (int l = 0; l < nlev; ++l) put_d(LR.rings ? o_ring[l] : o_long[l]);
        if (std::fclose(f) != 0) return 5;
    }
    std::printf("hand-offs per level: %ld, ring form %ld (its %d depth %d cycles %d)\n", h_plain[0],
                LR.rings ? h_ring[0] : -1, its, depth, cycles);
    std::printf("stale reads: %ld %ld %ld\n", stale_plain, stale_long, stale_ring);
    std::printf("list errors: %ld, hand-off count errors: %ld\n", bad_lists, bad_counts);
    std::printf("mismatches: %ld of %d\n", bad, nlev * n);
    return bad || stale || bad_lists || bad_counts ? 1 : 0;
}
