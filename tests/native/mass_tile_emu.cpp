// CPU emulation of the launch schedule of the batched mass solves on tiles
// (control_amd/csrc/mass_tile_kernels.hip, planned by SchurPC::fuse_mass_tiles) on the plan that
// control_amd/csrc/tiles.cpp builds with depth = K: ceil(its / K) launches; a launch loads the two
// newest iterates on the rows within distance k of a tile from one pair of global vectors, runs k
// steps on a region that shrinks by one ring per step -- each step overwrites the older iterate in
// place -- and stores the own rows of the two newest iterates into the other pair, the last launch
// the result and the zeros of the Dirichlet rows.  Compared bit for bit with the global three-term
// recurrence; every value carries the number of the step that produced it, and a read of a value of
// the wrong step (a stale row) is counted.  Test infrastructure: checks the plan and the schedule,
// not the GPU kernel.
//   usage: mass_tile_emu <nx> <ny> <nz> <ntiles> <K> <its>
//          nz > 1: 3-D grid with the 15-point structure of Kuhn cubes, else the 7-point P1 structure
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../control_amd/csrc/tiles.hpp"

using namespace kkt;
namespace kkt {
void fail(int, const std::string &m) { std::fprintf(stderr, "fail: %s\n", m.c_str()); std::exit(2); }
void hip_check(hipError_t, const char *, const char *, int) {}
}

static int any_halo(int, int, int) { return 1 << 20; }

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: mass_tile_emu nx ny nz ntiles K its\n");
        return 2;
    }
    const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::max(1, std::atoi(argv[3]));
    const int ntiles = std::atoi(argv[4]), K = std::atoi(argv[5]), its = std::atoi(argv[6]);
    const int T = 64;
    Pattern P;
    const int n = nx * ny * nz;
    P.nrows = P.ncols = n;
    P.R = 2;
    P.h_indptr.push_back(0);
    const int dx[7] = {-1, 0, -1, 0, 1, 0, 1}, dy[7] = {-1, -1, 0, 0, 0, 1, 1};
    const int ex[7] = {1, 0, 0, 1, 0, 1, 1}, ey[7] = {0, 1, 0, 1, 1, 0, 1}, ez[7] = {0, 0, 1, 0, 1, 1, 1};
    const int WS = nz > 1 ? 15 : 7;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                std::vector<int32_t> row;
                if (nz == 1) {
                    for (int q = 0; q < 7; ++q) {
                        const int ii = i + dx[q], jj = j + dy[q];
                        if (ii >= 0 && ii < nx && jj >= 0 && jj < ny) row.push_back(jj * nx + ii);
                    }
                } else {
                    row.push_back((k * ny + j) * nx + i);
                    for (int q = 0; q < 7; ++q)
                        for (int sg = -1; sg <= 1; sg += 2) {
                            const int ii = i + sg * ex[q], jj = j + sg * ey[q], kk = k + sg * ez[q];
                            if (ii >= 0 && ii < nx && jj >= 0 && jj < ny && kk >= 0 && kk < nz)
                                row.push_back((kk * ny + jj) * nx + ii);
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
    // Dirichlet rows: the mesh boundary (they belong to no tile)
    std::vector<uint8_t> mask(n, 0);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                if (i == 0 || j == 0 || i == nx - 1 || j == ny - 1 || (nz > 1 && (k == 0 || k == nz - 1)))
                    mask[(k * ny + j) * nx + i] = 1;
    TilePlan tp;
    if (!build_tile_plan(P, ntiles, K, T, 1 << 14, tp, mask.data(), 0, nullptr, 0, any_halo)) {
        std::printf("plan does not fit\n");
        return 3;
    }
    const int W = tp.W, RPT = tp.rpt, nkp = tp.nk_pad, NT = tp.ntiles;
    auto nt = [&](int t, int j) { return tp.n[(size_t)t * (TILE_MAX_DEPTH + 1) + j]; };
    auto grow = [&](int t, int l) { return tp.grow[(size_t)t * nkp + l]; };
    // tiles whose rings reach the mesh boundary before distance K: a ring row nearer than K that
    // has a Dirichlet row among its columns
    int cut_short = 0;
    for (int t = 0; t < NT; ++t) {
        bool cut = false;
        for (int l = nt(t, 0); l < nt(t, K - 1) && !cut; ++l)
            for (int32_t q = P.h_indptr[grow(t, l)]; q < P.h_indptr[grow(t, l) + 1]; ++q)
                cut = cut || mask[P.h_indices[q]];
        cut_short += cut;
    }
    std::printf("plan: %d tiles K %d rpt %d nk_pad %d max own %lld rows %lld red %.2f; tiles with rings "
                "cut short: %d\n", NT, tp.depth, RPT, nkp, (long long)tp.max_own, (long long)tp.max_rows,
                tp.mean_redundancy, cut_short);
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> M(P.npadded, 0.0), dinv(n, 1.0), b(n);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < P.h_indptr[r + 1] - P.h_indptr[r]; ++k) {
            const int c = P.h_indices[P.h_indptr[r] + k];
            M[P.sell_index(r, k)] = mask[c] ? 0.0 : (c == r ? 4.0 + U(rng) : 0.3 * U(rng));
            if (c == r && !mask[r]) dinv[r] = 1.0 / M[P.sell_index(r, k)];
        }
    for (auto &x : b) x = U(rng);
    std::vector<double> c1(its + 1, 0.0), c2(its + 1, 0.0), c3(its + 1, 0.37);
    for (int s = 2; s <= its; ++s) {
        c1[s] = 0.1 * U(rng);
        c2[s] = 1.0 + 0.1 * U(rng);
        c3[s] = 0.4 + 0.1 * U(rng);
    }
    const double post1 = 1.0 / 0.03, post2 = 1.0 / 0.7;
    // one step of one row: the chain of pc_rows_il
    auto epilogue = [&](int s, double p0, double p1, double d, double rhs, double acc) {
        double t = s >= 3 ? c1[s] * p0 : 0.0;
        if (s >= 2) t = std::fma(c2[s], p1, t);
        t = std::fma(c3[s], d * (rhs - acc), t);
        const bool fin = s == its;
        return (fin ? post2 : 1.0) * ((fin ? post1 : 1.0) * t);
    };
    // ---- reference: the global recurrence
    std::vector<double> ref(n, 0.0);
    {
        std::vector<double> pa(n, 0.0), pb(n, 0.0), pn(n, 0.0);
        for (int s = 1; s <= its; ++s) {
            for (int r = 0; r < n; ++r) {
                double acc = 0.0;
                if (s >= 2)
                    for (int k = 0; k < W; ++k) {
                        const int len = P.h_indptr[r + 1] - P.h_indptr[r];
                        const double v = k < len ? M[P.sell_index(r, k)] : 0.0;
                        const int c = k < len ? P.h_indices[P.h_indptr[r] + k] : r;
                        acc = std::fma(v, pb[c], acc);
                    }
                pn[r] = mask[r] ? 0.0 : epilogue(s, pa[r], pb[r], dinv[r], b[r], acc);
            }
            pa.swap(pb);
            pb.swap(pn);
        }
        ref = pb;
    }
    // ---- emulation.  Global pairs G[pair][0 newest / 1 older] with the step of every value
    // (-1: never written); the API-layout result is poisoned so that a row nobody writes shows.
    struct Val {
        double x = NAN;
        int step = -1;
    };
    std::vector<Val> G[2][2];
    for (auto &pr : G)
        for (auto &g : pr) g.assign(n, Val{});
    std::vector<double> out(n, NAN);
    long stale = 0, loads = 0, stores = 0, computed = 0;
    auto lval = [&](int t, int r, int k) {
        const int sl = r / T, tid = r % T;
        const size_t at = (((size_t)t * RPT + sl) * W + k) * T + tid;
        const int g = tp.gpos[at];
        return std::make_pair(g >= 0 ? M[g] : 0.0, (int)tp.lcol[at]);
    };
    const int nl = (its + K - 1) / K;
    for (int j = 0; j < nl; ++j) {
        const int s0 = j * K, k = std::min(K, its - s0), wr = j & 1, rd = wr ^ 1;
        const bool last = j + 1 == nl;
        // tiles in any order: a launch reads pair `rd` only and writes pair `wr` only
        for (int t = NT - 1; t >= 0; --t) {
            std::vector<Val> X[2];
            X[0].assign(nkp, Val{});
            X[1].assign(nkp, Val{});
            // the zero slot holds the (zero) iterate of every step
            const int nk = nt(t, k), nk1 = nt(t, k - 1), n0 = nt(t, 0);
            int cur = 0;
            for (int l = 0; l < nk; ++l) {
                if (s0 == 0) {
                    X[0][l] = Val{0.0, 0};
                    X[1][l] = Val{0.0, -1};
                } else {
                    X[0][l] = G[rd][0][grow(t, l)];
                    X[1][l] = s0 >= 2 ? G[rd][1][grow(t, l)] : Val{0.0, -1};
                    loads += s0 >= 2 ? 2 : 1;
                }
            }
            std::vector<double> bl(nk1);
            for (int r = 0; r < nk1; ++r) bl[r] = b[grow(t, r)];
            loads += nk1;
            for (int q = 1; q <= k; ++q) {
                const int s = s0 + q, nv = nt(t, k - q);
                std::vector<Val> &Xc = X[cur], &Xo = X[cur ^ 1];
                for (int r = 0; r < nv; ++r) {
                    double acc = 0.0;
                    if (s >= 2)
                        for (int e = 0; e < W; ++e) {
                            const auto vc = lval(t, r, e);
                            double xv = 0.0;
                            if (vc.second != nkp - 1) {
                                // (padding entries multiply 0 with the row's own value)
                                if (Xc[vc.second].step != s - 1) ++stale;
                                xv = Xc[vc.second].x;
                            }
                            acc = std::fma(vc.first, xv, acc);
                        }
                    if (s >= 3 && Xo[r].step != s - 2) ++stale;
                    if (s >= 2 && Xc[r].step != s - 1) ++stale;
                    const int g = grow(t, r);
                    // in place over the older iterate
                    Xo[r] = Val{epilogue(s, Xo[r].x, Xc[r].x, dinv[g], bl[r], acc), s};
                    ++computed;
                }
                cur ^= 1;
            }
            for (int r = 0; r < n0; ++r) {
                const int g = grow(t, r);
                if (last) {
                    if (X[cur][r].step != its) ++stale;
                    out[g] = X[cur][r].x;
                    stores += 1;
                } else {
                    if (X[cur][r].step != s0 + k || X[cur ^ 1][r].step != s0 + k - 1) ++stale;
                    G[wr][0][g] = X[cur][r];
                    G[wr][1][g] = X[cur ^ 1][r];
                    stores += 2;
                }
            }
        }
        if (last)
            for (int r = 0; r < n; ++r)
                if (mask[r]) out[r] = 0.0;
    }
    long bad = 0, neg_zero = 0;
    for (int r = 0; r < n; ++r) {
        if (!(ref[r] == out[r])) ++bad;
        if (mask[r] && (out[r] != 0.0 || std::signbit(out[r]))) ++neg_zero;
    }
    long own = 0;
    for (int t = 0; t < NT; ++t) own += nt(t, 0);
    std::printf("launches: %d; rows computed %ld of %ld necessary; loads %ld stores %ld\n", nl, computed,
                own * its, loads, stores);
    std::printf("mismatches: %ld of %d, stale reads: %ld, boundary rows not +0: %ld\n", bad, n, stale,
                neg_zero);
    return bad || stale || neg_zero ? 1 : 0;
}
