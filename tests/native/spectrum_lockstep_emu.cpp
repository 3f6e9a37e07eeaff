// The lock-step controller of the batched spectrum estimates (control_amd/csrc/spectrum_host.hpp)
// against the one-matrix loop, on small dense matrices in plain C++.
//
// one_matrix() is jacobi_spectrum's loop written out: its own alpha / beta vectors, its break
// rules, the Ritz check every 10 steps from step 30.  lock_step() is jacobi_spectrum_batch's
// shape: the "device" side keeps step-major alpha / beta arrays, counts, <r, z> and an `active`
// word per matrix and runs the per-step scalars of spectrum_host.hpp (the functions the second
// stage of the batched dot calls); the host side is spec::LockStep, which absorbs what is new at
// the steps the one-matrix loop runs its Ritz check at and clears the words of matrices that are
// done.  Step counts and intervals must be identical, bit for bit.
//
// The batch mixes matrices that stop at different steps by the 1 % rule, by a vanished residual,
// at step 0 before alpha (A = 0) and after it (A = 2 I), one that never starts (<r, z> = 0) and
// one that reaches max_steps; it is run with max_steps 400 and with 45 (a last stretch that is no
// multiple of 10).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spectrum_host.hpp"

using kkt::Spectrum;
namespace spec = kkt::spec;

struct Dense {
    const char *name;
    int n;
    std::vector<double> a, dinv;
};

static std::vector<double> start_vector(int n) {
    std::vector<double> h(n);
    uint64_t sd = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < n; ++i) {
        sd = sd * 6364136223846793005ull + 1442695040888963407ull;
        h[i] = (double)(sd >> 11) / (double)(1ull << 53) - 0.5;
    }
    return h;
}
static double dot(const std::vector<double> &x, const std::vector<double> &y) {
    double s = 0.0;
    for (size_t i = 0; i < x.size(); ++i) s = std::fma(x[i], y[i], s);
    return s;
}
static void matvec(const Dense &A, const std::vector<double> &x, std::vector<double> &y) {
    for (int i = 0; i < A.n; ++i) {
        double s = 0.0;
        for (int j = 0; j < A.n; ++j) s = std::fma(A.a[(size_t)i * A.n + j], x[j], s);
        y[i] = s;
    }
}
static void jacobi(const Dense &A, const std::vector<double> &r, std::vector<double> &z) {
    for (int i = 0; i < A.n; ++i) z[i] = A.dinv[i] * r[i];
}

static Spectrum one_matrix(const Dense &A, int max_steps) {
    const int n = A.n;
    std::vector<double> r = start_vector(n), z(n), p(n), w(n);
    jacobi(A, r, z);
    p = z;
    double rz = dot(r, z);
    std::vector<double> alpha, beta;
    double last_lo = 0.0;
    for (int k = 0; k < max_steps && rz > 0.0 && std::isfinite(rz); ++k) {
        if (k >= 30 && k % 10 == 0) {
            double lo, hi;
            spec::ritz(alpha, beta, &lo, &hi);
            if (last_lo > 0.0 && std::fabs(lo - last_lo) <= 0.01 * last_lo) break;
            last_lo = lo;
        }
        matvec(A, p, w);
        const double pAp = dot(p, w);
        if (!(pAp > 0.0) || !std::isfinite(pAp)) break;
        const double a = rz / pAp;
        alpha.push_back(a);
        for (int i = 0; i < n; ++i) r[i] = std::fma(-a, w[i], r[i]);
        jacobi(A, r, z);
        const double rz_new = dot(r, z);
        if (!(rz_new > 1e-28 * rz) || !std::isfinite(rz_new)) break;
        const double b = rz_new / rz;
        beta.push_back(b);
        for (int i = 0; i < n; ++i) p[i] = std::fma(1.0, z[i], b * p[i]);
        rz = rz_new;
    }
    Spectrum out{0.0, 0.0, (int)alpha.size()};
    if (alpha.empty()) return out;
    spec::ritz(alpha, beta, &out.emin, &out.emax);
    return out;
}

static std::vector<Spectrum> lock_step(const std::vector<Dense> &mats, int max_steps, int *host_checks) {
    const int B = (int)mats.size();
    // ---- the device's memory
    std::vector<std::vector<double>> r(B), z(B), p(B), w(B);
    std::vector<double> alpha((size_t)max_steps * B, -1.0), beta((size_t)max_steps * B, -1.0);
    std::vector<int32_t> na(B, 0), nb(B, 0);
    std::vector<double> rz(B, 0.0), coef(B, 0.0);
    std::vector<uint32_t> active(B, 1u);
    for (int b = 0; b < B; ++b) {
        const int n = mats[b].n;
        r[b] = start_vector(n);
        z[b].assign(n, 0.0), p[b].assign(n, 0.0), w[b].assign(n, 0.0);
        jacobi(mats[b], r[b], z[b]);
        p[b] = z[b];
        if (!spec::lanczos_start(dot(r[b], z[b]), &rz[b])) active[b] = 0u;
    }
    // ---- the host
    spec::LockStep L(B);
    *host_checks = 0;
    auto absorb = [&](int k) {
        const size_t row = (size_t)L.absorbed * B;
        L.absorb(k, alpha.data() + row, beta.data() + row, na.data(), nb.data(), active.data());
        ++*host_checks;
    };
    int k = 0;
    for (; k < max_steps; ++k) {
        if (spec::ritz_due(k)) {
            absorb(k);
            if (L.check(k)) active = L.active;      // the copy of the words back to the device
            if (!L.any_active()) break;
        }
        for (int b = 0; b < B; ++b) {               // one launch per stage: every active matrix
            if (!active[b]) continue;
            const int n = mats[b].n;
            matvec(mats[b], p[b], w[b]);
            if (!spec::lanczos_alpha(dot(p[b], w[b]), rz[b], &coef[b])) {
                active[b] = 0u;
                continue;
            }
            alpha[(size_t)na[b]++ * B + b] = coef[b];
            for (int i = 0; i < n; ++i) r[b][i] = std::fma(-coef[b], w[b][i], r[b][i]);
            jacobi(mats[b], r[b], z[b]);
            const double rz_new = dot(r[b], z[b]);
            if (!spec::lanczos_beta(rz_new, rz[b], &coef[b])) {
                active[b] = 0u;
                continue;
            }
            beta[(size_t)nb[b]++ * B + b] = coef[b];
            rz[b] = rz_new;
            for (int i = 0; i < n; ++i) p[b][i] = std::fma(1.0, z[b][i], coef[b] * p[b][i]);
        }
    }
    if (L.absorbed < k) absorb(k);
    std::vector<Spectrum> out(B);
    for (int b = 0; b < B; ++b) out[b] = L.result(b);
    return out;
}

static Dense laplacian(const char *name, int n, double shift, bool neumann) {
    Dense A{name, n, std::vector<double>((size_t)n * n, 0.0), std::vector<double>(n)};
    for (int i = 0; i < n; ++i) {
        double d = 2.0 + shift;
        if (neumann && (i == 0 || i == n - 1)) d = 1.0 + shift;
        A.a[(size_t)i * n + i] = d;
        if (i > 0) A.a[(size_t)i * n + i - 1] = -1.0;
        if (i + 1 < n) A.a[(size_t)i * n + i + 1] = -1.0;
        A.dinv[i] = 1.0 / d;
    }
    return A;
}
static Dense scaled_identity(const char *name, int n, double d, double dinv) {
    Dense A{name, n, std::vector<double>((size_t)n * n, 0.0), std::vector<double>(n, dinv)};
    for (int i = 0; i < n; ++i) A.a[(size_t)i * n + i] = d;
    return A;
}
// a graded diagonal plus a weak coupling: a wide spectrum whose ends settle at another pace
static Dense graded(const char *name, int n, double ratio) {
    Dense A{name, n, std::vector<double>((size_t)n * n, 0.0), std::vector<double>(n)};
    for (int i = 0; i < n; ++i) {
        const double d = std::pow(ratio, (double)i / (n - 1));
        A.a[(size_t)i * n + i] = d;
        if (i + 1 < n) A.a[(size_t)i * n + i + 1] = A.a[(size_t)(i + 1) * n + i] = 0.01;
        A.dinv[i] = 1.0;      // unscaled on purpose: the interval is the matrix's own
    }
    return A;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    std::vector<Dense> mats;
    mats.push_back(laplacian("laplacian 300", 300, 0.0, false));
    mats.push_back(laplacian("laplacian 40 (residual vanishes)", 40, 0.0, false));
    mats.push_back(laplacian("shifted laplacian 120", 120, 0.05, false));
    mats.push_back(laplacian("neumann laplacian 90 (singular)", 90, 0.0, true));
    mats.push_back(scaled_identity("2 I (stops at step 0 after alpha)", 17, 2.0, 0.5));
    mats.push_back(scaled_identity("0 (stops at step 0 before alpha)", 9, 0.0, 1.0));
    mats.push_back(scaled_identity("D^-1 = 0 (never starts)", 5, 1.0, 0.0));
    mats.push_back(graded("graded 200", 200, 1.0e6));
    mats.push_back(laplacian("laplacian 400", 400, 0.0, false));
    int failures = 0;
    for (int max_steps : {400, 45}) {
        int checks = 0;
        const std::vector<Spectrum> batch = lock_step(mats, max_steps, &checks);
        std::vector<int> steps;
        for (size_t b = 0; b < mats.size(); ++b) {
            const Spectrum one = one_matrix(mats[b], max_steps);
            const bool ok = one.steps == batch[b].steps && same_bits(one.emin, batch[b].emin) &&
                            same_bits(one.emax, batch[b].emax);
            std::printf("max_steps %3d  %-40s one-matrix %3d steps [%.17g, %.17g]  lock-step %3d steps  %s\n",
                        max_steps, mats[b].name, one.steps, one.emin, one.emax, batch[b].steps,
                        ok ? "equal" : "DIFFERENT");
            failures += !ok;
            steps.push_back(one.steps);
        }
        // the cases the batch is meant to hold
        auto count = [&](int s) {
            int c = 0;
            for (int v : steps) c += v == s;
            return c;
        };
        int distinct_late = 0;      // different stopping steps beyond the first Ritz check
        for (size_t b = 0; b < steps.size(); ++b) {
            bool first = steps[b] >= spec::RITZ_FIRST;
            for (size_t c = 0; c < b; ++c) first = first && steps[c] != steps[b];
            distinct_late += first;
        }
        const bool covered = count(0) == 2 && count(1) == 1 && count(max_steps) >= 1 &&
                             (max_steps < 400 || distinct_late >= 3);
        if (!covered) {
            std::printf("max_steps %d: the batch does not cover its cases (steps 0: %d, 1: %d, max: %d, "
                        "distinct late stops: %d)\n", max_steps, count(0), count(1), count(max_steps),
                        distinct_late);
            ++failures;
        }
        // one host check per 10 steps from step 30, and one at the end at most
        if (checks > (max_steps + 9) / 10 + 1) {
            std::printf("max_steps %d: %d host checks\n", max_steps, checks);
            ++failures;
        }
    }
    std::printf("spectrum lock-step: %d failures\n", failures);
    return failures ? 1 : 0;
}
