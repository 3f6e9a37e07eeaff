// The scalar side of the spectrum estimates (spectrum.cpp), free of HIP so that the native test
// tests/native/spectrum_lockstep_emu.cpp compiles it as it is: the Lanczos tridiagonal's
// eigenvalues, the per-step scalar work of the conjugate-gradient recurrences (what the second
// stage of a batched dot runs on the device and the one-matrix loop runs on the host), and the
// host's half of the lock-step loop -- the Ritz check every 10 steps -- and the grouping of the
// twin search (tests/native/twin_groups.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define KKT_SPEC_HD __host__ __device__ inline
#else
#define KKT_SPEC_HD inline
#endif

namespace kkt {

// [emin, emax] of the Jacobi-scaled matrix D^-1 A by `steps` Lanczos steps on the device
// (spectrum.cpp); Ritz values: emin is an upper estimate of the smallest eigenvalue, emax a
// lower estimate of the largest.
struct Spectrum {
    double emin, emax;
    int steps;
};

namespace spec {

constexpr int RITZ_FIRST = 30, RITZ_EVERY = 10;   // the 1 % rule runs at steps 30, 40, ...
constexpr int POWER_MIN_STEPS = 8;                // the 0.5 % rule of the power iteration from here

// eigenvalues of the symmetric tridiagonal matrix (d, e) by implicit QL (EISPACK tql1)
inline std::vector<double> tridiag_eigenvalues(std::vector<double> d, std::vector<double> e) {
    const int n = (int)d.size();
    e.resize(n, 0.0);
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= 1e-16 * dd) break;
            }
            if (m != l) {
                if (++iter > 200) break;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = std::hypot(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
            }
        } while (m != l);
    }
    std::sort(d.begin(), d.end());
    return d;
}

// extreme eigenvalues of the Lanczos matrix of m PCG steps (alpha[0, m), beta[0, m - 1))
inline void ritz(const std::vector<double> &alpha, const std::vector<double> &beta, double *lo,
                 double *hi) {
    const int m = (int)alpha.size();
    std::vector<double> d(m), e(m > 1 ? m - 1 : 0);
    for (int k = 0; k < m; ++k) {
        d[k] = 1.0 / alpha[k] + (k > 0 ? beta[k - 1] / alpha[k - 1] : 0.0);
        if (k + 1 < m) e[k] = std::sqrt(beta[k]) / alpha[k];
    }
    const std::vector<double> ev = tridiag_eigenvalues(d, e);
    *lo = ev.front();
    *hi = ev.back();
}
inline bool ritz_due(int k) { return k >= RITZ_FIRST && k % RITZ_EVERY == 0; }
// the smallest Ritz value is the slow one: stop when it moved by less than 1 % over the last 10
// steps
inline bool ritz_settled(double lo, double last_lo) {
    return last_lo > 0.0 && std::fabs(lo - last_lo) <= 0.01 * last_lo;
}
inline Spectrum ritz_result(const std::vector<double> &alpha, const std::vector<double> &beta) {
    Spectrum out{0.0, 0.0, (int)alpha.size()};
    if (!alpha.empty()) ritz(alpha, beta, &out.emin, &out.emax);
    return out;
}

KKT_SPEC_HD bool finite_d(double x) { return __builtin_isfinite(x); }

// ---- one matrix's scalars of the recurrence.  Plain IEEE double: a quotient or a comparison per
// call, nothing a compiler could contract.
// start: rz = <r, z>; the loop runs while rz > 0 and finite
KKT_SPEC_HD bool lanczos_start(double rz0, double *rz) {
    *rz = rz0;
    return rz0 > 0.0 && finite_d(rz0);
}
// after pAp = <p, A p>: false (before alpha is recorded) when pAp is not positive or not finite
KKT_SPEC_HD bool lanczos_alpha(double pAp, double rz, double *a) {
    if (!(pAp > 0.0) || !finite_d(pAp)) return false;
    *a = rz / pAp;
    return true;
}
// after rz_new = <r, z> of the updated r: false (after alpha and the r update, before beta) when
// the residual is gone or not finite
KKT_SPEC_HD bool lanczos_beta(double rz_new, double rz, double *b) {
    if (!(rz_new > 1e-28 * rz) || !finite_d(rz_new)) return false;
    *b = rz_new / rz;
    return true;
}

// ---- power iteration on -(D^-1 S)^2: nv = ||v|| after a step
KKT_SPEC_HD bool power_live(double nv) { return nv > 0.0 && finite_d(nv); }
// after step k (0-based) with mu2 = nv: true when the estimate moved by at most 0.5 %
KKT_SPEC_HD bool power_settled(int k, double mu2, double last) {
    const double diff = mu2 - last;
    return k >= POWER_MIN_STEPS && (diff < 0.0 ? -diff : diff) <= 0.005 * mu2;
}

// ---- the host's half of a batch of B recurrences in lock-step.  The device keeps alpha / beta
// step-major (entry s of matrix b at [s * B + b]), their counts and an `active` word per matrix;
// the host absorbs what is new at the steps ritz_due() names, applies the 1 % rule per matrix and
// names the matrices whose `active` word it clears.
struct LockStep {
    int B = 0;
    std::vector<std::vector<double>> alpha, beta;
    std::vector<double> last_lo;
    std::vector<uint32_t> active;   // the device's words as of the last absorb, minus the host's own stops
    int absorbed = 0;               // steps [0, absorbed) of the device arrays are on the host

    explicit LockStep(int nb) : B(nb), alpha(nb), beta(nb), last_lo(nb, 0.0), active(nb, 1u) {}

    // rows [absorbed, k) of the device's step-major arrays (new_alpha / new_beta start at row
    // `absorbed`), and the counts and words as they stand after step k - 1
    void absorb(int k, const double *new_alpha, const double *new_beta, const int32_t *na,
                const int32_t *nb, const uint32_t *dev_active) {
        for (int b = 0; b < B; ++b) {
            for (int s = absorbed; s < k; ++s) {
                if (s < na[b] && (int)alpha[b].size() == s)
                    alpha[b].push_back(new_alpha[(size_t)(s - absorbed) * B + b]);
                if (s < nb[b] && (int)beta[b].size() == s)
                    beta[b].push_back(new_beta[(size_t)(s - absorbed) * B + b]);
            }
            if (!dev_active[b]) active[b] = 0u;
        }
        absorbed = std::max(absorbed, k);
    }
    // the check at the top of step k: true when a matrix was stopped here (write `active` back)
    bool check(int k) {
        bool changed = false;
        if (!ritz_due(k)) return false;
        for (int b = 0; b < B; ++b) {
            if (!active[b]) continue;
            double lo, hi;
            ritz(alpha[b], beta[b], &lo, &hi);
            if (ritz_settled(lo, last_lo[b])) {
                active[b] = 0u;
                changed = true;
            } else {
                last_lo[b] = lo;
            }
        }
        return changed;
    }
    bool any_active() const {
        for (uint32_t a : active)
            if (a) return true;
        return false;
    }
    Spectrum result(int b) const { return ritz_result(alpha[b], beta[b]); }
};

// ---- the grouping of the twin search (SchurPC::collect_matrices).  Candidates come in creation
// order with the bits of their shift and the folded fingerprint of their values.  A candidate whose
// (shift, fingerprint) was seen before is compared bit for bit with the FIRST candidate that had
// it; a fingerprint only prunes, it never makes a twin.  `tag` (optional, one per candidate) keeps
// kinds of candidates apart that share a search: only candidates of one tag are ever compared.
struct TwinGroups {
    std::vector<int> first_of;                  // i itself: candidate i opens its group
    std::vector<std::pair<int, int>> pairs;     // (group's first, candidate): to compare
    std::vector<int> pair_of;                   // the candidate's pair, -1 for a group's first
};
inline TwinGroups group_twins(const std::vector<uint64_t> &shift_bits,
                              const std::vector<uint64_t> &fingerprint,
                              const std::vector<int> &tag = {}) {
    const int C = (int)shift_bits.size();
    TwinGroups T;
    T.first_of.resize(C);
    T.pair_of.assign(C, -1);
    std::map<std::pair<int, std::pair<uint64_t, uint64_t>>, int> groups;
    for (int i = 0; i < C; ++i) {
        T.first_of[i] = i;
        const auto g = std::make_pair(tag.empty() ? 0 : tag[i],
                                      std::make_pair(shift_bits[i], fingerprint[i]));
        const auto it = groups.find(g);
        if (it == groups.end()) {
            groups[g] = i;
            continue;
        }
        T.first_of[i] = it->second;
        T.pair_of[i] = (int)T.pairs.size();
        T.pairs.emplace_back(it->second, i);
    }
    return T;
}
// The comparison's flags (one per pair, non-zero: the arrays differ) into classes: cls[i] is the
// class of candidate i, numbered in order of their first members (`reps`).  Equal fingerprints but
// different bits: first_of = -1 and no class (-1) -- such a candidate is left to the caller's own
// comparison, and nothing shares with it.
inline std::vector<int> twin_classes(TwinGroups &T, const std::vector<unsigned> &differ,
                                     std::vector<int> *reps) {
    const int C = (int)T.first_of.size();
    for (int i = 0; i < C; ++i)
        if (T.pair_of[i] >= 0 && differ[T.pair_of[i]]) T.first_of[i] = -1;
    std::vector<int> cls(C, -1);
    reps->clear();
    for (int i = 0; i < C; ++i) {
        if (T.first_of[i] == i) {
            cls[i] = (int)reps->size();
            reps->push_back(i);
        } else if (T.first_of[i] >= 0) {
            cls[i] = cls[T.first_of[i]];
        }
    }
    return cls;
}

}  // namespace spec
}  // namespace kkt
