// Coefficients of the Jacobi-Chebyshev sub-solves: the one place the recurrence is written, so
// that the plain launches, the interleaved steps, the tile programs and the pressure-space chains
// of both preconditioners run the same doubles.  Host-only, no HIP include.
#pragma once
#include <vector>

namespace kkt {

struct TileCoef { double c1, c2, c3; };

// KSPSolve_Chebyshev (first kind) + PCJACOBI on [emin, emax], zero initial guess:
// p_1 = scale D^-1 b, then p_s = c1 p_{s-2} + c2 p_{s-1} + c3 D^-1 (b - A p_{s-1}).
struct ChebCoefficients {
    double scale;                  // the first step
    std::vector<TileCoef> steps;   // steps 2 .. its
    // step s >= 2 (the callers write step 1 themselves: it has no matrix term, or starts from a
    // coarse correction)
    const TileCoef &step(int s) const { return steps[(size_t)s - 2]; }
};

// eimag > 0: the spectrum lies in the ellipse with centre d = (emax + emin) / 2 and semi-axes
// a = (emax - emin) / 2, eimag (blocks with a convection term).  Manteuffel's recurrence
// (Numer. Math. 28, 1977) for the same three-term sweep: alpha_1 = 2d / (2d^2 - c^2),
// alpha_n = 1 / (d - (c^2 / 4) alpha_{n-1}), beta_n = d alpha_n - 1 with c^2 = a^2 - eimag^2,
// which may be negative -- only c^2 enters, the arithmetic stays real.  Restated in the
// oracle (chebyshev_ellipse_coefficients); for eimag == 0 PETSc's form is kept, bit for bit what
// rounds 1 and 2 ran.  No expression here may be reordered: tests/test_cheb_coefficients.py
// compares every coefficient bit for bit.
inline ChebCoefficients cheb_coefficients(int its, double emin, double emax, double eimag = 0.0) {
    ChebCoefficients out;
    const double scale = 2.0 / (emax + emin);
    out.scale = scale;
    const double alpha = 1.0 - scale * emin;
    const double mu = 1.0 / alpha, omegaprod = 2.0 / alpha;
    double c_km1 = 1.0, c_k = mu;
    const double ell_d = 0.5 * (emax + emin), ell_a = 0.5 * (emax - emin);
    const double ell_c2 = ell_a * ell_a - eimag * eimag;
    double ell_alpha = 1.0 / ell_d;
    for (int step = 2; step <= its; ++step) {
        if (eimag > 0.0) {
            ell_alpha = 1.0 / (ell_d - (step == 2 ? 0.5 : 0.25) * ell_c2 * ell_alpha);
            const double beta = ell_d * ell_alpha - 1.0;
            out.steps.push_back(TileCoef{-beta, 1.0 + beta, ell_alpha});
        } else {
            const double c_kp1 = 2.0 * mu * c_k - c_km1;
            const double omega = omegaprod * c_k / c_kp1;
            out.steps.push_back(TileCoef{1.0 - omega, omega, scale * omega});
            c_km1 = c_k;
            c_k = c_kp1;
        }
    }
    return out;
}

}  // namespace kkt
