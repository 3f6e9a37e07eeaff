// Spectrum of a Jacobi-scaled sub-solve matrix on the device: the interval for the
// Jacobi-Chebyshev sweeps that stand in for the reference's BoomerAMG cycles
// (control/control.py:2242-2431; BASELINE.json north_star).  The reference gives no interval for
// these solves (it uses AMG); a fixed hand-set one fits only the mesh it was found for.
//
// Lanczos through the conjugate-gradient recurrences with the Jacobi preconditioner
// (the coefficients alpha_k, beta_k of PCG define the Lanczos tridiagonal matrix of
// D^-1/2 A D^-1/2): k SpMVs with the existing block-row kernel, two reductions and three
// vector updates per step, the k x k tridiagonal eigenproblem on the host.  Extreme Ritz
// values converge first and from inside the spectrum, so the interval is widened a little.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pc.hpp"

namespace kkt {

namespace {

// deterministic start vector with all frequencies, zero on the boundary rows (one blocking copy of
// the mask); zero_mean: see jacobi_spectrum
std::vector<double> start_vector(int64_t n, uint64_t seed, const uint8_t *rowmask, bool zero_mean) {
    std::vector<double> h(n);
    uint64_t sd = seed;
    for (int64_t i = 0; i < n; ++i) {
        sd = sd * 6364136223846793005ull + 1442695040888963407ull;
        h[i] = (double)(sd >> 11) / (double)(1ull << 53) - 0.5;
    }
    if (rowmask) {
        std::vector<uint8_t> m(n);
        HIPCHK(hipMemcpy(m.data(), rowmask, n, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            if (m[i]) h[i] = 0.0;
    }
    if (zero_mean) {
        long double sum = 0.0L;
        for (int64_t i = 0; i < n; ++i) sum += h[i];
        const double mean = (double)(sum / (long double)n);
        for (int64_t i = 0; i < n; ++i) h[i] -= mean;
    }
    return h;
}
constexpr uint64_t LANCZOS_SEED = 0x9e3779b97f4a7c15ull, POWER_SEED = 0x2545f4914f6cdd1dull;

// the ops of the matrices still running, in batch order, as one launch list
struct OpList {
    RowOp *d = nullptr;
    int n = 0;
};
OpList live_ops(DevPool &mem, const std::vector<RowOp> &all, const std::vector<uint32_t> &active) {
    std::vector<RowOp> live;
    for (size_t b = 0; b < all.size(); ++b)
        if (active[b]) live.push_back(all[b]);
    OpList L;
    L.n = (int)live.size();
    if (L.n) L.d = mem.upload(live.data(), live.size());
    return L;
}

}  // namespace

// `zero_mean`: the matrix is singular with the constants in its kernel (a Neumann Laplacian):
// the start vector gets zero mean, so the recurrence stays in the range and the smallest Ritz
// value approaches the smallest NON-ZERO eigenvalue.
Spectrum jacobi_spectrum(System &S, int pattern, const double *vals, const double *dinv,
                         const uint8_t *rowmask, int max_steps, bool zero_mean) {
    const Pattern &P = S.patterns[pattern];
    const int64_t n = P.nrows;
    hipStream_t st = S.stream;
    DevPool tmp;   // released on every way out
    auto vec = [&]() {
        double *p = tmp.alloc<double>(n + 32);
        HIPCHK(hipMemsetAsync(p, 0, (n + 32) * sizeof(double), st));
        return p;
    };
    double *r = vec(), *z = vec(), *p = vec(), *w = vec();
    double *scratch = tmp.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX);
    double *d_out = tmp.alloc<double>(4);
    {
        const std::vector<double> h = start_vector(n, LANCZOS_SEED, rowmask, zero_mean);
        HIPCHK(hipMemcpy(r, h.data(), n * sizeof(double), hipMemcpyHostToDevice));
    }
    // w = A p (boundary rows 0) and z = D^-1 r as single RowOps through the kernel arguments
    const RowOp opA = lin_op(P, n, rowmask, LinStep{{RowTerm{vals, p}}, w});
    const RowOp opZ = cheb_op(P, n, rowmask,
                              ChebStep{nullptr, dinv, r, nullptr, nullptr, z, 0.0, 0.0, 1.0});
    RowOp *d_ops = nullptr;
    {
        RowOp both[2] = {opA, opZ};
        d_ops = tmp.upload(both, 2);
    }
    const Bases B{{nullptr, nullptr, nullptr, nullptr}};
    auto run = [&](int which) {
        launch_rowops(st, d_ops + which, 1, P.nslices, P.R, B, 1, which == 0 ? P.uniform_w : 0);
    };
    double host[2];
    auto dot = [&](const double *a, const double *b) {
        VecList L{};
        L.v[0] = b;
        launch_mdot(st, a, L, 1, n, scratch, d_out);
        HIPCHK(hipMemcpyAsync(host, d_out, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return host[0];
    };
    run(1);                                   // z = D^-1 r
    launch_copy(st, p, z, n);
    double rz = dot(r, z);
    std::vector<double> alpha, beta;
    auto ritz = [&](double *lo_, double *hi_) { spec::ritz(alpha, beta, lo_, hi_); };
    double last_lo = 0.0;
    for (int k = 0; k < max_steps && rz > 0.0 && std::isfinite(rz); ++k) {
        // the smallest Ritz value is the slow one: stop when it moved by less than 1 % over the
        // last 10 steps
        if (k >= 30 && k % 10 == 0) {
            double lo_, hi_;
            ritz(&lo_, &hi_);
            if (last_lo > 0.0 && std::fabs(lo_ - last_lo) <= 0.01 * last_lo) break;
            last_lo = lo_;
        }
        run(0);                               // w = A p
        const double pAp = dot(p, w);
        if (!(pAp > 0.0) || !std::isfinite(pAp)) break;
        const double a = rz / pAp;
        alpha.push_back(a);
        launch_axpby(st, r, -a, w, 1.0, n);   // r -= a w
        run(1);                               // z = D^-1 r
        const double rz_new = dot(r, z);
        if (!(rz_new > 1e-28 * rz) || !std::isfinite(rz_new)) break;
        const double b = rz_new / rz;
        beta.push_back(b);
        launch_axpby(st, p, 1.0, z, b, n);    // p = z + b p
        rz = rz_new;
    }
    Spectrum out{0.0, 0.0, (int)alpha.size()};
    const int m = (int)alpha.size();
    if (m == 0) return out;
    ritz(&out.emin, &out.emax);
    return out;
}

// rho(D^-1 S) for a skew-symmetric S (the convection part of a sub-solve matrix): its eigenvalues
// are +- i mu_j, so (D^-1 S)^2 is similar to a negative semi-definite matrix with eigenvalues
// -mu_j^2; power iteration v <- (D^-1 S)^2 v, mu^2 ~ ||(D^-1 S)^2 v|| / ||v||.  Two SpMVs and one
// reduction per step; the estimate approaches mu_max from below (the caller widens it).
double jacobi_skew_radius(System &S, int pattern, const double *skew_vals, const double *dinv,
                          const uint8_t *rowmask, int max_steps, int *steps_out) {
    const Pattern &P = S.patterns[pattern];
    const int64_t n = P.nrows;
    hipStream_t st = S.stream;
    DevPool tmp;   // released on every way out
    auto vec = [&]() {
        double *p = tmp.alloc<double>(n + 32);
        HIPCHK(hipMemsetAsync(p, 0, (n + 32) * sizeof(double), st));
        return p;
    };
    double *v = vec(), *z = vec();
    double *scratch = tmp.alloc<double>((size_t)REDUCE_BLOCKS * MDOT_MAX);
    double *d_out = tmp.alloc<double>(4);
    {
        const std::vector<double> h = start_vector(n, POWER_SEED, rowmask, false);
        HIPCHK(hipMemcpy(v, h.data(), n * sizeof(double), hipMemcpyHostToDevice));
    }
    // y = -D^-1 (0 - S x): the Chebyshev epilogue with c3 = -1 and no right-hand side
    auto op = [&](const double *x, double *y) {
        return cheb_op(P, n, rowmask,
                       ChebStep{skew_vals, dinv, nullptr, nullptr, nullptr, y, 0.0, 0.0, -1.0, 1.0, 1.0, x});
    };
    const RowOp both[2] = {op(v, z), op(z, v)};
    RowOp *d_ops = tmp.upload(both, 2);
    const Bases B{{nullptr, nullptr, nullptr, nullptr}};
    double host[2];
    auto norm = [&](const double *a) {
        VecList L{};
        L.v[0] = a;
        launch_mdot(st, a, L, 1, n, scratch, d_out);
        HIPCHK(hipMemcpyAsync(host, d_out, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return std::sqrt(host[0]);
    };
    double nv = norm(v), mu2 = 0.0, last = -1.0;
    int k = 0;
    for (; k < max_steps && nv > 0.0 && std::isfinite(nv); ++k) {
        launch_axpby(st, v, 0.0, z, 1.0 / nv, n);      // v /= ||v||
        launch_rowops(st, d_ops, 1, P.nslices, P.R, B, 1, P.uniform_w);       // z = D^-1 S v
        launch_rowops(st, d_ops + 1, 1, P.nslices, P.R, B, 1, P.uniform_w);   // v = D^-1 S z
        nv = norm(v);
        mu2 = nv;
        if (k >= 8 && std::fabs(mu2 - last) <= 0.005 * mu2) {
            ++k;
            break;
        }
        last = mu2;
    }
    if (steps_out) *steps_out = k;
    return (mu2 > 0.0 && std::isfinite(mu2)) ? std::sqrt(mu2) : 0.0;
}

// ---- the same estimates for a batch of matrices on one pattern, in lock-step: one launch per
// stage for the whole batch, the scalars of the recurrences on the device (spectrum_kernels.hip),
// the host back in only where its stopping rule reads the coefficients.  Per matrix the arithmetic
// and its order are jacobi_spectrum's / jacobi_skew_radius's, so the results are theirs bit for bit.

namespace {

// the vectors of a batch (zeroed), its partial sums and its per-matrix scalars
struct BatchMem {
    SpecBatch S{};
    int32_t *ints = nullptr;      // na | nb | active: one copy back
    size_t bytes = 0;
    BatchMem(DevPool &tmp, hipStream_t st, int B, int64_t n, int nvec, int max_steps) {
        S.B = B;
        S.max_steps = max_steps;
        S.n = n;
        S.stride = spec_batch_stride(n);
        const size_t nv = (size_t)nvec * B * S.stride;
        double *v = tmp.alloc<double>(nv);
        HIPCHK(hipMemsetAsync(v, 0, nv * sizeof(double), st));
        S.r = v;
        S.z = v + (size_t)B * S.stride;
        if (nvec == 4) {
            S.p = v + 2 * (size_t)B * S.stride;
            S.w = v + 3 * (size_t)B * S.stride;
        }
        S.part = tmp.alloc<double>((size_t)B * REDUCE_BLOCKS);
        const size_t nab = 2 * (size_t)max_steps * B, nsc = 4 * (size_t)B;
        S.alpha = tmp.alloc<double>(nab);
        S.beta = S.alpha + (size_t)max_steps * B;
        double *sc = tmp.alloc<double>(nsc);
        HIPCHK(hipMemsetAsync(sc, 0, nsc * sizeof(double), st));
        S.rz = sc;
        S.coef = sc + B;
        S.mu2 = sc + 2 * (size_t)B;
        S.last = sc + 3 * (size_t)B;
        std::vector<int32_t> h(3 * (size_t)B, 0);
        for (int b = 0; b < B; ++b) h[2 * (size_t)B + b] = 1;
        ints = tmp.upload(h.data(), h.size());
        S.na = ints;
        S.nb = ints + B;
        S.active = reinterpret_cast<uint32_t *>(ints + 2 * (size_t)B);
        bytes = (nv + (size_t)B * REDUCE_BLOCKS + nab + nsc) * sizeof(double) + h.size() * sizeof(int32_t);
    }
    double *vec(double *family, int b) const { return family + (size_t)b * S.stride; }
};

// the start vector into vector b of `family`, for every b
void spread_start(hipStream_t st, const BatchMem &M, double *family, const std::vector<double> &h) {
    // (on the stream: behind the memset that zeroed the vectors)
    HIPCHK(hipMemcpyAsync(family, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 1; b < M.S.B; ++b)
        HIPCHK(hipMemcpyAsync(M.vec(family, b), family, h.size() * sizeof(double),
                              hipMemcpyDeviceToDevice, st));
}

}  // namespace

std::vector<Spectrum> jacobi_spectrum_batch(System &S, int pattern, const std::vector<const double *> &vals,
                                            const std::vector<const double *> &dinv, const uint8_t *rowmask,
                                            int max_steps, SpectrumCounters *cnt) {
    const int B = (int)vals.size();
    std::vector<Spectrum> out(B, Spectrum{0.0, 0.0, 0});
    if (B == 0) return out;
    const Pattern &P = S.patterns[pattern];
    const int64_t n = P.nrows;
    hipStream_t st = S.stream;
    DevPool tmp;   // released on every way out
    BatchMem M(tmp, st, B, n, 4, max_steps);
    const SpecBatch &Sb = M.S;
    int64_t launches = 0, syncs = 0;
    spread_start(st, M, Sb.r, start_vector(n, LANCZOS_SEED, rowmask, false));
    syncs += rowmask ? 2 : 1;   // the mask's copy, the blocking upload
    // w = A p (boundary rows 0) and z = D^-1 r: jacobi_spectrum's RowOps, one per matrix and launch
    std::vector<RowOp> opsA(B), opsZ(B);
    for (int b = 0; b < B; ++b) {
        opsA[b] = lin_op(P, n, rowmask, LinStep{{RowTerm{vals[b], M.vec(Sb.p, b)}}, M.vec(Sb.w, b)});
        opsZ[b] = cheb_op(P, n, rowmask, ChebStep{nullptr, dinv[b], M.vec(Sb.r, b), nullptr, nullptr,
                                                  M.vec(Sb.z, b), 0.0, 0.0, 1.0});
    }
    spec::LockStep L(B);
    OpList A = live_ops(tmp, opsA, L.active), Z = live_ops(tmp, opsZ, L.active);
    const Bases bases{{nullptr, nullptr, nullptr, nullptr}};
    auto run = [&](const OpList &o, int w) {
        launch_rowops(st, o.d, o.n, P.nslices, P.R, bases, 1, w);
        ++launches;
    };
    auto dot = [&](const double *x, const double *y, int mode) {
        launch_spec_dot(st, Sb, x, y, mode);
        launches += 2;
    };
    auto update = [&](int kind) {
        launch_spec_update(st, Sb, kind);
        ++launches;
    };
    std::vector<int32_t> h_ints(3 * (size_t)B);
    std::vector<double> h_alpha, h_beta;
    // steps [absorbed, k) of the device's coefficients, the counts and the words: one round trip
    auto absorb = [&](int k) {
        const int s0 = L.absorbed;
        const size_t rows = k > s0 ? (size_t)(k - s0) : 0;
        h_alpha.resize(rows * B + 1);
        h_beta.resize(rows * B + 1);
        if (rows) {
            HIPCHK(hipMemcpyAsync(h_alpha.data(), Sb.alpha + (size_t)s0 * B, rows * B * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_beta.data(), Sb.beta + (size_t)s0 * B, rows * B * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipMemcpyAsync(h_ints.data(), M.ints, h_ints.size() * sizeof(int32_t),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++syncs;
        L.absorb(k, h_alpha.data(), h_beta.data(), h_ints.data(), h_ints.data() + B,
                 reinterpret_cast<const uint32_t *>(h_ints.data() + 2 * (size_t)B));
    };
    run(Z, 0);                                // z = D^-1 r
    update(SPEC_UPD_COPY);                    // p = z
    dot(Sb.r, Sb.z, SPEC_DOT_START);          // rz
    int k = 0;
    for (; k < max_steps; ++k) {
        if (spec::ritz_due(k)) {
            const std::vector<uint32_t> before = L.active;
            absorb(k);
            if (L.check(k))
                HIPCHK(hipMemcpyAsync(Sb.active, L.active.data(), (size_t)B * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, st));
            if (!L.any_active()) break;
            if (L.active != before) {
                A = live_ops(tmp, opsA, L.active);
                Z = live_ops(tmp, opsZ, L.active);
            }
        }
        run(A, P.uniform_w);                  // w = A p
        dot(Sb.p, Sb.w, SPEC_DOT_PAP);        // alpha, or stop
        update(SPEC_UPD_R);                   // r -= a w
        run(Z, 0);                            // z = D^-1 r
        dot(Sb.r, Sb.z, SPEC_DOT_RZ);         // beta, or stop
        update(SPEC_UPD_P);                   // p = z + b p
    }
    if (L.absorbed < k) absorb(k);
    for (int b = 0; b < B; ++b) out[b] = L.result(b);
    if (cnt) {
        cnt->launches += launches;
        cnt->syncs += syncs;
        cnt->lanczos_syncs_max = std::max(cnt->lanczos_syncs_max, syncs);
        cnt->bytes = std::max<int64_t>(cnt->bytes, (int64_t)M.bytes);
    }
    return out;
}

std::vector<double> jacobi_skew_radius_batch(System &S, int pattern,
                                             const std::vector<const double *> &skew_vals,
                                             const std::vector<const double *> &dinv,
                                             const uint8_t *rowmask, int max_steps,
                                             std::vector<int> *steps_out, SpectrumCounters *cnt) {
    const int B = (int)skew_vals.size();
    std::vector<double> out(B, 0.0);
    if (steps_out) steps_out->assign(B, 0);
    if (B == 0) return out;
    const Pattern &P = S.patterns[pattern];
    const int64_t n = P.nrows;
    hipStream_t st = S.stream;
    DevPool tmp;   // released on every way out
    BatchMem M(tmp, st, B, n, 2, 1);
    const SpecBatch &Sb = M.S;      // v = r, z = z
    int64_t launches = 0, syncs = 0;
    spread_start(st, M, Sb.r, start_vector(n, POWER_SEED, rowmask, false));
    syncs += rowmask ? 2 : 1;
    const std::vector<double> last(B, -1.0);
    HIPCHK(hipMemcpyAsync(Sb.last, last.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    // y = -D^-1 (0 - S x): the Chebyshev epilogue with c3 = -1 and no right-hand side
    std::vector<RowOp> ops1(B), ops2(B);
    for (int b = 0; b < B; ++b) {
        auto op = [&](const double *x, double *y) {
            return cheb_op(P, n, rowmask, ChebStep{skew_vals[b], dinv[b], nullptr, nullptr, nullptr, y,
                                                   0.0, 0.0, -1.0, 1.0, 1.0, x});
        };
        ops1[b] = op(M.vec(Sb.r, b), M.vec(Sb.z, b));
        ops2[b] = op(M.vec(Sb.z, b), M.vec(Sb.r, b));
    }
    std::vector<uint32_t> active(B, 1u);
    OpList O1 = live_ops(tmp, ops1, active), O2 = live_ops(tmp, ops2, active);
    const Bases bases{{nullptr, nullptr, nullptr, nullptr}};
    std::vector<int32_t> h_ints(3 * (size_t)B);
    auto read_back = [&]() {
        HIPCHK(hipMemcpyAsync(h_ints.data(), M.ints, h_ints.size() * sizeof(int32_t),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++syncs;
        for (int b = 0; b < B; ++b) active[b] = (uint32_t)h_ints[2 * (size_t)B + b];
    };
    launch_spec_dot(st, Sb, Sb.r, Sb.r, SPEC_DOT_NORM0);
    launches += 2;
    for (int k = 0; k < max_steps; ++k) {
        // the rule itself runs on the device every step; the host looks every 10 steps whether
        // anything is left to launch for
        if (k > 0 && k % 10 == 0) {
            const std::vector<uint32_t> before = active;
            read_back();
            bool any = false;
            for (uint32_t a : active) any = any || a;
            if (!any) break;
            if (active != before) {
                O1 = live_ops(tmp, ops1, active);
                O2 = live_ops(tmp, ops2, active);
            }
        }
        launch_spec_update(st, Sb, SPEC_UPD_SCALE);                                     // v /= ||v||
        launch_rowops(st, O1.d, O1.n, P.nslices, P.R, bases, 1, P.uniform_w);           // z = D^-1 S v
        launch_rowops(st, O2.d, O2.n, P.nslices, P.R, bases, 1, P.uniform_w);           // v = D^-1 S z
        launch_spec_dot(st, Sb, Sb.r, Sb.r, SPEC_DOT_NORM, k);
        launches += 5;
    }
    std::vector<double> mu2(B);
    HIPCHK(hipMemcpyAsync(mu2.data(), Sb.mu2, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    read_back();
    for (int b = 0; b < B; ++b) {
        if (steps_out) (*steps_out)[b] = h_ints[b];
        out[b] = (mu2[b] > 0.0 && std::isfinite(mu2[b])) ? std::sqrt(mu2[b]) : 0.0;
    }
    if (cnt) {
        cnt->launches += launches;
        cnt->syncs += syncs;
        cnt->bytes = std::max<int64_t>(cnt->bytes, (int64_t)M.bytes);
    }
    return out;
}

}  // namespace kkt
