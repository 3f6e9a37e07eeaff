"""The two host references of the Stokes preconditioner's pressure stage
(``tests/stokes_stage_ref.py``) against each other and against the oracle they restate; no GPU.

``D_CASE`` records the distance of the float64 oracle stage from the extended-precision stage
per case and input kind -- the yardstick of ``tests/test_gpu_stokes_pressure_stage.py``, which
recomputes it for the ``u_0`` the GPU returns.  Largest value over all cases here: 1.2e-15
(Crank-Nicolson, short ``K_p`` chains); the Jacobi cases are at 2e-16.
"""
import numpy as np
import pytest

import common
import stokes_stage_ref as ref

D_CASE = {}


def test_longdouble_is_wider_than_double():
    assert np.finfo(ref.XP).eps < 1e-3 * ref.EPS


@pytest.mark.parametrize("CN", [False, True])
def test_float64_stage_is_the_oracles_bit_for_bit(CN):
    """With the problem's own scalings and the oracle's own nested ``u_0`` the float64 stage
    reproduces ``pc_instationary_incompressible`` exactly, plain and two-grid ``K_p``."""
    p = common.stokes_problem(n=4, n_t=4, CN=CN)
    th, m, tau = p["th"], p["m"], p["tau"]
    rng = np.random.default_rng(common.SEED)
    b0 = rng.standard_normal((2 * m, th.n_v))
    b0[:, th.boundary_v] = 0.0
    b1 = rng.standard_normal((2 * m, th.n_p))
    from control_amd.coarse import multilinear_coarse_space
    Pp = multilinear_coarse_space(th.coords_p, (), cells=2)
    for specs, kpc in ((common.STOKES_SPECS, None),
                       (dict(common.STOKES_SPECS, kp=(3, 0.15, 2.1)), (Pp, 2))):
        _, opc = common.stokes_oracle(p, specs, kp_coarse=kpc)
        u0, u1 = np.zeros_like(b0), np.zeros_like(b1)
        opc(u0, u1, b0, b1)
        assert np.abs(u0).max() > 0 and np.abs(u1).max() > 0
        v0, v1 = np.zeros_like(b0), np.zeros_like(b1)
        ref.oracle_stage_pc_fn(p, specs, u0, b_scale=tau, post_scale=1.0 / tau**2,
                               kp_coarse=kpc)(v0, v1, b0, b1)
        assert np.array_equal(v0, u0) and np.array_equal(v1, u1)


def test_extended_inverse_and_coefficients():
    rng = np.random.default_rng(common.SEED)
    A = rng.standard_normal((9, 9)) + 9.0 * np.eye(9)
    Ai = ref.xp_inverse(A)
    assert Ai.dtype == ref.XP
    assert np.abs(Ai @ A.astype(ref.XP) - np.eye(9)).max() < 1e-17
    from oracle import kkt_oracle as ko
    # the float64 coefficients of the oracle's recurrence are the rounded extended ones
    scale, coefs = ref.xp_cheb_coefficients(0.02, 2.2, 30)
    alpha = 1.0 - (2.0 / 2.22) * 0.02
    c_km1, c_k = 1.0, 1.0 / alpha
    for c1, c2, c3 in coefs:
        c_kp1 = 2.0 / alpha * c_k - c_km1
        omega = 2.0 / alpha * c_k / c_kp1
        assert abs(float(c2) - omega) < 64 * ref.EPS * omega
        assert abs(float(c3) - float(scale) * omega) < 64 * ref.EPS * omega
        c_km1, c_k = c_k, c_kp1
    # ... and one solve against chebyshev_jacobi / chebyshev_jacobi_from
    p = common.stokes_problem(n=3, n_t=2)
    K = p["th"].K_p.tocsr()
    dinv = 1.0 / K.diagonal()
    b = rng.standard_normal(K.shape[0])
    Kx, dx, bx = K.toarray().astype(ref.XP), dinv.astype(ref.XP), b.astype(ref.XP)
    for its in (1, 2, 7):
        got = ref.xp_chebyshev_from(Kx, dx, bx, None, 0.02, 2.2, its)
        assert common.rel_err(ko.chebyshev_jacobi(K, dinv, b, 0.02, 2.2, its), got) < 1e-14
        got = ref.xp_chebyshev_from(Kx, dx, bx, bx, 0.02, 2.2, its)
        assert common.rel_err(ko.chebyshev_jacobi_from(K, dinv, b, b, 0.02, 2.2, its), got) < 1e-14


@pytest.mark.parametrize("c", ref.CASES, ids=ref.case_id)
def test_extended_and_float64_stages_agree(c):
    """Every case of the GPU test, both input kinds, for one and the same ``u_0`` (here: 0 for
    the zero velocity right-hand side, a random interior velocity for the other kind)."""
    p = ref.problem(c)
    th, m = p["th"], p["m"]
    rng = np.random.default_rng(common.SEED + 5)
    u0_rand = rng.standard_normal((2 * m, th.n_v))
    u0_rand[:, th.boundary_v] = 0.0
    x1, x2 = ref.inputs(c)
    for kind, x, u0 in (("zero_b0", x1, np.zeros((2 * m, th.n_v))), ("random", x2, u0_rand)):
        px, po, d = ref.references(c, x, u0)
        D_CASE[(ref.case_id(c), kind)] = d
        print(f"d_case {ref.case_id(c)} {kind}: {d:.2e}")
        assert np.isfinite(d) and np.abs(np.asarray(px, dtype=np.float64)).max() > 0
        # float64 recurrences of its_total steps on matrices with at most 19 entries per row and
        # Jacobi-scaled spectra inside [0, 2.25]: every step adds a rounding error of a few eps
        # of the iterate; the polynomials are bounded by 1 on the interval and by its_total^2
        # at 0 (the constants of K_p, which the zero-mean input does not excite beyond round-off)
        assert d < 64 * ref.EPS * ref.its_total(c) ** 2 + 16 * ref.EPS
        # the constant of every pressure block is the post-correction's: the mean of b_1
        b1 = ref.split(p, x)[1]
        assert np.allclose(np.asarray(px.mean(axis=1), dtype=np.float64), b1.mean(axis=1),
                           rtol=0, atol=1e-12 * np.abs(np.asarray(px, dtype=np.float64)).max())
