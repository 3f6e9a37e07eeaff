"""The Chebyshev intervals the library estimates for its sub-solves (``ChebSpec(-1, 0, 0)``, the
drivers' defaults, the automatic K_p sweeps, the two-grid form's ``emax / 30``) against dense
eigensolves of the same matrices.

Every sub-solve the built-in preconditioner emits is read back (``pc_solves``, ``pc_matrices``)
and compared with ``A = assemble_with_bcs(blk + c M)`` on the interior dofs, D = diag(A),
H~ = D^-1/2 (A + A^T)/2 D^-1/2, S~ = D^-1/2 (A - A^T)/2 D^-1/2 (tests/spectrum_ref.py; the
(sweep, level) -> (block, shift) map is checked against the oracle in test_spectrum_map.py):

* Ritz values lie inside the spectrum, the widening is 0.85 / 1.05: emax <= 1.05 lmax(H~) and,
  without coarse cycles, emin >= 0.85 lmin(H~) -- a wrong recurrence, Ritz formula, Jacobi
  scaling or mask breaks these;
* the widened interval brackets the spectrum: emax >= lmax(H~), emin <= lmin(H~) (two-grid:
  emax / 30 <= emin <= max(lmin(H~), emax / 30));
* convection blocks: max |Im lambda(D^-1 A)| <= eimag <= 1.2 rho(S~), and the Bendixson box
  [emin, emax] x [-eimag, eimag] holds every eigenvalue of D^-1 A; symmetric blocks: eimag == 0;
* the degree follows 1.6 (CN: 2.6) sqrt(emax / emin) of the middle level, in [4, 600]; 8 sweeps
  per cycle in the two-grid form;
* one estimate per distinct value set, none (and no coarse inverse) for matrices only multiplied
  with;
* K_p (pure Neumann): the two-grid form's zero-mean Lanczos interval brackets the non-zero
  spectrum, the plain form's upper end the largest eigenvalue.

Only rounding is allowed for: relative slack 1e-8.
"""
import collections
import math

import numpy as np
import pytest

import common
import spectrum_ref
from control_amd import picard
from control_amd.blocks import instationary_blocks, stationary_blocks
from control_amd.coarse import multilinear_coarse_space
from control_amd.fem import unit_square_p1
from control_amd.multiblock import ChebSpec, MultiBlockSystem, SchurPC

pytestmark = pytest.mark.gpu

AUTO = (-1, 0.0, 0.0)
MASS = (20, 0.5, 2.0)
SLACK = 1e-8
EPSILON = 1.0e-3


def _sweep_kind(p):
    return "CN" if p["CN"] else "BE"


def check_records(name, kind, blocks, n, tau, beta, M, nodes, g, coarse=False):
    """Every sub-solve record of the handle ``g`` against the dense reference (the per-case
    ratios are printed); returns ``(pc_solves(), pc_matrices())``."""
    solves, mats = g.pc_solves(), g.pc_matrices()
    expect = spectrum_ref.schur_solve_map(kind, blocks, n, tau, beta, EPSILON)
    assert len(solves) == len(expect), (len(solves), len(expect))
    cache, keys = {}, []
    ratios = collections.defaultdict(list)
    outside_ellipse = 0
    for rec, (sweep, level, blk, c) in zip(solves, expect):
        where = (name, sweep, level)
        assert (rec["sweep"], rec["level"]) == (sweep, level), where
        assert rec["c"] == pytest.approx(c, rel=1e-14, abs=0.0), where
        assert rec["estimate"] in ("lanczos", "shared"), where
        assert mats[rec["matrix"]]["estimate"] == rec["estimate"]
        assert mats[rec["matrix"]]["c"] == rec["c"]
        A = spectrum_ref.assembled(blk, c, M, nodes)
        key = spectrum_ref.value_key(A, c)
        keys.append(key)
        if key not in cache:
            cache[key] = spectrum_ref.jacobi_spectra(A, nodes)
        r = cache[key]
        emin, emax, eimag = rec["emin"], rec["emax"], rec["eimag"]
        lmin, lmax = r["lmin"], r["lmax"]
        ratios["emin/lmin"].append(emin / lmin)
        ratios["emax/lmax"].append(emax / lmax)
        # exact-arithmetic facts (Ritz values inside the spectrum) and the bracket
        assert emax <= 1.05 * lmax * (1 + SLACK), (where, emax, lmax)
        assert emax >= lmax * (1 - SLACK), (where, emax, lmax)
        if coarse:
            assert emin >= emax / 30.0 * (1 - SLACK), (where, emin, emax)
            assert emin <= max(lmin, emax / 30.0) * (1 + SLACK), (where, emin, lmin, emax)
        else:
            assert emin >= 0.85 * lmin * (1 - SLACK), (where, emin, lmin)
            assert emin <= lmin * (1 + SLACK), (where, emin, lmin)
        tiny = 1e-12 * lmax
        if r["symmetric"]:
            assert eimag == 0.0, (where, eimag)
        elif r["rho_skew"] <= tiny:
            # symmetric up to the rounding of the assembly (3-D P1): the skew part is noise of
            # the last bit, and so is the semi-axis estimated from it
            assert eimag <= tiny, (where, eimag, r["rho_skew"])
        else:
            ev = r["ev"]
            im = float(np.max(np.abs(ev.imag)))
            ratios["eimag/max|Im|"].append(eimag / im if im > 0 else math.inf)
            assert eimag >= im * (1 - SLACK), (where, eimag, im)
            assert eimag <= 1.2 * r["rho_skew"] * (1 + SLACK), (where, eimag, r["rho_skew"])
            if not coarse:
                assert np.all(ev.real >= emin * (1 - SLACK)) and np.all(ev.real <= emax * (1 + SLACK)), where
                assert np.all(np.abs(ev.imag) <= eimag * (1 + SLACK)), where
            d, a = 0.5 * (emax + emin), 0.5 * (emax - emin)
            outside_ellipse += int(np.sum(((ev.real - d) / a) ** 2 + (ev.imag / eimag) ** 2 > 1.0))
    # degree: of the middle level's matrix (the first sub-solve of the stationary form)
    imid = n // 2
    mid = next(rec for rec in solves
               if rec["sweep"] in ("forward", "first") and rec["level"] == imid)
    if coarse:
        its = 8
    else:
        f = 2.6 if kind == "CN" else 1.6
        its = max(4, min(600, math.ceil(f * math.sqrt(mid["emax"] / mid["emin"]))))
    assert all(rec["its"] == its for rec in solves), (its, {rec["its"] for rec in solves})
    # one estimate per distinct value set; none for matrices that are only multiplied with
    distinct = set(keys)
    assert sum(m["estimate"] == "lanczos" for m in mats) == len(distinct)
    uses = collections.Counter(rec["matrix"] for rec in solves)
    for i, m in enumerate(mats):
        assert m["solves"] == uses.get(i, 0), (name, i, m)
        if m["solves"] == 0:
            assert m["estimate"] == "none" and not m["coarse"], (name, i, m)
            assert m["lanczos"] == 0 and m["power"] == 0, (name, i, m)
        else:
            assert m["estimate"] != "none" and m["coarse"] == coarse, (name, i, m)
            assert (m["lanczos"] > 0) == (m["estimate"] == "lanczos"), (name, i, m)
    for key, rec in zip(keys, solves):          # the skew part is estimated exactly when present
        m = mats[rec["matrix"]]
        r = cache[key]
        if m["estimate"] == "lanczos" and (r["symmetric"] or r["rho_skew"] > 1e-12 * r["lmax"]):
            assert (m["power"] > 0) == (not r["symmetric"]), (name, m)
    if coarse:
        assert g.coarse_setup_stats()["matrices"] == len(distinct)
    summary = {k: (min(v), max(v)) for k, v in ratios.items()}
    print(f"\n{name}: {len(solves)} sub-solves, {len(mats)} matrices, {len(distinct)} estimated, "
          f"degree {its}; " + ", ".join(f"{k} [{lo:.4f}, {hi:.4f}]" for k, (lo, hi) in summary.items())
          + (f"; eigenvalues outside the ellipse: {outside_ellipse}" if "eimag/max|Im|" in summary
             else ""))
    return solves, mats


def _heat(p, schur=AUTO, coarse=None):
    g = common.gpu_system(p)
    g.pc_apply(common.rng_vector(g.local_size), common.gpu_pc(p, MASS, schur, coarse=coarse))
    return g


def _check_heat(name, p, g, coarse=False):
    return check_records(name, _sweep_kind(p), p["blocks"], p["m"], p["tau"], p["beta"],
                         p["sd"].M, p["nodes"], g, coarse=coarse)


@pytest.mark.parametrize("space,n,n_t,CN", [("p1", 32, 8, False), ("p1", 32, 8, True),
                                             ("p1_3d", 12, 6, False), ("q2", 16, 6, False)])
def test_heat_estimates(space, n, n_t, CN):
    p = common.heat_problem(space=space, n=n, n_t=n_t, CN=CN, beta=1e-4)
    _check_heat(f"{space} {n} x {n_t} {'CN' if CN else 'BE'}", p, _heat(p))


def test_stationary_estimates():
    sd, beta = unit_square_p1(32), 1e-4
    blocks = stationary_blocks(sd.M, sd.K, beta)
    g = MultiBlockSystem(sd.n_dofs, sd.n_dofs, *blocks)
    pc = SchurPC(kind="stationary", M=sd.M, beta=beta, bc_nodes=sd.boundary,
                 mass=ChebSpec(*MASS), schur=ChebSpec(*AUTO))
    g.pc_apply(common.rng_vector(g.local_size), pc)
    check_records("stationary p1 32", "stationary", blocks, 1, 1.0, beta, sd.M, sd.boundary, g)


@pytest.mark.parametrize("CN", [False, True])
def test_time_dependent_operator_one_estimate_per_level(CN):
    p = common.heat_problem(n=24, n_t=6, CN=CN, beta=1e-4, time_dependent=True)
    solves, mats = _check_heat(f"time-dependent p1 24 {'CN' if CN else 'BE'}", p, _heat(p))
    # every level its own matrix
    assert sum(m["estimate"] == "lanczos" for m in mats) >= p["m"]


def test_shared_and_unshared_blocks_give_identical_intervals():
    """mode G (one stored copy per level) against shared blocks: equal values share one estimate,
    so every interval and degree is the same bit for bit."""
    out = {}
    for share in (True, False):
        p = common.heat_problem(n=16, n_t=6, beta=1e-4, share=share)
        solves, mats = _check_heat(f"share={share}", p, _heat(p))
        out[share] = [(r["sweep"], r["level"], r["c"], r["emin"], r["emax"], r["eimag"], r["its"])
                      for r in solves]
    assert out[True] == out[False]


@pytest.mark.parametrize("CN", [False, True])
def test_two_grid_p1(CN):
    p = common.heat_problem(n=32, n_t=8, CN=CN, beta=1e-4)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=8)
    g = _heat(p, coarse=(P, 1))
    _check_heat(f"two-grid p1 32 {'CN' if CN else 'BE'}", p, g, coarse=True)


@pytest.mark.parametrize("n,beta,multigrid", [(8, 1.0, False), (32, 1e-4, False), (32, 1e-4, True)])
def test_cn_product_only_matrices_are_not_estimated(n, beta, multigrid):
    """Crank-Nicolson forms c M~ and the upper blocks h K^T + (c - 1) M only for products (c < 1:
    indefinite, beta = 1 on 8 x 8): neither gets an interval nor a coarse inverse."""
    p = common.heat_problem(n=n, n_t=10 if n == 8 else 8, CN=True, beta=beta)
    coarse = None
    if multigrid:
        coarse = (multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=8), 1)
    g = _heat(p, coarse=coarse)
    solves, mats = _check_heat(f"CN p1 {n} beta {beta}{' two-grid' if multigrid else ''}", p, g,
                               coarse=multigrid)
    product_only = [m for m in mats if m["solves"] == 0]
    assert len(product_only) >= 2             # c M~ and the upper blocks
    assert all(m["estimate"] == "none" and not m["coarse"] for m in product_only)


def _mms_convection_problem(N, CN, n_t=10):
    """The operators of ``common.mms_convection_diffusion_control``: K + (wind(t_i) . grad) per
    level on ``rectangle_p1(N, N, 2, 2)``, beta = 1."""
    from control_amd.fem import rectangle_p1
    disc = rectangle_p1(N, N, 2.0, 2.0)
    beta, T = 1.0, 2.0
    tau = T / (n_t - 1.0)

    def wind(X, t):
        x, y = X[:, 0] - 1.0, X[:, 1] - 1.0
        return np.cos(0.5 * np.pi * t) * np.stack([2.0 * y * (1.0 - x * x), -2.0 * x * (1.0 - y * y)], 1)
    Ks = [(disc.K + disc.convection(lambda Xq, t=i * tau: wind(Xq, t))).tocsr() for i in range(n_t)]
    b00, b01, b10, b11, m = instationary_blocks(disc.M, Ks, tau, beta, n_t, CN, share=True)
    return dict(sd=disc, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=disc.boundary)


@pytest.mark.parametrize("CN", [False, True])
def test_convection_diffusion_mms(CN):
    p = _mms_convection_problem(16, CN)
    solves, mats = _check_heat(f"convection-diffusion MMS 16 {'CN' if CN else 'BE'}", p, _heat(p))
    assert any(r["eimag"] > 0.0 for r in solves)


def _neumann_checks(name, rec, K_p, inner_solves, coarse):
    lam2, lmax = spectrum_ref.neumann_spectrum(K_p)
    print(f"{name} K_p ({rec['estimate']}): kp_emin / lambda_2 {rec['kp_emin'] / lam2:.4f}, "
          f"kp_emax / lambda_max {rec['kp_emax'] / lmax:.4f}, {rec['kp_its']} sweeps")
    assert lmax * (1 - SLACK) <= rec["kp_emax"] <= 1.05 * lmax * (1 + SLACK)
    if coarse:
        assert rec["estimate"] == "zero_mean"
        assert 0.85 * lam2 * (1 - SLACK) <= rec["kp_emin"] <= lam2 * (1 + SLACK)
        its = max(4, min(600, math.ceil(5.0 * math.sqrt(rec["kp_emax"] / rec["kp_emin"]))))
        assert rec["kp_its"] == its
    else:
        assert rec["estimate"] == "upper"
        n = 1 + max(r["level"] for r in inner_solves)
        mid = next(r for r in inner_solves if r["sweep"] == "forward" and r["level"] == n // 2)
        assert rec["kp_emin"] == mid["emin"] and rec["kp_its"] == mid["its"]


def test_stokes_velocity_and_kp():
    specs = dict(mass=(20, 0.3924, 2.0598), schur=AUTO, kp=AUTO, mp=(20, 0.5, 2.0))
    p = common.stokes_problem(n=8, n_t=6, beta=1.0e-2)
    th = p["th"]
    outer, gpc = common.stokes_gpu(p, specs)
    outer.pc_apply(common.rng_vector(outer.local_size), gpc)
    inner = gpc.inner
    solves, _ = check_records("Stokes P2 8 x 6 BE velocity", "BE", p["blocks"]["inner"], p["m"],
                              p["tau"], p["beta"], th.M_v, th.boundary_v, inner)
    kp = outer.pc_solves()
    assert len(kp) == 1 and kp[0]["sweep"] == "kp"
    _neumann_checks("Stokes P2 8", kp[0], th.K_p, solves, coarse=False)


@pytest.mark.parametrize("CN,multigrid", [(False, False), (True, False), (False, True)])
def test_navier_stokes_cavity(CN, multigrid):
    """Linearised about a non-zero velocity: every level its own convection block."""
    pb, v_init, _ = common.navier_stokes_cavity_problem(n=8, n_t=10, CN=CN)
    th = pb.disc
    v = v_init + 0.5 * pb.v_d
    D = [pb.D_v(v[i]) for i in range(pb.n_t)]
    Dp = [pb.D_p(v[i]) for i in range(pb.n_t)]
    gls = picard.GpuLinearSolver(pb, Multigrid=multigrid, kp=AUTO)
    bl = gls._blocks(D, Dp)
    gls._build(bl)
    gls.outer.pc_apply(common.rng_vector(gls.outer.local_size), gls.pc)
    name = f"cavity 8 {'CN' if CN else 'BE'}{' two-grid' if multigrid else ''}"
    solves, _ = check_records(name, "CN" if CN else "BE", bl["inner"], bl["m"], pb.tau, pb.beta,
                              th.M_v, th.boundary_v, gls.inner, coarse=multigrid)
    assert any(r["eimag"] > 0.0 for r in solves)
    kp = gls.outer.pc_solves()
    assert len(kp) == 1
    _neumann_checks(name, kp[0], th.K_p, solves, coarse=multigrid)
