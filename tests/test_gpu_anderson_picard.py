"""The device Picard loops with ``anderson=`` (the device mixer between ``solve`` and ``update`` of
``relinearise.device_picard_loop``) against the plain device loops and the host loops with the
NumPy mirror.

For every case: the accelerated loop converges in no more Picard iterations than the plain one of
the same test, ``non_linear_info["anderson"]`` is consistent with the depth, the Dirichlet values
are those of the plain loop bit for bit and ``zeta`` is zero there, and the fields lie within ten
times the distance between the PLAIN device loop's fields at non-linear rtol 1e-9 and at 1e-11 on
that case -- how far an iterate converged to 1e-9 still moves.  That distance is measured per case
and printed next to the accelerated loop's; measured values are in the table of
``profiles/anderson_picard.md``."""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import fem, picard
from control_amd.control import GpuBackend, Instationary, Stationary

pytestmark = pytest.mark.gpu

KAT_SP = reaction_ref.KAT_SP
COEFFICIENTS = (2.0, 0.0, 0.5)


# Desired states large enough for the reaction to matter: the plain loops then need more Picard
# iterations than the ring is deep, so every case fills the ring and its iterates at rtol 1e-9 and
# 1e-11 differ.  (With the amplitude-1, beta = 1 data of the stationary known-answer test the
# plain loop ends after 2 iterations, on the 8 interior nodes of box_p1(3, 3, 3) at amplitude 8
# after 5, in both below 1e-11 already: nothing to accelerate and no distance to measure.)
def _desired(X, t, amplitude=8.0):
    return amplitude * (1.0 + t) * np.prod(np.sin(np.pi * X), axis=1) * np.exp(X[:, 0])


def _instationary(disc, CN, n_t, amplitude=8.0, **kw):
    return Instationary(disc, fem.ReactionTerm(disc, COEFFICIENTS),
                        desired_state=lambda X, t: _desired(X, t, amplitude), CN=CN,
                        n_t=n_t, time_interval=(0.0, 1.0), beta=1.0e-2, **kw)


def _stationary(**kw):
    disc = fem.unit_square_p1(8)

    def v_d(X):
        return 8.0 * np.prod(np.sin(np.pi * X), axis=1) * np.exp(X[:, 0] + X[:, 1])
    return Stationary(disc, fem.ReactionTerm(disc, COEFFICIENTS), desired_state=v_d, beta=1.0e-2,
                      **kw)


# name -> (problem, lambda_v_bounds, Schur Chebyshev triple): the settings of the plain loops'
# tests on these elements (tests/test_gpu_reaction*_picard.py)
SCALAR = {
    "p1-be": (lambda **kw: _instationary(fem.unit_square_p1(6), False, 4, **kw), (0.5, 2.0),
              (40, 0.02, 2.2)),
    "p1-cn": (lambda **kw: _instationary(fem.unit_square_p1(6), True, 4, **kw), (0.5, 2.0),
              (40, 0.02, 2.2)),
    "p2-cn": (lambda **kw: _instationary(fem.unit_square_p2(6), True, 4, **kw), (0.3924, 2.0598),
              (15, 0.043, 2.24)),
    "q2-be": (lambda **kw: _instationary(fem.rectangle_q2(4, 4), False, 4, **kw), (0.25, 1.5625),
              (8, 0.12, 1.54)),
    "box-be": (lambda **kw: _instationary(fem.box_p1(3, 3, 3), False, 3, 40.0, **kw), (0.5, 2.5),
               (40, 0.02, 2.2)),
    "stationary": (_stationary, (0.5, 2.0), (40, 0.02, 2.2)),
}
LIFTED = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0]),
              initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]))


def _scalar_loop(case, rtol=1.0e-9, device=True, problem_kw=None, **kw):
    make, mass, schur = SCALAR[case]
    ctl = make(**(problem_kw or {}))
    its, solve = [], ctl.linear_solve

    def recording(**a):
        ksp = solve(**a)
        its.append(ksp.getIterationNumber())
        return ksp
    if not device:
        ctl.linear_solve = recording
    norms = ctl.non_linear_solve(solver_parameters=KAT_SP, lambda_v_bounds=mass,
                                 relative_non_linear_tol=rtol, absolute_non_linear_tol=0.0,
                                 max_non_linear_iter=60, backend=GpuBackend(schur=schur),
                                 device=device, **kw)
    info = getattr(ctl, "non_linear_info", None) or {}
    return dict(norms=norms, fields=(ctl._v.copy(), ctl._zeta.copy()), info=info, ctl=ctl,
                its=list(info.get("linear_iterations", its)))


def _distance(a, b):
    return max(np.abs(x - y).max() for x, y in zip(a, b))


def _check(case, depth, plain, tighter, mixed, boundary):
    """The assertions every case shares; returns the bar."""
    bar = 10.0 * _distance(plain["fields"], tighter["fields"])
    dist = _distance(mixed["fields"], plain["fields"])
    n_plain, n_mixed = len(plain["norms"]) - 1, len(mixed["norms"]) - 1
    print(f"{case}: Picard iterations plain {n_plain}, anderson={depth} {n_mixed}; plain fields "
          f"at 1e-9 and 1e-11 lie {bar / 10.0:.2e} apart (bar {bar:.2e}); accelerated to plain "
          f"{dist:.2e}; mixer {mixed['info']['anderson']}")
    assert plain["norms"][-1] <= 1.0e-9 * plain["norms"][0]
    assert mixed["norms"][-1] <= 1.0e-9 * mixed["norms"][0]          # it converges
    assert n_mixed <= n_plain
    hist = mixed["info"]["anderson"]
    assert len(hist) == n_mixed and hist[0] == (0, 0)
    assert all(0 <= c <= depth and d >= 0 for c, d in hist)
    assert dist <= bar
    for got, want in zip(mixed["fields"][:2], plain["fields"][:2]):
        assert got.shape == want.shape
    v, zeta = mixed["fields"][:2]
    assert np.array_equal(v[..., boundary], plain["fields"][0][..., boundary])
    assert np.all(zeta[..., boundary] == 0.0)
    return bar


@pytest.mark.parametrize("case", list(SCALAR))
def test_scalar_loops(case):
    plain, tighter = _scalar_loop(case), _scalar_loop(case, rtol=1.0e-11)
    mixed = _scalar_loop(case, anderson=3)
    nodes = plain["ctl"]._disc.boundary
    bar = _check(case, 3, plain, tighter, mixed, nodes)
    hist = mixed["info"]["anderson"]
    assert [c for c, _ in hist[:4]] == [0, 1, 2, 3][:len(hist)] or any(d for _, d in hist)
    # the device loop against the host loop with the mirror, through the same backend
    host = _scalar_loop(case, device=False, anderson=3)
    print(f"{case}: host loop {len(host['norms']) - 1} iterations, fields to the device loop's "
          f"{_distance(host['fields'], mixed['fields']):.2e}")
    assert len(host["norms"]) == len(mixed["norms"])
    assert _distance(host["fields"], mixed["fields"]) <= bar
    assert host["info"]["anderson"] == hist


def test_boundary_lift_resets_the_mixer():
    """Inhomogeneous boundary data and an initial condition the starting iterate does not carry:
    ``after_first_update`` puts them in, outside any step, so the second call has no pair."""
    kw = dict(problem_kw=LIFTED)
    plain, tighter = _scalar_loop("p1-be", **kw), _scalar_loop("p1-be", rtol=1.0e-11, **kw)
    mixed = _scalar_loop("p1-be", anderson=3, **kw)
    ctl = plain["ctl"]
    nodes = ctl._disc.boundary
    bar = _check("p1-be lifted", 3, plain, tighter, mixed, nodes)
    hist = mixed["info"]["anderson"]
    assert hist[1] == (0, 0) and hist[2][0] == 1              # the reset happened
    for i in range(ctl._n_t):
        assert np.array_equal(mixed["fields"][0][i, nodes], ctl._bc_values(i)[nodes])
    host = _scalar_loop("p1-be", device=False, anderson=3, **kw)
    assert host["info"]["anderson"] == hist
    assert _distance(host["fields"], mixed["fields"]) <= bar


def test_anderson_zero_is_the_call_without_the_keyword():
    for case in ("p2-cn", "stationary"):
        a, b = _scalar_loop(case), _scalar_loop(case, anderson=0, anderson_beta=0.5)
        assert a["norms"] == b["norms"] and a["its"] == b["its"]
        for x, y in zip(a["fields"], b["fields"]):
            assert np.array_equal(x.view(np.int64), y.view(np.int64))
        assert "anderson" not in b["info"]


# ------------------------------------------------------------------ incompressible
def _cavity_loop(rtol=1.0e-9, **kw):
    from test_gpu_device_picard import _solver
    pb, v_init, _ = common.navier_stokes_cavity_problem(n=4, n_t=4, CN=False)
    out = picard.incompressible_non_linear_solve(
        pb, _solver(pb, "device"), v=v_init, device=True, print_error_non_linear=False,
        max_non_linear_iter=60, relative_non_linear_tol=rtol, absolute_non_linear_tol=0.0, **kw)
    return dict(norms=out["norms"], fields=(out["v"], out["zeta"], out["p"], out["mu"]),
                info=out, boundary=pb.disc.boundary_v)


def test_instationary_cavity_loop():
    plain, tighter, mixed = _cavity_loop(), _cavity_loop(1.0e-11), _cavity_loop(anderson=2)
    _check("cavity", 2, plain, tighter, mixed, plain["boundary"])


def _stationary_ns_loop(rtol=1.0e-9, **kw):
    from test_gpu_stationary_ns_picard import BOUNDS, MMS_STOKES_SP, SCHUR, _problem
    ctl = _problem(4, 1.0, False)
    norms = ctl.incompressible_non_linear_solve(
        solver_parameters=MMS_STOKES_SP, **BOUNDS, max_non_linear_iter=60,
        relative_non_linear_tol=rtol, absolute_non_linear_tol=0.0,
        backend=GpuBackend(schur=SCHUR), device=True, **kw)
    return dict(norms=norms, fields=(ctl._v.copy(), ctl._zeta.copy(), ctl._p.copy(),
                                     ctl._mu.copy()), info=ctl.non_linear_info,
                boundary=ctl._disc.boundary)


def test_stationary_navier_stokes_loop():
    plain, tighter = _stationary_ns_loop(), _stationary_ns_loop(1.0e-11)
    mixed = _stationary_ns_loop(anderson=2)
    _check("stationary Navier-Stokes", 2, plain, tighter, mixed, plain["boundary"])
