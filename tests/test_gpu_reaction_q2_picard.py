"""The scalar Picard / Gauss-Newton loop on the device on Q2 quadrilaterals (``fem.rectangle_q2``)
against the host path with the same ``fem.ReactionTerm``: the device-built system and whole loops,
``Instationary`` and ``Stationary``, by the scheme and with the bars of
``tests/test_gpu_reaction_p2_picard.py`` -- equal non-linear iteration counts, norms within 1e-8
relative, iterates within 1e-9, equal linear iteration counts.

The instationary problem is the reference's non-linear reaction problem ``grad-grad + (2 + 0.5
v_old^2) mass`` on ``rectangle_q2(4, 4)``, ``n_t = 4``, ``beta = 1e-2``, with a smooth desired
state of amplitude 8: large enough for the reaction to matter.  The stationary one is the
reference's own (``test/test_control.py:710-1024`` at degree 2): ``rectangle_q2(6, 6)``, ``beta =
1``, desired state ``sin(pi x) sin(pi y) exp(x + y)``.

Sub-solve settings, the same on both paths.  The mass solves run on the reference's interval for
Q2, ``(0.25, 1.5625)`` (``test/test_control.py:93``).  The Chebyshev triples are
``control.suggest_chebyshev``'s on these meshes at the zero iterate, computed on the host: ``tau D
+ M`` with the shift ``tau / sqrt(beta)`` on ``rectangle_q2(4, 4)`` gives (8, 0.1238, 1.530) for
``tau = 1/3``, (8, 0.1205, 1.532) for ``tau = 1/2`` (the two-grid case's ``n_t = 3``) and
(7, 0.1334, 1.523) for Crank-Nicolson's ``tau / 2 = 1/6``; ``D`` with the shift ``1 / sqrt(beta)
= 1`` on ``rectangle_q2(6, 6)`` (14, 0.0373, 1.597); the intervals below contain them.
"""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import fem
from control_amd.control import GpuBackend, Instationary, Stationary
from test_gpu_reaction_picard import _device_system, _host_system, _iterate, _same_blocks

pytestmark = pytest.mark.gpu

SCHUR = (8, 0.12, 1.54)
SCHUR_STATIONARY = (14, 0.037, 1.6)
MASS = (0.25, 1.5625)
KAT_SP = reaction_ref.KAT_SP
LIFTED = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0]),
              initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]))


def reaction_heat_control_q2(CN, n=4, n_t=4, **kw):
    """``reaction_ref.reaction_heat_control`` on Q2 quadrilaterals, with the amplitude-8 desired state."""
    disc = fem.rectangle_q2(n, n)

    def v_d(X, t):
        return 8.0 * (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.exp(X[:, 0])
    return Instationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d, CN=CN,
                        n_t=n_t, time_interval=(0.0, 1.0), beta=1.0e-2, **kw)


def reference_stationary_problem(newton=False):
    disc = fem.rectangle_q2(6, 6)

    def v_d(X):
        return np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.exp(X[:, 0] + X[:, 1])
    ctl = Stationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d, beta=1.0)
    if newton:
        ctl.set_Gauss_Newton()
    return ctl


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("newton", [False, True])
def test_device_built_system_equals_the_host_built_one(CN, newton):
    ctl = reaction_heat_control_q2(CN, **LIFTED)
    ctl.set_Gauss_Newton(newton)
    assert ctl._forward.cells.shape[1] == 9
    backend = GpuBackend(schur=SCHUR)
    rng = np.random.default_rng(common.SEED + 1)
    state = _iterate(ctl, rng)
    system, dev, _, full = _device_system(ctl, backend, state)
    host, _, D = _host_system(ctl, backend, state[0])
    term = ctl._forward
    want = term.jacobian(state[0][1], 0.0) if newton else term(state[0][1], 0.0)
    assert np.array_equal(D[1].data, want.data)              # D = term(v), as the host builds it
    x = rng.standard_normal(host.local_size)
    assert common.rel_err(system.mult(x), host.mult(x)) <= 1e-13
    _same_blocks(host, system, full)
    # a second re-linearisation at another iterate: the same again (nothing cached stale)
    state = _iterate(ctl, rng, 0.3)
    dev.set_state(*state)
    dev.assemble()
    dev.relinearise()
    host, _, _ = _host_system(ctl, backend, state[0])
    assert common.rel_err(system.mult(x), host.mult(x)) <= 1e-13
    _same_blocks(host, system, full)


def _loop(ctl, device, schur=SCHUR, Multigrid=False, **kw):
    """One loop; the host path's linear iteration counts are read off ``linear_solve``."""
    its, solve = [], ctl.linear_solve

    def recording(**a):
        ksp = solve(**a)
        its.append(ksp.getIterationNumber())
        return ksp
    if not device:
        ctl.linear_solve = recording
    norms = ctl.non_linear_solve(solver_parameters=KAT_SP, lambda_v_bounds=MASS,
                                 relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                 backend=GpuBackend(schur=schur), Multigrid=Multigrid,
                                 device=device, **kw)
    if device:
        its = ctl.non_linear_info["linear_iterations"]
    return norms, ctl._v.copy(), ctl._zeta.copy(), list(its)


def _compare_loops(make, **kw):
    ref = _loop(make(), False, **kw)
    out = _loop(make(), True, **kw)
    worst_norm = max(abs(a - b) / b for a, b in zip(out[0], ref[0]))
    worst_field = max(np.abs(out[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
                      for k in (1, 2))
    print(f"non-linear iterations host / device: {len(ref[0]) - 1} / {len(out[0]) - 1}; "
          f"linear iterations {ref[3]} / {out[3]}; worst norm difference {worst_norm:.2e} "
          f"relative, worst field difference {worst_field:.2e}; last norm {ref[0][-1]:.2e} of "
          f"{ref[0][0]:.2e}")
    assert len(out[0]) == len(ref[0])
    for a, b in zip(out[0], ref[0]):
        assert abs(a - b) <= 1e-8 * b
    for k in (1, 2):
        assert out[k].shape == ref[k].shape
        assert np.abs(out[k] - ref[k]).max() <= 1e-9 * max(1.0, np.abs(ref[k]).max()), k
    assert out[3] == ref[3]
    return ref, out


@pytest.mark.parametrize("CN", [False, True])
def test_picard_loop(CN):
    ref, out = _compare_loops(lambda: reaction_heat_control_q2(CN), max_non_linear_iter=30)
    assert out[0][-1] <= 1.0e-9 * out[0][0] and len(out[0]) > 4


def test_gauss_newton_loop():
    def make():
        ctl = reaction_heat_control_q2(False)
        ctl.set_Gauss_Newton()
        return ctl
    _compare_loops(make, max_non_linear_iter=8)


def test_loop_with_boundary_values_and_an_initial_condition():
    make = lambda: reaction_heat_control_q2(False, **LIFTED)   # noqa: E731
    ref, out = _compare_loops(make, max_non_linear_iter=30)
    ctl = make()
    nodes = ctl._disc.boundary
    for i in range(ctl._n_t):
        assert np.array_equal(out[1][i, nodes], ctl._bc_values(i)[nodes])
    assert np.all(out[2][:, nodes] == 0.0)


def test_loop_with_two_grid_sub_solves():
    _compare_loops(lambda: reaction_heat_control_q2(False, n_t=3), Multigrid=True,
                   max_non_linear_iter=30)


# ------------------------------------------------------- the reference's stationary problem
@pytest.mark.parametrize("newton", [False, True])
def test_the_reference_stationary_problem_at_degree_two(newton):
    ref, out = _compare_loops(lambda: reference_stationary_problem(newton),
                              schur=SCHUR_STATIONARY, max_non_linear_iter=30)
    assert out[0][-1] <= 1.0e-9 * out[0][0]
    nodes = reference_stationary_problem()._disc.boundary
    assert np.all(out[1][nodes] == 0.0) and np.all(out[2][nodes] == 0.0)
