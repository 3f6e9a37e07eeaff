"""The scalar Picard / Gauss-Newton loop on the device on P1 tetrahedra
(``Instationary.non_linear_solve(device=True)`` on the unit cube, ``box_p1(n, n, n)``: the arrays of
``unit_cube_p1(n)`` with the cells a ``ReactionTerm`` needs) against the host path with the
same ``fem.ReactionTerm``: the device-built system and whole loops, by the scheme and with the bars
of ``tests/test_gpu_reaction_picard.py``.

The problem is the reference's non-linear reaction problem ``grad-grad + (2 + 0.5 v_old^2) mass``
on the unit cube, ``beta = 1e-2``, with a smooth desired state of amplitude 8: large enough for the
reaction to matter (the Picard loops take seven to eight iterations to ``1e-9``).

Sub-solve settings: the 2-D file's Chebyshev triple ``(40, 0.02, 2.2)`` suits the cube --
``control.suggest_chebyshev`` puts the Jacobi-scaled sub-solve matrices of the 6^3 cube on
[0.13, 1.96] -- and is used for both paths; the mass solves run on Wathen's interval for P1
tetrahedra, ``(0.5, 2.5)``, on both paths as well.
"""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import fem
from control_amd.control import GpuBackend, Instationary
from test_gpu_reaction_picard import _device_system, _host_system, _iterate, _same_blocks

pytestmark = pytest.mark.gpu

SCHUR = (40, 0.02, 2.2)
MASS = (0.5, 2.5)
KAT_SP = reaction_ref.KAT_SP
LIFTED = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0] + Xb[:, 2]),
              initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1])
              * np.sin(np.pi * X[:, 2]))


def reaction_heat_control_3d(CN, n=6, n_t=4, **kw):
    """``reaction_ref.reaction_heat_control`` on the unit cube."""
    disc = fem.box_p1(n, n, n)          # unit_cube_p1(n) array for array, with its cells

    def v_d(X, t):
        return (8.0 * (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1])
                * np.sin(np.pi * X[:, 2]) * np.exp(X[:, 0]))
    return Instationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d, CN=CN,
                        n_t=n_t, time_interval=(0.0, 1.0), beta=1.0e-2, **kw)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("newton", [False, True])
def test_device_built_system_equals_the_host_built_one(CN, newton):
    ctl = reaction_heat_control_3d(CN, **LIFTED)
    ctl.set_Gauss_Newton(newton)
    assert ctl._forward.cells.shape[1] == 4
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


def _loop(ctl, device, Multigrid=False, **kw):
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
                                 backend=GpuBackend(schur=SCHUR), Multigrid=Multigrid,
                                 device=device, **kw)
    if device:
        its = ctl.non_linear_info["linear_iterations"]
    return norms, ctl._v.copy(), ctl._zeta.copy(), list(its)


def _compare_loops(make, **kw):
    ref = _loop(make(), False, **kw)
    out = _loop(make(), True, **kw)
    print(f"non-linear iterations host / device: {len(ref[0]) - 1} / {len(out[0]) - 1}; "
          f"linear iterations {ref[3]} / {out[3]}")
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
    ref, out = _compare_loops(lambda: reaction_heat_control_3d(CN), max_non_linear_iter=30)
    assert out[0][-1] <= 1.0e-9 * out[0][0] and len(out[0]) > 4


def test_gauss_newton_loop():
    def make():
        ctl = reaction_heat_control_3d(False)
        ctl.set_Gauss_Newton()
        return ctl
    _compare_loops(make, max_non_linear_iter=8)


def test_loop_with_boundary_values_and_an_initial_condition():
    make = lambda: reaction_heat_control_3d(False, **LIFTED)   # noqa: E731
    ref, out = _compare_loops(make, max_non_linear_iter=30)
    ctl = make()
    nodes = ctl._disc.boundary
    for i in range(ctl._n_t):
        assert np.array_equal(out[1][i, nodes], ctl._bc_values(i)[nodes])
    assert np.all(out[2][:, nodes] == 0.0)


def test_loop_with_two_grid_sub_solves():
    _compare_loops(lambda: reaction_heat_control_3d(False, n=8, n_t=3), Multigrid=True,
                   max_non_linear_iter=30)
