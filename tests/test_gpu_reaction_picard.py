"""The scalar Picard / Gauss-Newton loop on the device (``Instationary.non_linear_solve(
device=True)``, ``control_amd.reaction``) against the host path: the device-built system, the
preconditioner after a re-linearisation, and whole loops."""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import blocks, reaction
from control_amd.control import GpuBackend, _multigrid_kw

pytestmark = pytest.mark.gpu

SCHUR = (40, 0.02, 2.2)
KAT_SP = reaction_ref.KAT_SP
LIFTED = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0]),
              initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]))


def _iterate(ctl, rng, scale=1.0):
    shape = (ctl._n_t, ctl._disc.n_dofs)
    return scale * rng.standard_normal(shape), rng.standard_normal(shape)


def _host_system(ctl, backend, v, Multigrid=False):
    """What ``linear_solve`` builds at the iterate ``v``: the system and its preconditioner."""
    disc, n_t, CN, beta = ctl._disc, ctl._n_t, ctl._CN, ctl._beta
    t_0, _, tau = ctl._times()
    D = [blocks.conform_to(ctl.construct_D_v(v[i], t_0 + i * tau), disc.M) for i in range(n_t)]
    b00, b01, b10, b11, m = blocks.instationary_blocks(disc.M, D, tau, beta, n_t, CN)
    ns = tuple(backend.DirichletBCNullspace(disc.boundary) for _ in range(m))
    system = backend.MultiBlockSystem(disc.n_dofs, disc.n_dofs, b00, b01, b10, b11,
                                      n_blocks_00=m, n_blocks_11=m, nullspace_0=ns,
                                      nullspace_1=ns, CN=CN)
    pc = backend.construct_pc("CN" if CN else "BE", disc.M, b01, b10, n_t, tau, beta,
                              disc.boundary, (0.5, 2.0), 1.0e-3, **_multigrid_kw(disc, Multigrid))
    return system, pc, D


def _device_system(ctl, backend, state, Multigrid=False):
    plan = reaction.ReactionPlan(ctl)
    system, quads, full = reaction.build_system(ctl, backend, plan)
    dev = reaction.DeviceReaction(ctl, system, plan=plan)
    dev.set_state(*state)
    dev.assemble()
    dev.relinearise(recipes=full)
    disc = ctl._disc
    pc = backend.construct_pc("CN" if plan.CN else "BE", plan.term.M, quads[1], quads[2],
                              plan.n_t, plan.tau, plan.beta, disc.boundary, (0.5, 2.0), 1.0e-3,
                              **_multigrid_kw(disc, Multigrid))
    return system, dev, pc, full


def _same_blocks(host, device, recipes):
    for (q, i, j, *_) in recipes:
        assert np.array_equal(device.block_values(q, i, j)[0], host.block_values(q, i, j)[0]), \
            (q, i, j)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("newton", [False, True])
def test_device_built_system_equals_the_host_built_one(CN, newton):
    ctl = reaction_ref.reaction_heat_control(CN, **LIFTED)
    ctl.set_Gauss_Newton(newton)
    backend = GpuBackend(schur=SCHUR)
    rng = np.random.default_rng(common.SEED + 1)
    state = _iterate(ctl, rng)
    system, dev, _, full = _device_system(ctl, backend, state)
    host, _, _ = _host_system(ctl, backend, state[0])
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


def _pc_roundoff(ctl, backend, v, x, y_host, Multigrid):
    """How far the host path's preconditioner moves when every linearised block is perturbed by
    one unit in the last place (``_pc_roundoff`` of ``tests/test_gpu_device_picard.py``)."""
    disc, n_t, CN, beta = ctl._disc, ctl._n_t, ctl._CN, ctl._beta
    t_0, _, tau = ctl._times()
    D = [blocks.conform_to(ctl.construct_D_v(v[i], t_0 + i * tau), disc.M) for i in range(n_t)]
    for A in D:
        A.data *= 1.0 + 2.0 ** -52
    b00, b01, b10, b11, m = blocks.instationary_blocks(disc.M, D, tau, beta, n_t, CN)
    ns = tuple(backend.DirichletBCNullspace(disc.boundary) for _ in range(m))
    system = backend.MultiBlockSystem(disc.n_dofs, disc.n_dofs, b00, b01, b10, b11,
                                      n_blocks_00=m, n_blocks_11=m, nullspace_0=ns,
                                      nullspace_1=ns, CN=CN)
    pc = backend.construct_pc("CN" if CN else "BE", disc.M, b01, b10, n_t, tau, beta,
                              disc.boundary, (0.5, 2.0), 1.0e-3, **_multigrid_kw(disc, Multigrid))
    return common.rel_err(system.pc_apply(x, pc), y_host)


@pytest.mark.parametrize("Multigrid", [False, True])
def test_preconditioner_after_a_relinearisation(Multigrid):
    ctl = reaction_ref.reaction_heat_control(False)
    backend = GpuBackend(schur=SCHUR)
    rng = np.random.default_rng(common.SEED + 2)
    system, dev, pc, _ = _device_system(ctl, backend, _iterate(ctl, rng), Multigrid)
    # A smooth load on every block.  On a random vector the output is the mass solves' to five
    # parts in a million (the sub-solves with D damp it by h^2), and so is any change of D.
    disc = ctl._disc
    load = disc.M @ (np.sin(np.pi * disc.coords[:, 0]) * np.sin(np.pi * disc.coords[:, 1]))
    x = np.concatenate([np.outer(1.0 + np.arange(ctl._n_t), load).ravel(),
                        np.outer(np.ones(ctl._n_t), load).ravel()])
    assert x.size == system.local_size
    y0 = system.pc_apply(x, pc)                   # built at the first iterate
    state = _iterate(ctl, rng, 10.0)
    dev.set_state(*state)
    dev.assemble()
    dev.relinearise()
    y_d = system.pc_apply(x, pc)
    host, host_pc, _ = _host_system(ctl, backend, state[0], Multigrid)
    y_h = host.pc_apply(x, host_pc)
    e = common.rel_err(y_d, y_h)
    bar = max(1e-12, 100 * _pc_roundoff(ctl, backend, state[0], x, y_h, Multigrid))
    print(f"Multigrid={Multigrid}: device against host preconditioner {e:.2e}, bar {bar:.2e}")
    assert e <= bar
    assert common.rel_err(y_d, y0) > 1e-6         # the preconditioner did change


def _loop(ctl, device, Multigrid=False, **kw):
    """One loop; the host path's linear iteration counts are read off ``linear_solve``."""
    its, solve = [], ctl.linear_solve

    def recording(**a):
        ksp = solve(**a)
        its.append(ksp.getIterationNumber())
        return ksp
    if not device:
        ctl.linear_solve = recording
    norms = ctl.non_linear_solve(solver_parameters=KAT_SP, lambda_v_bounds=(0.5, 2.0),
                                 relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                 backend=GpuBackend(schur=SCHUR), Multigrid=Multigrid,
                                 device=device, **kw)
    if device:
        its = ctl.non_linear_info["linear_iterations"]
    return norms, ctl._v.copy(), ctl._zeta.copy(), list(its)


def _compare_loops(make, **kw):
    ref = _loop(make(), False, **kw)
    out = _loop(make(), True, **kw)
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
    ref, out = _compare_loops(lambda: reaction_ref.reaction_heat_control(CN),
                              max_non_linear_iter=30)
    assert out[0][-1] <= 1.0e-9 * out[0][0] and len(out[0]) > 3


@pytest.mark.parametrize("CN", [False, True])
def test_gauss_newton_loop(CN):
    def make():
        ctl = reaction_ref.reaction_heat_control(CN)
        ctl.set_Gauss_Newton()
        return ctl
    _compare_loops(make, max_non_linear_iter=8)


@pytest.mark.parametrize("CN", [False, True])
def test_loop_with_boundary_values_and_an_initial_condition(CN):
    make = lambda: reaction_ref.reaction_heat_control(CN, **LIFTED)   # noqa: E731
    ref, out = _compare_loops(make, max_non_linear_iter=30)
    ctl = make()
    nodes = ctl._disc.boundary
    for i in range(ctl._n_t):
        assert np.array_equal(out[1][i, nodes], ctl._bc_values(i)[nodes])
    assert np.all(out[2][:, nodes] == 0.0)


def test_loop_with_two_grid_sub_solves():
    _compare_loops(lambda: reaction_ref.reaction_heat_control(False), Multigrid=True,
                   max_non_linear_iter=30)


def test_a_second_call_starts_from_nothing_stale():
    ctl = reaction_ref.reaction_heat_control(True, **LIFTED)
    start = ctl._v.copy(), ctl._zeta.copy()
    first = _loop(ctl, True, max_non_linear_iter=30)
    # back to the starting iterate as it was (set_v would put the boundary values in)
    ctl._v, ctl._zeta = start[0].copy(), start[1].copy()
    second = _loop(ctl, True, max_non_linear_iter=30)
    assert second[0] == first[0] and second[3] == first[3]
    assert np.array_equal(second[1], first[1]) and np.array_equal(second[2], first[2])
