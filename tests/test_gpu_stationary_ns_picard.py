"""The stationary Navier-Stokes Picard loop on the device
(``Stationary.incompressible_non_linear_solve(device=True)``, ``control_amd.stationary_picard``)
against the host path with the same ``fem.ConvectionTerm``, by the scheme and with the bars of
``tests/test_gpu_device_picard.py`` and ``tests/test_gpu_stationary_reaction_picard.py``: the
device-built systems, the preconditioner after a re-linearisation, whole loops, a second call, and
no host assembly.

The problem is that of ``tests/test_control_driver.py::_stationary_navier_stokes_control`` --
``rectangle_p2p1(N, N, 2, 2)``, ``beta = 1e-2`` -- and its lid-driven variant: ``u_x = x^2 (2 -
x)^2 / 4`` on ``y = 2``, zero elsewhere, with a starting iterate that does not carry these values."""
import numpy as np
import pytest

import common
from control_amd import blocks, fem, relinearise, stationary_picard
from control_amd.control import GpuBackend, Stationary, _multigrid_stokes_kw
from test_control_driver import MMS_STOKES_SP

pytestmark = pytest.mark.gpu

SCHUR = (40, 0.01, 2.25)
BOUNDS = dict(lambda_v_bounds=(0.3924, 2.0598), lambda_p_bounds=(0.5, 2.0))
TWO_GRID_N = 8           # the smallest N of 8, 16, 32 at which the host path's two-grid loop converges


def _lid(Xb):
    ux = np.where(np.isclose(Xb[:, 1], 2.0), 0.25 * Xb[:, 0] ** 2 * (2.0 - Xb[:, 0]) ** 2, 0.0)
    return np.concatenate([ux, np.zeros(len(Xb))])


def _problem(N=4, nu=1.0, lid=False):
    th = fem.rectangle_p2p1(N, N, 2.0, 2.0)

    def v_d(X):
        return np.concatenate([np.sin(0.5 * np.pi * X[:, 0]) ** 2 * np.sin(np.pi * X[:, 1]),
                               -np.sin(np.pi * X[:, 0]) * np.sin(0.5 * np.pi * X[:, 1]) ** 2])
    return Stationary(th, fem.ConvectionTerm(th, nu), desired_state=v_d, beta=1.0e-2,
                      bcs_v=_lid if lid else None)


def _iterate(ctl, rng, scale=1.0):
    th = ctl._th
    return (scale * rng.standard_normal((1, th.n_v)), rng.standard_normal((1, th.n_v)),
            rng.standard_normal((1, th.n_p)), rng.standard_normal((1, th.n_p)))


def _host_systems(ctl, backend, v, Multigrid=False, perturb=1.0):
    """What ``incompressible_linear_solve`` builds at the iterate ``v``: the outer system and its
    ``StokesPC`` (which holds the host-built inner and commutator systems)."""
    th, beta = ctl._th, ctl._beta
    D_v = ctl.construct_D_v(v).copy()
    D_p = blocks.conform_to(ctl._forward.pressure(v), th.M_p).copy()
    D_v.data *= perturb
    D_p.data *= perturb
    nsv = tuple(backend.DirichletBCNullspace(th.boundary_v) for _ in range(2))
    nsp = tuple(backend.ConstantNullspace() for _ in range(2))
    outer = backend.MultiBlockSystem(
        th.n_v, th.n_p, *blocks.stationary_incompressible_blocks(th.M_v, D_v, th.B, beta),
        n_blocks_00=2, n_blocks_11=2, nullspace_0=nsv, nullspace_1=nsp)
    pc = backend.construct_stokes_pc_stationary(th, D_v, D_p, beta, *BOUNDS.values(),
                                                **_multigrid_stokes_kw(th, Multigrid))
    return outer, pc


def _device_systems(ctl, backend, state, Multigrid=False):
    pb = stationary_picard.StationaryNavierStokes(ctl)
    plan = relinearise.RelinearisationPlan(pb)
    systems = stationary_picard.build_systems(pb, backend, plan)
    dev = relinearise.DeviceRelinearisation(
        pb, systems[0], blocks.stationary_incompressible_relinearisation_recipes(pb.beta),
        plan=plan)
    dev.set_state(*state)
    dev.assemble()
    full = blocks.stationary_incompressible_build_recipes(pb.beta)
    for system, name in zip(systems, ("outer", "inner", "commutator")):
        dev.relinearise(system, name, recipes=full[name])
    pc = stationary_picard.attach_pc(pb, backend, systems[1], systems[2], *BOUNDS.values(),
                                     Multigrid=Multigrid)
    return systems, dev, pc


def _relinearise(systems, dev, state):
    dev.set_state(*state)
    dev.assemble()
    for system, name in zip(systems, ("outer", "inner", "commutator")):
        dev.relinearise(system, name)


def _same_systems(ctl, systems, host, host_pc, rng):
    th = ctl._th
    interior = np.setdiff1d(np.arange(th.n_v), th.boundary_v)
    for name, ds, hs in zip(("outer", "inner", "commutator"), systems,
                            (host, host_pc.inner, host_pc.commutator)):
        assert ds.info()["blocks_unset"] == 0 and hs.info()["blocks_unset"] == 0
        assert ds.info()["n_blocks_stored"] == hs.info()["n_blocks_stored"]
        assert ds.local_size == hs.local_size
        for _ in range(2):
            x = rng.standard_normal(hs.local_size)
            e = common.rel_err(ds.mult(x), hs.mult(x))
            print(f"{name}: mult rel_err {e:.2e}")
            assert e <= 1e-13, name
        # unit vectors of the second block: interior columns, and -- on the velocity space --
        # Dirichlet columns, whose result is the masked one exactly: the identity
        nx = th.n_p if name == "commutator" else th.n_v
        for c in rng.choice(nx if name == "commutator" else interior, 3, replace=False):
            e_c = np.zeros(hs.local_size)
            e_c[nx + c] = 1.0
            yh, yd = hs.mult(e_c), ds.mult(e_c)
            assert np.abs(yd - yh).max() <= 1e-13 * np.abs(yh).max(), (name, c)
        if name != "commutator":
            for c in rng.choice(th.boundary_v, 3, replace=False):
                for block in range(2):
                    e_c = np.zeros(hs.local_size)
                    e_c[block * nx + c] = 1.0
                    assert np.array_equal(hs.mult(e_c), e_c), (name, c)
                    assert np.array_equal(ds.mult(e_c), e_c), (name, c)


def test_device_built_systems_equal_the_host_built_ones():
    ctl = _problem(4, 0.1, lid=True)
    backend = GpuBackend(schur=SCHUR)
    rng = np.random.default_rng(common.SEED + 1)
    state = _iterate(ctl, rng)
    systems, dev, _ = _device_systems(ctl, backend, state)
    _same_systems(ctl, systems, *_host_systems(ctl, backend, state[0][0]), rng)
    # a second re-linearisation at another iterate: the same again (nothing cached stale)
    state = _iterate(ctl, rng, 0.3)
    _relinearise(systems, dev, state)
    _same_systems(ctl, systems, *_host_systems(ctl, backend, state[0][0]), rng)


@pytest.mark.parametrize("Multigrid", [False, True])
def test_preconditioner_after_a_relinearisation(Multigrid):
    ctl = _problem(8, 1.0)
    backend = GpuBackend(schur=SCHUR)
    rng = np.random.default_rng(common.SEED + 2)
    # winds of this size keep the spectra of the convection blocks inside the Chebyshev interval:
    # the preconditioner does not amplify round-off (tests/test_gpu_device_build.py)
    systems, dev, pc = _device_systems(ctl, backend, _iterate(ctl, rng, 0.1), Multigrid)
    outer = systems[0]
    x = rng.standard_normal(outer.local_size)
    y0 = outer.pc_apply(x, pc)                    # built at the first iterate
    state = _iterate(ctl, rng, 1.0)
    _relinearise(systems, dev, state)
    y_d = outer.pc_apply(x, pc)
    host, host_pc = _host_systems(ctl, backend, state[0][0], Multigrid)
    y_h = host.pc_apply(x, host_pc)
    # how far the host path's preconditioner moves under a one-ulp perturbation of D_v and D_p
    moved, moved_pc = _host_systems(ctl, backend, state[0][0], Multigrid,
                                    perturb=1.0 + 2.0 ** -52)
    roundoff = common.rel_err(moved.pc_apply(x, moved_pc), y_h)
    e = common.rel_err(y_d, y_h)
    bar = max(1e-12, 100 * roundoff)
    print(f"Multigrid={Multigrid}: device against host preconditioner {e:.2e}, bar {bar:.2e}; "
          f"moved by the re-linearisation {common.rel_err(y_d, y0):.2e}")
    assert e <= bar
    assert common.rel_err(y_d, y0) > 1e-6         # the preconditioner did change


def _loop(ctl, device, Multigrid=False):
    """One loop; the host path's linear iteration counts are read off
    ``incompressible_linear_solve``."""
    its, solve = [], ctl.incompressible_linear_solve

    def recording(*a, **k):
        ksp = solve(*a, **k)
        its.append(ksp.getIterationNumber())
        return ksp
    if not device:
        ctl.incompressible_linear_solve = recording
    norms = ctl.incompressible_non_linear_solve(
        solver_parameters=MMS_STOKES_SP, **BOUNDS, max_non_linear_iter=30,
        relative_non_linear_tol=1.0e-8, absolute_non_linear_tol=0.0,
        backend=GpuBackend(schur=SCHUR), Multigrid=Multigrid, device=device)
    if device:
        its = ctl.non_linear_info["linear_iterations"]
        assert ctl.non_linear_info["window"]["blocks"] == (0, 1)
    return dict(norms=norms, v=ctl._v.copy(), zeta=ctl._zeta.copy(), p=ctl._p.copy(),
                mu=ctl._mu.copy(), its=list(its))


def _compare_loops(make, Multigrid=False):
    ref, out = _loop(make(), False, Multigrid), _loop(make(), True, Multigrid)
    ctl = make()
    th, nodes = ctl._th, ctl._disc.boundary
    norm_0 = ref["norms"][0]
    worst_norm = max(abs(a - b) / b for a, b in zip(out["norms"], ref["norms"]))
    worst_field = max(np.abs(out[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
                      for k in ("v", "zeta", "p", "mu"))
    print(f"non-linear iterations host / device: {len(ref['norms']) - 1} / "
          f"{len(out['norms']) - 1}; linear iterations {ref['its']} / {out['its']}; worst norm "
          f"difference {worst_norm:.2e} relative, worst field difference {worst_field:.2e}; "
          f"norms {ref['norms'][0]:.2e} -> {ref['norms'][-1]:.2e}; "
          f"|B v| = {np.abs(th.B @ out['v']).max():.2e}")
    assert len(out["norms"]) == len(ref["norms"])
    assert out["its"] == ref["its"]
    # the loop drives the residual eight decades below its first norm: what is left is a
    # difference of terms of the first norm's size, and two evaluations of it agree no better than
    # 1e-12 of that size (tests/test_gpu_device_picard.py::test_device_loop_manufactured)
    for a, b in zip(out["norms"], ref["norms"]):
        assert abs(a - b) <= 1e-8 * b + 1e-12 * norm_0
    for k in ("v", "zeta", "p", "mu"):
        assert out[k].shape == ref[k].shape
        assert np.abs(out[k] - ref[k]).max() <= 1e-9 * max(1.0, np.abs(ref[k]).max()), k
    assert np.array_equal(out["v"][nodes], ctl._v_inhom()[nodes])
    assert np.all(out["zeta"][nodes] == 0.0)
    assert np.abs(th.B @ out["v"]).max() < 1e-8          # discretely divergence-free state
    assert out["norms"][-1] <= 1.0e-8 * out["norms"][0]
    return ref, out


@pytest.mark.parametrize("N,nu,lid", [(4, 1.0, False), (4, 1.0, True), (8, 0.1, True)])
def test_picard_loop(N, nu, lid):
    make = lambda: _problem(N, nu, lid)   # noqa: E731
    if lid:
        ctl = make()
        nodes = ctl._disc.boundary
        assert np.all(ctl._v[nodes] == 0.0) and np.any(ctl._v_inhom()[nodes] != 0.0)
    ref, out = _compare_loops(make)
    assert len(out["its"]) >= 3            # re-linearisations inside the loop


def test_loop_with_two_grid_sub_solves():
    _compare_loops(lambda: _problem(TWO_GRID_N, 1.0), Multigrid=True)


def test_a_second_call_starts_from_nothing_stale():
    ctl = _problem(4, 1.0, lid=True)
    start = ctl._v.copy(), ctl._zeta.copy()
    first = _loop(ctl, True)
    # back to the starting iterate as it was (set_v would put the boundary values in)
    ctl._v, ctl._zeta = start[0].copy(), start[1].copy()
    del ctl._p, ctl._mu
    second = _loop(ctl, True)
    assert second["norms"] == first["norms"] and second["its"] == first["its"]
    for k in ("v", "zeta", "p", "mu"):
        assert np.array_equal(second[k], first[k]), k


def test_a_call_continues_from_p_and_mu():
    """``p`` / ``mu`` start from ``_p`` / ``_mu`` when present, as the host loop's do: a call at
    the converged fields starts at the residual the first call ended with."""
    ctl = _problem(4, 1.0)
    first = _loop(ctl, True)
    again = ctl.incompressible_non_linear_solve(
        solver_parameters=MMS_STOKES_SP, **BOUNDS, max_non_linear_iter=1,
        relative_non_linear_tol=1.0e-8, absolute_non_linear_tol=0.0,
        backend=GpuBackend(schur=SCHUR), device=True)
    assert abs(again[0] - first["norms"][-1]) <= 1e-12 * first["norms"][0]
    ctl._p[:] = 0.0
    ctl._mu[:] = 0.0
    without = ctl.incompressible_non_linear_solve(
        solver_parameters=MMS_STOKES_SP, **BOUNDS, max_non_linear_iter=1,
        relative_non_linear_tol=1.0e-8, absolute_non_linear_tol=0.0,
        backend=GpuBackend(schur=SCHUR), device=True)
    assert without[0] > 1.0e3 * again[0]


def test_no_host_assembly(monkeypatch):
    ctl = _problem(4, 1.0, lid=True)
    th = ctl._th

    def refuse(*a, **k):
        raise AssertionError("host assembly on the device path")
    monkeypatch.setattr(th, "convection_v", refuse)
    monkeypatch.setattr(th, "convection_p", refuse)
    monkeypatch.setattr(blocks, "stationary_incompressible_blocks", refuse)
    monkeypatch.setattr(blocks, "stationary_blocks", refuse)
    out = _loop(ctl, True)
    assert out["norms"][-1] <= 1.0e-8 * out["norms"][0] and len(out["its"]) >= 2
