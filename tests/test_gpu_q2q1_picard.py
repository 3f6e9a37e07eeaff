"""The Navier-Stokes Picard loops on the device on Q2-Q1 quadrilaterals (``fem.rectangle_q2q1``)
against the host paths, by the schemes and with the bars of ``tests/test_gpu_device_picard.py``,
``tests/test_gpu_device_build.py`` and ``tests/test_gpu_stationary_ns_picard.py`` -- their helpers
are called as they are, with the Q2 / Q1 mass intervals of the reference in the place of the
triangles' ones:

* instationary, backward Euler and Crank-Nicolson, ``rectangle_q2q1(4, 4, 2, 2)``, ``n_t = 4``,
  ``nu = 1 / 10``: ``GpuLinearSolver(relinearise="device")``, also with ``build="device"``;
* stationary: the problem of ``tests/test_control_driver.py::_stationary_navier_stokes_control``
  and its lid-driven variant at ``N = 4``.

For each: the device-built systems equal the host-built ones, the device loop gives the host
loop's Picard and linear iteration counts and its fields, a second call works, and nothing is
assembled on the host during the loop.  The sub-solve polynomials of the velocity and ``K_p``
blocks come from the library's spectrum estimates (``(-1, 0, 0)``), as in
``test_device_loop_manufactured``: the ellipse of ``NS_SCHUR`` was fitted to the triangles."""
import numpy as np
import pytest

import common
import test_gpu_device_build as build
import test_gpu_device_picard as loop
import test_gpu_stationary_ns_picard as stat
from control_amd import blocks, fem, picard
from control_amd.control import GpuBackend, Stationary

pytestmark = pytest.mark.gpu

MASS, MP = (20, 0.25, 1.5625), (20, 0.25, 2.25)          # the reference's Q2 and Q1 intervals
AUTO = (-1, 0.0, 0.0)
SPECS = dict(mass=MASS, schur=AUTO, kp=AUTO, mp=MP)
Q2_BOUNDS = dict(lambda_v_bounds=MASS[1:], lambda_p_bounds=MP[1:])
MESH = (4, 4, 2.0, 2.0)


# ---------------------------------------------------------------------------- instationary
def _ns_problem(CN, n_t=4, nu=0.1):
    """``common.navier_stokes_problem`` on the quadrilateral mesh: Picard convection, zero force
    and initial state, a smooth desired state that vanishes on the boundary."""
    th = fem.rectangle_q2q1(*MESH)
    X, Y = th.coords_v[:, 0], th.coords_v[:, 1]
    T = 2.0
    tau = T / (n_t - 1.0)
    v_d = np.stack([np.cos(0.5 * np.pi * i * tau) * np.concatenate([
        np.sin(0.5 * np.pi * X) ** 2 * np.sin(np.pi * Y),
        -np.sin(np.pi * X) * np.sin(0.5 * np.pi * Y) ** 2]) for i in range(n_t)])
    return picard.NavierStokesControl(disc=th, nu=nu, beta=1.0e-2, n_t=n_t, T=T, v_d=v_d,
                                      f=np.zeros((n_t, th.n_v)), CN=CN)


@pytest.mark.parametrize("CN", [False, True])
def test_instationary_device_built_systems_equal_the_host_built_ones(CN):
    pb = _ns_problem(CN)
    th = pb.disc
    rng = np.random.default_rng(common.SEED + 8)
    state = build._iterate(pb, rng)
    host = build._solver(pb, "host", specs=SPECS)
    dev = build._solver(pb, "device", specs=SPECS)
    host.setup(*state)
    dev.setup(*state)
    assert dev.uploads == 0
    interior = np.setdiff1d(np.arange(th.n_v), th.boundary_v)
    for name in ("outer", "inner", "comm"):
        hs, ds = getattr(host, name), getattr(dev, name)
        assert ds.info()["blocks_unset"] == 0 and hs.info()["blocks_unset"] == 0
        assert ds.info()["n_blocks_stored"] == hs.info()["n_blocks_stored"]
        for _ in range(2):
            x = rng.standard_normal(hs.local_size)
            e = common.rel_err(ds.mult(x), hs.mult(x))
            print(f"{name} CN={CN}: mult rel_err {e:.2e}")
            assert e <= 1e-13, name
        nx = th.n_p if name == "comm" else th.n_v
        for c in rng.choice(nx if name == "comm" else interior, 3, replace=False):
            e_c = np.zeros(hs.local_size)
            e_c[nx + c] = 1.0
            yh, yd = hs.mult(e_c), ds.mult(e_c)
            assert np.abs(yd - yh).max() <= 1e-13 * np.abs(yh).max(), (name, c)
        if name != "comm":
            for c in rng.choice(th.boundary_v, 3, replace=False):
                e_c = np.zeros(hs.local_size)
                e_c[nx + c] = 1.0
                assert np.array_equal(hs.mult(e_c), e_c), (name, c)
                assert np.array_equal(ds.mult(e_c), e_c), (name, c)
    # a re-linearisation at another iterate against the host's update of its blocks
    state = build._iterate(pb, rng, 0.2)
    loop._relinearise_both(pb, host, dev, state)
    for name in ("outer", "inner", "comm"):
        hs, ds = getattr(host, name), getattr(dev, name)
        x = rng.standard_normal(hs.local_size)
        assert common.rel_err(ds.mult(x), hs.mult(x)) <= 1e-13, name


@pytest.mark.parametrize("CN", [False, True])
def test_instationary_device_loop_against_the_host_loop(CN):
    pb = _ns_problem(CN)
    ref, out = loop._compare_loops(pb, lambda r: loop._solver(pb, r, specs=SPECS))
    print(f"CN={CN}: norms {ref['norms']}, linear iterations {ref['linear_iterations']}")
    assert out["converged"] and len(out["linear_iterations"]) >= 2


@pytest.mark.parametrize("CN", [False, True])
def test_instationary_device_build_against_the_host_build(CN):
    """``build="device"`` against ``build="host"``, both loops on the device."""
    pb = _ns_problem(CN)
    made = {}

    def make(b):
        made[b] = build._solver(pb, b, specs=SPECS)
        return made[b]
    ref, out = build._compare_runs(pb, make)
    assert out["converged"] and made["device"].uploads == 0


@pytest.mark.parametrize("CN", [False, True])
def test_instationary_second_call(CN):
    """One device-built solver for both runs: the second call re-linearises the live systems at
    the starting iterate and gives the first call's run."""
    pb = _ns_problem(CN)
    ls = build._solver(pb, "device", specs=SPECS)
    first, second = build._compare_runs(pb, lambda b: ls)
    assert first["converged"] and second["converged"] and ls.uploads == 0


@pytest.mark.parametrize("CN", [False, True])
def test_instationary_no_host_assembly(CN, monkeypatch):
    pb = _ns_problem(CN)
    th = pb.disc

    def refuse(*a, **k):
        raise AssertionError("host assembly on the device path")
    monkeypatch.setattr(type(pb), "D_v", refuse)
    monkeypatch.setattr(type(pb), "D_p", refuse)
    monkeypatch.setattr(th, "convection_v", refuse)
    monkeypatch.setattr(th, "convection_p", refuse)
    monkeypatch.setattr(picard, "instationary_incompressible_blocks", refuse)
    ls = build._solver(pb, "device", specs=SPECS)
    out = picard.incompressible_non_linear_solve(pb, ls, device=True,
                                                 print_error_non_linear=False)
    assert out["converged"] and len(out["linear_iterations"]) >= 2
    assert ls.uploads == 0


# ------------------------------------------------------------------------------ stationary
@pytest.fixture(autouse=True)
def _q2_bounds(monkeypatch):
    """The helpers of the triangles' file read their mass intervals from ``BOUNDS``."""
    monkeypatch.setattr(stat, "BOUNDS", Q2_BOUNDS)


def _problem(N=4, nu=1.0, lid=False):
    th = fem.rectangle_q2q1(N, N, 2.0, 2.0)

    def v_d(X):
        return np.concatenate([np.sin(0.5 * np.pi * X[:, 0]) ** 2 * np.sin(np.pi * X[:, 1]),
                               -np.sin(np.pi * X[:, 0]) * np.sin(0.5 * np.pi * X[:, 1]) ** 2])
    return Stationary(th, fem.ConvectionTerm(th, nu), desired_state=v_d, beta=1.0e-2,
                      bcs_v=stat._lid if lid else None)


@pytest.mark.parametrize("lid", [False, True])
def test_stationary_device_built_systems_equal_the_host_built_ones(lid):
    ctl = _problem(4, 0.1, lid)
    backend = GpuBackend(schur=stat.SCHUR)
    rng = np.random.default_rng(common.SEED + 1)
    state = stat._iterate(ctl, rng)
    systems, dev, _ = stat._device_systems(ctl, backend, state)
    stat._same_systems(ctl, systems, *stat._host_systems(ctl, backend, state[0][0]), rng)
    state = stat._iterate(ctl, rng, 0.3)
    stat._relinearise(systems, dev, state)
    stat._same_systems(ctl, systems, *stat._host_systems(ctl, backend, state[0][0]), rng)


@pytest.mark.parametrize("lid", [False, True])
def test_stationary_device_loop_against_the_host_loop(lid):
    make = lambda: _problem(4, 1.0, lid)   # noqa: E731
    if lid:
        ctl = make()
        nodes = ctl._disc.boundary
        assert np.all(ctl._v[nodes] == 0.0) and np.any(ctl._v_inhom()[nodes] != 0.0)
    ref, out = stat._compare_loops(make)
    assert len(out["its"]) >= 3            # re-linearisations inside the loop


@pytest.mark.parametrize("lid", [False, True])
def test_stationary_second_call_starts_from_nothing_stale(lid):
    ctl = _problem(4, 1.0, lid)
    start = ctl._v.copy(), ctl._zeta.copy()
    first = stat._loop(ctl, True)
    ctl._v, ctl._zeta = start[0].copy(), start[1].copy()
    del ctl._p, ctl._mu
    second = stat._loop(ctl, True)
    assert second["norms"] == first["norms"] and second["its"] == first["its"]
    for k in ("v", "zeta", "p", "mu"):
        assert np.array_equal(second[k], first[k]), k


@pytest.mark.parametrize("lid", [False, True])
def test_stationary_no_host_assembly(lid, monkeypatch):
    ctl = _problem(4, 1.0, lid)
    th = ctl._th

    def refuse(*a, **k):
        raise AssertionError("host assembly on the device path")
    monkeypatch.setattr(th, "convection_v", refuse)
    monkeypatch.setattr(th, "convection_p", refuse)
    monkeypatch.setattr(blocks, "stationary_incompressible_blocks", refuse)
    monkeypatch.setattr(blocks, "stationary_blocks", refuse)
    out = stat._loop(ctl, True)
    assert out["norms"][-1] <= 1.0e-8 * out["norms"][0] and len(out["its"]) >= 2
