"""Picard re-linearisation on the device (``GpuLinearSolver(relinearise="device")``,
``incompressible_non_linear_solve(device=True)``) against the host path: block values,
preconditioner, residual, and the whole loop."""
import numpy as np
import pytest

import common
from control_amd import picard
from control_amd.relinearise import DeviceRelinearisation  # noqa: F401  (import check)

pytestmark = pytest.mark.gpu

NS_SCHUR = (30, 0.25, 2.3, 0.5)          # the ellipse of tests/test_picard.py
NS_SPECS = dict(common.STOKES_SPECS, schur=NS_SCHUR)


def _solver(pb, relinearise, multigrid=False, specs=NS_SPECS, sp=common.NS_SOLVER_PARAMETERS):
    if multigrid:
        return picard.GpuLinearSolver(pb, mass=specs["mass"], mp=specs["mp"],
                                      solver_parameters=sp, Multigrid=True,
                                      relinearise=relinearise)
    return picard.GpuLinearSolver(pb, mass=specs["mass"], schur=specs["schur"], kp=specs["kp"],
                                  mp=specs["mp"], solver_parameters=sp, relinearise=relinearise)


def _iterate(pb, rng, scale=0.1):
    """A random iterate; winds of this size keep the convection blocks' spectra inside the
    Chebyshev ellipse of NS_SCHUR, so the preconditioner does not amplify round-off."""
    th, n_t = pb.disc, pb.n_t
    m = n_t - 1 if pb.CN else n_t
    v = scale * rng.standard_normal((n_t, th.n_v))
    zeta = rng.standard_normal((n_t, th.n_v))
    zeta[n_t - 1] = 0.0
    return v, zeta, rng.standard_normal((m, th.n_p)), rng.standard_normal((m, th.n_p))


def _pair(pb, rng, multigrid=False):
    """Host- and device-path solvers built at one iterate, then re-linearised at another."""
    v_a = _iterate(pb, rng)[0]
    v_b, zeta, p, mu = _iterate(pb, rng)
    host, dev = _solver(pb, "host", multigrid), _solver(pb, "device", multigrid)
    D_a = [pb.D_v(x) for x in v_a]
    Dp_a = [pb.D_p(x) for x in v_a]
    for ls in (host, dev):
        ls._build(ls._blocks(D_a, Dp_a))
    return host, dev, (v_b, zeta, p, mu)


def _relinearise_both(pb, host, dev, state):
    v_b = state[0]
    host._update(host._blocks([pb.D_v(x) for x in v_b], [pb.D_p(x) for x in v_b]))
    plan = dev.device_plan()
    plan.set_state(*state)
    plan.assemble()
    dev.device_relinearise()
    return plan


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n,n_t", [(8, 4), (32, 8)])
def test_device_relinearisation_matches_host_blocks(CN, n, n_t):
    pb = common.navier_stokes_problem(n=n, n_t=n_t, CN=CN)
    rng = np.random.default_rng(common.SEED + n)
    host, dev, state = _pair(pb, rng)
    _relinearise_both(pb, host, dev, state)
    for name in ("outer", "inner", "comm"):
        hs, ds = getattr(host, name), getattr(dev, name)
        x = rng.standard_normal(hs.local_size)
        assert common.rel_err(ds.mult(x), hs.mult(x)) <= 1e-13, name
    if n == 8:
        x = rng.standard_normal(host.outer.local_size)
        e = common.rel_err(dev.outer.pc_apply(x, dev.pc), host.outer.pc_apply(x, host.pc))
        assert e <= max(1e-12, 100 * _pc_roundoff(pb, state, x, host)), e
    # a second re-linearisation at another point: the same again (nothing cached stale)
    state2 = _iterate(pb, rng, 0.2)
    _relinearise_both(pb, host, dev, state2)
    x = rng.standard_normal(host.inner.local_size)
    assert common.rel_err(dev.inner.mult(x), host.inner.mult(x)) <= 1e-13


def _pc_roundoff(pb, state, x, host, multigrid=False):
    """How far the host path's preconditioner moves when every linearised block is perturbed
    by one unit in the last place: the scale of agreement two assemblies of one operator can
    reach (the inner GMRES and the Chebyshev sweeps amplify round-off)."""
    ls = _solver(pb, "host", multigrid)
    v_b = state[0]
    D = [pb.D_v(v) for v in v_b]
    Dp = [pb.D_p(v) for v in v_b]
    ls._build(ls._blocks(D, Dp))
    for A in D + Dp:
        A.data *= 1.0 + 2.0 ** -52
    ls._update(ls._blocks(D, Dp))
    return common.rel_err(ls.outer.pc_apply(x, ls.pc), host.outer.pc_apply(x, host.pc))


def test_device_relinearisation_rebuilds_the_two_grid_preconditioner():
    pb = common.navier_stokes_problem(n=8, n_t=4)
    rng = np.random.default_rng(common.SEED)
    host, dev, state = _pair(pb, rng, multigrid=True)
    x = rng.standard_normal(host.outer.local_size)
    y0 = dev.outer.pc_apply(x, dev.pc)           # built at the first iterate
    host.outer.pc_apply(x, host.pc)
    before = dev.inner.coarse_setup_stats()
    _relinearise_both(pb, host, dev, state)
    y_d = dev.outer.pc_apply(x, dev.pc)
    y_h = host.outer.pc_apply(x, host.pc)
    after = dev.inner.coarse_setup_stats()
    e = common.rel_err(y_d, y_h)
    assert e <= max(1e-12, 100 * _pc_roundoff(pb, state, x, host, multigrid=True)), e
    assert common.rel_err(y_d, y0) > 1e-6        # the preconditioner did change
    assert after["matrices"] == before["matrices"] > 0 and after["launches"] > 0


@pytest.mark.parametrize("CN", [False, True])
def test_device_residual_matches_host(CN):
    pb = common.navier_stokes_problem(n=8, n_t=5, CN=CN)
    rng = np.random.default_rng(common.SEED + 7)
    host, dev, _ = _pair(pb, rng)
    v, zeta, p, mu = _iterate(pb, rng)
    plan = dev.device_plan()
    plan.set_state(v, zeta, p, mu)
    plan.assemble()
    out = np.zeros(dev.outer.local_size)
    import ctypes as C
    lib, h = dev.outer._lib, dev.outer.handle
    d = C.c_void_p()
    dev.outer._ck(lib.kkt_vec_alloc(h, C.byref(d)))
    try:
        norm = plan.residual(d, rhs=False)
        dev.outer._ck(lib.kkt_vec_download(h, d, out.ctypes.data_as(C.POINTER(C.c_double))))
    finally:
        lib.kkt_vec_free(h, d)
    D = [pb.D_v(x) for x in v]
    r = picard.non_linear_res_eval(pb, D, v, zeta, p, mu)
    ref = np.concatenate([np.ravel(x) for x in r])
    assert common.rel_err(out, ref) <= 1e-12
    assert abs(norm - np.linalg.norm(ref)) <= 1e-12 * np.linalg.norm(ref)


def _compare_loops(pb, make, norm_floor=0.0, **kw):
    """``norm_floor``: an absolute allowance on the residual norms, relative to the first one."""
    ref = picard.incompressible_non_linear_solve(pb, make("host"), print_error_non_linear=False,
                                                 **kw)
    out = picard.incompressible_non_linear_solve(pb, make("device"), device=True,
                                                 print_error_non_linear=False, **kw)
    assert len(out["norms"]) == len(ref["norms"])
    assert out["linear_iterations"] == ref["linear_iterations"]
    assert out["converged"] == ref["converged"]
    for a, b in zip(out["norms"], ref["norms"]):
        assert abs(a - b) <= 1e-8 * b + norm_floor * ref["norms"][0]
    for key in ("v", "zeta", "p", "mu"):
        assert out[key].shape == ref[key].shape
        assert np.abs(out[key] - ref[key]).max() <= 1e-9 * max(1.0, np.abs(ref[key]).max()), key
    return ref, out


@pytest.mark.parametrize("CN", [False, True])
def test_device_loop_cavity(CN):
    pb, v_init, lid = common.navier_stokes_cavity_problem(n=8, n_t=10, CN=CN)
    pb.nu = 1.0 / 100.0
    ref, out = _compare_loops(pb, lambda r: _solver(pb, r), v=v_init)
    assert out["converged"]
    th = pb.disc
    assert np.array_equal(out["v"][:, th.boundary_v], v_init[:, th.boundary_v])


def test_device_loop_manufactured():
    """tests/test_picard.py's manufactured problem at N = 16 (nu = 1/50, estimated sub-solve
    ellipses)."""
    pb, v0, true_v = common.mms_navier_stokes_control(16, CN=False, n_t=30, nu=1.0 / 50.0)
    sp = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 200,
          "relative_tolerance": 1.0e-7, "absolute_tolerance": 1.0e-7,
          "monitor_convergence": False}
    auto = (-1, 0.0, 0.0)
    specs = dict(mass=(20, 0.3924, 2.0598), schur=auto, kp=auto, mp=(20, 0.5, 2.0))
    # the loop drives the residual six decades below its first norm (1.37 to 8e-7): what is left is
    # a difference of terms of the first norm's size, and two evaluations of it agree no better than
    # the 1e-12 of that size that test_device_residual_matches_host asks of one evaluation
    ref, out = _compare_loops(pb, lambda r: _solver(pb, r, specs=specs, sp=sp), norm_floor=1e-12, v=v0,
                              max_non_linear_iter=10, relative_non_linear_tol=1.0e-6,
                              absolute_non_linear_tol=1.0e-6)
    assert out["converged"]
    th, tau = pb.disc, pb.tau

    def err(res):
        e = 0.0
        for i in range(pb.n_t):
            d = res["v"][i] - true_v(i * tau)
            e += tau * (d @ (th.M_v @ d))
        return np.sqrt(e)
    assert abs(err(out) - err(ref)) <= 1e-8 * err(ref)
