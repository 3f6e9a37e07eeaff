"""The first build on the device (``GpuLinearSolver(relinearise="device", build="device")``)
against the host build: the three systems, the preconditioner, whole Picard runs, no host
assembly, and the refusal of blocks that have a structure but no values yet."""
import ctypes as C

import numpy as np
import pytest

import common
from control_amd import _lib, picard
from control_amd.multiblock import MultiBlockSystem, PatternOnly

pytestmark = pytest.mark.gpu

NS_SCHUR = (30, 0.25, 2.3, 0.5)          # the ellipse of tests/test_picard.py
NS_SPECS = dict(common.STOKES_SPECS, schur=NS_SCHUR)


def _solver(pb, build, multigrid=False, specs=NS_SPECS, sp=common.NS_SOLVER_PARAMETERS):
    if multigrid:
        return picard.GpuLinearSolver(pb, mass=specs["mass"], mp=specs["mp"],
                                      solver_parameters=sp, Multigrid=True,
                                      relinearise="device", build=build)
    return picard.GpuLinearSolver(pb, mass=specs["mass"], schur=specs["schur"], kp=specs["kp"],
                                  mp=specs["mp"], solver_parameters=sp, relinearise="device",
                                  build=build)


def _iterate(pb, rng, scale=0.1):
    """A random iterate; winds of this size keep the convection blocks' spectra inside the
    Chebyshev ellipse of NS_SCHUR, so the preconditioner does not amplify round-off."""
    th, n_t = pb.disc, pb.n_t
    m = n_t - 1 if pb.CN else n_t
    v = scale * rng.standard_normal((n_t, th.n_v))
    zeta = rng.standard_normal((n_t, th.n_v))
    zeta[n_t - 1] = 0.0
    return v, zeta, rng.standard_normal((m, th.n_p)), rng.standard_normal((m, th.n_p))


def _pc_roundoff(pb, state, x, host, multigrid=False):
    """How far the host build's preconditioner moves when every linearised block is perturbed
    by one unit in the last place: the scale of agreement two assemblies of one operator can
    reach (the inner GMRES and the Chebyshev sweeps amplify round-off).  As in
    tests/test_gpu_device_picard.py."""
    ls = picard.GpuLinearSolver(pb, mass=NS_SPECS["mass"], mp=NS_SPECS["mp"],
                                solver_parameters=common.NS_SOLVER_PARAMETERS,
                                **(dict(Multigrid=True) if multigrid else
                                   dict(schur=NS_SPECS["schur"], kp=NS_SPECS["kp"])))
    D = [pb.D_v(v) for v in state[0]]
    Dp = [pb.D_p(v) for v in state[0]]
    ls._build(ls._blocks(D, Dp))
    for A in D + Dp:
        A.data *= 1.0 + 2.0 ** -52
    ls._update(ls._blocks(D, Dp))
    return common.rel_err(ls.outer.pc_apply(x, ls.pc), host.outer.pc_apply(x, host.pc))


@pytest.mark.parametrize("multigrid", [False, True])
@pytest.mark.parametrize("CN", [False, True])
def test_same_systems_and_preconditioner(CN, multigrid):
    pb = common.navier_stokes_problem(n=8, n_t=4, CN=CN)
    th = pb.disc
    rng = np.random.default_rng(common.SEED + 8)
    state = _iterate(pb, rng)
    host, dev = _solver(pb, "host", multigrid), _solver(pb, "device", multigrid)
    host.setup(*state)
    dev.setup(*state)
    assert dev.uploads == 0 and dev.setup_s > 0.0 and host.setup_s > 0.0
    interior = np.setdiff1d(np.arange(th.n_v), th.boundary_v)
    for name in ("outer", "inner", "comm"):
        hs, ds = getattr(host, name), getattr(dev, name)
        assert ds.info()["blocks_unset"] == 0 and hs.info()["blocks_unset"] == 0
        assert ds.info()["n_blocks_stored"] == hs.info()["n_blocks_stored"]
        for _ in range(2):
            x = rng.standard_normal(hs.local_size)
            e = common.rel_err(ds.mult(x), hs.mult(x))
            print(f"{name} CN={CN} mg={multigrid}: mult rel_err {e:.2e}")
            assert e <= 1e-13, name
        # unit vectors of one level (the second block): three interior columns, and -- on the
        # velocity spaces -- three Dirichlet columns, whose result is the masked one exactly:
        # P A P e = 0 and alpha (I - P) e = e
        nx = th.n_p if name == "comm" else th.n_v
        cols = rng.choice(nx if name == "comm" else interior, 3, replace=False)
        for c in cols:
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
    x = rng.standard_normal(host.outer.local_size)
    e = common.rel_err(dev.outer.pc_apply(x, dev.pc), host.outer.pc_apply(x, host.pc))
    bar = max(1e-12, 100 * _pc_roundoff(pb, state, x, host, multigrid))
    print(f"CN={CN} mg={multigrid}: pc rel_err {e:.2e}, bar {bar:.2e}")
    assert e <= bar, e


def _compare_runs(pb, make, **kw):
    ref = picard.incompressible_non_linear_solve(pb, make("host"), device=True,
                                                 print_error_non_linear=False, **kw)
    out = picard.incompressible_non_linear_solve(pb, make("device"), device=True,
                                                 print_error_non_linear=False, **kw)
    print("norms", ref["norms"], out["norms"], "its", ref["linear_iterations"],
          out["linear_iterations"])
    assert len(out["norms"]) == len(ref["norms"])
    assert out["linear_iterations"] == ref["linear_iterations"]
    assert out["converged"] == ref["converged"]
    for a, b in zip(out["norms"], ref["norms"]):
        assert abs(a - b) <= 1e-8 * b
    for key in ("v", "zeta", "p", "mu"):
        assert out[key].shape == ref[key].shape
        assert np.abs(out[key] - ref[key]).max() <= 1e-9 * max(1.0, np.abs(ref[key]).max()), key
    return ref, out


@pytest.mark.parametrize("multigrid", [False, True])
@pytest.mark.parametrize("CN", [False, True])
def test_same_picard_run_cavity(CN, multigrid):
    pb, v_init, lid = common.navier_stokes_cavity_problem(n=8, n_t=10, CN=CN)
    pb.nu = 1.0 / 100.0
    ref, out = _compare_runs(pb, lambda b: _solver(pb, b, multigrid), v=v_init)
    assert out["converged"]
    th = pb.disc
    assert np.array_equal(out["v"][:, th.boundary_v], v_init[:, th.boundary_v])


def test_same_picard_run_manufactured():
    """tests/test_picard.py's manufactured problem at N = 16 (nu = 1/50, estimated sub-solve
    ellipses)."""
    pb, v0, true_v = common.mms_navier_stokes_control(16, CN=False, n_t=30, nu=1.0 / 50.0)
    sp = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 200,
          "relative_tolerance": 1.0e-7, "absolute_tolerance": 1.0e-7,
          "monitor_convergence": False}
    auto = (-1, 0.0, 0.0)
    specs = dict(mass=(20, 0.3924, 2.0598), schur=auto, kp=auto, mp=(20, 0.5, 2.0))
    ref, out = _compare_runs(pb, lambda b: _solver(pb, b, specs=specs, sp=sp), v=v0,
                             max_non_linear_iter=10, relative_non_linear_tol=1.0e-6,
                             absolute_non_linear_tol=1.0e-6)
    assert out["converged"]


@pytest.mark.parametrize("CN", [False, True])
def test_no_host_assembly(CN, monkeypatch):
    pb, v_init, lid = common.navier_stokes_cavity_problem(n=8, n_t=6, CN=CN)

    def refuse(*a, **k):
        raise AssertionError("host assembly on the device build path")
    monkeypatch.setattr(type(pb), "D_v", refuse)
    monkeypatch.setattr(type(pb), "D_p", refuse)
    monkeypatch.setattr(picard, "instationary_incompressible_blocks", refuse)
    ls = _solver(pb, "device")
    out = picard.incompressible_non_linear_solve(pb, ls, device=True, v=v_init,
                                                 print_error_non_linear=False)
    assert out["converged"] and len(out["linear_iterations"]) >= 2
    assert ls.uploads == 0


def test_unset_blocks_are_refused():
    """An argument check on the host side of the call: nothing is launched."""
    pb = common.navier_stokes_problem(n=4, n_t=3)
    th = pb.disc
    rng = np.random.default_rng(common.SEED)
    M = th.M_p.tocsr()
    M.sort_indices()
    pat = PatternOnly(M.indptr, M.indices, M.shape)
    none = {(i, j): None for i in range(2) for j in range(2)}
    b00 = dict(none)
    b00[(0, 0)] = M
    b00[(1, 1)] = pat
    b01 = dict(none)
    b01[(1, 0)] = pat
    sys_ = MultiBlockSystem(th.n_p, th.n_p, b00, b01, dict(none), dict(none), n_blocks_00=2,
                            n_blocks_11=2)
    lib, h = sys_._lib, sys_.handle
    assert sys_.info()["blocks_unset"] == 2 and sys_.info()["n_blocks_stored"] == 3
    x = rng.standard_normal(sys_.local_size)
    y = np.full_like(x, 7.0)
    f64 = lambda a: a.ctypes.data_as(_lib.c_f64p)
    assert lib.kkt_apply(h, f64(x), f64(y)) == -3                 # KKT_ERR_STATE
    assert b"(0, 1, 1)" in lib.kkt_last_error(h)
    assert np.all(y == 7.0)
    assert lib.kkt_pc_apply(h, f64(x), f64(y)) == -3
    d = C.c_void_p()
    sys_._ck(lib.kkt_vec_alloc(h, C.byref(d)))
    try:
        assert lib.kkt_apply_device(h, d, d) == -3
        its, reason, nh, rnorm = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        assert lib.kkt_solve_device(h, d, d, C.byref(its), C.byref(reason), C.byref(rnorm),
                                    None, 0, C.byref(nh)) == -3
    finally:
        lib.kkt_vec_free(h, d)
    with pytest.raises(_lib.KktError) as err:
        sys_.mult(x)
    assert err.value.code == -3 and "(0, 1, 1)" in str(err.value)
    sys_.update_block_values(0, 1, 1, M)
    assert sys_.info()["blocks_unset"] == 1
    assert lib.kkt_apply(h, f64(x), f64(y)) == -3
    assert b"(1, 1, 0)" in lib.kkt_last_error(h)
    sys_.update_block_values(1, 1, 0, 2.0 * M)
    assert sys_.info()["blocks_unset"] == 0
    n = th.n_p
    want = np.concatenate([M @ x[:n], M @ x[n:2 * n] + 2.0 * (M @ x[2 * n:3 * n]),
                           np.zeros(2 * n)])
    assert common.rel_err(sys_.mult(x), want) <= 1e-14


@pytest.mark.parametrize("CN", [False, True])
def test_unset_count_goes_down_with_composition(CN):
    """The three handles of a device build before any composition: every block but the
    ``tau B`` couplings is unset, the preconditioner set-up is refused, and each composition
    clears its handle."""
    from control_amd.blocks import instationary_build_recipes
    pb = common.navier_stokes_problem(n=4, n_t=4, CN=CN)
    rng = np.random.default_rng(common.SEED)
    state = _iterate(pb, rng)
    ls = _solver(pb, "device")
    full = instationary_build_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
    composed = []
    from control_amd import relinearise
    real = relinearise.DeviceRelinearisation.relinearise

    def watch(self, system, name, recipes=None):
        before = system.info()["blocks_unset"]
        if name == "outer":
            with pytest.raises(_lib.KktError) as err:
                system.mult(np.zeros(system.local_size))
            assert err.value.code == -3
        real(self, system, name, recipes=recipes)
        composed.append((name, before, system.info()["blocks_unset"]))
    relinearise.DeviceRelinearisation.relinearise = watch
    try:
        ls.setup(*state)
    finally:
        relinearise.DeviceRelinearisation.relinearise = real
    assert composed == [(name, len(full[name]), 0) for name in ("outer", "inner", "commutator")]
