"""``Multigrid=True`` on the GPU: the drivers' two-grid sub-solves with the default backend, the
Picard solver's two-grid form on convection blocks, and the component-block coarse set-up
(option "coarse_blocks") that the velocity spaces take."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import common
from control_amd import picard
from control_amd.control import GpuBackend, Instationary, coarse_space

pytestmark = pytest.mark.gpu

MASS = (20, 0.5, 2.0)
SCHUR = (8, 0.07, 2.1)


def _heat_control(n, n_t, CN, beta=1.0e-4, T=2.0):
    from control_amd.fem import unit_square_p1
    disc = unit_square_p1(n)

    def v_d(X, t):
        return np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.cos(t)
    return Instationary(disc, desired_state=v_d, beta=beta, CN=CN, n_t=n_t,
                        time_interval=(0.0, T))


def test_heat_linear_solve_256_squared_be():
    """256^2 x 64 BE (the bench's size): GMRES(10) to the driver's 1e-6 in at most 19 iterations
    with the two-grid sub-solves (the bench takes 17); the default keeps the plain polynomials
    (no coarse set-up on the handle)."""
    its = {}
    for mg in (True, False):
        ctl = _heat_control(256, 64, False)
        ksp = ctl.linear_solve(Multigrid=mg)
        its[mg] = ksp.getIterationNumber()
        assert ksp.getConvergedReason() > 0, (mg, its)
    print(f"256^2 x 64 BE GMRES(10) iterations: two-grid {its[True]}, plain {its[False]}")
    assert its[True] <= 19


def test_heat_linear_solve_cn_agrees_with_the_plain_polynomials():
    sols = {}
    sp_ = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 300,
           "relative_tolerance": 1e-10, "absolute_tolerance": 0.0, "monitor_convergence": False}
    for mg in (True, False):
        ctl = _heat_control(64, 16, True, beta=1e-2)
        ksp = ctl.linear_solve(Multigrid=mg, solver_parameters=sp_)
        assert ksp.getConvergedReason() > 0
        sols[mg] = np.concatenate([ctl._v, ctl._zeta])
    assert common.rel_err(sols[True], sols[False]) < 1e-7


def test_stokes_linear_solve_128_squared():
    """128^2 P2-P1 x 32 (BASELINE configs[2]): the outer FGMRES(10) converges to 1e-6 with two-grid
    velocity sub-solves and the two-grid K_p solve (the bench leg needed 108 iterations: above
    the driver's default of 100, so 200 here)."""
    from control_amd.fem import rectangle_p2p1
    th = rectangle_p2p1(128, 128, 2.0, 2.0)

    def v_d(X, t):
        x, y = X[:, 0] - 1.0, X[:, 1] - 1.0
        s = (1.0 - x * x) * (1.0 - y * y)
        return np.concatenate([s * y, -s * x]) * np.cos(t)
    ctl = Instationary(th, desired_state=v_d, beta=1.0e-3, CN=False, n_t=32,
                       time_interval=(0.0, 2.0))
    sp_ = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 200,
           "relative_tolerance": 1.0e-6, "absolute_tolerance": 0.0, "monitor_convergence": False}
    t0 = time.time()
    ksp = ctl.incompressible_linear_solve(solver_parameters=sp_, Multigrid=True)
    print(f"128^2 P2-P1 x 32, Multigrid=True: {ksp.getIterationNumber()} FGMRES(10) iterations, "
          f"{time.time() - t0:.1f} s with assembly")
    assert ksp.getConvergedReason() > 0


def _ns_blocks(pb, v):
    from control_amd.blocks import instationary_incompressible_blocks
    th = pb.disc
    D = [pb.D_v(v[i]) for i in range(pb.n_t)]
    Dp = [pb.D_p(v[i]) for i in range(pb.n_t)]
    return D, Dp, instationary_incompressible_blocks(th.M_v, D, th.B, th.M_p, Dp, pb.tau,
                                                     pb.beta, pb.n_t, pb.CN)


@pytest.mark.parametrize("CN", [False, True])
def test_picard_two_grid_sub_solves_match_the_oracle(CN):
    """16^2 P2-P1, n_t = 8, nu = 1/100, linearised about a non-zero velocity (every level its own
    convection block): the velocity block-Schur preconditioner with two-grid sub-solves on an
    explicit ellipse applies as the oracle's."""
    from oracle import kkt_oracle as ko
    pb, v_init, _ = common.navier_stokes_cavity_problem(n=16, n_t=8, CN=CN)
    th = pb.disc
    v = v_init + 0.5 * pb.v_d
    D, Dp, bl = _ns_blocks(pb, v)
    ell = (8, 0.1, 2.3, 0.4)
    gls = picard.GpuLinearSolver(pb, Multigrid=True, schur=ell)
    gls._build(bl)
    m = bl["m"]
    x = common.rng_vector(2 * m * th.n_v)
    got = gls.inner.pc_apply(x, gls.pc.inner_pc)
    Pv = coarse_space(th.coords_v, th.boundary_v, copies=2)
    schur = ko.ChebSpec(*ell, coarse=ko.CoarseSpace(Pv, GpuBackend.TWO_GRID_CYCLES))
    i00, i01, i10, i11 = bl["inner"]
    nsv = tuple(ko.DirichletBCNullspace(th.boundary_v) for _ in range(m))
    osys = ko.OracleSystem(th.n_v, th.n_v, *bl["inner"], n_blocks_00=m, n_blocks_11=m,
                           nullspace_0=nsv, nullspace_1=nsv, CN=CN)
    f = ko.pc_instationary_CN if CN else ko.pc_instationary_BE
    kw = {} if CN else dict(epsilon=1.0e-3)
    opc = f(th.M_v, i01, i10, pb.n_t, pb.tau, pb.beta, th.boundary_v,
            ko.ChebSpec(*gls.specs["mass"]), schur, **kw)
    ref = osys.pc_apply(opc, x)
    st = gls.inner.coarse_setup_stats()
    assert st["blocks"] == 2 and st["block_n"] * 2 == Pv.shape[1]
    assert common.rel_err(got, ref) < 1e-9


@pytest.mark.parametrize("CN", [False, True])
def test_cavity_picard_with_multigrid(CN):
    """The lid-driven cavity of ``test/test_control.py:4171-4368`` at nu = 1/100 converges to
    1e-5 with ``Multigrid=True`` (6 BE / 4 CN Picard iterations without it)."""
    pb, v_init, _ = common.navier_stokes_cavity_problem(n=8, n_t=10, CN=CN)
    th = pb.disc
    sp_ = dict(common.NS_SOLVER_PARAMETERS, maximum_iterations=100)
    gls = picard.GpuLinearSolver(pb, solver_parameters=sp_, Multigrid=True)
    out = picard.incompressible_non_linear_solve(pb, gls, v=v_init, Multigrid=True,
                                                 print_error_non_linear=False)
    print(f"cavity {'CN' if CN else 'BE'} Multigrid=True: {len(out['norms']) - 1} Picard "
          f"iterations, FGMRES {out['linear_iterations']}")
    assert out["converged"] and len(out["norms"]) <= 8
    assert np.array_equal(out["v"][:, th.boundary_v], v_init[:, th.boundary_v])


def test_config5_linearised_solve_two_grid_and_plain():
    """BASELINE configs[4]: P2-P1 128 x 128, n_t = 64, nu = 1/100, linearised about a non-zero
    velocity (``test_gpu_full_size.py``'s shape).  FGMRES converges with the two-grid sub-solves;
    both counts, the coarse set-up times (component blocks against the whole matrix) and one
    rebuild against one linear solve are printed, not compared."""
    from oracle import kkt_oracle as ko
    t0 = time.time()
    pb = common.navier_stokes_problem(n=128, n_t=64, nu=1.0 / 100.0, beta=1.0e-2)
    th, n_t = pb.disc, pb.n_t
    v = 0.5 * pb.v_d
    D, Dp, bl = _ns_blocks(pb, v)
    m = bl["m"]
    osys = ko.OracleSystem(
        th.n_v, th.n_p, *bl["outer"], n_blocks_00=2 * m, n_blocks_11=2 * m,
        nullspace_0=tuple(ko.DirichletBCNullspace(th.boundary_v) for _ in range(2 * m)),
        nullspace_1=tuple(ko.ConstantNullspace() for _ in range(2 * m)))
    sp_ = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)
    rng = np.random.default_rng(common.SEED)
    x0 = rng.standard_normal((2 * m, th.n_v))
    x0[:, th.boundary_v] = 0.0
    x1 = rng.standard_normal((2 * m, th.n_p))
    x1 -= x1.mean(axis=1, keepdims=True)
    xs = osys.join(x0, x1)
    b = osys.mult(xs)
    b0, b1 = osys.split(b)
    print(f"\nconfig 5 assembly {time.time() - t0:.1f} s")
    res = {}
    for mg in (True, False):
        gls = picard.GpuLinearSolver(pb, mass=(20, 0.3924, 2.0598), solver_parameters=sp_,
                                     Multigrid=mg)
        t1 = time.time()
        u0, u1, its = gls.linear_solve(D, Dp, b0, b1)
        res[mg] = its
        r = b - osys.mult(osys.join(u0, u1))
        print(f"{'two-grid' if mg else 'plain ellipse'}: {its} FGMRES iterations, build and solve "
              f"{time.time() - t1:.1f} s, relative residual {np.linalg.norm(r) / np.linalg.norm(b):.2e}")
        assert np.linalg.norm(r) <= 2.0e-6 * np.linalg.norm(b)
        if mg:
            st = gls.inner.coarse_setup_stats()
            print("coarse set-up, component blocks:", st)
            assert st["matrices"] >= n_t and st["blocks"] == 2
            # one Picard re-linearisation: new values, rebuild (timed through the next solve)
            v2 = 0.6 * pb.v_d
            D2, Dp2, _ = _ns_blocks(pb, v2)
            t2 = time.time()
            gls.linear_solve(D2, Dp2, b0, b1)
            st2 = gls.inner.coarse_setup_stats()
            print(f"re-linearised solve {time.time() - t2:.1f} s, of which coarse set-up "
                  f"{st2['ms']:.0f} ms: {st2}")
            gls = None
    # the same build with the whole-matrix inverses (option coarse_blocks = 0), set-up only
    gfull = picard.GpuLinearSolver(pb, mass=(20, 0.3924, 2.0598), solver_parameters=sp_,
                                   Multigrid=True, options={"coarse_blocks": "0"})
    gfull._build(bl)
    gfull.inner.pc_apply(common.rng_vector(2 * m * th.n_v), gfull.pc.inner_pc)
    print("coarse set-up, whole matrices:", gfull.inner.coarse_setup_stats())
    print(f"config 5 FGMRES iterations: two-grid {res[True]}, plain ellipse {res[False]}")


# ------------------------------------------------------------- component-block set-up
def _two_component_convection_problem(n=40, n_t=6, beta=1e-4, scale=1.0):
    """``test_gpu_coarse_setup._convection_problem`` on a two-component space (component-major,
    each component its own copy of the per-level convection operator): the Galerkin matrices are
    block diagonal with two equal blocks."""
    from control_amd.blocks import instationary_blocks
    from control_amd.fem import unit_square_p1
    sd = unit_square_p1(n)
    K = sp.csr_matrix(sd.K)
    C = sp.triu(K, 1) - sp.tril(K, -1)
    I2 = sp.identity(2, format="csr")
    M2 = sp.kron(I2, sd.M, format="csr")
    T = 2.0
    tau = T / (n_t - 1.0)
    Ks = [sp.kron(I2, K + (0.1 * i) * sd.M + (0.3 * scale * (1 + i)) * C, format="csr")
          for i in range(n_t)]
    b00, b01, b10, b11, m = instationary_blocks(M2, Ks, tau, beta, n_t, False, share=True)

    class Sd:
        n_dofs = 2 * sd.n_dofs
    Sd.M = M2
    Sd.coords = np.vstack([sd.coords, sd.coords])
    nodes = np.concatenate([sd.boundary, sd.n_dofs + np.asarray(sd.boundary)])
    P = coarse_space(sd.coords, nodes, copies=2)
    return dict(sd=Sd, tau=tau, beta=beta, n_t=n_t, CN=False, m=m,
                blocks=(b00, b01, b10, b11), nodes=nodes), P


def _setup(p, P, blocks, keep=True, g=None):
    opts = {"coarse_keep": "1" if keep else "0", "coarse_blocks": blocks}
    g = g or common.gpu_system(p, options=opts)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    y = g.pc_apply(x, common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2)))
    return g, y


def test_block_setup_equals_the_full_matrix_inverses():
    p, P = _two_component_convection_problem()
    nc = P.shape[1]
    g1, y1 = _setup(p, P, "1")
    g0, y0 = _setup(p, P, "0")
    s1, s0 = g1.coarse_setup_stats(), g0.coarse_setup_stats()
    print("blocks:", s1, "\nwhole matrices:", s0)
    assert s1["blocks"] == 2 and s1["block_n"] * 2 == nc
    assert s0["blocks"] == 1 and s0["block_n"] == nc
    assert s1["matrices"] == s0["matrices"] >= p["n_t"]
    assert np.array_equal(g1.coarse_matrices(), g0.coarse_matrices())
    I1, I0 = g1.coarse_inverses(), g0.coarse_inverses()
    h = nc // 2
    for inv in (I1, I0):       # exact zeros outside the blocks, on both paths
        assert not inv[:, :h, h:].any() and not inv[:, h:, :h].any()
    # (not bit for bit: the 32-column panels of the elimination start at other columns)
    err = max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(I1, I0))
    print(f"block against whole-matrix inverses: {err:.1e}")
    assert err < 1e-12, err
    # fewer launches than the whole-matrix inverse: about 2 per 32-column panel of block_n
    assert s1["launches"] <= 2 * (-(-s1["block_n"] // 32)) + 8
    assert s1["launches"] <= s0["launches"]
    assert common.rel_err(y1, y0) < 1e-12


def test_scalar_space_keeps_one_block():
    p = common.heat_problem(n=32, n_t=4, beta=1e-4)
    from control_amd.coarse import multilinear_coarse_space
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=8)
    g, _ = _setup(p, P, "1", keep=False)
    st = g.coarse_setup_stats()
    assert st["blocks"] == 1 and st["block_n"] == P.shape[1]


def test_block_rebuild_after_update_block_values_equals_a_fresh_build():
    p, P = _two_component_convection_problem(n=24)
    q, _ = _two_component_convection_problem(n=24, scale=2.0)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    g = common.gpu_system(p, options={"coarse_keep": "1"})
    pc = common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2))
    before = g.pc_apply(x, pc)
    b10 = dict(p["blocks"][2])
    for i in range(p["n_t"]):
        g.update_block_values(2, i, i, q["blocks"][2][(i, i)])
        b10[(i, i)] = q["blocks"][2][(i, i)]
    rebuilt = g.pc_apply(x, pc)
    st = g.coarse_setup_stats()
    assert st["blocks"] == 2 and st["matrices"] >= p["n_t"]
    fresh_p = dict(p, blocks=(p["blocks"][0], p["blocks"][1], b10, p["blocks"][3]))
    gf = common.gpu_system(fresh_p, options={"coarse_keep": "1"})
    fresh = gf.pc_apply(x, common.gpu_pc(fresh_p, MASS, SCHUR, coarse=(P, 2)))
    assert common.rel_err(rebuilt, before) > 1e-6
    assert np.array_equal(g.coarse_inverses(), gf.coarse_inverses())
    assert np.array_equal(rebuilt, fresh)
