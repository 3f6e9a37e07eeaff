"""``Multigrid=True`` on the drop-in drivers (the reference's keyword): the two-grid sub-solves
``bench.py`` measures, on the CPU oracle.  A backend that understands ``coarse=`` is defined
here; it builds what ``GpuBackend`` builds, with the oracle's ``coarse_chebyshev``."""
import numpy as np
import pytest
import scipy.sparse as sp

import common
from control_amd import firedrake_adapter as fa
from control_amd import picard
from control_amd.control import GpuBackend, coarse_space


class MultigridOracleBackend(common.OracleBackend):
    """``common.OracleBackend`` plus the two-grid forms of ``GpuBackend`` (same cycles and
    sweeps); records every coarse space it is handed."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.coarse_seen = []

    def _two_grid(self, sweeps, P, deflate=False):
        ko = self._ko
        return ko.ChebSpec(*sweeps, coarse=ko.CoarseSpace(P, GpuBackend.TWO_GRID_CYCLES,
                                                          deflate=deflate))

    def construct_pc(self, kind, M, block_01, block_10, n_t, tau, beta, nodes, lambda_v_bounds,
                     epsilon, coarse=None, sweeps=None):
        if coarse is None:
            return super().construct_pc(kind, M, block_01, block_10, n_t, tau, beta, nodes,
                                        lambda_v_bounds, epsilon)
        self.coarse_seen.append(coarse)
        ko = self._ko
        mass = ko.ChebSpec(20, *lambda_v_bounds)
        schur = self._two_grid(sweeps or GpuBackend.TWO_GRID_SWEEPS[kind], coarse)
        if kind == "stationary":
            return ko.pc_stationary(M, block_10[(0, 0)], block_01[(0, 0)], beta, nodes, mass,
                                    schur)
        if kind == "CN":
            return ko.pc_instationary_CN(M, block_01, block_10, n_t, tau, beta, nodes, mass,
                                         schur)
        return ko.pc_instationary_BE(M, block_01, block_10, n_t, tau, beta, nodes, mass, schur,
                                     epsilon=epsilon)

    def construct_stokes_pc(self, th, blocks, n_t, tau, beta, CN, lambda_v_bounds,
                            lambda_p_bounds, epsilon, coarse=None):
        if coarse is None:
            return common._oracle_backend_stokes_pc(self, th, blocks, n_t, tau, beta, CN,
                                                    lambda_v_bounds, lambda_p_bounds, epsilon)
        self.coarse_seen.append(coarse)
        ko = self._ko
        return ko.pc_instationary_incompressible(
            th.M_v, blocks["inner"], th.B, th.M_p, th.K_p, blocks["commutator"], n_t, tau, beta,
            th.boundary_v, ko.ChebSpec(20, *lambda_v_bounds),
            self._two_grid(GpuBackend.TWO_GRID_STOKES, coarse[0]),
            self._two_grid(GpuBackend.TWO_GRID_KP, coarse[1], deflate=True),
            ko.ChebSpec(20, *lambda_p_bounds), CN=CN, epsilon=epsilon)


@pytest.mark.parametrize("CN", [False, True])
def test_heat_linear_solve_with_multigrid(CN):
    """Same converged solution as the plain polynomials; the backend gets a coarse space with one
    row per dof and empty Dirichlet rows."""
    out = {}
    for mg in (False, True):
        ctl, disc, _, _ = common.mms_heat_control(16, CN)
        be = MultigridOracleBackend()
        ksp = ctl.linear_solve(solver_parameters=common.MMS_SOLVER_PARAMETERS,
                               lambda_v_bounds=(0.5, 2.0), backend=be, Multigrid=mg)
        assert ksp.reason > 0
        out[mg] = (ctl._v.copy(), ctl._zeta.copy(), ksp.its, be.coarse_seen)
    assert out[False][3] == []                   # the default hands the backend nothing new
    (P,) = out[True][3]
    assert P.shape[0] == disc.n_dofs and 4 <= P.shape[1] < disc.n_dofs
    assert np.all(np.diff(sp.csr_matrix(P).indptr)[disc.boundary] == 0)
    for a, b in zip(out[True][:2], out[False][:2]):
        assert common.rel_err(a, b) < 1e-8
    print(f"{'CN' if CN else 'BE'}: FGMRES iterations two-grid {out[True][2]}, plain "
          f"{out[False][2]}")


@pytest.mark.parametrize("CN", [False, True])
def test_stokes_linear_solve_with_multigrid(CN):
    out = {}
    for mg in (False, True):
        ctl, th, _, _ = common.mms_stokes_control_instationary(8, CN)
        be = MultigridOracleBackend(schur=(40, 0.01, 2.3))
        ksp = ctl.incompressible_linear_solve(solver_parameters=common.MMS_SOLVER_PARAMETERS,
                                              lambda_v_bounds=(0.3924, 2.0598),
                                              lambda_p_bounds=(0.5, 2.0), backend=be,
                                              Multigrid=mg)
        assert ksp.reason > 0
        out[mg] = (ctl._v.copy(), ctl._zeta.copy(), ksp.its, be.coarse_seen)
    assert out[False][3] == []
    ((Pv, Pp),) = out[True][3]
    assert Pv.shape[0] == th.n_v and Pp.shape[0] == th.n_p
    # one copy of the coarse functions per velocity component: P_v is block diagonal
    Pv = sp.csr_matrix(Pv)
    nn, nc = th.n_v // 2, Pv.shape[1] // 2
    assert Pv.shape[1] == 2 * nc
    assert Pv[:nn, nc:].nnz == 0 and Pv[nn:, :nc].nnz == 0
    assert np.all(np.diff(Pv.indptr)[th.boundary_v] == 0)
    for a, b in zip(out[True][:2], out[False][:2]):
        assert common.rel_err(a, b) < 1e-8
    print(f"{'CN' if CN else 'BE'}: FGMRES iterations two-grid {out[True][2]}, plain "
          f"{out[False][2]}")


def test_stationary_linear_solve_with_multigrid():
    from control_amd.control import Stationary
    from control_amd.fem import rectangle_p1
    disc = rectangle_p1(16, 16, 2.0, 2.0)
    sols = {}
    for mg in (False, True):
        ctl = Stationary(disc, desired_state=lambda X: np.sin(X[:, 0]) * X[:, 1], beta=1e-2)
        be = MultigridOracleBackend()
        ksp = ctl.linear_solve(solver_parameters=common.MMS_SOLVER_PARAMETERS,
                               lambda_v_bounds=(0.5, 2.0), backend=be, Multigrid=mg)
        assert ksp.reason > 0 and len(be.coarse_seen) == int(mg)
        sols[mg] = np.concatenate([ctl._v, ctl._zeta])
    assert common.rel_err(sols[True], sols[False]) < 1e-8


def test_multigrid_needs_a_backend_that_takes_the_coarse_space():
    """``coarse=`` reaches the backend only with ``Multigrid=True``: a backend without two-grid
    support keeps working with the default and says so with it."""
    ctl, _, _, _ = common.mms_heat_control(8, False)
    with pytest.raises(TypeError, match="coarse"):
        ctl.linear_solve(solver_parameters=common.MMS_SOLVER_PARAMETERS,
                         lambda_v_bounds=(0.5, 2.0), backend=common.OracleBackend(),
                         Multigrid=True)


def test_coarse_space_sizes():
    """33^2 functions on 256^2 P1 and per component on 128^2 P2 (bench.py --coarse-cell 8 /
    --kp-coarse-cell 4); 9^3 on 64^3; small meshes a coarse grid of about twice their mesh width."""
    from control_amd.fem import rectangle_p1, rectangle_p2p1, unit_cube_p1, unit_square_p1
    sd = unit_square_p1(256)
    assert coarse_space(sd.coords, sd.boundary).shape == (sd.n_dofs, 33 ** 2)
    th = rectangle_p2p1(128, 128)
    assert coarse_space(th.coords_v, th.boundary_v, copies=2).shape == (th.n_v, 2 * 33 ** 2)
    assert coarse_space(th.coords_p).shape == (th.n_p, 33 ** 2)
    cube = unit_cube_p1(64)
    assert coarse_space(cube.coords, cube.boundary).shape == (cube.n_dofs, 9 ** 3)
    small = rectangle_p1(8, 8, 2.0, 2.0)        # 9^2 nodes: a coarse grid of 4 x 4 cells
    assert coarse_space(small.coords, small.boundary).shape[1] == 5 ** 2


def test_firedrake_adapter_coarse_space_from_the_interpolated_coordinates(monkeypatch):
    """Nodes of a vector space own ``block_size`` consecutive dofs: P's rows follow that numbering,
    component k of every node interpolates from copy k of the coarse functions, and the rows of
    the boundary condition's dofs are empty -- inhomogeneous conditions included."""
    th = __import__("control_amd.fem", fromlist=["rectangle_p2p1"]).rectangle_p2p1(16, 16)
    X = np.asarray(th.coords_v)
    nn = len(X)

    class Space:
        block_size = 2

        def mesh(self):
            return "mesh"

    seen = []

    def coords(space):
        seen.append(space)
        return X
    monkeypatch.setattr(fa, "_coordinates", coords)
    V = Space()
    bnodes = np.asarray(th.boundary_v[:len(th.boundary_v) // 2])

    class BC:
        nodes, function_arg = bnodes, 1.0

        def function_space(self):
            return V
    P = sp.csr_matrix(fa.coarse_space(V, BC()))
    assert seen == [V] and P.shape[0] == 2 * nn
    ref = sp.csr_matrix(coarse_space(X, th.boundary_v, copies=2))      # component-major
    perm = np.arange(2 * nn).reshape(2, nn).T.ravel()                  # interleaved dof -> row
    assert (P - ref[perm]).nnz == 0
    empty = np.diff(P.indptr) == 0
    assert empty[2 * bnodes].all() and empty[2 * bnodes + 1].all()
    assert empty.sum() == 2 * len(bnodes)


def test_picard_multigrid_keyword():
    """``Multigrid=True`` needs a linear solver built with it; ``GpuLinearSolver`` takes the
    keyword and defaults the sweeps of a cycle (nothing touches the GPU before the first
    solve)."""
    pb = common.navier_stokes_problem(n=4, n_t=4)
    with pytest.raises(ValueError, match="Multigrid"):
        picard.incompressible_non_linear_solve(pb, common.OracleLinearSolver(pb), Multigrid=True,
                                               print_error_non_linear=False)
    gls = picard.GpuLinearSolver(pb, Multigrid=True)
    assert gls.multigrid and gls.specs["kp"] == GpuBackend.TWO_GRID_KP
    assert gls.specs["schur"] == (-1, 0.0, 0.0)
    assert gls.solver_parameters["maximum_iterations"] == 100
    plain = picard.GpuLinearSolver(pb)
    assert not plain.multigrid and plain.specs["kp"] == (-1, 0.0, 0.0)
