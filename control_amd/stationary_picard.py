"""The stationary Navier-Stokes Picard loop on the device (``kkt_set_relinearisation`` with
``n_t = 1``): ``Stationary.incompressible_non_linear_solve(device=True)``
for a forward operator declared as a ``fem.ConvectionTerm``.

The outer system, the velocity KKT system and the pressure commutator system are built once from
patterns and composed on the device (``blocks.stationary_incompressible_build_recipes``), one
``StokesPC`` is attached to the live handles, and every iteration assembles ``D_v`` / ``D_p`` at
the device iterate, evaluates the rows of the host loop's ``evaluate()`` (they are the right-hand
side), re-composes ``D^T`` and ``D`` on the three handles (the preconditioner is marked stale and
rebuilt by the next solve), solves and updates on the GPU.  The host reads one norm per iteration
and the fields once at the end.
"""
from __future__ import annotations

import numpy as np

from .fem import ConvectionTerm
from .relinearise import (DeviceRelinearisation, RelinearisationPlan, device_picard_loop,
                          device_vectors)

__all__ = ["StationaryNavierStokes", "build_systems", "attach_pc",
           "device_stationary_incompressible_non_linear_solve"]


def _check(ctl, forward_operator_p=None, P=None, backend=None):
    """The ``ValueError``s of ``incompressible_non_linear_solve(device=True)``: nothing here
    touches the GPU."""
    from .control import GpuBackend
    th, term = ctl._th, ctl._forward
    if th is None:
        raise ValueError("Undefined space_p")
    if not isinstance(term, ConvectionTerm):
        raise ValueError("device=True needs the forward operator declared as a fem.ConvectionTerm")
    if P is not None:
        raise ValueError("device=True does not take P=: a host callback as preconditioner would "
                         "bring every application back to the host")
    if forward_operator_p is not None and forward_operator_p != term.pressure:
        raise ValueError("device=True assembles the pressure-space operator of the ConvectionTerm: "
                         "forward_operator_p must be None or its pressure")
    if getattr(th, "elem", None) is None:
        raise ValueError("device=True needs a discretisation with element data "
                         "(fem.rectangle_p2p1 or fem.rectangle_q2q1)")
    if term.disc is not th:
        raise ValueError("the ConvectionTerm was declared on another discretisation")
    if backend is not None and not isinstance(backend, GpuBackend):
        raise ValueError("device=True runs on a GpuBackend")


class StationaryNavierStokes:
    """What ``RelinearisationPlan`` / ``DeviceRelinearisation`` read of a problem, for a
    ``Stationary`` on a Taylor-Hood discretisation with a ``fem.ConvectionTerm``: one level
    (``n_t = 1``, ``m = 1``), no time step, and the data rows ``[M v_d | M f]``."""

    stationary, n_t, CN, tau = True, 1, False, 0.0

    def __init__(self, ctl):
        _check(ctl)
        self.ctl, self.disc = ctl, ctl._th
        self.nu, self.beta = ctl._forward.nu, ctl._beta

    def data_rows(self):
        return np.stack(self.ctl._data())


def build_systems(pb, backend, plan, nullspace_p=None):
    """``(outer, inner, commutator)`` from patterns: every velocity- and pressure-space block of
    ``stationary_incompressible_blocks`` / ``stationary_blocks`` is a ``PatternOnly`` of the
    plan's pattern, in the row-major dict order of the host path; ``B^T`` / ``B`` go by value, one
    value set each.  The blocks stay unset until the device composes them."""
    from .blocks import _csr
    from .multiblock import PatternOnly
    th = pb.disc
    pat_v = PatternOnly(*plan.velocity_pattern(), (th.n_v, th.n_v))
    pat_p = PatternOnly(*plan.pressure_pattern(), (th.n_p, th.n_p))
    B = _csr(th.B)
    B_T = _csr(B.T)
    keys = [(0, 0), (0, 1), (1, 0), (1, 1)]
    nsv = tuple(backend.DirichletBCNullspace(th.boundary_v) for _ in range(2))
    nsp = tuple((nullspace_p.__class__() if nullspace_p is not None
                 else backend.ConstantNullspace()) for _ in range(2))
    outer = backend.MultiBlockSystem(
        th.n_v, th.n_p, {k: pat_v for k in keys},
        {(0, 0): B_T, (0, 1): None, (1, 0): None, (1, 1): B_T},
        {(0, 0): B, (0, 1): None, (1, 0): None, (1, 1): B}, {k: None for k in keys},
        n_blocks_00=2, n_blocks_11=2, nullspace_0=nsv, nullspace_1=nsp)
    inner = backend.MultiBlockSystem(th.n_v, th.n_v, *({(0, 0): pat_v} for _ in range(4)),
                                     nullspace_0=nsv[:1], nullspace_1=nsv[:1])
    if getattr(th, "coords_v", None) is not None and 2 * len(th.coords_v) == th.n_v:
        inner.set_tile_coordinates(np.vstack([th.coords_v, th.coords_v]))
    comm = backend.MultiBlockSystem(th.n_p, th.n_p, *({(0, 0): pat_p} for _ in range(4)))
    return outer, inner, comm


def attach_pc(pb, backend, inner, comm, lambda_v_bounds=None, lambda_p_bounds=None,
              Multigrid=False):
    """The ``StokesPC`` of ``GpuBackend.construct_stokes_pc_stationary`` over the live inner and
    commutator handles (``b_scale = post_scale = 1``, ``n_p_blocks = 1``)."""
    from .control import _multigrid_stokes_kw
    from .multiblock import ChebSpec, StokesPC
    th = pb.disc
    coarse = _multigrid_stokes_kw(th, Multigrid).get("coarse")
    kw = {} if coarse is None else dict(coarse=coarse[0], sweeps=backend.TWO_GRID_STOKES)
    inner_pc = backend.construct_pc("stationary", th.M_v, None, None, 1, 0.0, pb.beta,
                                    th.boundary_v, lambda_v_bounds or (0.3924, 2.0598), 0.0, **kw)
    return StokesPC(inner=inner, inner_pc=inner_pc, commutator=comm, B=th.B, K_p=th.K_p,
                    M_p=th.M_p, kp=backend._kp(inner_pc, coarse),
                    mp=ChebSpec(20, *(lambda_p_bounds or (0.5, 2.0))))


def device_stationary_incompressible_non_linear_solve(
        ctl, nullspace_p=None, *, forward_operator_p=None, P=None, solver_parameters=None,
        lambda_v_bounds=None, lambda_p_bounds=None, max_non_linear_iter=10,
        relative_non_linear_tol=1.0e-5, absolute_non_linear_tol=1.0e-8,
        print_error_non_linear=False, backend=None, Multigrid=False, anderson=0,
        anderson_beta=1.0):
    """``Stationary.incompressible_non_linear_solve`` with the iterate in HBM; returns the
    residual norms (initial one first) and leaves ``_v``, ``_zeta``, ``_p``, ``_mu`` and
    ``non_linear_info`` on ``ctl``.  ``anderson > 0``: the updates go through the device mixer
    on the outer system (``control_amd.anderson``)."""
    from .anderson import DeviceAnderson, check_anderson
    check_anderson(anderson, anderson_beta, None, getattr(ctl, "_Gauss_Newton", False))
    from .blocks import (stationary_incompressible_build_recipes,
                         stationary_incompressible_relinearisation_recipes)
    from .control import GpuBackend
    backend = backend or GpuBackend()
    _check(ctl, forward_operator_p, P, backend)
    th, nodes = ctl._th, ctl._disc.boundary
    v_old, zeta_old = ctl._v.copy(), ctl._zeta.copy()
    p_old = getattr(ctl, "_p", np.zeros(th.n_p)).copy()
    mu_old = getattr(ctl, "_mu", np.zeros(th.n_p)).copy()
    # the values the iterate keeps on the Dirichlet dofs from the first update on (the host loop:
    # v_old[nodes] = v_inhom[nodes], only with bcs_v)
    v_fixed = v_old.copy()
    if ctl._bcs_v is not None:
        v_fixed[nodes] = ctl._v_inhom()[nodes]
    lift = not np.array_equal(v_fixed, v_old)
    if solver_parameters is None:              # incompressible_linear_solve's
        solver_parameters = {"linear_solver": "fgmres", "fgmres_restart": 10,
                             "maximum_iterations": 100, "relative_tolerance": 1.0e-6,
                             "absolute_tolerance": 0.0, "monitor_convergence": False}

    pb = StationaryNavierStokes(ctl)
    plan = RelinearisationPlan(pb)
    full = stationary_incompressible_build_recipes(pb.beta)
    systems = build_systems(pb, backend, plan, nullspace_p)
    outer, inner, comm = systems
    named = ((outer, "outer"), (inner, "inner"), (comm, "commutator"))
    try:
        dev = DeviceRelinearisation(
            pb, outer, stationary_incompressible_relinearisation_recipes(pb.beta), plan=plan)
        dev.set_state(v_old[None], zeta_old[None], p_old[None], mu_old[None])
        dev.assemble()
        for system, name in named:
            dev.relinearise(system, name, recipes=full[name])
        pc = attach_pc(pb, backend, inner, comm, lambda_v_bounds, lambda_p_bounds, Multigrid)

        def solve(d_b, d_u):
            ksp = outer.solve_device(d_b, d_u, solver_parameters=solver_parameters, pc_fn=pc)
            return ksp.getIterationNumber()

        def relinearise():
            for system, name in named:
                dev.relinearise(system, name)

        def lift_boundary():
            v, zeta, p, mu = dev.get_state()
            v[:, nodes] = v_fixed[nodes]
            dev.set_state(v, zeta, p, mu)
        mixer = DeviceAnderson(outer, anderson, anderson_beta) if anderson else None
        with device_vectors(outer) as (d_b, d_u):
            norm_0 = dev.residual(d_b, rhs=True)
            norms, lin_its = device_picard_loop(
                dev, d_b, d_u, norm_0, solve, relinearise, True, relative_non_linear_tol,
                absolute_non_linear_tol, max_non_linear_iter, print_error_non_linear,
                after_first_update=lift_boundary if lift else None, mixer=mixer)
            v_new, zeta_new, p_new, mu_new = dev.get_state()
    finally:
        for system in systems:
            system.close()
    if lin_its:              # the host loop ends every iteration in set_v / set_zeta
        ctl.set_v(v_new[0])
        ctl.set_zeta(zeta_new[0])
        ctl._p, ctl._mu = p_new[0].copy(), mu_new[0].copy()
    ctl.non_linear_info = {"linear_iterations": lin_its, "window": dev.window}
    if mixer is not None:
        ctl.non_linear_info["anderson"] = mixer.history
    return norms
