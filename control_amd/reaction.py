"""The scalar Picard / Gauss-Newton loop on the device (``kkt_set_reaction_relinearisation``,
DESIGN.md section 6.6a): ``Instationary.non_linear_solve(device=True)`` and
``Stationary.non_linear_solve(device=True)`` for a forward operator declared as a
``fem.ReactionTerm``, on P1 or P2 triangles, P1 tetrahedra or Q2 quadrilaterals, on one GPU or -- the instationary loop,
with ``comm=`` -- on time shards.

Host side: ``ReactionPlan`` -- the element tables of the term, the contribution lists that make
the device assembly deterministic (``relinearise.contribution_lists``), the transpose permutation
and the constant data rows of the residual -- and ``DeviceReaction``, a thin binding of the device
entry points.  ``device_non_linear_solve`` is the loop of ``Instationary.non_linear_solve`` with
one block system and one preconditioner kept alive and the iterate in HBM, and
``device_stationary_non_linear_solve`` that of ``Stationary.non_linear_solve``: the stationary
system is the plan with one level (``n_t = 1``), so both loops share every part but the driver.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .anderson import DeviceAnderson
from .fem import ReactionTerm
from .relinearise import (DevicePlanBinding, _marshal, _recipe_array, contribution_lists,
                          device_picard_loop, device_vectors, transpose_permutation)

__all__ = ["ReactionPlan", "DeviceReaction", "device_non_linear_solve",
           "device_stationary_non_linear_solve"]


def _check(ctl, P=None, comm=None, host_allreduce=None):
    """The ``ValueError``s of ``non_linear_solve(device=True)``: nothing here touches the GPU.
    A ``fem.ReactionTerm`` is on P1 or P2 triangles, P1 tetrahedra or Q2 quadrilaterals
    (``fem.rectangle_q2``) by construction (its own ``ValueError`` names them), and all four run
    here."""
    if comm is not None and comm.world > 1:
        if not callable(getattr(comm, "attach", None)):
            raise ValueError("comm must be a transport of control_amd.dist (it attaches itself to "
                             "the system)")
        if host_allreduce is None:
            raise ValueError("a time-sharded device loop needs host_allreduce")
    if not isinstance(ctl._forward, ReactionTerm):
        raise ValueError("device=True needs the forward operator declared as a fem.ReactionTerm")
    if P is not None:
        raise ValueError("device=True does not take P=: a host callback as preconditioner would "
                         "bring every application back to the host")
    if ctl._th is not None:
        raise ValueError("device=True is the scalar driver's: not for a Taylor-Hood discretisation")
    if ctl._forward.disc is not ctl._disc:
        raise ValueError("the ReactionTerm was declared on another discretisation")


class ReactionPlan:
    """Everything ``kkt_set_reaction_relinearisation`` uploads, built once per problem on the
    host from an ``Instationary`` or a ``Stationary`` whose forward operator is a
    ``fem.ReactionTerm``.  A ``Stationary`` gives the plan with one level: ``n_t = 1``,
    ``stationary`` set, ``tau`` unused."""

    def __init__(self, ctl):
        _check(ctl)
        term, disc = ctl._forward, ctl._disc
        self.ctl, self.term = ctl, term
        self.stationary = not hasattr(ctl, "_n_t")
        if self.stationary:
            self.n_t, self.CN, self.tau = 1, False, 0.0
        else:
            self.n_t, self.CN = ctl._n_t, ctl._CN
            _, _, self.tau = ctl._times()
        self.m = self.n_t - 1 if self.CN else self.n_t
        self.beta = ctl._beta
        #: the coefficients every D of the loop is built from (``construct_D_v``)
        self.coefficients = term.jacobian_coefficients if ctl._Gauss_Newton else term.coefficients
        self.lists = contribution_lists(term.cells, term.M)
        self.tperm = transpose_permutation(term.M)
        self.data = self._data_rows()

    def _data_rows(self):
        """The rows of ``non_linear_res_eval`` at the zero iterate: what does not depend on
        ``(v, zeta)`` -- desired state, forces, and backward Euler's initial-condition row
        ``tau D(v_0) v_0 + M v_0``.  Boundary values live in the iterate (``v`` keeps them on the
        Dirichlet dofs), and the Dirichlet rows of the residual are zero."""
        ctl, disc, n_t, tau = self.ctl, self.ctl._disc, self.n_t, self.tau
        if self.stationary:          # [M v_d | M f] of Stationary._data()
            rows = np.stack(ctl._data()).astype(np.float64)
            rows[:, disc.boundary] = 0.0
            return np.ascontiguousarray(rows)
        v_d, f = ctl.construct_v_d(), ctl.construct_f()
        if self.CN:
            h = 0.5 * tau
            r0 = np.stack([h * (v_d[i] + v_d[i + 1]) for i in range(self.m)])
            r1 = np.stack([h * (f[i] + f[i + 1]) for i in range(self.m)])
        else:
            t_0 = ctl._time_interval[0]
            v_0 = (np.zeros(disc.n_dofs) if ctl._initial_condition is None
                   else np.asarray(ctl._initial_condition(disc.coords), dtype=np.float64))
            r0 = tau * v_d
            r0[n_t - 1] = 0.0
            r1 = tau * f
            r1[0] = tau * (ctl.construct_D_v(v_0, t_0) @ v_0) + disc.M @ v_0
        r0[:, disc.boundary] = 0.0
        r1[:, disc.boundary] = 0.0
        return np.ascontiguousarray(np.concatenate([r0, r1]))

    def pattern(self):
        """``(indptr, indices)`` of every block: the structure of ``M``."""
        M = self.term.M
        return M.indptr.astype(np.int32), M.indices.astype(np.int32)

    def descriptor(self):
        """``kkt_reaction_desc`` over this plan's arrays (valid while ``keep`` lives).  ``nq``, the
        number of quadrature points of the term's rule, tells the library the element: 7 for P1
        triangles, 15 for P1 tetrahedra, 25 for P2 triangles and for Q2 quadrilaterals, which
        ``nv`` (the nodes per cell, 6 or 9) tells apart; the tables go as the term holds them
        (``lam``: ``term.basis``, the shape functions at the points)."""
        term, disc = self.term, self.ctl._disc
        i32, f64, keep = _marshal()
        c = (C.c_double * 5)(*self.coefficients)
        d = _lib.ReactionDesc(
            n_t=self.n_t, cn=int(self.CN), nq=term.W.shape[1], nv=term.nv, ne=len(term.cells),
            n1=disc.n_dofs, tau=float(self.tau), beta=float(self.beta), cells=i32(term.cells),
            W=f64(term.W), lam=f64(term.basis), nnz=term.M.nnz, indptr=i32(term.M.indptr),
            indices=i32(term.M.indices), tperm=i32(self.tperm), cptr=i32(self.lists[0]),
            clist=i32(self.lists[1]), L=f64(term.L.data), M=f64(term.M.data),
            degree=len(self.coefficients) - 1, c=c, n_bc=len(disc.boundary),
            bc_idx=i32(disc.boundary), data=f64(self.data))
        return d, keep


def owned(recipes, lo, hi):
    """The recipes of the block rows ``[lo, hi)`` (``(q, i, j, ...)``: row ``i``)."""
    return [r for r in recipes if lo <= r[1] < hi]


class DeviceReaction(DevicePlanBinding):
    """The plan on a scalar instationary (or, a stationary plan, stationary)
    ``MultiBlockSystem`` and the iterate in HBM -- a stationary plan's as one level, ``(1, n)``.

    On a time-sharded system every rank keeps its own levels of the iterate, of the element
    matrices and of ``D`` (``window``), assembles, evaluates the residual of and updates those, and
    trades one level of ``v`` and one of ``zeta`` with its neighbours before every assembly;
    ``assemble``, ``residual`` and ``get_state`` are then collective."""

    _SET, _WINDOW = "kkt_set_reaction_relinearisation", "kkt_reaction_window"
    _STATE, _RESIDUAL = "kkt_reaction_state", "kkt_reaction_residual_device"
    _UPDATE, _DEBUG = "kkt_reaction_update_device", "kkt_debug_reaction_array"

    def __init__(self, ctl, system, recipes=None, plan=None, host_allreduce=None):
        """``recipes``: the blocks every re-linearisation rewrites (default: the ``"inner"`` list
        of ``blocks.instationary_relinearisation_recipes``, on a time shard those of the rank's
        own block rows; a stationary plan: ``blocks.stationary_relinearisation_recipes``).  ``host_allreduce(array, op)`` (a time shard): what ``get_state`` gathers
        the iterate with."""
        from .blocks import (instationary_relinearisation_recipes,
                             stationary_relinearisation_recipes)
        self.plan = ReactionPlan(ctl) if plan is None else plan
        self.ctl, self.system = ctl, system
        self._attach(system, host_allreduce)
        if recipes is None:
            p = self.plan
            recipes = owned(
                stationary_relinearisation_recipes(p.beta) if p.stationary else
                instationary_relinearisation_recipes(p.tau, p.beta, p.n_t, p.CN)["inner"],
                *self.window["blocks"])
        self.recipes = (_recipe_array(recipes, 0), len(recipes))

    def _block_shapes(self):
        """``v``, ``zeta``."""
        return ((self.plan.n_t, self.ctl._disc.n_dofs),) * 2

    def _debug_arrays(self):
        """``kkt_debug_reaction_array``: ``"E"`` (n_t, ne, nv, nv) or ``"D"`` (n_t, nnz) of the
        last assembly, ``"v"`` / ``"zeta"`` (n_t, n) of the iterate (P1 or P2 triangles, P1
        tetrahedra, Q2 quadrilaterals: ``nv`` = 3 or 6 nodes per triangle, 4 per tetrahedron, 9 per
        quadrilateral) -- on a time shard the levels of ``window["D"]``, ``window["v"]`` and
        ``window["zeta"]``, halo levels included."""
        n, (ne, nv) = self.ctl._disc.n_dofs, self.plan.term.cells.shape
        return {"E": ("D", (ne, nv, nv)), "D": ("D", (self.plan.term.M.nnz,)),
                "v": ("v", (n,)), "zeta": ("zeta", (n,))}

    def set_state(self, v, zeta):
        """Global arrays (a stationary plan's one level may come as a vector); a time shard takes
        its windows from them, halo levels included."""
        super().set_state(np.atleast_2d(v), np.atleast_2d(zeta))

    def assemble(self):
        """Element matrices and ``D`` of every level of the D window at the device iterate's
        ``v`` (a time shard first refreshes its halo levels from the neighbour ranks)."""
        self.system._ck(self._lib.kkt_reaction_relinearise(self.system.handle, self.system.handle,
                                                           1, 0, None))

    def relinearise(self, system=None, recipes=None):
        """Rewrite the recipe blocks of ``system`` (default: the plan's own) from the last
        assembly.  ``recipes``: another list for this call (the first build composes every
        block, ``blocks.instationary_build_recipes``)."""
        system = self.system if system is None else system
        arr, n = self.recipes if recipes is None else (_recipe_array(recipes, 0), len(recipes))
        system._ck(self._lib.kkt_reaction_relinearise(system.handle, self.system.handle, 0, n, arr))


def build_system(ctl, backend, plan, comm=None):
    """The scalar block system from patterns: every block of ``blocks.instationary_blocks`` (a
    stationary plan: of ``blocks.stationary_blocks``) is a ``PatternOnly`` of the structure of
    ``M``, in the row-major dict order of the host path.
    Returns ``(system, block dicts, build recipes)``; the blocks are unset until the device
    composes them.  ``comm``: a time shard registers the blocks of its own rows
    (``MultiBlockSystem`` skips the others), and the build recipes are those rows'."""
    from .blocks import instationary_build_recipes, stationary_build_recipes
    from .multiblock import PatternOnly
    disc, m = ctl._disc, plan.m
    full = (stationary_build_recipes(plan.beta) if plan.stationary else
            instationary_build_recipes(plan.tau, plan.beta, plan.n_t, plan.CN)["inner"])
    n = disc.n_dofs
    pat = PatternOnly(*plan.pattern(), (n, n))
    quads = [{(i, j): None for i in range(m) for j in range(m)} for _ in range(4)]
    for (q, i, j, *_) in full:
        quads[q][(i, j)] = pat
    ns = tuple(backend.DirichletBCNullspace(disc.boundary) for _ in range(m))
    kw = {} if comm is None or comm.world == 1 else {"comm": comm}
    system = backend.MultiBlockSystem(n, n, *quads, n_blocks_00=m, n_blocks_11=m, nullspace_0=ns,
                                      nullspace_1=ns, CN=plan.CN, **kw)
    if kw:
        full = owned(full, system._lo, system._hi)
    return system, quads, full


def device_non_linear_solve(ctl, *, P=None, solver_parameters=None, lambda_v_bounds=None,
                            max_non_linear_iter=10, relative_non_linear_tol=1.0e-5,
                            absolute_non_linear_tol=1.0e-8, print_error_non_linear=False,
                            backend=None, Multigrid=False, comm=None, host_allreduce=None,
                            anderson=0, anderson_beta=1.0):
    """``Instationary.non_linear_solve`` with the iterate in HBM.  One ``MultiBlockSystem`` is
    built from patterns and composed on the device, one ``SchurPC`` is attached to it; every
    iteration then assembles, evaluates the residual (the host reads its norm), re-composes the
    blocks that carry ``D`` (the preconditioner is marked stale and rebuilt by the next solve),
    solves and updates on the GPU.  The stopping logic is the host loop's.  The term may be on P1
    or P2 triangles, P1 tetrahedra or Q2 quadrilaterals; ``lambda_v_bounds`` stays the caller's, as
    in the reference (P2 triangles: ``(0.3924, 2.0598)``, ``test/test_control.py:3476``; Q2:
    ``(0.25, 1.5625)``, ``test/test_control.py:93``).

    ``comm`` (``control_amd.dist``): the system is time-sharded, every rank makes this call on the
    same global problem and runs the loop on its own levels (``DeviceReaction``); the first build
    is still by pattern, composed on the device from the rank's rows of the build recipes, so no
    block values ever cross from the host.  The boundary lift and the final download go through
    the collective ``get_state`` (``host_allreduce``): ``ctl._v`` and ``ctl._zeta`` end whole on
    every rank.

    ``anderson`` (depth 1..8; 0: off) and ``anderson_beta``: Anderson acceleration of the loop in
    update space by the device mixer (``control_amd.anderson``); not on
    time shards, not under ``set_Gauss_Newton()``.  ``non_linear_info["anderson"]``: per
    iteration the pairs used and dropped."""
    from .anderson import check_anderson
    from .control import GpuBackend, _multigrid_kw
    check_anderson(anderson, anderson_beta, comm, ctl._Gauss_Newton)
    _check(ctl, P, comm, host_allreduce)
    backend = backend or GpuBackend()
    if not isinstance(backend, GpuBackend):
        raise ValueError("device=True runs on a GpuBackend")
    disc, n_t, CN = ctl._disc, ctl._n_t, ctl._CN
    nodes = disc.boundary
    v_0 = (np.zeros(disc.n_dofs) if ctl._initial_condition is None
           else np.asarray(ctl._initial_condition(disc.coords), dtype=np.float64))
    v_old, zeta_old = ctl._v.copy(), ctl._zeta.copy()
    if CN:
        v_old[0] = v_0                                           # control.py:3425-3426
    zeta_old[n_t - 1] = 0.0
    # the values the iterate keeps on the Dirichlet dofs from the first update on (:3490-3493)
    v_fixed = v_old.copy()
    for i in range(n_t):
        v_fixed[i, nodes] = ctl._bc_values(i)[nodes]
    lift = not np.array_equal(v_fixed, v_old)

    plan = ReactionPlan(ctl)
    system, quads, full = build_system(ctl, backend, plan, comm)
    dev = DeviceReaction(ctl, system, plan=plan, host_allreduce=host_allreduce)
    dev.set_state(v_old, zeta_old)
    dev.assemble()
    dev.relinearise(recipes=full)
    pc_fn = backend.construct_pc("CN" if CN else "BE", plan.term.M, quads[1], quads[2], n_t,
                                 plan.tau, plan.beta, nodes, lambda_v_bounds or (0.5, 2.0),
                                 1.0e-3, **_multigrid_kw(disc, Multigrid))
    norms, lin_its, v_new, zeta_new, mixed = _run_loop(
        dev, pc_fn, solver_parameters, v_fixed if lift else None, relative_non_linear_tol,
        absolute_non_linear_tol, max_non_linear_iter, print_error_non_linear,
        anderson, anderson_beta)
    ctl._v, ctl._zeta = v_new, zeta_new
    ctl.non_linear_info = {"linear_iterations": lin_its, "window": dev.window, **mixed}
    return norms


def _run_loop(dev, pc_fn, solver_parameters, v_fixed, rtol, atol, max_iter, verbose,
              anderson=0, anderson_beta=1.0):
    """What both drivers do with a composed system: the first residual, ``device_picard_loop``
    and the download; the system is closed afterwards.  ``v_fixed`` (``(levels, n)``, or ``None``):
    the starting iterate did not carry these boundary values -- they are put in once, after the
    first update.  ``anderson > 0``: the loop's updates go through a ``DeviceAnderson`` on the
    system.  Returns ``(norms, linear iterations, v, zeta, info)``; ``info``: ``{"anderson": the
    mixer's (columns, dropped) per iteration}``, or empty without a mixer."""
    system, nodes = dev.system, dev.ctl._disc.boundary
    if solver_parameters is None:              # linear_solve's, control.py:3260-3266 and 556-562
        solver_parameters = {"linear_solver": "gmres", "gmres_restart": 10,
                             "maximum_iterations": 50, "relative_tolerance": 1.0e-6,
                             "absolute_tolerance": 0.0, "monitor_convergence": False}

    def solve(d_b, d_u):
        ksp = system.solve_device(d_b, d_u, solver_parameters=solver_parameters, pc_fn=pc_fn)
        return ksp.getIterationNumber()

    def lift_boundary():
        v_new, zeta_new = dev.get_state()
        v_new[:, nodes] = v_fixed[:, nodes]
        dev.set_state(v_new, zeta_new)
    try:
        mixer = DeviceAnderson(system, anderson, anderson_beta) if anderson else None
        with device_vectors(system) as (d_b, d_u):
            norm_0 = dev.residual(d_b, rhs=True)
            norms, lin_its = device_picard_loop(
                dev, d_b, d_u, norm_0, solve, dev.relinearise, True, rtol, atol, max_iter,
                verbose, after_first_update=lift_boundary if v_fixed is not None else None,
                mixer=mixer)
            v_new, zeta_new = dev.get_state()
    finally:
        system.close()
    return norms, lin_its, v_new, zeta_new, ({"anderson": mixer.history} if mixer else {})


def device_stationary_non_linear_solve(ctl, *, P=None, solver_parameters=None,
                                       lambda_v_bounds=None, max_non_linear_iter=10,
                                       relative_non_linear_tol=1.0e-5,
                                       absolute_non_linear_tol=1.0e-8,
                                       print_error_non_linear=False, backend=None,
                                       Multigrid=False, anderson=0, anderson_beta=1.0):
    """``Stationary.non_linear_solve`` with the iterate in HBM: the loop of
    ``device_non_linear_solve`` on the one-level plan.  One ``MultiBlockSystem`` of four
    ``PatternOnly`` blocks is composed on the device, one ``SchurPC(kind="stationary")`` is
    attached to it; every iteration assembles ``D`` at the device iterate, evaluates the rows of
    ``Stationary.non_linear_res_eval`` (they are the right-hand side), re-composes ``D^T`` and
    ``D`` (the preconditioner is marked stale and rebuilt by the next solve), solves and updates
    on the GPU.  P1 or P2 triangles, P1 tetrahedra, Q2 quadrilaterals; ``lambda_v_bounds`` is the
    caller's (P2 triangles: ``(0.3924, 2.0598)``, Q2: ``(0.25, 1.5625)``).  ``anderson``,
    ``anderson_beta``: as in ``device_non_linear_solve``."""
    from .anderson import check_anderson
    from .control import GpuBackend, _multigrid_kw
    check_anderson(anderson, anderson_beta, None, ctl._Gauss_Newton)
    _check(ctl, P)
    backend = backend or GpuBackend()
    if not isinstance(backend, GpuBackend):
        raise ValueError("device=True runs on a GpuBackend")
    disc, nodes = ctl._disc, ctl._disc.boundary
    v_old, zeta_old = ctl._v.copy(), ctl._zeta.copy()
    # the values the iterate keeps on the Dirichlet dofs from the first update on
    # (Stationary.non_linear_solve: v_old[boundary] = v_inhom[boundary], only with bcs_v)
    v_fixed = v_old.copy()
    if ctl._bcs_v is not None:
        v_fixed[nodes] = ctl._v_inhom()[nodes]
    lift = not np.array_equal(v_fixed, v_old)

    plan = ReactionPlan(ctl)
    system, quads, full = build_system(ctl, backend, plan)
    dev = DeviceReaction(ctl, system, plan=plan)
    dev.set_state(v_old, zeta_old)
    dev.assemble()
    dev.relinearise(recipes=full)
    pc_fn = backend.construct_pc("stationary", plan.term.M, quads[1], quads[2], 1, 0.0,
                                 plan.beta, nodes, lambda_v_bounds or (0.5, 2.0), 0.0,
                                 **_multigrid_kw(disc, Multigrid))
    norms, lin_its, v_new, zeta_new, mixed = _run_loop(
        dev, pc_fn, solver_parameters, v_fixed[None] if lift else None, relative_non_linear_tol,
        absolute_non_linear_tol, max_non_linear_iter, print_error_non_linear,
        anderson, anderson_beta)
    if lin_its:              # the host loop ends every iteration in set_v / set_zeta
        ctl.set_v(v_new[0])
        ctl.set_zeta(zeta_new[0])
    ctl.non_linear_info = {"linear_iterations": lin_its, "window": dev.window, **mixed}
    return norms
