"""Picard outer loop of instationary Navier-Stokes control (BE and CN).

Host-side mirror of ``Control.Instationary.incompressible_non_linear_solve``
(``control/control.py:4886-5232``): evaluate the non-linear residual at the current iterate
(``:2442-2620`` for the velocity rows, ``:4976-5082`` for the pressure couplings), solve the
linearised Stokes-control system for the update (``incompressible_linear_solve`` with the
convection term frozen at ``v_old``, ``construct_D_v`` ``:1887-1896``), add it, repeat until
``||r_k|| <= max(rtol ||r_0||, atol)`` or ``max_non_linear_iter``.

The loop, the residual and the re-assembly of the convection blocks stay on the host, as in
the reference; each outer iteration re-uploads only the values of the blocks that changed
(``kkt_update_block_values``: same sparsity structure, no index traffic, preconditioner
matrices refreshed on the device) and runs the linear solve on the GPU through
``MultiBlockSystem.solve`` with a ``StokesPC``.

Dirichlet velocity conditions: the updates vanish on the boundary (``bcs_v`` homogenised,
``bcs_zeta``); inhomogeneous, time-dependent values ride on the initial iterate ``v`` the
caller passes (``control.py:4925-4959`` applies the conditions to ``v_old`` before the loop),
as in the lid-driven cavity of ``test/test_control.py:4171-4268``.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from .blocks import instationary_incompressible_blocks

__all__ = ["NavierStokesControl", "GpuLinearSolver", "incompressible_non_linear_solve",
           "non_linear_res_eval"]


@dataclass
class NavierStokesControl:
    """What ``Control.Instationary`` holds for this driver: the Taylor-Hood discretisation,
    ``forward_form = nu (grad u, grad v) + ((w . grad) u, v)`` (``test_control.py:4194-4199``),
    nodal desired states ``v_d[i]`` and forces ``f[i]`` per time level, the initial
    condition, ``beta`` and the time interval."""
    disc: object
    nu: float
    beta: float
    n_t: int
    T: float
    v_d: np.ndarray                      # (n_t, n_v)
    f: np.ndarray                        # (n_t, n_v)
    v_0: np.ndarray = None               # (n_v,), zero when omitted
    t_0: float = 0.0
    CN: bool = False                     # Crank-Nicolson instead of backward Euler

    @property
    def tau(self):
        return (self.T - self.t_0) / (self.n_t - 1.0)

    def D_v(self, w):
        """``construct_D_v(v_trial, v_test, w, t)`` (Picard, ``control.py:1888-1889``)."""
        return _same_structure_sum(self.disc.K_v, [(self.nu, self.disc.K_v),
                                                   (1.0, self.disc.convection_v(w))])

    def D_p(self, w):
        """The same form on the pressure space (``control.py:3783-3785``)."""
        return _same_structure_sum(self.disc.K_p, [(self.nu, self.disc.K_p),
                                                   (1.0, self.disc.convection_p(w))])


def _apply_T_1(b):            # preconditioner.py:33-45
    out = b.copy()
    out[:-1] += b[1:]
    return out


def _apply_T_2(b):            # preconditioner.py:48-60
    out = b.copy()
    out[1:] += b[:-1]
    return out


def _same_structure_sum(like, terms):
    """``sum c_k A_k`` on the structure of ``like`` (explicit zeros kept, so the result can
    replace a stored block's values entry by entry)."""
    data = np.zeros_like(like.data)
    for c, A in terms:
        if A.nnz != like.nnz or not (np.array_equal(A.indptr, like.indptr)
                                     and np.array_equal(A.indices, like.indices)):
            raise ValueError("matrices assembled over different connectivities")
        data += c * A.data
    return sp.csr_matrix((data, like.indices.copy(), like.indptr.copy()), shape=like.shape)


def non_linear_res_eval(pb: NavierStokesControl, D, v, zeta, p, mu):
    """Residual rows of the BE Navier-Stokes control system at ``(v, zeta, p, mu)``
    (``control.py:2456-2620`` + ``5003-5041``); ``D[i] = D_v(v[i])``.  Returns
    ``(rhs_00, rhs_01, rhs_10, rhs_11)`` with Dirichlet rows zeroed (``bc.apply``)."""
    th, n_t, tau, beta = pb.disc, pb.n_t, pb.tau, pb.beta
    M, B = th.M_v, th.B
    BT = sp.csr_matrix(B.T)
    v_0 = np.zeros(th.n_v) if pb.v_0 is None else pb.v_0
    if pb.CN:
        # control.py:2621-2808 + 5043-5082: row i couples the levels i and i + 1; v[0] is the
        # initial condition, zeta[n_t - 1] = 0; mu, p live on the n_t - 1 intervals
        m, h = n_t - 1, 0.5 * tau
        r00 = np.zeros((m, th.n_v))
        r01 = np.zeros((m, th.n_v))
        for i in range(m):
            r00[i] = (h * (M @ (pb.v_d[i] + pb.v_d[i + 1])) - h * (M @ (v[i] + v[i + 1]))
                      - (h * (D[i].T @ zeta[i]) + M @ zeta[i])
                      - (h * (D[i + 1].T @ zeta[i + 1]) - M @ zeta[i + 1])
                      - tau * (BT @ mu[i]))
            r01[i] = (h * (M @ (pb.f[i] + pb.f[i + 1]))
                      - (h * (D[i] @ v[i]) - M @ v[i])
                      - (h * (D[i + 1] @ v[i + 1]) + M @ v[i + 1])
                      + (h / beta) * (M @ (zeta[i] + zeta[i + 1]))
                      - tau * (BT @ p[i]))
        r00[:, th.boundary_v] = 0.0
        r01[:, th.boundary_v] = 0.0
        r10 = np.stack([-(B @ v[i + 1]) for i in range(m)])
        r11 = np.stack([-(B @ zeta[i]) for i in range(m)])
        return r00, r01, r10, r11
    r00 = np.zeros((n_t, th.n_v))
    r01 = np.zeros((n_t, th.n_v))
    for i in range(n_t):
        Dz = tau * (D[i].T @ zeta[i]) + M @ zeta[i]
        if i < n_t - 1:          # :2469-2497, :2552-2584
            r00[i] = tau * (M @ pb.v_d[i]) - tau * (M @ v[i]) - Dz + M @ zeta[i + 1]
        else:                    # :2541-2546
            r00[i] = -Dz
        Dv = tau * (D[i] @ v[i]) + M @ v[i]
        if i == 0:               # :2499-2512: the initial-condition row
            # v_0 omitted: D0 multiplies zeros, any finite matrix gives the same +0.0 rows --
            # no assembly (a given initial condition costs this one, for a constant data row)
            D0 = D[0] if pb.v_0 is None else pb.D_v(v_0)
            r01[0] = tau * (D0 @ v_0) + M @ v_0 - Dv
        else:                    # :2518-2540, :2586-2615
            r01[i] = (tau * (M @ pb.f[i]) + M @ v[i - 1] - Dv
                      + (tau / beta) * (M @ zeta[i]))
        r00[i] -= tau * (BT @ mu[i])        # :5004-5012
        r01[i] -= tau * (BT @ p[i])         # :5017-5025
    r00[:, th.boundary_v] = 0.0
    r01[:, th.boundary_v] = 0.0
    r10 = np.stack([-(B @ v[i]) for i in range(n_t)])       # :5030-5034
    r11 = np.stack([-(B @ zeta[i]) for i in range(n_t)])    # :5036-5041
    return r00, r01, r10, r11


_DEFAULT_SOLVER_PARAMETERS = {"linear_solver": "fgmres", "fgmres_restart": 10,
                              "maximum_iterations": 100, "relative_tolerance": 1.0e-6,
                              "absolute_tolerance": 0.0, "monitor_convergence": False}


class GpuLinearSolver:
    """The linearised solve of one Picard iteration on the GPU: builds the outer, inner
    (velocity KKT) and commutator (pressure) systems once, afterwards only re-uploads the
    values of the blocks that carry the re-linearised operator.

    ``Multigrid=True`` (the reference's keyword): the velocity sub-solves and the ``K_p`` solve
    take their two-grid form -- ``GpuBackend.TWO_GRID_CYCLES`` x [Galerkin correction on the
    coarse space of ``control.coarse_space`` (33^2 functions per velocity component; the
    pressure space's with the constants deflated), Chebyshev sweeps].  ``schur`` and ``kp`` are
    then the sweeps of a cycle.  Their default for the velocity blocks, which carry the
    convection term, is ``(-1, 0, 0)``: per level matrix the library estimates ``emax`` and the
    ellipse's imaginary semi-axis and sweeps 8 times on ``[emax / 30, emax]`` -- the upper part of
    the spectrum, which the two-grid form needs (pc.cpp, ``SchurPC`` matrix set-up).  Explicit
    ``(its, emin, emax, eimag)`` bounds replace the estimates.  ``kp`` defaults to 12 sweeps on
    ``[0.05, 2.1]``.  Without ``Multigrid`` both default to ``(-1, 0, 0)``: plain polynomials
    from the spectrum estimates.  Every re-linearisation rebuilds the ``2 n_t`` coarse
    inverses on the device (``coarse_setup_stats`` of ``self.inner``)."""

    def __init__(self, pb: NavierStokesControl, *, mass=(20, 0.3924, 2.0598), schur=None,
                 kp=None, mp=(20, 0.5, 2.0), solver_parameters=None, device=0, comm=None,
                 host_allreduce=None, options=None, Multigrid=False, relinearise="host",
                 build="host"):
        """``comm`` (``control_amd.dist``): the three systems are time-sharded (BASELINE
        configs[4] names 8 GPUs) -- every rank runs the same Picard loop on the whole iterate
        (residual and re-linearisation are host work on replicated data, as cheap as in the
        reference), uploads the blocks of its own levels, solves for its shard of the update,
        and the shards are summed into the whole update with ``host_allreduce(array, op)``
        (in place over ranks, op 0 = sum: e.g. ``GlooTransport.allreduce``).

        ``relinearise="device"``: ``incompressible_non_linear_solve(..., device=True)`` keeps the
        Picard iterate in HBM -- the first linear solve builds the three systems (``build``),
        every later re-linearisation re-assembles the convection blocks, the
        residual and the update on the GPU (``control_amd.relinearise``).  Needs the element
        data of ``fem.rectangle_p2p1`` or ``fem.rectangle_q2q1``.  With ``comm`` every rank keeps, assembles, evaluates and
        updates its own time levels only and trades one level of ``v`` and one of ``zeta`` (CN:
        and the boundary residual rows) with its neighbours per iteration; ``host_allreduce``
        then only gathers the fields once at the end.

        ``build="device"`` (with ``relinearise="device"``): the first build crosses to the GPU
        as patterns, the constant matrices of the plan and the starting iterate only --
        ``_build_device`` registers every block of the three systems by its structure
        (``PatternOnly``; ``tau B`` / ``tau B^T`` excepted: one value set each) and the device
        composes them all (``blocks.instationary_build_recipes``).  No ``D_v`` / ``D_p`` assembly
        and no block sums on the host.  Not with ``comm``: registering the blocks of a time
        shard by pattern is not supported."""
        if relinearise not in ("host", "device"):
            raise ValueError("relinearise must be 'host' or 'device'")
        if build not in ("host", "device"):
            raise ValueError("build must be 'host' or 'device'")
        if build == "device" and relinearise != "device":
            raise ValueError("build='device' needs relinearise='device'")
        if comm is not None and comm.world > 1 and not callable(getattr(comm, "attach", None)):
            raise ValueError("comm must be a transport of control_amd.dist (it attaches itself to "
                             "the three systems)")
        if build == "device" and comm is not None and comm.world > 1:
            raise ValueError("build='device' does not support time-sharded solvers (comm): "
                             "use build='host' with relinearise='device'")
        if relinearise == "device":
            if getattr(pb.disc, "elem", None) is None:
                raise ValueError("relinearise='device' needs a discretisation with element data "
                                 "(fem.rectangle_p2p1 or fem.rectangle_q2q1)")
        self.relinearise, self.build = relinearise, build
        self.setup_s = None             # wall time of setup(): the builds and the preconditioner
        self._device = None             # control_amd.relinearise.DeviceRelinearisation
        self.solve_times = []           # (start, end) perf_counter of every linearised solve
        self.pb, self.device = pb, device
        from .control import GpuBackend
        self.options = options          # execution options of the three systems (kkt_set_option)
        self.multigrid = bool(Multigrid)
        if kp is None:
            kp = GpuBackend.TWO_GRID_KP if self.multigrid else (-1, 0.0, 0.0)
        self.specs = dict(mass=mass, schur=(-1, 0.0, 0.0) if schur is None else schur, kp=kp,
                          mp=mp)
        self.solver_parameters = (dict(_DEFAULT_SOLVER_PARAMETERS) if solver_parameters is None
                                  else solver_parameters)
        self.outer = None
        self.uploads = 0
        self.dist = comm if comm is not None and comm.world > 1 else None
        self.host_allreduce = host_allreduce
        if self.dist is not None and host_allreduce is None:
            raise ValueError("a time-sharded GpuLinearSolver needs host_allreduce")

    def _blocks(self, D, Dp):
        th, pb = self.pb.disc, self.pb
        return instationary_incompressible_blocks(th.M_v, list(D), th.B, th.M_p, list(Dp),
                                                  pb.tau, pb.beta, pb.n_t, pb.CN)

    def _build(self, bl):
        self._build_systems(bl)
        self._attach_pc(bl["m"])

    def _build_systems(self, bl):
        from .multiblock import ConstantNullspace, DirichletBCNullspace, MultiBlockSystem
        th, pb, m = self.pb.disc, self.pb, bl["m"]
        nsv = DirichletBCNullspace(th.boundary_v)
        kw = dict(sub_n_blocks_00_0=m, sub_n_blocks_11_0=m) if pb.CN else {}
        self.outer = MultiBlockSystem(
            th.n_v, th.n_p, *bl["outer"], n_blocks_00=2 * m, n_blocks_11=2 * m,
            nullspace_0=(nsv,) * (2 * m),
            nullspace_1=tuple(ConstantNullspace() for _ in range(2 * m)), device=self.device,
            CN=pb.CN, comm=self.dist, shard_families=2, options=self.options, **kw)
        self.inner = MultiBlockSystem(th.n_v, th.n_v, *bl["inner"], n_blocks_00=m,
                                      n_blocks_11=m, nullspace_0=(nsv,) * m,
                                      nullspace_1=(nsv,) * m, device=self.device, CN=pb.CN,
                                      comm=self.dist, options=self.options)
        if getattr(th, "coords_v", None) is not None and 2 * len(th.coords_v) == th.n_v:
            self.inner.set_tile_coordinates(np.vstack([th.coords_v, th.coords_v]))
        self.comm = MultiBlockSystem(th.n_p, th.n_p, *bl["commutator"], n_blocks_00=m,
                                     n_blocks_11=m, device=self.device, comm=self.dist,
                                     options=self.options)

    def _attach_pc(self, m):
        from .multiblock import ChebSpec, SchurPC, StokesPC
        th, pb = self.pb.disc, self.pb
        s = self.specs
        schur, kp = ChebSpec(*s["schur"]), ChebSpec(*s["kp"])
        if self.multigrid:
            from .control import GpuBackend, coarse_space
            from .multiblock import CoarseSpace
            Xv = np.asarray(th.coords_v)
            cycles = GpuBackend.TWO_GRID_CYCLES
            schur.coarse = CoarseSpace(coarse_space(Xv, th.boundary_v, copies=th.n_v // len(Xv)),
                                       cycles)
            kp.coarse = CoarseSpace(coarse_space(th.coords_p), cycles)
        inner_pc = SchurPC(kind="CN" if pb.CN else "BE", M=th.M_v, beta=pb.beta, bc_nodes=th.boundary_v,
                           mass=ChebSpec(*s["mass"]), schur=schur, n_t=pb.n_t, tau=pb.tau)
        self.pc = StokesPC(inner=self.inner, inner_pc=inner_pc, commutator=self.comm, B=th.B,
                           K_p=th.K_p, M_p=th.M_p, kp=kp, mp=ChebSpec(*s["mp"]),
                           n_p_blocks=m, b_scale=pb.tau, post_scale=1.0 / pb.tau**2, cn=pb.CN)

    def _build_device(self, v, zeta, p, mu):
        """The three systems from patterns: every velocity- and pressure-space block is a
        ``PatternOnly`` of the plan's pattern, in the dict order of
        ``instationary_incompressible_blocks`` (row-major: the apply order); the plan goes on the
        finalized outer handle, the iterate is uploaded, ``D`` assembled and all blocks composed.
        The preconditioner descriptors come last: their set-up reads composed values."""
        from .blocks import (_csr, instationary_build_recipes,
                             instationary_relinearisation_recipes)
        from .multiblock import PatternOnly
        from .relinearise import DeviceRelinearisation, RelinearisationPlan
        pb, th = self.pb, self.pb.disc
        plan = RelinearisationPlan(pb)
        full = instationary_build_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
        m = full["m"]
        pat_v = PatternOnly(*plan.velocity_pattern(), (th.n_v, th.n_v))
        pat_p = PatternOnly(*plan.pressure_pattern(), (th.n_p, th.n_p))

        def dicts(n, recipes, pat):
            quads = [{(i, j): None for i in range(n) for j in range(n)} for _ in range(4)]
            for (q, i, j, *_) in recipes:
                quads[q][(i, j)] = pat
            return quads
        outer = dicts(2 * m, full["outer"], pat_v)
        tB = _csr(pb.tau * sp.csr_matrix(th.B))
        tBT = _csr(tB.T)
        for i in range(2 * m):
            outer[1][(i, i)] = tBT
            outer[2][(i, i)] = tB
        self._build_systems({"outer": outer, "inner": dicts(m, full["inner"], pat_v),
                             "commutator": dicts(m, full["commutator"], pat_p), "m": m})
        recipes = instationary_relinearisation_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
        self._device = dev = DeviceRelinearisation(pb, self.outer, recipes, plan=plan)
        dev.set_state(v, zeta, p, mu)
        dev.assemble()
        for system, name in ((self.outer, "outer"), (self.inner, "inner"),
                             (self.comm, "commutator")):
            dev.relinearise(system, name, recipes=full[name])
        self._attach_pc(m)

    def setup(self, v, zeta, p, mu):
        """Everything before the first linearised solve at the iterate ``(v, zeta, p, mu)``: the
        three systems (``build="host"``: host assembly, block sums, uploads; ``"device"``:
        ``_build_device``) and the preconditioner's set-up.  ``setup_s``: its wall time."""
        t0 = time.perf_counter()
        if self.build == "device":
            self._build_device(v, zeta, p, mu)
        else:
            n_t = self.pb.n_t
            self._build(self._blocks([self.pb.D_v(v[i]) for i in range(n_t)],
                                     [self.pb.D_p(v[i]) for i in range(n_t)]))
        self.outer._set_pc(self.pc)
        self.setup_s = time.perf_counter() - t0

    def _update(self, bl):
        """Blocks that carry the linearised operator: all of ``block_01_int`` / ``block_10_int``
        (``control.py:3806-3808`` BE, ``3851-3885`` CN; the pure mass couplings among them are
        re-sent unchanged), their copies inside the outer ``block_00``, and the
        pressure-space analogues."""
        m = bl["m"]
        i00, i01, i10, i11 = bl["inner"]
        c00, c01, c10, c11 = bl["commutator"]
        own = self._owns
        for (i, j), A in i01.items():          # -> outer block_00 (i, m + j)
            if A is not None and own(i):
                self.inner.update_block_values(1, i, j, A)
                self.outer.update_block_values(0, i, m + j, A)
                self.uploads += 2
        for (i, j), A in i10.items():          # -> outer block_00 (m + i, j)
            if A is not None and own(i):
                self.inner.update_block_values(2, i, j, A)
                self.outer.update_block_values(0, m + i, j, A)
                self.uploads += 2
        for q, blk in ((1, c01), (2, c10)):
            for (i, j), A in blk.items():
                if A is not None and own(i):
                    self.comm.update_block_values(q, i, j, A)
                    self.uploads += 1

    def _owns(self, level):
        """Block rows of time level ``level`` live on this rank."""
        return self.dist is None or self.inner._lo <= level < self.inner._hi

    def linear_solve(self, D, Dp, b_0, b_1):
        if self.outer is None and self.build == "device":
            raise RuntimeError("a build='device' solver is set up from the iterate: setup(), or "
                               "incompressible_non_linear_solve(..., device=True)")
        bl = self._blocks(D, Dp)
        if self.outer is None:
            self._build(bl)
        else:
            self._update(bl)
        u_0 = np.zeros_like(b_0)
        u_1 = np.zeros_like(b_1)
        if self.dist is None:
            t0 = time.perf_counter()
            ksp = self.outer.solve(u_0, u_1, b_0, b_1, solver_parameters=self.solver_parameters,
                                   pc_fn=self.pc)
            self.solve_times.append((t0, time.perf_counter()))
            return u_0, u_1, ksp.getIterationNumber()
        # this rank's levels of both block families of a variable: rows [lo, hi) and m + [lo, hi)
        m, lo, hi = bl["m"], self.inner._lo, self.inner._hi
        pick = list(range(lo, hi)) + list(range(m + lo, m + hi))
        l_0, l_1 = np.zeros_like(b_0[pick]), np.zeros_like(b_1[pick])
        t0 = time.perf_counter()
        ksp = self.outer.solve(l_0, l_1, np.ascontiguousarray(b_0[pick]),
                               np.ascontiguousarray(b_1[pick]),
                               solver_parameters=self.solver_parameters, pc_fn=self.pc)
        self.solve_times.append((t0, time.perf_counter()))
        u_0[pick], u_1[pick] = l_0, l_1
        for u in (u_0, u_1):            # the other ranks' rows are zero here: a sum gathers
            flat = u.reshape(-1)
            self.host_allreduce(flat, 0)
        return u_0, u_1, ksp.getIterationNumber()


    # -- the device loop (relinearise="device")
    def device_plan(self):
        """The re-linearisation plan on the outer system (built after the first solve)."""
        if self._device is None:
            from .blocks import instationary_relinearisation_recipes
            from .relinearise import DeviceRelinearisation
            pb = self.pb
            recipes = instationary_relinearisation_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
            m = recipes["m"]        # (outer block rows: both families by their time level)
            recipes = {name: [r for r in recipes[name] if self._owns(r[1] % m)]
                       for name in ("outer", "inner", "commutator")}
            self._device = DeviceRelinearisation(pb, self.outer, recipes,
                                                 host_allreduce=self.host_allreduce)
        return self._device

    def device_relinearise(self):
        """Rewrite the linearised blocks of the outer, inner and commutator systems from the
        plan's last assembly (``_update`` of the host path; a time shard: the blocks of its own
        rows, as ``_update``'s ``own``)."""
        dev = self.device_plan()
        dev.relinearise(self.outer, "outer")
        dev.relinearise(self.inner, "inner")
        dev.relinearise(self.comm, "commutator")

    def device_solve(self, d_b, d_u):
        t0 = time.perf_counter()
        ksp = self.outer.solve_device(d_b, d_u, solver_parameters=self.solver_parameters,
                                      pc_fn=self.pc)
        self.solve_times.append((t0, time.perf_counter()))
        return ksp.getIterationNumber()


def _device_non_linear_solve(pb, ls, v, zeta, p, mu, max_non_linear_iter, rtol, atol,
                             print_error_non_linear, anderson=0, anderson_beta=1.0):
    """``incompressible_non_linear_solve`` with the iterate in HBM: per iteration one assembly
    of the convection blocks, one residual (the host reads its norm), one linearised solve and
    one update, all on the device -- on a time-sharded solver every rank on its own levels, the
    norm the same on all of them.  ``anderson > 0``: the updates go through the device mixer on
    the outer system, which is removed again afterwards (the solver outlives the call)."""
    from .anderson import DeviceAnderson
    from .relinearise import device_picard_loop, device_vectors
    fresh = ls.outer is None
    if fresh:                # the first call builds the systems (host blocks or patterns)
        ls.setup(v, zeta, p, mu)
    dev = ls.device_plan()
    dev.set_state(v, zeta, p, mu)
    mixer = DeviceAnderson(ls.outer, anderson, anderson_beta) if anderson else None
    try:
        with device_vectors(ls.outer) as (d_b, d_u):
            dev.assemble()
            norm_0 = dev.residual(d_b, rhs=True)
            if print_error_non_linear:
                print(f"Initial non-linear residual: {norm_0:.16e}")
            norms, lin_its = device_picard_loop(dev, d_b, d_u, norm_0, ls.device_solve,
                                                ls.device_relinearise, fresh, rtol, atol,
                                                max_non_linear_iter, print_error_non_linear,
                                                mixer=mixer)
            v, zeta, p, mu = dev.get_state()
    finally:
        if mixer is not None:
            mixer.close()
    norm_k = norms[-1]
    out = dict(v=v, zeta=zeta, p=p, mu=mu, norms=norms, linear_iterations=lin_its,
               converged=bool(norm_k <= rtol * norm_0 or norm_k <= atol))
    if mixer is not None:
        out["anderson"] = mixer.history
    return out


def incompressible_non_linear_solve(pb: NavierStokesControl, linear_solver=None, *,
                                    max_non_linear_iter=10, relative_non_linear_tol=1.0e-5,
                                    absolute_non_linear_tol=1.0e-8, v=None, zeta=None, p=None,
                                    mu=None, print_error_non_linear=True, Multigrid=False,
                                    device=False, anderson=0, anderson_beta=1.0):
    """``control.py:4886-5232`` (BE).  ``linear_solver.linear_solve(D, Dp, b_0, b_1)`` returns
    the update ``(u_0, u_1, iterations)`` of the linearised system whose forward operator at
    time level ``i`` is ``D[i]`` (velocity space) / ``Dp[i]`` (pressure space).  ``None``: a
    ``GpuLinearSolver(pb, Multigrid=Multigrid)`` with its defaults.  ``Multigrid=True`` with a
    given solver requires one built with ``Multigrid=True``.

    ``device=True``: the same loop with the iterate in HBM (residual, re-linearisation and
    update on the GPU; the host reads one norm per iteration and the fields once at the end).
    Needs a ``GpuLinearSolver(..., relinearise="device")`` (``None``: one is built).

    ``anderson`` (depth 1..8; 0, the default: off), ``anderson_beta``: Anderson acceleration of
    the loop in update space (``control_amd.anderson``): the flat update ``(u_0, u_1)`` is mixed
    with the last ``anderson`` secant pairs before it is added, on the GPU with ``device=True``,
    by the NumPy mirror otherwise.  ``ValueError`` on a time-sharded solver and outside 0..8.

    Returns a dict with the converged fields, the non-linear residual norms (``norm_0``
    first) and the linear iteration counts (with ``anderson > 0`` also ``anderson``: per
    iteration the pairs used and dropped)."""
    from .anderson import HostAnderson, check_anderson
    check_anderson(anderson, anderson_beta, getattr(linear_solver, "dist", None))
    if device and getattr(pb.disc, "elem", None) is None:
        raise ValueError("device=True needs a discretisation with element data "
                         "(fem.rectangle_p2p1 or fem.rectangle_q2q1)")
    if linear_solver is None:
        linear_solver = GpuLinearSolver(pb, Multigrid=Multigrid,
                                        relinearise="device" if device else "host")
    elif Multigrid and not getattr(linear_solver, "multigrid", False):
        raise ValueError("Multigrid=True: the linear solver was not built with Multigrid=True")
    if device and getattr(linear_solver, "relinearise", None) != "device":
        raise ValueError("device=True needs a GpuLinearSolver built with relinearise='device'")
    th, n_t, tau = pb.disc, pb.n_t, pb.tau
    m = n_t - 1 if pb.CN else n_t
    v = np.zeros((n_t, th.n_v)) if v is None else np.array(v, dtype=np.float64)
    zeta = np.zeros((n_t, th.n_v)) if zeta is None else np.array(zeta, dtype=np.float64)
    p = np.zeros((m, th.n_p)) if p is None else np.array(p, dtype=np.float64)
    mu = np.zeros((m, th.n_p)) if mu is None else np.array(mu, dtype=np.float64)
    if pb.CN:
        v[0] = np.zeros(th.n_v) if pb.v_0 is None else pb.v_0   # :4961-4962
    zeta[n_t - 1] = 0.0                                          # :4963
    if device:
        return _device_non_linear_solve(pb, linear_solver, v, zeta, p, mu, max_non_linear_iter,
                                        relative_non_linear_tol, absolute_non_linear_tol,
                                        print_error_non_linear, anderson, anderson_beta)
    mixer = HostAnderson(anderson, anderson_beta) if anderson else None

    def evaluate():
        D = [pb.D_v(v[i]) for i in range(n_t)]
        r = non_linear_res_eval(pb, D, v, zeta, p, mu)
        return D, r, float(np.sqrt(sum(np.vdot(x, x) for x in r)))

    D, (r00, r01, r10, r11), norm_0 = evaluate()
    norm_k = norm_0
    norms, lin_its = [norm_0], []
    if print_error_non_linear:
        print(f"Initial non-linear residual: {norm_0:.16e}")
    k = 0
    while norm_k > relative_non_linear_tol * norm_0 and norm_k > absolute_non_linear_tol:
        Dp = [pb.D_p(v[i]) for i in range(n_t)]
        s10, s11 = tau * r10, tau * r11                          # :5102-5105
        if pb.CN:    # the linear solve transforms the rows it is given (control.py:4266-4269)
            r00, r01 = _apply_T_1(r00), _apply_T_2(r01)
            s10, s11 = _apply_T_2(s10), _apply_T_1(s11)
        b_0 = np.concatenate([r00, r01])
        b_1 = np.concatenate([s10, s11])
        u_0, u_1, its = linear_solver.linear_solve(D, Dp, b_0, b_1)
        lin_its.append(its)
        if mixer is not None:
            u_0, u_1 = mixer.step(u_0, u_1)
        if pb.CN:                # unknown block i: v at level i + 1, zeta at level i
            v[1:] += u_0[:m]
            zeta[:m] += u_0[m:]
        else:
            v += u_0[:m]                                         # :5127-5147
            zeta += u_0[m:]
        zeta[:, th.boundary_v] = 0.0
        mu += u_1[:m]            # pressure blocks: mu with the v rows, p with the zeta rows
        p += u_1[m:]
        D, (r00, r01, r10, r11), norm_k = evaluate()
        norms.append(norm_k)
        k += 1
        if print_error_non_linear:
            print(f"Non-linear solver: iteration {k:d}, non-linear residual norm {norm_k:.16e}")
        if k + 1 > max_non_linear_iter:                          # :5186-5187
            break
    out = dict(v=v, zeta=zeta, p=p, mu=mu, norms=norms, linear_iterations=lin_its,
               converged=bool(norm_k <= relative_non_linear_tol * norm_0
                              or norm_k <= absolute_non_linear_tol))
    if mixer is not None:
        out["anderson"] = mixer.history
    return out
