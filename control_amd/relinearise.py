"""Picard re-linearisation on the device (``kkt_set_relinearisation``).

Host side: the plan of a Taylor-Hood discretisation with element data (``fem.rectangle_p2p1``,
``fem.rectangle_q2q1``) --
element tables, the contribution lists that make the device assembly deterministic, transpose
permutations, the data rows of the residual -- and a thin binding of the device entry points.
The lists are CSR over stored positions: position ``k`` of the scalar P2 (P1) pattern sums the
flat element entries ``clist[cptr[k]:cptr[k + 1]]`` in that (ascending) order, which is the order
in which ``np.bincount`` sums them in ``fem.TaylorHoodDiscretisation.convection_v_data``.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib
from .fem import _row_positions

__all__ = ["contribution_lists", "gather", "transpose_permutation", "RelinearisationPlan",
           "DevicePlanBinding", "DeviceRelinearisation", "device_vectors", "device_picard_loop"]


def contribution_lists(conn, pattern):
    """``(cptr, clist)`` of the element matrices over connectivity ``conn`` (ne x k) on the
    sorted CSR ``pattern``: flat entry ``e k^2 + a k + b`` (row ``conn[e, a]``, column
    ``conn[e, b]``) contributes to the position of that pair."""
    conn = np.asarray(conn)
    k = conn.shape[1]
    rows = np.repeat(conn, k, axis=1).ravel()
    cols = np.tile(conn, (1, k)).ravel()
    pos = pattern.indptr[rows].astype(np.int64) + _row_positions(pattern, rows, cols)
    clist = np.argsort(pos, kind="stable").astype(np.int32)     # ascending within a position
    cptr = np.zeros(pattern.nnz + 1, dtype=np.int32)
    cptr[1:] = np.cumsum(np.bincount(pos, minlength=pattern.nnz))
    return cptr, clist


def gather(E, cptr, clist):
    """Reference gather: position ``k`` = the sum of ``E.ravel()[clist[cptr[k]:cptr[k + 1]]]``
    from 0.0, term by term in list order (what the device kernel does)."""
    E = np.ravel(E)
    counts = np.diff(cptr)
    out = np.zeros(len(counts))
    for t in range(int(counts.max()) if len(counts) else 0):
        has = counts > t
        out[has] += E[clist[cptr[:-1][has] + t]]
    return out


def transpose_permutation(A):
    """``perm[k]``: the position of the transposed entry of position ``k`` of a structurally
    symmetric sorted CSR matrix (``A^T.data = A.data[perm]``)."""
    A = sp.csr_matrix(A)
    n = A.nnz
    T = sp.csr_matrix((np.arange(1, n + 1, dtype=np.float64), A.indices, A.indptr),
                      shape=A.shape).T.tocsr()
    T.sort_indices()
    if not (T.nnz == n and np.array_equal(T.indptr, A.indptr)
            and np.array_equal(T.indices, A.indices)):
        raise ValueError("the pattern is not structurally symmetric")
    return (T.data.astype(np.int64) - 1).astype(np.int32)


def _marshal():
    """``(i32, f64, keep)``: pointers for a descriptor, into contiguous arrays that ``keep``
    holds alive."""
    keep = []

    def pointer(a, dtype, ctype):
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data_as(ctype)
    return (lambda a: pointer(a, np.int32, _lib.c_i32p),
            lambda a: pointer(a, np.float64, _lib.c_f64p), keep)


class RelinearisationPlan:
    """Everything ``kkt_set_relinearisation`` uploads, built once per problem on the host.
    ``pb``: a ``picard.NavierStokesControl``, or the stationary problem
    (``stationary_picard.StationaryNavierStokes``: ``n_t = 1``, ``m = 1``, ``tau`` unused)."""

    def __init__(self, pb):
        from .picard import non_linear_res_eval
        th = pb.disc
        if getattr(th, "elem", None) is None:
            raise ValueError("device re-linearisation needs a discretisation with element data "
                             "(fem.rectangle_p2p1 or fem.rectangle_q2q1)")
        e = th.elem
        n2 = th.n_v // 2
        K2 = th.K_v[:n2, :n2].tocsr()
        K2.sort_indices()
        M2 = th.M_v[:n2, :n2].tocsr()
        M2.sort_indices()
        if not (np.array_equal(M2.indptr, K2.indptr) and np.array_equal(M2.indices, K2.indices)):
            raise ValueError("M_v and K_v must share one sparsity structure")
        Kp, Mp = sp.csr_matrix(th.K_p), sp.csr_matrix(th.M_p)
        if not (np.array_equal(Mp.indptr, Kp.indptr) and np.array_equal(Mp.indices, Kp.indices)):
            raise ValueError("M_p and K_p must share one sparsity structure")
        self.pb, self.n2, self.K2, self.M2, self.Kp, self.Mp = pb, n2, K2, M2, Kp, Mp
        self.V = np.ascontiguousarray(e["V"], dtype=np.int32)
        self.P = np.ascontiguousarray(e["P"], dtype=np.int32)
        #: "p2p1" (triangles: per-cell physical gradients) or "q2q1" (quadrilaterals: the
        #: descriptor carries the reference gradients and the cells' inverse Jacobians)
        self.kind = e.get("kind", "p2p1")
        names = {"W": "W", "phi": "phi", "gphi": "gphi", "lam": "lam", "glam": "glam"}
        if self.kind == "q2q1":
            names.update(gphi="gref", glam="lref", jinv="jinv")
        self.tables = {k: np.ascontiguousarray(e[src], dtype=np.float64)
                       for k, src in names.items()}
        self.v_lists = contribution_lists(self.V, K2)
        self.p_lists = contribution_lists(self.P, Kp)
        self.v_tperm = transpose_permutation(K2)
        self.p_tperm = transpose_permutation(Kp)
        self.B = sp.csr_matrix(th.B)
        self.B.sort_indices()
        m = pb.n_t - 1 if pb.CN else pb.n_t
        self.m = m
        #: one level (``n_t = 1``): the stationary system; ``pb.data_rows()``: [M v_d | M f]
        self.stationary = bool(getattr(pb, "stationary", False))
        if self.stationary:
            self.data = np.ascontiguousarray(pb.data_rows(), dtype=np.float64)
            return
        z = np.zeros((pb.n_t, th.n_v))
        r00, r01, _, _ = non_linear_res_eval(pb, [th.K_v] * pb.n_t, z, z.copy(),
                                             np.zeros((m, th.n_p)), np.zeros((m, th.n_p)))
        self.data = np.ascontiguousarray(np.concatenate([r00, r01]))

    def velocity_pattern(self):
        """``(indptr, indices)`` of a velocity-space block: the scalar P2 pattern once per
        component, component-major (the structure of ``M_v`` / ``K_v``)."""
        ip, ix, nnz = self.K2.indptr, self.K2.indices, self.K2.nnz
        return (np.concatenate([ip, nnz + ip[1:]]).astype(np.int32),
                np.concatenate([ix, self.n2 + ix]).astype(np.int32))

    def pressure_pattern(self):
        return self.Kp.indptr.astype(np.int32), self.Kp.indices.astype(np.int32)

    def descriptor(self):
        """``kkt_relin_desc`` over this plan's arrays (valid while the plan lives)."""
        pb, th, t = self.pb, self.pb.disc, self.tables
        i32, f64, keep = _marshal()
        d = _lib.RelinDesc(
            n_t=pb.n_t, cn=int(bool(pb.CN)), nq=t["W"].shape[1], ne=len(self.V), n2=self.n2,
            n1=th.n_p, nu=float(pb.nu), tau=float(pb.tau), beta=float(pb.beta), V=i32(self.V),
            W=f64(t["W"]), phi=f64(t["phi"]), gphi=f64(t["gphi"]), lam=f64(t["lam"]),
            glam=f64(t["glam"]), nnz2=self.K2.nnz, v_indptr=i32(self.K2.indptr),
            v_indices=i32(self.K2.indices), v_tperm=i32(self.v_tperm),
            v_cptr=i32(self.v_lists[0]), v_clist=i32(self.v_lists[1]), K2=f64(self.K2.data),
            M2=f64(self.M2.data), nnz1=self.Kp.nnz, p_indptr=i32(self.Kp.indptr),
            p_indices=i32(self.Kp.indices), p_tperm=i32(self.p_tperm),
            p_cptr=i32(self.p_lists[0]), p_clist=i32(self.p_lists[1]), Kp=f64(self.Kp.data),
            Mp=f64(self.Mp.data), nnz_b=self.B.nnz, b_indptr=i32(self.B.indptr),
            b_indices=i32(self.B.indices), b_values=f64(self.B.data),
            n_bc=len(th.boundary_v), bc_idx=i32(th.boundary_v), data=f64(self.data))
        if self.kind == "q2q1":
            d.nv, d.jinv = self.V.shape[1], f64(t["jinv"])
        return d, keep


def _recipe_array(recipes, space):
    arr = (_lib.RelinRecipe * max(1, len(recipes)))()
    for k, (q, i, j, level, alpha, transpose, gamma) in enumerate(recipes):
        arr[k] = _lib.RelinRecipe(quadrant=q, i=i, j=j, space=space, level=level,
                                  transpose=int(bool(transpose)), alpha=alpha, gamma=gamma)
    return arr


class DevicePlanBinding:
    """What the bindings of both device plans share: the plan set on its system, the ``window``
    read-out, the iterate's way to and from the host, residual, update and the debug copies.  A
    subclass names the library's entry points (``_SET`` ... ``_DEBUG``), gives the global shapes of
    its iterate blocks in the state entry's order (``_block_shapes()``) and its debug arrays in the
    library's order (``_debug_arrays()``: ``{name: (window key, shape of one level)}``), and calls
    ``_attach`` once ``self.plan`` stands."""

    def _call(self, entry, *args):
        self._system._ck(getattr(self._lib, entry)(self._system.handle, *args))

    def _attach(self, system, host_allreduce):
        self._system, self._lib, self.host_allreduce = system, system._lib, host_allreduce
        d, keep = self.plan.descriptor()
        self._call(self._SET, C.byref(d))
        del keep
        w = (C.c_int * 8)()
        self._call(self._WINDOW, w)
        #: half-open ranges of global levels held in HBM: v, zeta, D, and the owned block rows
        self.window = {k: (w[2 * n], w[2 * n + 1])
                       for n, k in enumerate(("v", "zeta", "D", "blocks"))}

    def set_state(self, *blocks):
        """Global arrays; a time shard takes its windows from them, halo levels included."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in blocks]
        for a, shape in zip(arrs, self._block_shapes()):
            if a.shape != shape:
                raise ValueError(f"iterate block of shape {a.shape}, expected {shape}")
        self._call(self._STATE, 0, *[a.ctypes.data_as(_lib.c_f64p) for a in arrs])

    def get_state(self):
        """The whole iterate on the host.  A time shard downloads the levels it owns into zeros
        and the ranks' arrays are summed (``host_allreduce``): every rank returns the same."""
        out = [np.zeros(shape) for shape in self._block_shapes()]
        self._call(self._STATE, 1, *[a.ctypes.data_as(_lib.c_f64p) for a in out])
        if self.window["blocks"] != (0, self.plan.m):
            if self.host_allreduce is None:
                raise ValueError("a time-sharded plan needs host_allreduce to gather the iterate")
            for a in out:            # the other ranks' levels are zero here: a sum gathers
                self.host_allreduce(a.reshape(-1), 0)
        return out

    def residual(self, d_out, rhs):
        norm = C.c_double()
        self._call(self._RESIDUAL, d_out, int(rhs), C.byref(norm))
        return norm.value

    def update(self, d_u):
        self._call(self._UPDATE, d_u)

    def debug_array(self, which):
        """The array ``which`` of ``_debug_arrays`` on the host: on a time shard the levels of its
        window, halo levels included."""
        table = self._debug_arrays()
        key, per_level = table[which]
        out = np.empty((self.window[key][1] - self.window[key][0],) + per_level)
        self._call(self._DEBUG, list(table).index(which), out.ctypes.data_as(_lib.c_f64p),
                   out.size)
        return out


class DeviceRelinearisation(DevicePlanBinding):
    """The plan on the outer system of a ``GpuLinearSolver`` and the Picard iterate in HBM.

    On a time-sharded outer system every rank keeps its own levels of the iterate, of the element
    matrices and of ``D`` (``window``), assembles, evaluates the residual of and updates those, and
    trades one level of ``v`` and one of ``zeta`` with its neighbours before every assembly;
    ``assemble``, ``residual`` and ``get_state`` are then collective."""

    _SET, _WINDOW, _STATE = "kkt_set_relinearisation", "kkt_picard_window", "kkt_picard_state"
    _RESIDUAL, _UPDATE = "kkt_picard_residual_device", "kkt_picard_update_device"
    _DEBUG = "kkt_debug_relin_array"

    def __init__(self, pb, outer, recipes, plan=None, host_allreduce=None):
        """``recipes``: the blocks every re-linearisation rewrites, per system
        (``blocks.instationary_relinearisation_recipes``); on a time shard those of the rank's own
        block rows, with their global indices.  ``host_allreduce(array, op)`` (a time shard):
        what ``get_state`` gathers the iterate with."""
        self.pb, self.outer = pb, outer
        self.plan = RelinearisationPlan(pb) if plan is None else plan
        self._attach(outer, host_allreduce)
        self.recipes = {name: (_recipe_array(recipes[name], 1 if name == "commutator" else 0),
                               len(recipes[name])) for name in ("outer", "inner", "commutator")}
        ptr = [C.c_void_p() for _ in range(4)]
        self._call("kkt_picard_iterate", *[C.byref(p) for p in ptr])
        self.d_v = ptr[0]

    def _block_shapes(self):
        """``v``, ``zeta``, ``p``, ``mu``."""
        th, n_t, m = self.pb.disc, self.pb.n_t, self.plan.m
        return (n_t, th.n_v), (n_t, th.n_v), (m, th.n_p), (m, th.n_p)

    def _debug_arrays(self):
        """``kkt_debug_relin_array``: ``"Ev"`` (n_t, ne, 6, 6), ``"Ep"`` (n_t, ne, 3, 3) (Q2-Q1:
        (n_t, ne, 9, 9) and (n_t, ne, 4, 4)), ``"D2"``
        (n_t, nnz2) or ``"Dp"`` (n_t, nnz1) of the last assembly -- on a time shard the levels of
        ``window["D"]``; ``"v"`` / ``"zeta"``: the iterate's windows, halo levels included."""
        ne, n_v = len(self.plan.V), self.pb.disc.n_v
        kv, kp = self.plan.V.shape[1], self.plan.P.shape[1]
        return {"Ev": ("D", (ne, kv, kv)), "Ep": ("D", (ne, kp, kp)),
                "D2": ("D", (self.plan.K2.nnz,)),
                "Dp": ("D", (self.plan.Kp.nnz,)), "v": ("v", (n_v,)), "zeta": ("zeta", (n_v,))}

    def assemble(self):
        """D_v, D_p of every level of the D window at the device iterate's v (a time shard first
        refreshes its halo levels from the neighbour ranks)."""
        self.outer._ck(self._lib.kkt_relinearise_device(self.outer.handle, self.outer.handle,
                                                        self.d_v, 0, None))

    def relinearise(self, system, name, recipes=None):
        """Rewrite ``system``'s recipe blocks (``name``: "outer", "inner" or "commutator") from
        the last assembly.  ``recipes``: another list for this call (the first build composes
        every block, ``blocks.instationary_build_recipes``)."""
        arr, n = self.recipes[name]
        if recipes is not None:
            arr, n = _recipe_array(recipes, 1 if name == "commutator" else 0), len(recipes)
        system._ck(self._lib.kkt_relinearise_device(system.handle, self.outer.handle, None, n, arr))


@contextlib.contextmanager
def device_vectors(system):
    """``(d_b, d_u)``: right-hand side and (zeroed) update of a device loop on ``system``."""
    lib = system._lib
    d_b, d_u = C.c_void_p(), C.c_void_p()
    system._ck(lib.kkt_vec_alloc(system.handle, C.byref(d_b)))
    try:
        system._ck(lib.kkt_vec_alloc(system.handle, C.byref(d_u)))
        yield d_b, d_u
    finally:
        lib.kkt_vec_free(system.handle, d_b)
        if d_u:
            lib.kkt_vec_free(system.handle, d_u)


def device_picard_loop(dev, d_b, d_u, norm_0, solve, relinearise, fresh, rtol, atol, max_iter,
                       verbose, after_first_update=None, mixer=None):
    """The device Picard iterations from the assembled iterate of ``dev`` with right-hand side
    ``d_b`` and residual norm ``norm_0``: re-linearise (unless the blocks are ``fresh`` from the
    build), ``solve(d_b, d_u)`` (it returns the linear iterations), update, assemble, residual,
    until the host loops' stopping rule holds.  ``after_first_update()`` runs once, before the
    first re-assembly.  ``mixer`` (``anderson.DeviceAnderson``): ``mixer.step(d_u)`` turns the
    solver's update into the accelerated step before it is added; after ``after_first_update``,
    which moves the iterate outside any step, ``mixer.reset()``: no secant pair spans the lift.
    Returns the norms (``norm_0`` first) and the linear iteration counts."""
    norm_k, k = norm_0, 0
    norms, lin_its = [norm_0], []
    while norm_k > rtol * norm_0 and norm_k > atol:
        if not fresh:
            relinearise()
        fresh = False
        lin_its.append(solve(d_b, d_u))
        if mixer is not None:
            mixer.step(d_u)
        dev.update(d_u)
        if k == 0 and after_first_update is not None:
            after_first_update()
            if mixer is not None:
                mixer.reset()
        dev.assemble()
        norm_k = dev.residual(d_b, rhs=True)
        norms.append(norm_k)
        k += 1
        if verbose:
            print(f"Non-linear solver: iteration {k:d}, non-linear residual norm "
                  f"{norm_k:.16e}")
        if k + 1 > max_iter:
            break
    return norms, lin_its
