"""Host references for the pressure stage of the Stokes preconditioner, separated from the
nested velocity solve in front of it.

The stage is everything of ``oracle.kkt_oracle.pc_instationary_incompressible`` after
``inner.solve``: ``h = s2 (sB B u_0 - b_1)`` (Crank-Nicolson: ``T_2`` / ``T_1`` before the
subtraction, their inverse scans after the scaling), the ``K_p`` solve per block (Jacobi,
Jacobi-Chebyshev or two-grid cycles with the constants deflated), the commutator block product
and the ``M_p`` solve per block.  Both references below take ``u_0`` as data:

* ``ExtendedStage``: dense ``numpy.longdouble`` matrices and vectors throughout, the Chebyshev
  coefficients and the deflated coarse inverse in ``longdouble`` too, the nullspace wrapping by
  an ``OracleSystem`` of that dtype;
* ``oracle_stage_pc_fn``: the float64 stage put together from the oracle's own functions
  (``_inner_solve``, ``apply_T_*``, SciPy CSR products) -- with the problem's own scalings and the
  oracle's own ``u_0`` it reproduces ``pc_instationary_incompressible`` bit for bit
  (``tests/test_stokes_stage_ref.py``).

Their distance ``d_case`` on the pressure half is the yardstick of
``tests/test_gpu_stokes_pressure_stage.py``: the GPU evaluates the same float64 recurrences in
another order (SELL row order, fused multiply-adds), so its distance from the extended result is
of the size of the oracle's; a case passes when ``rel_err(gpu, extended) <= 8 max(d_case,
eps its_total)``.  ``CASES`` lists the shapes, degrees and forms both test files walk through.
"""
import functools

import numpy as np
import scipy.sparse as sp

import common

XP = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FACTOR = 8.0
# not the problem's own tau and 1 / tau^2: a swapped or squared factor cannot cancel
B_SCALE, POST_SCALE = 0.37, 5.3
KP_BOUNDS, MP_BOUNDS, KP_TWO_GRID_BOUNDS = (0.02, 2.2), (0.25, 2.25), (0.15, 2.1)


# ------------------------------------------------------------------------------- the cases
def case(n, m, CN, kp_its=30, mp_its=20, two_grid=None):
    """``two_grid``: (cycles, sweeps) of the two-grid ``K_p`` form on the multilinear coarse
    space with 3 x 3 cells; ``kp_its`` is then the number of sweeps."""
    if two_grid is not None:
        kp_its = two_grid[1]
    return dict(n=n, m=m, CN=CN, kp_its=kp_its, mp_its=mp_its,
                cycles=0 if two_grid is None else two_grid[0])


def case_id(c):
    s = f"n{c['n']}-m{c['m']}-{'CN' if c['CN'] else 'BE'}-kp{c['kp_its']}-mp{c['mp_its']}"
    return s + (f"-cyc{c['cycles']}" if c["cycles"] else "")


# pressure sizes 16, 25, 64, 81: below, odd, exactly and just over one wavefront
SIZES = [case(n, 3, CN) for n in (3, 4, 7, 8) for CN in (False, True)]
# 2m = 4, 6, 10 pressure blocks per step: a multiple of the four blocks a thread of the
# shared-matrix form takes, then not, then not again.  m = 2 is the smallest the library takes (the
# nested velocity preconditioner refuses a single block: "need at least two blocks"), so the
# Crank-Nicolson transforms without any neighbour do not occur through kkt_pc_apply
LEVELS = [case(4, m, CN) for CN in (False, True) for m in (2, 3, 5)]
# emit_cheb: Jacobi; return after the first step; no p_{k-1}; first step with one; every residue
# of the three-buffer rotation with the last step redirected; 7 | 8 plain launches | captured
# graph; the default
DEGREES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 30)
KP_DEGREES = [case(4, 3, False, kp_its=k, mp_its=5) for k in DEGREES] + \
             [case(4, 3, True, kp_its=k, mp_its=5) for k in (0, 7, 8)]
MP_DEGREES = [case(4, 3, False, kp_its=5, mp_its=k) for k in DEGREES] + \
             [case(4, 3, True, kp_its=5, mp_its=k) for k in (0, 7, 8)]
# with 4 sweeps the next cycle's first target is the buffer that holds the current iterate
TWO_GRID = [case(8, 3, False, two_grid=(cyc, sw)) for cyc in (1, 2, 3) for sw in (1, 2, 4)] + \
           [case(8, 3, True, two_grid=(2, 4)), case(8, 2, True, two_grid=(3, 2))]
CASES = []
for _c in SIZES + LEVELS + KP_DEGREES + MP_DEGREES + TWO_GRID:
    if _c not in CASES:          # (a shape that two of the lists name runs once)
        CASES.append(_c)


def its_total(c):
    """Steps of the two recurrences of one block (a Jacobi application counts as one, a coarse
    correction as one): the number of float64 roundings in sequence that ``eps its_total``
    allows for where the two references happen to agree more closely than that."""
    kp = c["cycles"] * (c["kp_its"] + 1) if c["cycles"] else max(c["kp_its"], 1)
    return kp + max(c["mp_its"], 1)


def bound(d_case, c):
    return FACTOR * max(d_case, EPS * its_total(c))


@functools.lru_cache(maxsize=4)
def _problem(n, m, CN):
    return common.stokes_problem(n=n, n_t=m + 1 if CN else m, CN=CN)


def problem(c):
    return _problem(c["n"], c["m"], c["CN"])


def specs(c):
    kp = KP_TWO_GRID_BOUNDS if c["cycles"] else KP_BOUNDS
    return dict(common.STOKES_SPECS, kp=(c["kp_its"], *kp), mp=(c["mp_its"], *MP_BOUNDS))


@functools.lru_cache(maxsize=2)
def _coarse_space(n):
    from control_amd.coarse import multilinear_coarse_space
    return multilinear_coarse_space(_problem(n, 3, False)["th"].coords_p, (), cells=3)


def kp_coarse(c):
    return (_coarse_space(c["n"]), c["cycles"]) if c["cycles"] else None


def stage_gpu(c, options=None, comm=None):
    """(outer system, StokesPC) of a case on the GPU, with the scalings of this module."""
    return common.stokes_gpu(problem(c), specs(c), options=options, comm=comm,
                             kp_coarse=kp_coarse(c), b_scale=B_SCALE, post_scale=POST_SCALE)


def inputs(c, seed=0):
    """The two input kinds: zero velocity right-hand side with a ``b_1`` that is NOT zero-mean
    (the nested solve returns ``u_0 = 0`` exactly: the stage applied to ``-s2 b_1``), and random
    ``b_0`` and ``b_1`` (``u_0`` is then read back from the GPU's own output)."""
    p = problem(c)
    th, m = p["th"], p["m"]
    rng = np.random.default_rng(common.SEED + 1000 * seed + 7 * c["n"] + m)
    b1 = rng.standard_normal((2 * m, th.n_p)) + 0.7
    x1 = np.concatenate([np.zeros(2 * m * th.n_v), b1.ravel()])
    x2 = rng.standard_normal(2 * m * (th.n_v + th.n_p))
    x2[2 * m * th.n_v:] += 0.3
    return x1, x2


def split(p, y):
    th, m = p["th"], p["m"]
    k = 2 * m * th.n_v
    return y[:k].reshape(2 * m, th.n_v), y[k:].reshape(2 * m, th.n_p)


def interior_u0(p, y):
    """``u_0`` of the nested solve from a preconditioner output: the velocity half with the
    Dirichlet dofs -- which the post-correction overwrites, and which are exactly 0 inside --
    zeroed."""
    u0 = split(p, y)[0].copy()
    u0[:, p["th"].boundary_v] = 0.0
    return u0


def oracle_system(p, dtype=np.float64):
    from oracle import kkt_oracle as ko
    th, m, CN, bl = p["th"], p["m"], p["CN"], p["blocks"]
    kw = dict(sub_n_blocks_00_0=m, sub_n_blocks_11_0=m) if CN else {}
    return ko.OracleSystem(th.n_v, th.n_p, *bl["outer"], n_blocks_00=2 * m, n_blocks_11=2 * m,
                           nullspace_0=tuple(ko.DirichletBCNullspace(th.boundary_v)
                                             for _ in range(2 * m)),
                           nullspace_1=tuple(ko.ConstantNullspace() for _ in range(2 * m)),
                           CN=CN, dtype=dtype, **kw)


# ------------------------------------------------------------- float64: the oracle's own parts
def oracle_stage_pc_fn(p, sp_, u0, b_scale=B_SCALE, post_scale=POST_SCALE, kp_coarse=None):
    """Lines 1055-1081 of ``pc_instationary_incompressible`` for a given ``u_0``."""
    from oracle import kkt_oracle as ko
    th, m, CN = p["th"], p["m"], p["CN"]
    c00, c01, c10, c11 = p["blocks"]["commutator"]
    B, K_p, M_p = sp.csr_matrix(th.B), sp.csr_matrix(th.K_p), sp.csr_matrix(th.M_p)
    kp_spec, mp_spec = ko.ChebSpec(*sp_["kp"]), ko.ChebSpec(*sp_["mp"])
    if kp_coarse is not None:
        kp_spec.coarse = ko.CoarseSpace(kp_coarse[0], int(kp_coarse[1]), deflate=True)
    npr = th.n_p

    def pc_fn(u_0, u_1, b_0, b_1):
        u_0[:] = u0
        v, z = u0[:m], u0[m:]
        h0 = np.stack([b_scale * (B @ v[i]) for i in range(m)])
        h1 = np.stack([b_scale * (B @ z[i]) for i in range(m)])
        if CN:
            h0, h1 = ko.apply_T_2(h0), ko.apply_T_1(h1)
        h0 = (h0 - b_1[:m]) * post_scale
        h1 = (h1 - b_1[m:]) * post_scale
        if CN:
            h0, h1 = ko.apply_T_2_inv(h0), ko.apply_T_1_inv(h1)
        m0 = np.stack([ko._inner_solve(K_p, kp_spec, h0[i]) for i in range(m)])
        m1 = np.stack([ko._inner_solve(K_p, kp_spec, h1[i]) for i in range(m)])
        g0, g1 = np.zeros((m, npr)), np.zeros((m, npr))
        for blocks, g, src in ((c00, g0, m0), (c01, g0, m1), (c10, g1, m0), (c11, g1, m1)):
            for (i, j), A in blocks.items():
                if A is not None:
                    g[i] += A @ src[j]
        for i in range(m):
            u_1[i] = ko._inner_solve(M_p, mp_spec, g0[i])
            u_1[m + i] = ko._inner_solve(M_p, mp_spec, g1[i])
    return pc_fn


# ---------------------------------------------------------------------- extended precision
def _dense(A):
    return sp.csr_matrix(A).toarray().astype(XP)


def xp_inverse(E):
    """Inverse of a small dense matrix in ``longdouble`` (Gauss-Jordan with partial pivoting;
    ``numpy.linalg`` has no extended-precision path)."""
    n = E.shape[0]
    A = np.concatenate([np.array(E, dtype=XP), np.eye(n, dtype=XP)], axis=1)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
        A[k] = A[k] / A[k, k]
        for i in range(n):
            if i != k and A[i, k] != 0:
                A[i] = A[i] - A[i, k] * A[k]
    return A[:, n:]


def xp_cheb_coefficients(emin, emax, its):
    """``scale`` and ``[(c1, c2, c3)]`` of steps ``2 .. its`` (``KSPSolve_Chebyshev``)."""
    emin, emax, one, two = XP(emin), XP(emax), XP(1), XP(2)
    scale = two / (emax + emin)
    alpha = one - scale * emin
    mu, omegaprod = one / alpha, two / alpha
    c_km1, c_k, out = one, mu, []
    for _ in range(1, its):
        c_kp1 = two * mu * c_k - c_km1
        omega = omegaprod * c_k / c_kp1
        out.append((one - omega, omega, scale * omega))
        c_km1, c_k = c_k, c_kp1
    return scale, out


def xp_chebyshev_from(A, dinv, b, x0, emin, emax, its):
    """``its`` steps from ``x0`` (``None``: the zero guess); ``its == 0``: Jacobi."""
    if its == 0:
        return dinv * b if x0 is None else x0.copy()
    scale, coefs = xp_cheb_coefficients(emin, emax, its)
    if x0 is None:
        p_km1, p_k = np.zeros_like(b), scale * (dinv * b)
    else:
        p_km1, p_k = x0, x0 + scale * (dinv * (b - A @ x0))
    for c1, c2, c3 in coefs:
        p_km1, p_k = p_k, c1 * p_km1 + c2 * p_k + c3 * (dinv * (b - A @ p_k))
    return p_k


def xp_T_1(x):        # new_i = old_i + old_{i+1}
    return np.stack([x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(len(x))])


def xp_T_2(x):        # new_i = old_i + old_{i-1}
    return np.stack([x[i] + x[i - 1] if i > 0 else x[i] for i in range(len(x))])


def xp_T_1_inv(x):    # for i = n-2 .. 0: x_i -= x_{i+1}, the updated one
    y = [r for r in x]
    for i in range(len(y) - 2, -1, -1):
        y[i] = y[i] - y[i + 1]
    return np.stack(y)


def xp_T_2_inv(x):    # for i = 1 .. n-1: x_i -= x_{i-1}, the updated one
    y = [r for r in x]
    for i in range(1, len(y)):
        y[i] = y[i] - y[i - 1]
    return np.stack(y)


class ExtendedStage:
    """The stage of one problem and one set of sub-solve specifications in ``longdouble``."""

    def __init__(self, p, sp_, b_scale=B_SCALE, post_scale=POST_SCALE, kp_coarse=None):
        th = p["th"]
        self.p, self.m, self.CN = p, p["m"], p["CN"]
        self.sB, self.s2 = XP(b_scale), XP(post_scale)
        self.B, self.Kp, self.Mp = _dense(th.B), _dense(th.K_p), _dense(th.M_p)
        self.kp_dinv, self.mp_dinv = XP(1) / np.diag(self.Kp), XP(1) / np.diag(self.Mp)
        self.kp, self.mp = sp_["kp"], sp_["mp"]
        dense = {}
        self.comm = [{ij: dense.setdefault(id(A), _dense(A)) for ij, A in blk.items()
                      if A is not None} for blk in p["blocks"]["commutator"]]
        self.cycles = 0
        if kp_coarse is not None:
            self.P, self.cycles = _dense(kp_coarse[0]), int(kp_coarse[1])
            E = self.P.T @ (self.Kp @ self.P)
            # constants deflated: E + (trace E / n_c^2) 1 1^T, as coarse_inverse(deflate=True)
            self.Einv = xp_inverse(E + np.trace(E) / XP(E.shape[0]) ** 2)

    def solve_kp(self, b):
        its, emin, emax = self.kp
        if not self.cycles:
            return xp_chebyshev_from(self.Kp, self.kp_dinv, b, None, emin, emax, its)
        x = np.zeros_like(b)
        for cyc in range(self.cycles):
            r = b if cyc == 0 else b - self.Kp @ x
            x = x + self.P @ (self.Einv @ (self.P.T @ r))
            x = xp_chebyshev_from(self.Kp, self.kp_dinv, b, x, emin, emax, its)
        return x

    def solve_mp(self, b):
        its, emin, emax = self.mp
        return xp_chebyshev_from(self.Mp, self.mp_dinv, b, None, emin, emax, its)

    def pc_fn(self, u0):
        m, CN = self.m, self.CN
        u0 = np.asarray(u0, dtype=XP)

        def pc_fn(u_0, u_1, b_0, b_1):
            u_0[:] = u0
            b1 = np.asarray(b_1, dtype=XP)
            h0 = np.stack([self.sB * (self.B @ u0[i]) for i in range(m)])
            h1 = np.stack([self.sB * (self.B @ u0[m + i]) for i in range(m)])
            if CN:
                h0, h1 = xp_T_2(h0), xp_T_1(h1)
            h0, h1 = (h0 - b1[:m]) * self.s2, (h1 - b1[m:]) * self.s2
            if CN:
                h0, h1 = xp_T_2_inv(h0), xp_T_1_inv(h1)
            mm = [np.stack([self.solve_kp(h[i]) for i in range(m)]) for h in (h0, h1)]
            g = [np.zeros_like(h0), np.zeros_like(h1)]
            for q, blk in enumerate(self.comm):          # c00, c01, c10, c11
                for (i, j), A in blk.items():
                    g[q // 2][i] = g[q // 2][i] + A @ mm[q % 2][j]
            for i in range(m):
                u_1[i] = self.solve_mp(g[0][i])
                u_1[m + i] = self.solve_mp(g[1][i])
        return pc_fn


@functools.lru_cache(maxsize=2)
def _extended_stage(key):
    c = dict(key)
    return ExtendedStage(problem(c), specs(c), kp_coarse=kp_coarse(c))


def references(c, x, u0):
    """Pressure halves ``(extended, float64 oracle stage)`` of ``pc_apply`` for the input ``x``
    and the nested solve's ``u_0``, both through the oracle's nullspace wrapping, and their
    distance ``d_case``."""
    p = problem(c)
    ext = _extended_stage(tuple(sorted(c.items())))
    yx = oracle_system(p, XP).pc_apply(ext.pc_fn(u0), np.asarray(x, dtype=XP))
    yo = oracle_system(p).pc_apply(oracle_stage_pc_fn(p, specs(c), u0, kp_coarse=kp_coarse(c)), x)
    px, po = split(p, yx)[1], split(p, yo)[1]
    return px, po, float(common.rel_err(po, px))
