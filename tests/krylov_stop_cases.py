"""The case table of the stopping-rule tests, shared by the oracle test on the CPU
(``test_krylov_stop_ref.py``), the device test (``test_gpu_krylov_stopping.py``) and the device
test on time shards (``test_gpu_krylov_stopping_sharded.py`` with ``sharded_stop_worker.py``).

Systems are two-variable block systems with one CSR block per quadrant, no nullspaces, and
``N = 2 nx`` unknowns with ``nx`` in {24, 33} (or 2 for the MINRES instance): neither 48 nor 66
is a multiple of 32 or of the double2 width.  The dense matrix the reference works on is
``np.block`` of the same arrays.  Preconditioners are the identity (``pc_fn=None``) and a host
callback that multiplies by a fixed positive diagonal, so ``B`` is known exactly.  The *layered*
systems (``LAYERS``) have ``m`` time levels per variable, ``N = 2 m nx`` with ``nx = 5``, in the
block structure a time shard accepts (``layer_mask``), so that several ranks can own whole
levels; ``layer_cases()`` lists the table on them.

A *backend* runs a solve: ``OracleBackend`` below, the device one in the GPU test.  Every check
takes a backend, so both tests assert the same things.  Expected values come from
``krylov_stop_ref`` and from the table, never from a backend.

Value bar (history entry ``k`` and the iterate after ``k`` steps, relative):
``10 N u kappa r_0 / r_k`` with ``u = 1.1e-16`` and ``kappa`` the 2-norm condition number of the
preconditioned operator; entries whose bar is 1e-8 or more are not compared, and in cases A and
B at least 80 % of every history must be under it.
"""
import functools
import math
from dataclasses import dataclass, replace

import numpy as np
import scipy.sparse as sp

import krylov_stop_ref as ref

U_ROUND = 1.1e-16
BAR_CAP = 1.0e-8
NO_DIV = 1.0e300
GMRES_FORMS = ("left", "right", "flexible")


# ------------------------------------------------------------------------------------ systems
def layer_mask(m, nx):
    """The structure a single-family time shard accepts for every world (``System::add_block``):
    blocks of column variable 0 at ``j`` in ``{i-1, i}``, of column variable 1 at ``{i, i+1}``."""
    k = np.arange(m)
    col0 = (k[None, :] == k[:, None]) | (k[None, :] == k[:, None] - 1)
    col1 = (k[None, :] == k[:, None]) | (k[None, :] == k[:, None] + 1)
    one = np.ones((nx, nx), dtype=bool)
    return np.block([[np.kron(col0, one), np.kron(col1, one)],
                     [np.kron(col0, one), np.kron(col1, one)]])


class Sys:
    def __init__(self, name, A, b, nx, diag=None, m=1):
        self.name, self.nx, self.m, self.N = name, nx, m, 2 * m * nx
        self.A = np.array(A, dtype=np.float64)
        self.b = np.array(b, dtype=np.float64)
        assert self.A.shape == (self.N, self.N) and self.b.shape == (self.N,)
        assert m == 1 or not self.A[~layer_mask(m, nx)].any()
        # the fixed positive diagonal of the callback preconditioner
        self.diag = (0.5 + np.random.default_rng(77).random(self.N)) if diag is None \
            else np.array(diag, dtype=np.float64)
        self.guesses = {"zero": np.zeros(self.N)}
        self.rhs = {"b": self.b, "zero": np.zeros(self.N)}

    def split(self, v):
        """A flat vector as its two ``(m, nx)`` variables (views)."""
        k = self.m * self.nx
        return v[:k].reshape(self.m, self.nx), v[k:].reshape(self.m, self.nx)

    def only_levels(self, v, levels):
        """``v`` with every time level but ``levels`` set to zero, in both variables."""
        out = np.zeros(self.N)
        for part, src in zip(self.split(out), self.split(np.asarray(v, dtype=np.float64))):
            part[list(levels)] = src[list(levels)]
        return out

    def present(self, q, i, j):
        if self.m == 1:
            return True
        return j in ((i - 1, i) if q in (0, 2) else (i, i + 1))

    def blocks(self):
        """The four quadrants as block dictionaries with all ``m * m`` keys: CSR matrices with
        every entry stored (explicit zeros too: the structure is the dense one) where the layer
        structure has a block, None elsewhere."""
        nx, m = self.nx, self.m
        ip = np.arange(0, nx * nx + 1, nx, dtype=np.int32)
        ix = np.tile(np.arange(nx, dtype=np.int32), nx)

        def quad(q):
            r, c = divmod(q, 2)
            out = {}
            for i in range(m):
                for j in range(m):
                    if not self.present(q, i, j):
                        out[(i, j)] = None
                        continue
                    r0, c0 = (r * m + i) * nx, (c * m + j) * nx
                    M = self.A[r0:r0 + nx, c0:c0 + nx]
                    out[(i, j)] = sp.csr_matrix((M.ravel().copy(), ix, ip), shape=(nx, nx))
            return out
        return quad(0), quad(1), quad(2), quad(3)

    def diag_blocks(self):
        """Diagonal operators as diagonal CSR blocks, no couplings."""
        nx, m = self.nx, self.m
        d = np.diag(self.A)
        assert np.array_equal(self.A, np.diag(d))
        d0, d1 = self.split(d)
        none = {(i, j): None for i in range(m) for j in range(m)}
        b00, b11 = dict(none), dict(none)
        for i in range(m):
            b00[(i, i)] = sp.diags(d0[i], format="csr")
            b11[(i, i)] = sp.diags(d1[i], format="csr")
        return b00, dict(none), dict(none), b11

    def B(self, pc):
        return None if pc == "id" else self.diag

    def op_dense(self, form, pc):
        Bm = np.eye(self.N) if pc == "id" else np.diag(self.diag)
        return Bm @ self.A if form in ("left", "minres") else self.A @ Bm


@functools.lru_cache(maxsize=None)
def system(name):
    if name in ("A24", "A33"):          # case A: nonsymmetric, kappa about 7
        nx = int(name[1:])
        # (seeds picked so that the reference meets the table's conditions -- threshold gaps of
        # 1.5 in GMRES(3) for both guesses, 80 % of GMRES(10)'s 22 entries under the bar cap;
        # test_krylov_stop_ref.py asserts them from the reference alone)
        rng = np.random.default_rng({24: 20319, 33: 20273}[nx])
        N = 2 * nx
        s = Sys(name, 4.0 * np.eye(N) + 0.35 * rng.standard_normal((N, N)),
                rng.standard_normal(N), nx)
        g = np.random.default_rng(1002).standard_normal(N)
        # a guess whose residual is about 30 times the right-hand side
        s.guesses["far"] = g * (30.0 * np.linalg.norm(s.b) / np.linalg.norm(s.A @ g))
        return s
    if name == "S24":                   # symmetric positive definite, for MINRES
        rng = np.random.default_rng(20264)
        G = rng.standard_normal((48, 48))
        return Sys(name, 4.0 * np.eye(48) + 0.25 * (G + G.T) / 2, rng.standard_normal(48), 24)
    if name == "two":                   # case E: A = 2 I, b = e_1
        e1 = np.zeros(48)
        e1[0] = 1.0
        return Sys(name, 2.0 * np.eye(48), e1, 24,
                   diag=np.r_[np.full(24, 0.5), np.full(24, 0.25)])
    if name == "sing":                  # case F: A b = 0 exactly
        A = np.eye(48)
        A[:2, :2] = [[1.0, -1.0], [-1.0, 1.0]]
        b = np.zeros(48)
        b[:2] = 1.0
        return Sys(name, A, b, 24)
    if name.startswith("eig"):          # case G: d distinct eigenvalues 1..d, repeated
        d = int(name[3:])
        return Sys(name, np.diag(1.0 + (np.arange(48) % d)), np.ones(48), 24)
    if name == "mr4":                   # case I: diag(1, 1, 0, 0), b = 1
        return Sys(name, np.diag([1.0, 1.0, 0.0, 0.0]), np.ones(4), 2)
    if name in LAYERS:
        return layered(name)
    raise KeyError(name)


# Layered systems: m time levels of nx = 5 unknowns per variable, the structure of layer_mask,
# so that 2, 3 and 5 ranks can each own whole levels (local lengths of 10 to 40 doubles, none a
# multiple of 32).  Name -> (m, family).
LAYER_NX = 5
LAYERS = {"L5": (5, "nonsym"), "L7": (7, "nonsym"), "LS5": (5, "spd"), "Ltwo": (5, "two"),
          "Lsing": (5, "sing"), "Leig3": (5, "eig"), "Leig5": (5, "eig"), "Leig6": (5, "eig"),
          "Lmr": (5, "mr")}
# (a, seed) of the non-symmetric instances: picked so that the reference meets the table's
# conditions (test_krylov_stop_ref.py asserts them from the reference alone)
LAYER_SEEDS = {"L5": (0.55, 4), "L7": (0.55, 9)}


def layered(name):
    m, family = LAYERS[name]
    nx = LAYER_NX
    N = 2 * m * nx
    mask = layer_mask(m, nx)
    if family == "nonsym":              # cases A, B, C, D, H, J
        a, seed = LAYER_SEEDS[name]
        rng = np.random.default_rng(seed)
        s = Sys(name, 4.0 * np.eye(N) + a * rng.standard_normal((N, N)) * mask,
                rng.standard_normal(N), nx, m=m)
        g = np.random.default_rng(1002).standard_normal(N)
        s.guesses["far"] = g * (30.0 * np.linalg.norm(s.b) / np.linalg.norm(s.A @ g))
        for level in (0, m // 2, m - 1):
            # first, a middle and the last rank of 3 and 5 ranks (2 ranks: first, first, last)
            s.guesses[f"far@{level}"] = s.only_levels(s.guesses["far"], [level])
            s.rhs[f"b@{level}"] = s.only_levels(s.b, [level])
        return s
    if family == "spd":
        # quadrants 00 and 11 block diagonal and symmetric, 01 upper bidiagonal, 10 its transpose
        rng = np.random.default_rng(20264)
        G = rng.standard_normal((N, N)) * mask
        k = m * nx
        G[:k, :k] *= np.kron(np.eye(m), np.ones((nx, nx)))
        G[k:, k:] *= np.kron(np.eye(m), np.ones((nx, nx)))
        G[k:, :k] = G[:k, k:].T
        # (0.4: with S24's 0.25 the banded matrix converges too fast for 80 % of 13 entries to
        # stay under the cap of the value bar)
        A = 4.0 * np.eye(N) + 0.4 * (G + G.T) / 2
        return Sys(name, A, rng.standard_normal(N), nx, m=m)
    if family == "two":                 # b = e_1 lies in level 0: on the first rank only
        e1 = np.zeros(N)
        e1[0] = 1.0
        return Sys(name, 2.0 * np.eye(N), e1, nx, m=m,
                   diag=np.r_[np.full(N // 2, 0.5), np.full(N // 2, 0.25)])
    if family == "sing":
        A = np.eye(N)
        A[:2, :2] = [[1.0, -1.0], [-1.0, 1.0]]
        b = np.zeros(N)
        b[:2] = 1.0
        return Sys(name, A, b, nx, m=m)
    if family == "eig":
        d = int(name[4:])
        return Sys(name, np.diag(1.0 + (np.arange(N) % d)), np.ones(N), nx, m=m)
    if family == "mr":
        # case I on levels of three ranks: the identity with two zeros on the diagonal; b has a
        # one in two entries of the range (level 0 of variable 0, the last level of variable 1)
        # and in the two of the kernel (the middle level of either variable), zero elsewhere
        d, b = np.ones(N), np.zeros(N)
        in_range = [1, N - 2]
        kernel = [(m // 2) * nx + 2, m * nx + (m // 2) * nx + 3]
        d[kernel] = 0.0
        b[in_range + kernel] = 1.0
        return Sys(name, np.diag(d), b, nx, m=m)
    raise KeyError(name)


# ------------------------------------------------------------------------------------- solves
@dataclass(frozen=True)
class Spec:
    form: str                    # left / right / flexible / minres
    restart: int = 10
    rtol: float = 0.0
    atol: float = 0.0
    divtol: float = NO_DIV
    max_it: int = 1000
    keep: bool = True            # "preconditioner": True -- the result is returned, not raised

    def parameters(self):
        p = {"linear_solver": {"left": "gmres", "right": "gmres", "flexible": "fgmres",
                               "minres": "minres"}[self.form],
             "gmres_restart": self.restart, "relative_tolerance": self.rtol,
             "absolute_tolerance": self.atol, "divergence limit": self.divtol,
             "maximum_iterations": self.max_it, "monitor_convergence": False,
             "preconditioner": self.keep}
        if self.form == "right":
            p["pc_side"] = "right"
        return p


@dataclass
class Result:
    reason: int
    its: int
    history: np.ndarray
    x: np.ndarray
    op_applies: int = -1         # info()["last_op_applies"]; the oracle does not count

    def same_bits(self, other):
        return (self.reason == other.reason and self.its == other.its
                and self.history.tobytes() == other.history.tobytes()
                and self.x.tobytes() == other.x.tobytes())


def diag_pc(s):
    d_0, d_1 = s.split(s.diag)

    def pc(u_0, u_1, b_0, b_1):
        u_0[:] = d_0 * b_0
        u_1[:] = d_1 * b_1
    return pc


class nan_pc:
    """The diagonal preconditioner, but its ``call``-th application (1-based) returns NaN in
    one entry of variable 0: ``entry`` of time level ``level``.  (An object with its count in
    an attribute, so that a copy counts on its own.)"""

    def __init__(self, s, call, entry=5, level=0):
        self.inner, self.call, self.at, self.n = diag_pc(s), call, (level, entry), 0

    def __call__(self, u_0, u_1, b_0, b_1):
        self.inner(u_0, u_1, b_0, b_1)
        self.n += 1
        if self.n == self.call:
            u_0[self.at] = np.nan


def make_pc(s, pc):
    if callable(pc):
        return pc
    return None if pc == "id" else diag_pc(s)


class OracleBackend:
    name = "oracle"

    def __init__(self, module=None):
        if module is None:
            from oracle import kkt_oracle as module
        self.ko = module

    def pointer(self):
        """The backend that solves on vectors of the handle: the oracle has one kind only."""
        return self

    def handle(self, s, diagonal=False):
        return self.ko.OracleSystem(s.nx, s.nx, *(s.diag_blocks() if diagonal else s.blocks()),
                                    n_blocks_00=s.m, n_blocks_11=s.m)

    def solve(self, h, s, spec, pc="id", x0=None, b=None):
        x = np.array(s.guesses["zero"] if x0 is None else x0, dtype=np.float64)
        b = s.b if b is None else b
        with np.errstate(all="ignore"):
            r = h.solve(*s.split(x), *s.split(b), solver_parameters=spec.parameters(),
                        pc_fn=make_pc(s, pc))
        return Result(int(r.reason), int(r.its), np.array(r.history, dtype=np.float64), x)


# ---------------------------------------------------------------------------------- reference
def ref_steps(restart):
    return max(2 * restart + 1, restart + 3)


@dataclass
class Traj:
    """What the checks read of a ``krylov_stop_ref.Trajectory``, as plain arrays: the form in
    which the parent of a sharded run hands the reference to its ranks."""
    history: np.ndarray
    iterates: list
    rnorm0: float


_TRAJ = {}


def trajectory(name, form, pc, restart, guess="zero", steps=None, rhs="b"):
    """Reference history and iterates, computed once per (system, form, restart, guess, right-hand
    side) at the longest length any case asks for.  ``flexible`` with a fixed ``B`` is ``right``."""
    key = (name, form, pc, restart, guess, steps, rhs)
    if key not in _TRAJ:
        _TRAJ[key] = _trajectory(*key)
    return _TRAJ[key]


def _trajectory(name, form, pc, restart, guess, steps, rhs):
    s = system(name)
    steps = ref_steps(restart) if steps is None else steps
    if form == "minres":
        return ref.minres_trajectory(s.A, s.B(pc), s.rhs[rhs], s.guesses[guess], steps)
    if form == "flexible":
        return trajectory(name, "right", pc, restart, guess, steps, rhs)
    return ref.gmres_trajectory(s.A, s.B(pc), s.rhs[rhs], s.guesses[guess], restart, form, steps)


@functools.lru_cache(maxsize=None)
def kappa(name, form, pc):
    return float(np.linalg.cond(system(name).op_dense(form, pc)))


WORST = {}       # backend name -> largest relative deviation seen, history and iterate


def check_values(backend, s, form, pc, traj, res, need_share=True):
    """History entries and the returned iterate against the reference, at the bar of the module
    text.  Returns nothing; records the worst deviation per backend."""
    k_all = np.arange(len(res.history))
    want = traj.history[:len(res.history)]
    bar = 10 * s.N * U_ROUND * kappa(s.name, form, pc) * want[0] / want
    use = bar < BAR_CAP
    if need_share:
        assert use.mean() >= 0.8, (s.name, form, pc, bar)
    dev = np.abs(res.history - want) / want
    worst = WORST.setdefault(backend.name, {"history": 0.0, "iterate": 0.0})
    if use.any():
        worst["history"] = max(worst["history"], float(dev[use].max()))
    assert np.all(dev[use] <= bar[use]), (s.name, form, pc, k_all[use][dev[use] > bar[use]],
                                          dev[use].max())
    if use[res.its]:
        xr = traj.iterates[res.its]
        d = float(np.linalg.norm(res.x - xr) / max(np.linalg.norm(xr), 1e-300))
        worst["iterate"] = max(worst["iterate"], d)
        assert d <= bar[res.its], (s.name, form, pc, res.its, d, bar[res.its])


# ------------------------------------------------------------------ A: counts at restart boundaries
A_RESTARTS = (1, 3, 10)
A_COMBOS = tuple((name, form, pc, m)
                 for name, form, pc in (("A24", "left", "diag"), ("A24", "right", "diag"),
                                        ("A24", "flexible", "diag"), ("A24", "left", "id"),
                                        ("A33", "left", "diag"), ("A33", "flexible", "diag"))
                 for m in A_RESTARTS if name == "A24" or m == 3)
# the layered instances: restart 10 is where the all-reduced column outgrows one multi-dot pass
A_LAYER_COMBOS = tuple((name, form, pc, m)
                       for name, form, pc in (("L5", "left", "diag"), ("L5", "right", "diag"),
                                              ("L5", "flexible", "diag"), ("L7", "left", "diag"),
                                              ("L7", "flexible", "diag"))
                       for m in A_RESTARTS if name == "L5" or m == 3)


def a_max_its(m):
    return sorted({0, 1, m - 1, m, m + 1, 2 * m, 2 * m + 1})


def check_a(backend, name, form, pc, m):
    s = system(name)
    traj = trajectory(name, form, pc, m)
    h = backend.handle(s)
    out = []
    for max_it in a_max_its(m):
        res = backend.solve(h, s, Spec(form, restart=m, max_it=max_it), pc)
        assert (res.reason, res.its) == (ref.DIVERGED_ITS, max_it), (max_it, res.reason, res.its)
        assert len(res.history) == max_it + 1
        check_values(backend, s, form, pc, traj, res)
        out.append(res)
    return out


# ---------------------------------------------------------------- B: thresholds fire at their step
B_RESTART = 3
B_COMBOS = tuple((name, form, pc, guess)
                 for name, form, pc in (("A24", "left", "diag"), ("A24", "right", "diag"),
                                        ("A24", "flexible", "diag"), ("A24", "left", "id"))
                 for guess in ("zero", "far"))
B_LAYER_COMBOS = tuple((name, form, pc, guess)
                       for name, form, pc in (("L5", "left", "diag"), ("L5", "right", "diag"),
                                              ("L5", "flexible", "diag"), ("L5", "left", "id"),
                                              ("L7", "left", "diag"), ("L7", "flexible", "diag"))
                       for guess in ("zero", "far"))


def b_steps(m=B_RESTART):
    return (1, m, m + 1, m + 3)


def b_specs(name, form, pc, guess, m=B_RESTART):
    """``(spec, expected reason, expected its)`` for the three kinds of threshold at each k."""
    traj = trajectory(name, form, pc, m, guess)
    hist, out = traj.history, []
    for k in b_steps(m):
        rtol = ref.gap_tolerance(hist, k, traj.rnorm0)
        atol = ref.gap_tolerance(hist, k)
        base = Spec(form, restart=m, max_it=50)
        out.append((replace(base, rtol=rtol), ref.CONVERGED_RTOL, k))
        out.append((replace(base, atol=atol), ref.CONVERGED_ATOL, k))
        # both set, atol below rtol * rnorm0 and below the norm that passes: still RTOL
        out.append((replace(base, rtol=rtol, atol=0.5 * float(hist[k])), ref.CONVERGED_RTOL, k))
    return out


def check_b_conditions(name, form, pc, guess, m=B_RESTART):
    """What the table needs of the instance, from the reference alone."""
    s = system(name)
    traj = trajectory(name, form, pc, m, guess)
    hist = traj.history
    for k in b_steps(m):
        assert hist[k - 1] / hist[k] >= 1.5, (k, hist[k - 1] / hist[k])
    for spec, reason, k in b_specs(name, form, pc, guess, m):
        got = ref.expected_stop(hist, traj.rnorm0, rtol=spec.rtol, atol=spec.atol,
                                divtol=spec.divtol, max_it=spec.max_it)
        assert got == (reason, k)
    if guess == "far":
        r0 = s.b - s.A @ s.guesses["far"]
        assert np.linalg.norm(r0) > 3 * np.linalg.norm(s.b)
        for spec, reason, k in b_specs(name, form, pc, guess, m):
            if spec.rtol and not spec.atol and k >= m:
                # rnorm0 read as the first residual would stop at least two steps early
                _, k_wrong = ref.expected_stop(hist, float(hist[0]), rtol=spec.rtol, atol=0.0,
                                               divtol=spec.divtol, max_it=spec.max_it)
                assert k_wrong <= k - 2, (k, k_wrong)


def check_b(backend, name, form, pc, guess, m=B_RESTART):
    s = system(name)
    traj = trajectory(name, form, pc, m, guess)
    h = backend.handle(s)
    out = []
    for spec, reason, k in b_specs(name, form, pc, guess, m):
        res = backend.solve(h, s, spec, pc, x0=s.guesses[guess])
        assert (res.reason, res.its) == (reason, k), (spec, res.reason, res.its)
        assert len(res.history) == k + 1
        check_values(backend, s, form, pc, traj, res)
        out.append(res)
    return out


MINRES_STEPS, MINRES_GAP_STEP = 12, 5


def check_minres_values(backend, name="S24"):
    """MINRES on the symmetric positive definite instance with the diagonal callback: the
    monitored recurrence against the reference's B-norm minimiser, and one threshold."""
    s = system(name)
    traj = trajectory(name, "minres", "diag", 0, "zero", MINRES_STEPS)
    hist, k = traj.history, MINRES_GAP_STEP
    assert hist[k - 1] / hist[k] >= 1.5
    h = backend.handle(s)
    res = backend.solve(h, s, Spec("minres", max_it=MINRES_STEPS), "diag")
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_ITS, MINRES_STEPS,
                                                       MINRES_STEPS + 1)
    check_values(backend, s, "minres", "diag", traj, res)
    rtol = ref.gap_tolerance(hist, k, traj.rnorm0)
    res2 = backend.solve(h, s, Spec("minres", rtol=rtol, max_it=MINRES_STEPS), "diag")
    assert (res2.reason, res2.its, len(res2.history)) == (ref.CONVERGED_RTOL, k, k + 1)
    check_values(backend, s, "minres", "diag", traj, res2)
    return [res, res2]


# ---------------------------------------------------------------------------- C: divergence limit
C_LIMIT = 10.0


def c_guess(s, form, pc, factor):
    """``c * 1`` with monitored first residual ``factor`` times the reference norm."""
    Bv = s.diag if (pc == "diag" and form in ("left", "minres")) else np.ones(s.N)
    one = np.ones(s.N)
    c = factor * np.linalg.norm(Bv * s.b) / np.linalg.norm(Bv * (s.A @ one))
    return c * one, float(np.linalg.norm(Bv * (s.b - s.A @ (c * one))) / np.linalg.norm(Bv * s.b))


def check_c(backend, form, pc, names=("A24", "S24")):
    s = system(names[form == "minres"])
    h = backend.handle(s)
    x0, ratio = c_guess(s, form, pc, 4 * C_LIMIT)
    assert ratio >= 2 * C_LIMIT
    res = backend.solve(h, s, Spec(form, restart=3, divtol=C_LIMIT, max_it=5), pc, x0=x0)
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_DTOL, 0, 1)
    assert res.x.tobytes() == x0.tobytes()
    if res.op_applies >= 0:
        assert res.op_applies == 1
    x1, ratio = c_guess(s, form, pc, C_LIMIT / 4)
    assert 0 < ratio <= C_LIMIT / 2
    res2 = backend.solve(h, s, Spec(form, restart=3, divtol=C_LIMIT, max_it=5), pc, x0=x1)
    assert (res2.reason, res2.its, len(res2.history)) == (ref.DIVERGED_ITS, 5, 6)
    return [res, res2]


# --------------------------------------------------------- D: zero right-hand side and zero guess
def check_d(backend, form, pc, name="A24"):
    s = system(name)
    res = backend.solve(backend.handle(s), s, Spec(form, restart=3, rtol=1e-8, max_it=5), pc,
                        b=np.zeros(s.N))
    assert res.its == 0 and res.history.tolist() == [0.0]
    assert not res.x.any()
    if form != "minres":
        assert res.reason == ref.CONVERGED_ATOL
    # MINRES has no exact-zero exit of its own: its code is the convergence test's for a zero
    # norm (RTOL with atol = 0); the table leaves it open, so the oracle's reading stands and
    # the device test compares with it
    return [res]


D_ONE_RESTART = 3


def d_one_level_step(name, form, pc, part, level):
    """Case D with the data of one time level only -- on a time shard, of one rank: ``part`` is
    ``guess`` (zero right-hand side, the far guess non-zero in ``level`` alone: the convergence
    test's "zero RHS and nonzero guess" rule, the first residual in place of ``rnorm0``) or
    ``rhs`` (zero guess, the right-hand side non-zero in ``level`` alone).  Returns the reference
    trajectory, the norm the test is relative to and the first step in 2..6 whose gap is 1.5."""
    guess, rhs = (f"far@{level}", "zero") if part == "guess" else ("zero", f"b@{level}")
    traj = trajectory(name, form, pc, D_ONE_RESTART, guess, None, rhs)
    hist = traj.history
    if part == "guess":
        assert traj.rnorm0 == 0.0 and hist[0] > 0.0
    else:
        assert traj.rnorm0 > 0.0
    scale = float(hist[0]) if part == "guess" else traj.rnorm0
    steps = [k for k in range(2, 7) if hist[k - 1] / hist[k] >= 1.5]
    assert steps, (name, form, pc, part, level, hist)
    return traj, scale, steps[0]


def check_d_one_level(backend, name, form, pc, part, level):
    s = system(name)
    traj, scale, k = d_one_level_step(name, form, pc, part, level)
    rtol = ref.gap_tolerance(traj.history, k, scale)
    # the rule from the reference: a zero rnorm0 is replaced by the first norm seen
    assert ref.expected_stop(traj.history, traj.rnorm0, rtol=rtol, atol=0.0, divtol=NO_DIV,
                             max_it=50) == (ref.CONVERGED_RTOL, k)
    guess, rhs = (f"far@{level}", "zero") if part == "guess" else ("zero", f"b@{level}")
    res = backend.solve(backend.handle(s), s, Spec(form, restart=D_ONE_RESTART, rtol=rtol, max_it=50),
                        pc, x0=s.guesses[guess], b=s.rhs[rhs])
    assert (res.reason, res.its, len(res.history)) == (ref.CONVERGED_RTOL, k, k + 1), \
        (res.reason, res.its, len(res.history), k)
    check_values(backend, s, form, pc, traj, res, need_share=False)
    return [res]


# -------------------------------------------------------------------------- E: exact happy step
def check_e(backend, form, pc, name="two"):
    s = system(name)
    h = backend.handle(s, diagonal=True)
    first = float(np.linalg.norm(s.diag * s.b)) if (form == "left" and pc == "diag") else 1.0
    want_x = 0.5 * s.b
    out = []
    for atol, reason in ((0.0, ref.CONVERGED_RTOL), (1e-300, ref.CONVERGED_ATOL)):
        res = backend.solve(h, s, Spec(form, restart=5, rtol=1e-8, atol=atol, max_it=20), pc)
        assert (res.reason, res.its) == (reason, 1)
        assert res.history.tolist() == [first, 0.0]
        assert np.isfinite(res.x).all() and res.x.tobytes() == want_x.tobytes()
        out.append(res)
    return out


# --------------------------------------------------------------------------- F: singular breakdown
def check_f(backend, form, name="sing"):
    s = system(name)
    assert not (s.A @ s.b).any()
    h = backend.handle(s)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=1e-8, max_it=20), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_BREAKDOWN, 0, 1)
    assert res.history[0] == math.sqrt(2.0)
    assert not res.x.any()
    return [res]


# --------------------------------------------------------------------------- G: finite termination
def check_g_terminates(backend, form, d, prefix="eig"):
    s = system(f"{prefix}{d}")
    h = backend.handle(s, diagonal=True)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=1e-10, max_it=40), "id")
    assert (res.reason, res.its) == (ref.CONVERGED_RTOL, d)
    assert len(res.history) == d + 1
    assert res.history[-1] <= 1e-12 * res.history[0]
    exact = s.b / np.diag(s.A)
    assert np.linalg.norm(res.x - exact) <= 1e-12 * np.linalg.norm(exact)
    return [res]


G_GAP_STEP = 8       # d = 6 against restart 5: no finite termination; stop in the second cycle


def check_g_restarted(backend, form, name="eig6"):
    s = system(name)
    traj = trajectory(name, form, "id", 5, "zero", 12)
    hist = traj.history
    k = G_GAP_STEP
    assert hist[k - 1] / hist[k] >= 1.5 and hist[6] > 1e-6 * hist[0]
    rtol = ref.gap_tolerance(hist, k, traj.rnorm0)
    h = backend.handle(s, diagonal=True)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=rtol, max_it=40), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.CONVERGED_RTOL, k, k + 1)
    check_values(backend, s, form, "id", traj, res, need_share=False)
    return [res]


def check_g_long_restart(backend, form, name="A24"):
    s = system(name)
    h = backend.handle(s)
    res = backend.solve(h, s, Spec(form, restart=60, rtol=1e-8, max_it=200), "diag")
    assert res.reason == ref.CONVERGED_RTOL and 0 < res.its <= s.N
    assert len(res.history) == res.its + 1
    traj = trajectory(name, form, "diag", 10)         # the first ten steps are one cycle's
    assert res.its > 10
    want = traj.history[:11]
    bar = 10 * s.N * U_ROUND * kappa(name, form, "diag") * want[0] / want
    assert bar.max() < BAR_CAP
    assert np.all(np.abs(res.history[:11] - want) / want <= bar)
    r = s.b - s.A @ res.x
    assert np.linalg.norm(r) <= 1e-6 * np.linalg.norm(s.b)
    return [res]


# ---------------------------------------------------------------------------- H: non-finite values
H_RESTART = 3
# The step at which a NaN written by the callback's j-th application is seen, per form.
#   left      call 1 is ||B b|| (rnorm0), call 2 the first residual, call 2 + s step s
#   right     call s is step s of the first cycle, call m + 1 builds the cycle's solution, which
#             the next cycle's first residual (logged in place of step m) shows
#   flexible  call s is step s; no call when a solution is built
H_NAN_STEPS = {("left", 1): 0, ("left", 4): 2,
               ("right", 1): 1, ("right", 4): 3,
               ("flexible", 1): 1, ("flexible", 4): 4}


def check_h_nan(backend, form, call, name="A24", at=(0, 5)):
    """``at``: the (time level, entry) of variable 0 the NaN is written to."""
    s = system(name)
    h = backend.handle(s)
    spec = Spec(form, restart=H_RESTART, rtol=1e-12, max_it=12)
    res = backend.solve(h, s, spec, nan_pc(s, call, entry=at[1], level=at[0]))
    its = H_NAN_STEPS[form, call]
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, its, its + 1)
    clean = backend.solve(h, s, spec, "diag")
    fresh = backend.solve(backend.handle(s), s, spec, "diag")
    assert clean.reason == ref.DIVERGED_ITS and clean.same_bits(fresh)
    return [res, clean]


def check_h_nan_then_other_solver(backend, name="A24", at=(0, 5)):
    """A solve that ended non-finite leaves NaNs in the basis; the next solver on the handle
    (same arena: GMRES(10) holds the nine vectors MINRES wants) must not read them."""
    s = system(name)
    h = backend.handle(s)
    res = backend.solve(h, s, Spec("left", restart=10, rtol=1e-12, max_it=12),
                        nan_pc(s, 5, entry=at[1], level=at[0]))
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, 3, 4)
    out = [res]
    for spec in (Spec("minres", max_it=4), Spec("flexible", restart=6, max_it=8)):
        clean = backend.solve(h, s, spec, "diag")
        fresh = backend.solve(backend.handle(s), s, spec, "diag")
        assert np.isfinite(clean.history).all() and np.isfinite(clean.x).all()
        assert clean.same_bits(fresh), spec
        out.append(clean)
    return out


def check_h_inf(backend, form, name="A24", where=7):
    s = system(name)
    h = backend.handle(s)
    b = s.b.copy()
    b[where] = np.inf
    spec = Spec(form, restart=H_RESTART, rtol=1e-12, max_it=12)
    res = backend.solve(h, s, spec, "diag", b=b)
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, 0, 1)
    clean = backend.solve(h, s, spec, "diag")
    fresh = backend.solve(backend.handle(s), s, spec, "diag")
    assert clean.same_bits(fresh)
    return [res, clean]


# ----------------------------------------------------------------- I: MINRES, singular operator
def check_i(backend, name="mr4"):
    """``b`` is a one in two entries of the range and in two of the kernel of a diagonal of ones
    and zeros (``mr4``: nothing else; ``Lmr``: zeros elsewhere, so the numbers are the same)."""
    s = system(name)
    res = backend.solve(backend.handle(s), s, Spec("minres", rtol=1e-8, max_it=10), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_INDEFINITE_MAT, 2, 3)
    # a least-squares solution: the residual left is the part of b outside the range
    assert res.history[0] == 2.0 and abs(res.history[2] - math.sqrt(2.0)) <= 4e-16
    assert np.isfinite(res.x).all()
    assert np.abs(s.b - s.A @ res.x - s.b * (np.diag(s.A) == 0.0)).max() <= 1e-15
    return [res]


# --------------------------------------------------------------------------- J: workspace reuse
J_ORDER = (Spec("left", restart=10, max_it=21), Spec("left", restart=3, max_it=7),
           Spec("flexible", restart=6, max_it=13), Spec("minres", max_it=9),
           Spec("left", restart=10, max_it=21))


def check_j(backend, name="A24"):
    s = system(name)
    h = backend.handle(s)
    out = []
    for spec in J_ORDER:
        res = backend.solve(h, s, spec, "diag")
        fresh = backend.solve(backend.handle(s), s, spec, "diag")
        assert res.same_bits(fresh), spec
        assert len(res.history) == res.its + 1
        out.append(res)
    assert out[0].same_bits(out[-1])
    return out


# ----------------------------------------------------------------------------- L: Python layer
def l_cases(names=("A24", "sing")):
    s = system(names[0])
    x_far, _ = c_guess(s, "left", "diag", 4 * C_LIMIT)
    return {ref.DIVERGED_ITS: (s, Spec("left", restart=3, max_it=4), "diag", None),
            ref.DIVERGED_DTOL: (s, Spec("left", restart=3, divtol=C_LIMIT, max_it=5), "diag", x_far),
            ref.DIVERGED_BREAKDOWN: (system(names[1]), Spec("left", restart=5, rtol=1e-8, max_it=20),
                                     "id", None),
            ref.DIVERGED_NANORINF: (s, Spec("flexible", restart=3, rtol=1e-12, max_it=12),
                                    ("nan", 1), None)}


def check_l(backend, reason, names=("A24", "sing"), at=(0, 5)):
    import pytest
    s, spec, pc, x0 = l_cases(names)[reason]

    def the_pc():
        return nan_pc(s, pc[1], entry=at[1], level=at[0]) if isinstance(pc, tuple) else pc
    h = backend.handle(s)
    res = backend.solve(h, s, spec, the_pc(), x0=x0)
    assert res.reason == reason
    with pytest.raises(RuntimeError, match="Solver failed to converge"):
        backend.solve(h, s, replace(spec, keep=False), the_pc(), x0=x0)
    return [res]


# ------------------------------------------------------------- K: device vectors of the handle
K_LAYER_CASES = (("L5", "far", "left", 3, 7), ("L5", "far", "flexible", 10, 11),
                 ("L5", "far", "right", 3, 4), ("LS5", "zero", "minres", 10, 6))


def check_k(backend, name, guess, form, m, max_it):
    """The solve on vectors of the handle (``backend.pointer()``: ``kkt_solve_device``) is the
    solve on host arrays bit for bit."""
    s = system(name)
    spec = Spec(form, restart=m, max_it=max_it)
    host = backend.solve(backend.handle(s), s, spec, "diag", x0=s.guesses[guess])
    ptr = backend.pointer()
    dev = ptr.solve(ptr.handle(s), s, spec, "diag", x0=s.guesses[guess])
    assert (host.reason, host.its) == (ref.DIVERGED_ITS, max_it)
    assert dev.same_bits(host) and dev.op_applies == host.op_applies
    return [host, dev]


# ------------------------------------------------- the table on the layered systems, as a list
LAYER_LEVELS = (0, 2, 4)     # of m = 5: owned by the first, a middle and the last rank of 3 and 5
H_LAYER_ENTRY = 3
PC_COMBOS = tuple((f, "diag") for f in GMRES_FORMS + ("minres",)) + (("left", "id"),)


def layer_cases():
    """``(id, name of the check, arguments, keyword arguments)`` of every case the layered
    systems run, in the order the ranks of a time shard go through them."""
    out = []

    def add(case_id, fn, *args, **kw):
        out.append((case_id, fn, args, kw))
    for name, form, pc, m in A_LAYER_COMBOS:
        add(f"a-{name}-{form}-{pc}-{m}", "check_a", name, form, pc, m)
    for name, form, pc, guess in B_LAYER_COMBOS:
        add(f"b-{name}-{form}-{pc}-{guess}", "check_b", name, form, pc, guess)
    add("b-minres", "check_minres_values", name="LS5")
    for form, pc in PC_COMBOS:
        add(f"c-{form}-{pc}", "check_c", form, pc, names=("L5", "LS5"))
        add(f"d-{form}-{pc}", "check_d", form, pc, name="L5")
    for form in GMRES_FORMS:
        for part in ("guess", "rhs"):
            for level in LAYER_LEVELS:
                add(f"d-{part}-on-level-{level}-{form}", "check_d_one_level", "L5", form, "diag",
                    part, level)
    for form in GMRES_FORMS:
        for pc in ("id", "diag"):
            add(f"e-{form}-{pc}", "check_e", form, pc, name="Ltwo")
        add(f"f-{form}", "check_f", form, name="Lsing")
        for d in (3, 5):
            add(f"g-terminates-{form}-{d}", "check_g_terminates", form, d, prefix="Leig")
        add(f"g-restarted-{form}", "check_g_restarted", form, name="Leig6")
        add(f"g-long-restart-{form}", "check_g_long_restart", form, name="L5")
    add("g-terminates-minres-6", "check_g_terminates", "minres", 6, prefix="Leig")
    for level in LAYER_LEVELS:
        at = (level, H_LAYER_ENTRY)
        for form, call in sorted(H_NAN_STEPS):
            add(f"h-nan-{form}-{call}-level-{level}", "check_h_nan", form, call, name="L5", at=at)
        add(f"h-nan-then-other-level-{level}", "check_h_nan_then_other_solver", name="L5", at=at)
        for form in GMRES_FORMS + ("minres",):
            add(f"h-inf-{form}-level-{level}", "check_h_inf", form, name="L5",
                where=level * LAYER_NX + H_LAYER_ENTRY)
    add("i-minres-singular", "check_i", name="Lmr")
    add("j-one-handle", "check_j", name="L5")
    for name, guess, form, m, max_it in K_LAYER_CASES:
        add(f"k-{name}-{form}-{m}", "check_k", name, guess, form, m, max_it)
    for reason in sorted(l_cases(("L5", "Lsing"))):
        add(f"l-{-reason}", "check_l", reason, names=("L5", "Lsing"), at=(4, H_LAYER_ENTRY))
    assert len({c[0] for c in out}) == len(out)
    return out


def run_case(backend, case):
    _, fn, args, kw = case
    return globals()[fn](backend, *args, **kw)


def layer_trajectories():
    """Every reference trajectory the layered cases read, as ``Traj``: computed once, by going
    through the list on the oracle, for ``preload_trajectories`` in the ranks of a sharded run
    (a rank computes for itself whatever it does not find)."""
    oracle = OracleBackend()
    for case in layer_cases():
        try:
            run_case(oracle, case)
        except AssertionError:
            pass                  # the oracle's own test reports it; the reference was read
    return {k: Traj(np.array(t.history), [np.array(x) for x in t.iterates], float(t.rnorm0))
            for k, t in _TRAJ.items() if k[0] in LAYERS}


def preload_trajectories(trajectories):
    for k, t in trajectories.items():
        _TRAJ.setdefault(k, t)
