"""The case table of the stopping-rule tests, shared by the oracle test on the CPU
(``test_krylov_stop_ref.py``) and the device test (``test_gpu_krylov_stopping.py``).

Systems are two-variable block systems with one CSR block per quadrant, no nullspaces, and
``N = 2 nx`` unknowns with ``nx`` in {24, 33} (or 2 for the MINRES instance): neither 48 nor 66
is a multiple of 32 or of the double2 width.  The dense matrix the reference works on is
``np.block`` of the same arrays.  Preconditioners are the identity (``pc_fn=None``) and a host
callback that multiplies by a fixed positive diagonal, so ``B`` is known exactly.

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
class Sys:
    def __init__(self, name, A, b, nx, diag=None):
        self.name, self.nx, self.N = name, nx, 2 * nx
        self.A = np.array(A, dtype=np.float64)
        self.b = np.array(b, dtype=np.float64)
        # the fixed positive diagonal of the callback preconditioner
        self.diag = (0.5 + np.random.default_rng(77).random(self.N)) if diag is None \
            else np.array(diag, dtype=np.float64)
        self.guesses = {"zero": np.zeros(self.N)}

    def blocks(self):
        """The four quadrants as one-entry block dictionaries of CSR matrices with every entry
        stored (explicit zeros too: the structure is the dense one)."""
        nx = self.nx

        def quad(i, j):
            M = self.A[i * nx:(i + 1) * nx, j * nx:(j + 1) * nx]
            ip = np.arange(0, nx * nx + 1, nx, dtype=np.int32)
            ix = np.tile(np.arange(nx, dtype=np.int32), nx)
            return {(0, 0): sp.csr_matrix((M.ravel().copy(), ix, ip), shape=(nx, nx))}
        return quad(0, 0), quad(0, 1), quad(1, 0), quad(1, 1)

    def diag_blocks(self):
        """Diagonal operators as diagonal CSR blocks, no couplings."""
        nx = self.nx
        d = np.diag(self.A)
        assert np.array_equal(self.A, np.diag(d))
        none = {(0, 0): None}
        return ({(0, 0): sp.diags(d[:nx], format="csr")}, dict(none), dict(none),
                {(0, 0): sp.diags(d[nx:], format="csr")})

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
    nx, d = s.nx, s.diag

    def pc(u_0, u_1, b_0, b_1):
        u_0[:] = d[:nx] * b_0
        u_1[:] = d[nx:] * b_1
    return pc


def nan_pc(s, call, entry=5):
    """The diagonal preconditioner, but its ``call``-th application (1-based) returns NaN in
    one entry."""
    inner, n = diag_pc(s), [0]

    def pc(u_0, u_1, b_0, b_1):
        inner(u_0, u_1, b_0, b_1)
        n[0] += 1
        if n[0] == call:
            u_0[0, entry] = np.nan
    return pc


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

    def handle(self, s, diagonal=False):
        return self.ko.OracleSystem(s.nx, s.nx, *(s.diag_blocks() if diagonal else s.blocks()))

    def solve(self, h, s, spec, pc="id", x0=None, b=None):
        x = np.array(s.guesses["zero"] if x0 is None else x0, dtype=np.float64)
        b = s.b if b is None else b
        u0, u1 = x[:s.nx].reshape(1, -1), x[s.nx:].reshape(1, -1)
        with np.errstate(all="ignore"):
            r = h.solve(u0, u1, b[:s.nx].reshape(1, -1), b[s.nx:].reshape(1, -1),
                        solver_parameters=spec.parameters(), pc_fn=make_pc(s, pc))
        return Result(int(r.reason), int(r.its), np.array(r.history, dtype=np.float64), x)


# ---------------------------------------------------------------------------------- reference
def ref_steps(restart):
    return max(2 * restart + 1, restart + 3)


@functools.lru_cache(maxsize=None)
def trajectory(name, form, pc, restart, guess="zero", steps=None):
    """Reference history and iterates, computed once per (system, form, restart, guess) at the
    longest length any case asks for.  ``flexible`` with a fixed ``B`` is ``right``."""
    s = system(name)
    steps = ref_steps(restart) if steps is None else steps
    if form == "minres":
        return ref.minres_trajectory(s.A, s.B(pc), s.b, s.guesses[guess], steps)
    if form == "flexible":
        return trajectory(name, "right", pc, restart, guess, steps)
    return ref.gmres_trajectory(s.A, s.B(pc), s.b, s.guesses[guess], restart, form, steps)


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


def check_minres_values(backend):
    """MINRES on the symmetric positive definite instance with the diagonal callback: the
    monitored recurrence against the reference's B-norm minimiser, and one threshold."""
    s = system("S24")
    traj = trajectory("S24", "minres", "diag", 0, "zero", MINRES_STEPS)
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


def check_c(backend, form, pc):
    s = system("S24" if form == "minres" else "A24")
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
def check_d(backend, form, pc):
    s = system("A24")
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


# -------------------------------------------------------------------------- E: exact happy step
def check_e(backend, form, pc):
    s = system("two")
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
def check_f(backend, form):
    s = system("sing")
    assert not (s.A @ s.b).any()
    h = backend.handle(s)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=1e-8, max_it=20), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_BREAKDOWN, 0, 1)
    assert res.history[0] == math.sqrt(2.0)
    assert not res.x.any()
    return [res]


# --------------------------------------------------------------------------- G: finite termination
def check_g_terminates(backend, form, d):
    s = system(f"eig{d}")
    h = backend.handle(s, diagonal=True)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=1e-10, max_it=40), "id")
    assert (res.reason, res.its) == (ref.CONVERGED_RTOL, d)
    assert len(res.history) == d + 1
    assert res.history[-1] <= 1e-12 * res.history[0]
    exact = s.b / np.diag(s.A)
    assert np.linalg.norm(res.x - exact) <= 1e-12 * np.linalg.norm(exact)
    return [res]


G_GAP_STEP = 8       # d = 6 against restart 5: no finite termination; stop in the second cycle


def check_g_restarted(backend, form):
    s = system("eig6")
    traj = trajectory("eig6", form, "id", 5, "zero", 12)
    hist = traj.history
    k = G_GAP_STEP
    assert hist[k - 1] / hist[k] >= 1.5 and hist[6] > 1e-6 * hist[0]
    rtol = ref.gap_tolerance(hist, k, traj.rnorm0)
    h = backend.handle(s, diagonal=True)
    res = backend.solve(h, s, Spec(form, restart=5, rtol=rtol, max_it=40), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.CONVERGED_RTOL, k, k + 1)
    check_values(backend, s, form, "id", traj, res, need_share=False)
    return [res]


def check_g_long_restart(backend, form):
    s = system("A24")
    h = backend.handle(s)
    res = backend.solve(h, s, Spec(form, restart=60, rtol=1e-8, max_it=200), "diag")
    assert res.reason == ref.CONVERGED_RTOL and 0 < res.its <= s.N
    assert len(res.history) == res.its + 1
    traj = trajectory("A24", form, "diag", 10)        # the first ten steps are one cycle's
    assert res.its > 10
    want = traj.history[:11]
    bar = 10 * s.N * U_ROUND * kappa("A24", form, "diag") * want[0] / want
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


def check_h_nan(backend, form, call):
    s = system("A24")
    h = backend.handle(s)
    spec = Spec(form, restart=H_RESTART, rtol=1e-12, max_it=12)
    res = backend.solve(h, s, spec, nan_pc(s, call))
    its = H_NAN_STEPS[form, call]
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, its, its + 1)
    clean = backend.solve(h, s, spec, "diag")
    fresh = backend.solve(backend.handle(s), s, spec, "diag")
    assert clean.reason == ref.DIVERGED_ITS and clean.same_bits(fresh)
    return [res, clean]


def check_h_nan_then_other_solver(backend):
    """A solve that ended non-finite leaves NaNs in the basis; the next solver on the handle
    (same arena: GMRES(10) holds the nine vectors MINRES wants) must not read them."""
    s = system("A24")
    h = backend.handle(s)
    res = backend.solve(h, s, Spec("left", restart=10, rtol=1e-12, max_it=12), nan_pc(s, 5))
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, 3, 4)
    out = [res]
    for spec in (Spec("minres", max_it=4), Spec("flexible", restart=6, max_it=8)):
        clean = backend.solve(h, s, spec, "diag")
        fresh = backend.solve(backend.handle(s), s, spec, "diag")
        assert np.isfinite(clean.history).all() and np.isfinite(clean.x).all()
        assert clean.same_bits(fresh), spec
        out.append(clean)
    return out


def check_h_inf(backend, form):
    s = system("A24")
    h = backend.handle(s)
    b = s.b.copy()
    b[7] = np.inf
    spec = Spec(form, restart=H_RESTART, rtol=1e-12, max_it=12)
    res = backend.solve(h, s, spec, "diag", b=b)
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_NANORINF, 0, 1)
    clean = backend.solve(h, s, spec, "diag")
    fresh = backend.solve(backend.handle(s), s, spec, "diag")
    assert clean.same_bits(fresh)
    return [res, clean]


# ----------------------------------------------------------------- I: MINRES, singular operator
def check_i(backend):
    s = system("mr4")
    res = backend.solve(backend.handle(s), s, Spec("minres", rtol=1e-8, max_it=10), "id")
    assert (res.reason, res.its, len(res.history)) == (ref.DIVERGED_INDEFINITE_MAT, 2, 3)
    # a least-squares solution: the residual left is the part of b outside the range
    assert res.history[0] == 2.0 and abs(res.history[2] - math.sqrt(2.0)) <= 4e-16
    assert np.isfinite(res.x).all()
    assert np.abs(s.b - s.A @ res.x - [0.0, 0.0, 1.0, 1.0]).max() <= 1e-15
    return [res]


# --------------------------------------------------------------------------- J: workspace reuse
J_ORDER = (Spec("left", restart=10, max_it=21), Spec("left", restart=3, max_it=7),
           Spec("flexible", restart=6, max_it=13), Spec("minres", max_it=9),
           Spec("left", restart=10, max_it=21))


def check_j(backend):
    s = system("A24")
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
def l_cases():
    s = system("A24")
    x_far, _ = c_guess(s, "left", "diag", 4 * C_LIMIT)
    return {ref.DIVERGED_ITS: (s, Spec("left", restart=3, max_it=4), "diag", None),
            ref.DIVERGED_DTOL: (s, Spec("left", restart=3, divtol=C_LIMIT, max_it=5), "diag", x_far),
            ref.DIVERGED_BREAKDOWN: (system("sing"), Spec("left", restart=5, rtol=1e-8, max_it=20),
                                     "id", None),
            ref.DIVERGED_NANORINF: (s, Spec("flexible", restart=3, rtol=1e-12, max_it=12),
                                    ("nan", 1), None)}


def check_l(backend, reason):
    import pytest
    s, spec, pc, x0 = l_cases()[reason]

    def the_pc():
        return nan_pc(s, pc[1]) if isinstance(pc, tuple) else pc
    h = backend.handle(s)
    res = backend.solve(h, s, spec, the_pc(), x0=x0)
    assert res.reason == reason
    with pytest.raises(RuntimeError, match="Solver failed to converge"):
        backend.solve(h, s, replace(spec, keep=False), the_pc(), x0=x0)
    return [res]
