"""Independent reference for the stopping rules of the Krylov loops.

Plain Python on ``mpmath`` numbers (60 digits) with NumPy only for input and output; nothing of
``oracle/`` or ``control_amd/`` is imported.  The loops under test (``System::solve_once`` /
``System::solve_minres`` and their restatement ``oracle/kkt_oracle.py``) run Arnoldi / Lanczos
recurrences with Hessenberg matrices and Givens rotations.  None of that is here: on a system of a
few dozen unknowns the norms restarted GMRES reports are the *minimal residual norms over the
Krylov space*, and those follow from a projection at 60 digits.

Within a cycle that starts at ``x`` with ``r = b - A x``:

  left      monitored residual  B r,  space K_k(BA, B r),  correction z       in the space
  right     monitored residual  r,    space K_k(AB, r),    correction z = B z', z' in the space
  flexible  = right (the preconditioner here is a fixed matrix)

The residual after ``k`` steps is the cycle's initial (monitored) residual minus its orthogonal
projection onto ``Op K_k``; the projection uses twice-applied Gram-Schmidt.  The iterate is ``x``
plus the minimiser.  At a restart the loops log the recomputed residual in place of the cycle's
last recurrence value; in exact arithmetic the two are the same number, so the history expected
of a run of ``its`` steps is ``[||res(x_0)||, ..., ||res(x_its)||]``: ``its + 1`` entries.

MINRES (left only, ``B`` diagonal positive or the identity): the loop monitors the recurrence
``||B r_0||_2 * prod |s_k|`` (``kkt_oracle.minres``).  ``prod |s_k|`` is the reduction of the
residual in the ``B`` norm, which MINRES minimises over ``K_k(BA, B r_0)``, so the monitored
number is ``||B r_0||_2 / ||r_0||_B * min ||b - A(x_0 + z)||_B``: the same projection with
``S = B^(1/2)``, operator ``S A S`` and residual ``S r``.  With ``B = I`` it is the plain
minimal residual norm.  On an operator that is not symmetric the loop's numbers are no minimal
residual norm of anything simple; there only counts and bitwise repeatability are compared.

``converged_default`` is the stopping rule, ``expected_stop`` applies it to a reference history.
"""
import math

import mpmath as mp
import numpy as np

DPS = 60
mp.mp.dps = DPS

CONVERGED_RTOL = 2
CONVERGED_ATOL = 3
DIVERGED_ITS = -3
DIVERGED_DTOL = -4
DIVERGED_BREAKDOWN = -5
DIVERGED_NANORINF = -9
DIVERGED_INDEFINITE_MAT = -10


# ------------------------------------------------------------------------ small linear algebra
def _vec(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return [[mp.mpf(float(v)) for v in row] for row in a]


def _matvec(M, v):
    return [mp.fdot(row, v) for row in M]


def _norm(v):
    return mp.sqrt(mp.fdot(v, v))


def _axpy(y, a, x):
    return [yi + a * xi for yi, xi in zip(y, x)]


def _orthogonalise(w, basis):
    """Twice-applied Gram-Schmidt of ``w`` against an orthonormal ``basis``; returns the
    remainder and the coefficients (summed over both passes)."""
    coef = [mp.mpf(0)] * len(basis)
    for _ in range(2):
        for j, q in enumerate(basis):
            c = mp.fdot(q, w)
            coef[j] += c
            w = _axpy(w, -c, q)
    return w, coef


class _System:
    """``A``, ``B`` and ``b`` as multiprecision rows; ``B`` is None (identity), a vector (its
    diagonal) or a dense matrix."""

    def __init__(self, A, B, b):
        self.A = _rows(A)
        self.n = len(self.A)
        self.b = _vec(b)
        if B is None:
            self.Bd, self.Bm = [mp.mpf(1)] * self.n, None
        elif np.ndim(B) == 1:
            self.Bd, self.Bm = _vec(B), None
        else:
            self.Bd, self.Bm = None, _rows(B)

    def mulA(self, v):
        return _matvec(self.A, v)

    def mulB(self, v):
        if self.Bm is not None:
            return _matvec(self.Bm, v)
        return [d * vi for d, vi in zip(self.Bd, v)]

    def mulS(self, v):          # B^(1/2), diagonal B only
        if self.Bm is not None:
            raise ValueError("the MINRES reference takes a diagonal B")
        return [mp.sqrt(d) * vi for d, vi in zip(self.Bd, v)]

    def residual(self, x):
        return _axpy(self.b, -1, self.mulA(x))


def _cycle(op, res0, steps):
    """Minimal-residual norms and minimisers over K_k(op, res0), k = 1..steps.

    Yields ``(norm_k, y_k)`` with ``y_k`` the minimiser in the space.  ``Q`` is an orthonormal
    basis of the Krylov space, ``P`` one of ``op Q`` with ``op Q = P R``; the residual is ``res0``
    less its components along ``P``.  Stops early when the space stops growing."""
    beta = _norm(res0)
    if beta == 0:
        return
    Q = [[v / beta for v in res0]]
    P, R, c = [], [], []
    res = list(res0)
    for k in range(steps):
        w = op(Q[k])
        p, col = _orthogonalise(list(w), P)
        pn = _norm(p)
        if pn <= mp.mpf(10) ** (-DPS + 15) * _norm(w):
            return                                  # op q_k already in op K_k: singular on it
        p = [v / pn for v in p]
        P.append(p)
        R.append(col + [pn])                        # column k of R
        ck = mp.fdot(p, res)
        c.append(ck)
        res = _axpy(res, -ck, p)
        # y = R^-1 c, coefficients on Q
        y = [mp.mpf(0)] * (k + 1)
        for i in range(k, -1, -1):
            s = c[i]
            for j in range(i + 1, k + 1):
                s -= R[j][i] * y[j]
            y[i] = s / R[i][i]
        z = [mp.mpf(0)] * len(res0)
        for yi, q in zip(y, Q):
            z = _axpy(z, yi, q)
        yield _norm(res), z
        q, _ = _orthogonalise(list(w), Q)
        qn = _norm(q)
        if qn <= mp.mpf(10) ** (-DPS + 15) * _norm(w):
            return                                  # invariant subspace: the residual is zero
        Q.append([v / qn for v in q])


class Trajectory:
    """``history[k]`` and ``iterates[k]`` after ``k`` steps, ``k = 0..steps`` (fewer where the
    Krylov space stopped growing); ``rnorm0`` the norm the convergence test is relative to."""

    def __init__(self, history, iterates, rnorm0):
        self.history_mp = history
        self.history = np.array([float(h) for h in history])
        self.iterates_mp = iterates
        self.iterates = [np.array([float(v) for v in x]) for x in iterates]
        self.rnorm0 = float(rnorm0)


def gmres_trajectory(A, B, b, x0, restart, form, steps):
    """Restarted GMRES(``restart``) in the form ``left`` / ``right`` / ``flexible``."""
    if form not in ("left", "right", "flexible"):
        raise ValueError(form)
    S = _System(A, B, b)
    left = form == "left"
    if left:
        def op(v):
            return S.mulB(S.mulA(v))
        rnorm0 = _norm(S.mulB(S.b))
    else:
        def op(v):
            return S.mulA(S.mulB(v))
        rnorm0 = _norm(S.b)

    def monitored(x):
        r = S.residual(x)
        return S.mulB(r) if left else r

    x = _vec(x0)
    hist, iters = [_norm(monitored(x))], [x]
    while len(hist) <= steps:
        k_max = min(restart, steps + 1 - len(hist))
        grown = 0
        for rn, z in _cycle(op, monitored(x), k_max):
            dz = z if left else S.mulB(z)
            iters.append(_axpy(x, 1, dz))
            hist.append(rn)
            grown += 1
        if grown < k_max:
            break
        x = iters[-1]
        # the loops log the recomputed residual here; exact arithmetic makes it the same number
        assert abs(_norm(monitored(x)) - hist[-1]) <= mp.mpf(10) ** (-DPS + 20) * hist[0]
    return Trajectory(hist, iters, rnorm0)


def minres_trajectory(A, B, b, x0, steps):
    """Preconditioned MINRES on symmetric ``A`` with diagonal positive ``B`` (or None): the
    monitored recurrence norm and the iterates (see the module text)."""
    S = _System(A, B, b)

    def op(v):
        return S.mulS(S.mulA(S.mulS(v)))

    x = _vec(x0)
    r0 = S.residual(x)
    n_b = _norm(S.mulB(r0))
    n_s = _norm(S.mulS(r0))
    hist, iters = [n_b], [x]
    for rn, z in _cycle(op, S.mulS(r0), steps):
        hist.append(rn * n_b / n_s)
        iters.append(_axpy(x, 1, S.mulS(z)))
    return Trajectory(hist, iters, _norm(S.mulB(S.b)))


# ------------------------------------------------------------------------------ stopping rule
class converged_default:
    """The default convergence test with the norm of the (preconditioned) right-hand side as
    ``rnorm0`` -- ``||B b||`` for ``left`` and MINRES, ``||b||`` for ``right`` and ``flexible``,
    never the first residual.  Call it with each monitored norm in turn; 0 means continue."""

    def __init__(self, rtol, atol, divtol, rnorm0):
        self.rtol, self.atol, self.divtol, self.rnorm0 = rtol, atol, divtol, rnorm0

    def __call__(self, rn):
        if not (math.isfinite(rn) and math.isfinite(self.rnorm0)):
            return DIVERGED_NANORINF
        if self.rnorm0 == 0.0:
            self.rnorm0 = rn                 # zero right-hand side, non-zero guess
        ttol = max(self.rtol * self.rnorm0, self.atol)
        if rn <= ttol:
            return CONVERGED_ATOL if rn < self.atol else CONVERGED_RTOL
        if rn >= self.divtol * self.rnorm0:
            return DIVERGED_DTOL
        return 0


def expected_stop(history, rnorm0, *, rtol, atol, divtol, max_it):
    """``(reason, its)`` the loops must report when their norms are ``history``."""
    conv = converged_default(rtol, atol, divtol, rnorm0)
    for its, rn in enumerate(history):
        reason = conv(float(rn))
        if reason:
            return reason, its
        if its >= max_it:
            return DIVERGED_ITS, its
    raise ValueError("the history ends before any rule fires")


def gap_tolerance(history, k, scale=1.0):
    """Geometric mean of entries ``k - 1`` and ``k`` over ``scale``: a threshold that step ``k``
    is the first to pass, as far from both neighbours as it can be."""
    return math.sqrt(float(history[k - 1]) * float(history[k])) / scale
