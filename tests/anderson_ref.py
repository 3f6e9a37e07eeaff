"""Independent reference for the Anderson mixer (``control_amd/anderson.py``, ``kkt_anderson_*``).

Plain Python: ``fractions`` for the dot products (exact), ``mpmath`` at 60 digits for the Cholesky
factor and the solve, Python floats -- one rounding per operation -- for the unfused step.  Nothing
of ``control_amd/`` or ``oracle/`` is imported; NumPy only carries arrays in and out.
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 60
U = 2.0 ** -53           # unit round-off of binary64


def exact_dot(a, b):
    """``<a, b>`` as a Fraction."""
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))


def abs_dot(a, b):
    """``sum |a_i b_i|``, correctly rounded."""
    return math.fsum(abs(float(x) * float(y)) for x, y in zip(a, b))


def dot_bound(a, b):
    """The forward error bound of a length-n dot product in any summation order, fused or not:
    ``n u sum |a_i b_i|``."""
    return len(a) * U * abs_dot(a, b)


def gram_exact(dF, f):
    """``(G, r)`` of the columns ``dF`` (oldest first) and ``f`` as Fractions."""
    c = len(dF)
    G = [[exact_dot(dF[i], dF[j]) for j in range(c)] for i in range(c)]
    return G, [exact_dot(dF[i], f) for i in range(c)]


def cholesky_mp(G):
    """The unpivoted Cholesky factor of ``G`` at 60 digits (``None`` when a pivot is not
    positive) and ``max L_ii / min L_ii``."""
    with mp.workdps(DPS):
        c = len(G)
        L = mp.zeros(c, c)
        for i in range(c):
            for j in range(i + 1):
                s = mp.mpf(G[i][j]) - sum(L[i, k] * L[j, k] for k in range(j))
                if j < i:
                    L[i, j] = s / L[j, j]
                elif s <= 0:
                    return None, mp.inf
                else:
                    L[i, i] = mp.sqrt(s)
        d = [L[i, i] for i in range(c)]
        return L, (max(d) / min(d) if c else mp.mpf(1))


def solve_mp(G, r):
    """``gamma = G^-1 r`` at 60 digits (floats out), and the factor's diagonal ratio."""
    with mp.workdps(DPS):
        c = len(r)
        L, ratio = cholesky_mp([[float(G[i][j]) for j in range(c)] for i in range(c)])
        assert L is not None
        y = [mp.mpf(0)] * c
        for i in range(c):
            y[i] = (mp.mpf(float(r[i])) - sum(L[i, k] * y[k] for k in range(i))) / L[i, i]
        g = [mp.mpf(0)] * c
        for i in range(c - 1, -1, -1):
            g[i] = (y[i] - sum(L[k, i] * g[k] for k in range(i + 1, c))) / L[i, i]
        return np.array([float(x) for x in g]), float(ratio)


def gamma_bound(c, ratio):
    """Relative error of ``gamma`` from Cholesky and two triangular solves in double on the
    normal equations: ``4 c^3 u (max L_ii / min L_ii)^2``."""
    return 4.0 * c ** 3 * U * ratio ** 2


def mix_unfused(f, dX, dF, gamma, beta):
    """The step statement element by element in Python floats: every product and sum rounded on
    its own, columns oldest first."""
    out = np.empty(len(f))
    for i in range(len(f)):
        s = beta * float(f[i])
        for j in range(len(gamma)):
            t = float(dX[j][i]) + beta * float(dF[j][i])
            s = s - float(gamma[j]) * t
        out[i] = s
    return out


def expected_ring(fs, ss, depth, drops):
    """The pairs the statement keeps after the call that received ``fs[-1]``: ``fs`` the inputs
    and ``ss`` the steps of the calls so far (``ss`` one shorter), ``drops`` the pairs each call
    dropped.  Returns ``(dF, dX)``, oldest first, in double (the differences rounded once)."""
    dF, dX = [], []
    for k in range(1, len(fs)):
        dF.append(np.asarray(fs[k]) - np.asarray(fs[k - 1]))
        dX.append(np.asarray(ss[k - 1]))
        del dF[:-depth], dX[:-depth]
        del dF[:drops[k]], dX[:drops[k]]
    return dF, dX
