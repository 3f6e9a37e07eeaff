"""Exact P2-P1 convection element matrices in rational arithmetic (no quadrature).

The velocity element matrix ``N[a][b] = int phi_a (w . grad phi_b)`` with ``w`` the P2 interpolant
of nodal values has degree 5 per triangle, the pressure one ``int lam_c (w . grad lam_d)`` degree
3; both are sums of barycentric monomials, integrated by

    int lam_0^i lam_1^j lam_2^k = 2A i! j! k! / (i + j + k + 2)!.

Doubles (coordinates, nodal values) are taken as the rationals they are, so the result is the
exact value of the form for the data as stored.  Nothing here reads the quadrature tables of
``control_amd.fem``; only the local dof order is shared: vertices 0, 1, 2, then the midpoints of
the edges (0, 1), (1, 2), (0, 2).  ``scales`` is the exception by design: the magnitude a
rounding error is measured against is the quadrature sum of ``fem.py`` with every factor replaced
by its absolute value, so it takes those tables as an argument.  Imported like ``common``.
"""
from fractions import Fraction
from math import factorial

import numpy as np

U = 2.0 ** -53


# ---------------------------------------------------------------- polynomials in (lam_0, lam_1, lam_2)
def _mul(p, q):
    out = {}
    for (a, ca) in p.items():
        for (b, cb) in q.items():
            k = (a[0] + b[0], a[1] + b[1], a[2] + b[2])
            out[k] = out.get(k, 0) + ca * cb
    return out


def _integral(p):
    """int p over the triangle, divided by 2A."""
    return sum((c * Fraction(factorial(i) * factorial(j) * factorial(k),
                             factorial(i + j + k + 2)) for (i, j, k), c in p.items()),
               Fraction(0))


def _e(k, n=1):
    return tuple(n if d == k else 0 for d in range(3))


def _p2_basis():
    """phi_a and d phi_a / d lam_k (the lam_k as independent variables)."""
    phi, dphi = [], []
    for k in range(3):                       # lam_k (2 lam_k - 1)
        phi.append({_e(k, 2): Fraction(2), _e(k): Fraction(-1)})
        dphi.append([{_e(k): Fraction(4), (0, 0, 0): Fraction(-1)} if d == k else {}
                     for d in range(3)])
    for (i, j) in ((0, 1), (1, 2), (0, 2)):  # 4 lam_i lam_j
        key = tuple(int(d in (i, j)) for d in range(3))
        phi.append({key: Fraction(4)})
        dphi.append([{_e(j): Fraction(4)} if d == i else {_e(i): Fraction(4)} if d == j else {}
                     for d in range(3)])
    return phi, dphi


_PHI, _DPHI = _p2_basis()
_LAM = [{_e(k): Fraction(1)} for k in range(3)]
# T[c][a][b][k] = (1 / 2A) int phi_c phi_a d phi_b / d lam_k;  PL[c][a] = (1 / 2A) int phi_c lam_a
T = [[[[_integral(_mul(_mul(_PHI[c], _PHI[a]), _DPHI[b][k])) for k in range(3)]
       for b in range(6)] for a in range(6)] for c in range(6)]
PL = [[_integral(_mul(_PHI[c], _LAM[a])) for a in range(3)] for c in range(6)]


def triangle_geometry(xy):
    """``(2A, g)``: twice the area and ``g[k][d] = d lam_k / d x_d`` of the triangle with the
    vertex coordinates ``xy`` (3 x 2), exactly."""
    (x0, y0), (x1, y1), (x2, y2) = [[Fraction(float(v)) for v in p] for p in xy]
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    g = [[(y1 - y2) / det, (x2 - x1) / det], [(y2 - y0) / det, (x0 - x2) / det],
         [(y0 - y1) / det, (x1 - x0) / det]]
    return abs(det), g


def element_matrices(xy, wx, wy):
    """Exact ``(Nv, Np)`` (6 x 6 and 3 x 3 nested lists of ``Fraction``) on one triangle: ``xy``
    its vertices, ``wx`` / ``wy`` the six nodal values of the wind's components."""
    A2, g = triangle_geometry(xy)
    w = [[Fraction(float(v)) for v in wx], [Fraction(float(v)) for v in wy]]
    # s[c][k] = sum_d w_d,c d lam_k / d x_d: the wind's nodal values along grad lam_k
    s = [[w[0][c] * g[k][0] + w[1][c] * g[k][1] for k in range(3)] for c in range(6)]
    Nv = [[A2 * sum(s[c][k] * T[c][a][b][k] for c in range(6) for k in range(3))
           for b in range(6)] for a in range(6)]
    Np = [[A2 * sum(s[c][d] * PL[c][a] for c in range(6)) for d in range(3)] for a in range(3)]
    return Nv, Np


def mesh_element_matrices(th, w):
    """``element_matrices`` of every triangle of a ``fem.rectangle_p2p1`` discretisation (its
    connectivity and node coordinates, not its tables) for the wind ``w`` (component-major):
    object arrays (ne, 6, 6) and (ne, 3, 3) of ``Fraction``."""
    V = th.elem["V"]
    n2 = th.n_v // 2
    Nv = np.empty((len(V), 6, 6), dtype=object)
    Np = np.empty((len(V), 3, 3), dtype=object)
    for e, nodes in enumerate(V):
        a, b = element_matrices(th.coords_v[nodes[:3]], w[:n2][nodes], w[n2:][nodes])
        Nv[e], Np[e] = a, b
    return Nv, Np


def scales(elem, n2, w):
    """``(Sv, Sp)``: the quadrature sums of the two forms with every factor replaced by its
    absolute value,
    ``Sv[e, a, b] = sum_q W_eq |phi_qa| sum_d |gphi_eqbd| sum_c |phi_qc| |w_d,c|`` and
    ``Sp[e, a, b] = sum_q W_eq |lam_qa| sum_d |glam_ebd| sum_c |phi_qc| |w_d,c|``."""
    V = elem["V"]
    aphi = np.abs(elem["phi"])
    wq = np.stack([np.abs(w[:n2][V]) @ aphi.T, np.abs(w[n2:][V]) @ aphi.T], axis=2)  # (ne, nq, 2)
    adv = np.einsum("eqbd,eqd->eqb", np.abs(elem["gphi"]), wq)
    Sv = np.einsum("eq,qa,eqb->eab", np.abs(elem["W"]), aphi, adv)
    advp = np.einsum("ebd,eqd->eqb", np.abs(elem["glam"]), wq)
    Sp = np.einsum("eq,qa,eqb->eab", np.abs(elem["W"]), np.abs(elem["lam"]), advp)
    return Sv, Sp


def worst_ratio(got, exact, S, factor=1.0):
    """max over entries of ``|got - exact| / (factor u S)`` with the error taken exactly; an
    entry whose scale is zero must be exact (ratio ``inf`` otherwise)."""
    worst = 0.0
    for x, r, s in zip(np.ravel(got), np.ravel(exact), np.ravel(S)):
        err = abs(Fraction(float(x)) - r)
        if err == 0:
            continue
        if s == 0.0:
            return float("inf")
        worst = max(worst, float(err / (Fraction(factor * U) * Fraction(float(s)))))
    return worst
