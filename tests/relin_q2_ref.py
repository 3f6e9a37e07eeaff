"""Exact Q2-Q1 convection element matrices in rational arithmetic (no quadrature), in the manner
of ``tests/relin_ref.py``.

On an axis-parallel cell ``[x0, x0 + hx] x [y0, y0 + hy]`` the velocity element matrix
``N[a][b] = int phi_a (w . grad phi_b)`` with ``w`` the Q2 interpolant of nodal values is

    sum_c  wx_c hy T[c][a][b][0] + wy_c hx T[c][a][b][1],
    T[c][a][b][k] = int over the unit square of  phi_c phi_a d phi_b / d x_k,

and the pressure one ``int lam_c (w . grad lam_d)`` the same with the Q1 functions in the place of
``phi_a`` and ``phi_b``.  The integrands are sums of tensor monomials ``x^i y^j`` (degree at most
6 per variable for the velocity, 4 for the pressure), integrated by ``int_0^1 x^i = 1 / (i + 1)``.

Doubles (coordinates, nodal values) are taken as the rationals they are, so the result is the
exact value of the form for the data as stored.  Nothing here reads the quadrature tables of
``control_amd.fem``; only the local node order is shared: ``3 j + i`` for Q2 and ``2 j + i`` for
Q1, ``i`` along x and ``j`` along y.  ``scales`` is the exception by design: the magnitude a
rounding error is measured against is the quadrature sum of ``fem.py`` with every factor replaced
by its absolute value, so it takes those tables as an argument.  Imported like ``common``.
"""
from fractions import Fraction

import numpy as np

from relin_ref import U, worst_ratio  # noqa: F401  (re-exported: one ratio for both elements)

# Roundings on a path from the tables and the wind to one element entry, as fem.py and the device
# kernel evaluate it, to first order and relative to S (tests/test_relin_ref.py counts 27 on
# P2-P1 triangles the same way).  A 1-D table value at a Gauss point is the point itself (1) and
# the operations on it: l_i three (two differences or a difference and a product, a product;
# doubling is exact), l_i' two (a product by 4 or 8 is exact: one difference; counted 2 with the
# point), psi one.
#   W_eq = (wt_r wt_s) (hx hy): two weights as numpy returns them (2), their product (1), hx and
#        hy (2), their product (1), the scaling (1)                                          7
#   phi_qa = l_i l_j: (1 + 3) twice and the product: 9; it enters twice (phi_qa, and phi_qc in
#        the interpolation)                                                                 18
#   grad phi_eqb = gref jinv: l_i' (1 + 2), l_j (1 + 3), their product (1), jinv = 1 / h (1),
#        the scaling (1)                                                                    10
#   the nine-term interpolation of the wind: a term passes its product and at most eight
#        additions                                                                           9
#   the two-term dot w_q . grad phi: a term passes its product and one addition              2
#   the two scalings W phi_qa and (W phi_qa) adv                                             2
#   the 16-term sum from 0.0 (the first addition is exact)                                  15
# 63 -- rounded up to a power of two.  The pressure entries pass fewer (lam = psi_i psi_j: 5,
# grad lam: 6) and are held to the same bar.
ELEMENT_BAR_Q2 = 64


# ------------------------------------------------- polynomials in (x, y): {(i, j): Fraction}
def _mul(p, q):
    out = {}
    for (a, b), x in p.items():
        for (c, d), y in q.items():
            k = (a + c, b + d)
            out[k] = out.get(k, 0) + x * y
    return out


def _diff(p, k):
    out = {}
    for alpha, x in p.items():
        if alpha[k] == 0:
            continue
        beta = (alpha[0] - 1, alpha[1]) if k == 0 else (alpha[0], alpha[1] - 1)
        out[beta] = out.get(beta, 0) + alpha[k] * x
    return out


def _integral(p):
    """int p over the unit square: ``int_0^1 x^i = 1 / (i + 1)`` in each variable."""
    return sum((x * Fraction(1, (i + 1) * (j + 1)) for (i, j), x in p.items()), Fraction(0))


def _tensor(fs):
    """The functions ``f_i(x) f_j(y)`` in the local order ``len(fs) j + i``."""
    return [{(a, b): x * y for a, x in fs[i].items() for b, y in fs[j].items()}
            for j in range(len(fs)) for i in range(len(fs))]


# the 1-D quadratic Lagrange functions on [0, 1] (nodes 0, 1/2, 1) and the two linear ones, by
# their coefficients
_L = [{0: Fraction(1), 1: Fraction(-3), 2: Fraction(2)}, {1: Fraction(4), 2: Fraction(-4)},
      {1: Fraction(-1), 2: Fraction(2)}]
_PSI = [{0: Fraction(1), 1: Fraction(-1)}, {1: Fraction(1)}]
PHI = _tensor(_L)          # the nine Q2 shape functions
LAM = _tensor(_PSI)        # the four Q1 shape functions
# T[c][a][b][k] = int phi_c phi_a d phi_b / d x_k;  TP[c][a][d][k] = int phi_c lam_a d lam_d / d x_k
T = [[[[_integral(_mul(_mul(PHI[c], PHI[a]), _diff(PHI[b], k))) for k in range(2)]
       for b in range(9)] for a in range(9)] for c in range(9)]
TP = [[[[_integral(_mul(_mul(PHI[c], LAM[a]), _diff(LAM[d], k))) for k in range(2)]
        for d in range(4)] for a in range(4)] for c in range(9)]


def element_matrices(xy, wx, wy):
    """Exact ``(Nv, Np)`` (9 x 9 and 4 x 4 nested lists of ``Fraction``) on one axis-parallel
    cell: ``xy`` the coordinates of its nine nodes (only the corners 0 and 8 are read), ``wx`` /
    ``wy`` the nine nodal values of the wind's components."""
    (x0, y0), (x1, y1) = [[Fraction(float(v)) for v in p] for p in (xy[0], xy[8])]
    hx, hy = x1 - x0, y1 - y0
    assert hx > 0 and hy > 0
    fx = [Fraction(float(v)) * hy for v in wx]        # wx_c hy: against d / d x
    fy = [Fraction(float(v)) * hx for v in wy]
    Nv = [[sum(fx[c] * T[c][a][b][0] + fy[c] * T[c][a][b][1] for c in range(9))
           for b in range(9)] for a in range(9)]
    Np = [[sum(fx[c] * TP[c][a][d][0] + fy[c] * TP[c][a][d][1] for c in range(9))
           for d in range(4)] for a in range(4)]
    return Nv, Np


def mesh_element_matrices(th, w):
    """``element_matrices`` of every cell of a ``fem.rectangle_q2q1`` discretisation (its
    connectivity and node coordinates, not its tables) for the wind ``w`` (component-major):
    object arrays (ne, 9, 9) and (ne, 4, 4) of ``Fraction``."""
    V = th.elem["V"]
    n2 = th.n_v // 2
    Nv = np.empty((len(V), 9, 9), dtype=object)
    Np = np.empty((len(V), 4, 4), dtype=object)
    for e, nodes in enumerate(V):
        a, b = element_matrices(th.coords_v[nodes], w[:n2][nodes], w[n2:][nodes])
        Nv[e], Np[e] = a, b
    return Nv, Np


def scales(elem, n2, w):
    """``(Sv, Sp)``: the quadrature sums of the two forms with every factor replaced by its
    absolute value,
    ``Sv[e, a, b] = sum_q W_eq |phi_qa| sum_d |gphi_eqbd| sum_c |phi_qc| |w_d,c|`` and
    ``Sp[e, a, b] = sum_q W_eq |lam_qa| sum_d |glam_eqbd| sum_c |phi_qc| |w_d,c|``."""
    V = elem["V"]
    aphi = np.abs(elem["phi"])
    wq = np.stack([np.abs(w[:n2][V]) @ aphi.T, np.abs(w[n2:][V]) @ aphi.T], axis=2)  # (ne, nq, 2)
    adv = np.einsum("eqbd,eqd->eqb", np.abs(elem["gphi"]), wq)
    Sv = np.einsum("eq,qa,eqb->eab", np.abs(elem["W"]), aphi, adv)
    advp = np.einsum("eqbd,eqd->eqb", np.abs(elem["glam"]), wq)
    Sp = np.einsum("eq,qa,eqb->eab", np.abs(elem["W"]), np.abs(elem["lam"]), advp)
    return Sv, Sp


_EXACT = {}


def exact_elements(mesh, kind, winds):
    """Exact element matrices and scales per level of ``winds(kind, th)`` on
    ``fem.rectangle_q2q1(*mesh)``, computed once per (mesh, wind) and shared: callers do not
    modify them."""
    key = (mesh, kind)
    if key not in _EXACT:
        from control_amd import fem
        th = fem.rectangle_q2q1(*mesh)
        _EXACT[key] = [mesh_element_matrices(th, w) + scales(th.elem, th.n_v // 2, w)
                       for w in winds(kind, th)]
    return _EXACT[key]
