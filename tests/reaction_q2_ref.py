"""References for ``fem.ReactionTerm`` on Q2 quadrilaterals (``fem.rectangle_q2``), in rational
arithmetic: the construction of ``tests/reaction_p2_ref.py`` on the unit square.  The quadrature
sum of the term's statement and its scale are that file's (they read ``term.basis`` and
``term.area``, whatever the element); here are the 5 x 5 Gauss-Legendre product rule against the
exact integrals of the tensor monomials ``x^a y^b``, the element matrices of a polynomial
coefficient as exact tensor-monomial integrals (no quadrature), and the bars.  Imported like
``common``.
"""
from fractions import Fraction

import numpy as np

import reaction3d_ref
from reaction_p2_ref import (TABLE_ULPS, U, exact_element_matrices, scales,  # noqa: F401
                             worst_ratio)

# Roundings on the path from the tables and the nodal values to one entry of a Q2 element matrix,
# as fem.ReactionTerm and the device kernel evaluate it, to first order and relative to S
# (tests/reaction_p2_ref.py counts 60 on P2 triangles the same way):
#   W_eq = wq_q area_e                                                        1
#   s_q: every term phi v passes its product and at most eight additions: an error of 9 u sum
#        |phi| |v|, which the power s^k carries k times: degree 4              36
#   Horner: the leading coefficient passes 4 products and 4 additions          8
#   the scalings W g, (W g) phi_a and ((W g) phi_a) phi_b                      3
#   the 25-term sum from 0.0 (the first addition is exact)                    24
# 72 -- rounded up to a power of two.
ELEMENT_BAR_Q2 = 128

# An entry of ``basis`` against the exact polynomial at the float point: a 1-D value passes at
# most three roundings (l_0 = 2 (x - 1/2) (x - 1): two differences and a product; doubling is
# exact), the tensor product one more: 7 relative to |phi|.  An entry of the element matrix of a
# degree-2 coefficient sees phi_a, phi_b and s twice: 28 u S, which with the 72 above stays
# inside ELEMENT_BAR_Q2 -- the known-answer test needs no second bar.
BASIS_ROUNDINGS = 7

# M and K of rectangle_q2(n, n, L, L) against unit_square_q2(n, L): the roundings on both
# construction paths, to first order and relative to the sum of the absolute element contributions
# (which on the tensor path is the product of the 1-D sums of absolute values: the same number).
#   tensor path: a 1-D element entry h / 30 * m passes h = L / n, the quotient and the product
#   (3; stiffness 1 / (3 h) * k: 4), the 1-D assembly one addition (4; 5), the Kronecker product
#   one product: M 4 + 4 + 1 = 9, K 4 + 5 + 1 = 10 and the sum of its two products 11;
#   element path: an element entry is a product of two 1-D element entries, M 3 + 3 + 1 = 7,
#   K 3 + 4 + 1 = 8 and the sum of its two products 9; the assembly of at most four of them adds
#   3: M 10, K 12.
# M 19, K 23 -- rounded up to a power of two.
MESH_BAR = 32

MESHES = {"square": (2, 2, 2.0, 2.0), "stretched": (3, 2, 3.0, 0.5)}
ITERATES = reaction3d_ref.ITERATES
COEFFICIENTS = reaction3d_ref.COEFFICIENTS
iterate = reaction3d_ref.iterate
_frac = reaction3d_ref._frac

_EXACT = {}


def exact_elements(mesh_name, kind, c, seed):
    """Exact element matrices and scales per level of ``iterate(kind, ...)`` on a mesh, computed
    once per (mesh, iterate, coefficients) and shared: callers do not modify them."""
    key = (mesh_name, kind, c, seed)
    if key not in _EXACT:
        from control_amd import fem
        disc = fem.rectangle_q2(*MESHES[mesh_name])
        term = fem.ReactionTerm(disc, c)
        _EXACT[key] = [(exact_element_matrices(term, w), scales(term, w))
                       for w in iterate(kind, disc, seed=seed)]
    return _EXACT[key]


# ------------------------------------------------------------------------------- the rule
def monomial_integral(alpha):
    """``int x^a y^b`` over the unit square: ``1 / ((a + 1) (b + 1))``."""
    return Fraction(1, (alpha[0] + 1) * (alpha[1] + 1))


def monomial_sum(pts, wq, alpha):
    """The rule's value for ``x^a y^b``, exactly from the float tables."""
    X, w = _frac(pts), _frac(wq)
    return sum((w[q] * X[q, 0] ** alpha[0] * X[q, 1] ** alpha[1] for q in range(len(w))),
               Fraction(0))


def monomial_defect_bound(pts, wq, alpha):
    """``reaction_p2_ref.monomial_defect_bound`` on the square: how far ``monomial_sum`` may lie
    from ``monomial_integral`` for a rule that is exact at the exact nodes and weights, the tables
    being off by ``TABLE_ULPS`` (first order; relative for a weight, absolute for a coordinate in
    [0, 1]): with ``m = x^a y^b`` the 25-term sum

        eps sum_q wq_q m_q (1 + a / x_q + b / y_q),   eps = TABLE_ULPS u."""
    m = np.prod(pts ** np.array(alpha), axis=1)
    return float(TABLE_ULPS * U * (wq * m * (1.0 + (np.array(alpha) / pts).sum(axis=1))).sum())


# ------------------------------------------------------ polynomials in (x, y): {(a, b): Fraction}
def _mul(p, q):
    out = {}
    for (a, b), x in p.items():
        for (c, d), y in q.items():
            out[(a + c, b + d)] = out.get((a + c, b + d), 0) + x * y
    return out


def _scaled(p, f):
    return {alpha: coef * f for alpha, coef in p.items()}


def _added(p, q):
    out = dict(p)
    for alpha, coef in q.items():
        out[alpha] = out.get(alpha, 0) + coef
    return out


# the 1-D quadratic Lagrange functions on [0, 1] (nodes 0, 1/2, 1) by their coefficients
_L1D = [{0: Fraction(1), 1: Fraction(-3), 2: Fraction(2)}, {1: Fraction(4), 2: Fraction(-4)},
        {1: Fraction(-1), 2: Fraction(2)}]
#: the nine Q2 shape functions, local node 3 j + i: l_i(x) l_j(y)
PHI = [{(a, b): x * y for a, x in _L1D[i].items() for b, y in _L1D[j].items()}
       for j in range(3) for i in range(3)]

_DEFECT = {}


def polynomial_defect_bound(term, p):
    """``monomial_defect_bound`` summed over the monomials of ``p`` (degree <= 9 per variable) with
    the absolute values of its coefficients."""
    total = 0.0
    for alpha, coef in p.items():
        if coef == 0:
            continue
        if alpha not in _DEFECT:
            _DEFECT[alpha] = monomial_defect_bound(term.lam, term.wq, alpha)
        total += abs(float(coef)) * _DEFECT[alpha]
    return total


def integral(p):
    return sum((coef * monomial_integral(alpha) for alpha, coef in p.items()), Fraction(0))


def true_element_matrices(term, v, coefficients):
    """The element matrices ``int g(v_h) phi_a phi_b`` of the Q2 interpolant ``v_h`` as exact
    tensor-monomial integrals (nothing goes through the rule; the area is the float the term
    holds), for ``g`` of a degree that keeps the integrand's at 9 per variable or below.  Returns
    ``(E, defect)``: object array (ne, 9, 9) of ``Fraction`` and float array of
    ``polynomial_defect_bound`` of every integrand times the area."""
    c = [Fraction(float(x)) for x in coefficients]
    assert 2 * (len(c) - 1) + 4 <= 9
    v = _frac(np.asarray(v, dtype=np.float64))
    pairs = [[_mul(PHI[a], PHI[b]) for b in range(9)] for a in range(9)]
    E = np.empty((len(term.cells), 9, 9), dtype=object)
    defect = np.zeros((len(term.cells), 9, 9))
    for e, nodes in enumerate(term.cells):
        s = {}
        for k in range(9):
            s = _added(s, _scaled(PHI[k], v[nodes[k]]))
        g, power = {}, {(0, 0): Fraction(1)}
        for ck in c:
            g = _added(g, _scaled(power, ck))
            power = _mul(power, s)
        area = Fraction(float(term.area[e]))
        for a in range(9):
            for b in range(9):
                p = _mul(g, pairs[a][b])
                E[e, a, b] = area * integral(p)
                defect[e, a, b] = float(area) * polynomial_defect_bound(term, p)
    return E, defect
