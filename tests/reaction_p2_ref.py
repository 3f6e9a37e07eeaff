"""References for ``fem.ReactionTerm`` on P2 triangles (``fem.rectangle_p2``), in rational
arithmetic: ``tests/reaction3d_ref.py``'s construction generalised to the term's ``basis`` table,
the 5 x 5 conical rule against the exact integrals of the barycentric monomials, and the element
matrices of a polynomial coefficient as exact polynomial integrals (no quadrature).

``exact_element_matrices`` is the quadrature sum of the term's statement,
``E[a][b] = sum_q wq_q area_e g(s_q) phi_qa phi_qb`` with ``s_q = sum_c phi_qc v_c``, evaluated
exactly from the float tables; ``scales`` the same sum with every coefficient, nodal value and
table entry replaced by its absolute value (P2 shape functions change sign).  Imported like
``common``.
"""
from fractions import Fraction
from math import factorial

import numpy as np

import reaction3d_ref
from relin_ref import _PHI, _mul, U, worst_ratio  # noqa: F401  (U, worst_ratio re-exported)

# Roundings on the path from the tables and the nodal values to one entry of a P2 triangle's
# element matrix, as fem.ReactionTerm and the device kernel evaluate it, to first order and
# relative to S (tests/reaction3d_ref.py counts 42 on tetrahedra the same way):
#   W_eq = wq_q area_e                                                        1
#   s_q: every term phi v passes its product and at most five additions: an error of 6 u sum
#        |phi| |v|, which the power s^k carries k times: degree 4              24
#   Horner: the leading coefficient passes 4 products and 4 additions          8
#   the scalings W g, (W g) phi_a and ((W g) phi_a) phi_b                      3
#   the 25-term sum from 0.0 (the first addition is exact)                    24
# 60 -- rounded up to a power of two.
ELEMENT_BAR_P2 = 64

# How far an entry of the rule's tables may lie from the exact Gauss node or weight, in units of
# u: relative for a weight, absolute for a barycentric coordinate (they lie in [0, 1]).  NumPy and
# SciPy state no bound; the nodes are eigenvalues of a 5 x 5 Jacobi matrix polished by a Newton
# step, the Jacobi weights go through a quotient of Gamma functions, and the mapping to the
# triangle adds an affine map, a product and two differences: a few units each, 16 at the most.
TABLE_ULPS = 16

MESHES = {"square": (2, 2, 2.0, 2.0), "stretched": (3, 2, 3.0, 0.5)}
ITERATES = reaction3d_ref.ITERATES
COEFFICIENTS = reaction3d_ref.COEFFICIENTS
iterate = reaction3d_ref.iterate
_frac = reaction3d_ref._frac


# -------------------------------------------------------------------------- the statement
def exact_element_matrices(term, v, coefficients=None):
    """Object array (n_cells, nv, nv) of ``Fraction``: the quadrature sum over ``term.basis``."""
    c = [Fraction(float(x)) for x in (term.coefficients if coefficients is None
                                      else coefficients)]
    nv = term.cells.shape[1]
    phi, wq, size = _frac(term.basis), _frac(term.wq), _frac(term.area)
    v = _frac(np.asarray(v, dtype=np.float64))
    nq = len(wq)
    E = np.empty((len(term.cells), nv, nv), dtype=object)
    for e, nodes in enumerate(term.cells):
        wg = []
        for q in range(nq):
            s = sum((phi[q, k] * v[nodes[k]] for k in range(nv)), Fraction(0))
            wg.append(wq[q] * size[e] * sum((ck * s ** k for k, ck in enumerate(c)), Fraction(0)))
        for a in range(nv):
            wa = [wg[q] * phi[q, a] for q in range(nq)]
            for b in range(nv):
                E[e, a, b] = sum((wa[q] * phi[q, b] for q in range(nq)), Fraction(0))
    return E


def scales(term, v, coefficients=None):
    """``S[e, a, b] = sum_q wq_q area_e (sum_k |c_k| (sum_c |phi_qc| |v_c|)^k) |phi_qa| |phi_qb|``."""
    c = np.abs(term.coefficients if coefficients is None else coefficients)
    phi = np.abs(term.basis)
    s = np.abs(np.asarray(v, dtype=np.float64))[term.cells] @ phi.T                  # (ne, nq)
    g = sum(ck * s ** k for k, ck in enumerate(c))
    return np.einsum("eq,qa,qb->eab", np.abs(term.W) * g, phi, phi)


_EXACT = {}


def exact_elements(mesh_name, kind, c, seed):
    """Exact element matrices and scales per level of ``iterate(kind, ...)`` on a mesh, computed
    once per (mesh, iterate, coefficients) and shared: callers do not modify them."""
    key = (mesh_name, kind, c, seed)
    if key not in _EXACT:
        from control_amd import fem
        disc = fem.rectangle_p2(*MESHES[mesh_name])
        term = fem.ReactionTerm(disc, c)
        _EXACT[key] = [(exact_element_matrices(term, w), scales(term, w))
                       for w in iterate(kind, disc, seed=seed)]
    return _EXACT[key]


# ------------------------------------------------------------------------------- the rule
def monomial_integral(alpha):
    """``int lam^alpha`` over a triangle of area 1: ``2 a! b! c! / (a + b + c + 2)!``."""
    a, b, c = alpha
    return Fraction(2 * factorial(a) * factorial(b) * factorial(c), factorial(a + b + c + 2))


def monomial_sum(lam, wq, alpha):
    """The rule's value for ``lam^alpha``, exactly from the float tables."""
    L, w = _frac(lam), _frac(wq)
    return sum((w[q] * L[q, 0] ** alpha[0] * L[q, 1] ** alpha[1] * L[q, 2] ** alpha[2]
                for q in range(len(w))), Fraction(0))


def monomial_defect_bound(lam, wq, alpha):
    """How far ``monomial_sum`` may lie from ``monomial_integral`` for a rule that is exact at the
    exact nodes and weights, the tables being off by ``TABLE_ULPS`` (first order): with
    ``m = lam^alpha``, a weight off by ``eps`` relative moves term ``q`` by ``eps wq_q m_q``, a
    coordinate off by ``eps`` absolute by ``eps wq_q alpha_k m_q / lam_qk`` -- the 25-term sum

        eps sum_q wq_q m_q (1 + sum_k alpha_k / lam_qk),   eps = TABLE_ULPS u."""
    m = np.prod(lam ** np.array(alpha), axis=1)
    return float(TABLE_ULPS * U * (wq * m * (1.0 + (np.array(alpha) / lam).sum(axis=1))).sum())


_DEFECT = {}


def polynomial_defect_bound(term, p):
    """``monomial_defect_bound`` summed over the monomials of the polynomial ``p`` (a dict
    ``{alpha: Fraction}``, degree <= 9) with the absolute values of its coefficients."""
    total = 0.0
    for alpha, coef in p.items():
        if coef == 0:
            continue
        if alpha not in _DEFECT:
            _DEFECT[alpha] = monomial_defect_bound(term.lam, term.wq, alpha)
        total += abs(float(coef)) * _DEFECT[alpha]
    return total


def integral(p):
    """``int p`` over a triangle of area 1."""
    return sum((coef * monomial_integral(alpha) for alpha, coef in p.items()), Fraction(0))


def _scaled(p, f):
    return {alpha: coef * f for alpha, coef in p.items()}


def _added(p, q):
    out = dict(p)
    for alpha, coef in q.items():
        out[alpha] = out.get(alpha, 0) + coef
    return out


def true_element_matrices(term, v, coefficients):
    """The element matrices ``int g(v_h) phi_a phi_b`` of the P2 interpolant ``v_h`` as exact
    polynomial integrals by the monomial formula (nothing goes through the rule; the area is the
    float the term holds), for ``g`` of a degree that keeps the integrand's at 9 or below.
    Returns ``(E, defect)``: object array (ne, 6, 6) of ``Fraction`` and float array of
    ``polynomial_defect_bound`` of every integrand times the area."""
    c = [Fraction(float(x)) for x in coefficients]
    assert 2 * (len(c) - 1) + 4 <= 9
    v = _frac(np.asarray(v, dtype=np.float64))
    pairs = [[_mul(_PHI[a], _PHI[b]) for b in range(6)] for a in range(6)]
    E = np.empty((len(term.cells), 6, 6), dtype=object)
    defect = np.zeros((len(term.cells), 6, 6))
    for e, nodes in enumerate(term.cells):
        s = {}
        for k in range(6):
            s = _added(s, _scaled(_PHI[k], v[nodes[k]]))
        g, power = {}, {(0, 0, 0): Fraction(1)}
        for ck in c:
            g = _added(g, _scaled(power, ck))
            power = _mul(power, s)
        area = Fraction(float(term.area[e]))
        for a in range(6):
            for b in range(6):
                p = _mul(g, pairs[a][b])
                E[e, a, b] = area * integral(p)
                defect[e, a, b] = float(area) * polynomial_defect_bound(term, p)
    return E, defect
