"""The reaction element matrices of ``fem.ReactionTerm`` in rational arithmetic, for any number of
nodes per cell: ``tests/reaction_ref.py``'s construction on triangles and tetrahedra alike.

``E[a][b] = sum_q wq_q |cell_e| g(s_q) lam_qa lam_qb`` with ``s_q = sum_c lam_qc v_c`` and
``g(s) = sum_k c_k s^k``: the quadrature sum of the term's statement, evaluated exactly from its
float tables (``wq``, the cells' measure -- ``area`` or ``volume`` --, ``lam``), the coefficients
and the nodal values, all taken as the rationals they are.  ``scales`` is the same sum with every
coefficient, nodal value and term replaced by its absolute value: the magnitude ``S`` a rounding
error is measured against.  Imported like ``common``.
"""
from fractions import Fraction

import numpy as np

from relin_ref import U, worst_ratio  # noqa: F401  (re-exported)

# Roundings on the path from the tables and the nodal values to one entry of a tetrahedron's element
# matrix, as fem.ReactionTerm and the device kernel evaluate it, to first order and relative to S
# (tests/reaction_ref.py counts 30 on triangles the same way):
#   W_eq = wq_q volume_e                                                      1
#   s_q: every term lam v passes its product and at most three additions: an error of 4 u sum
#        lam |v|, which the power s^k carries k times: degree 4                16
#   Horner: the leading coefficient passes 4 products and 4 additions          8
#   the scalings W g, (W g) lam_a and ((W g) lam_a) lam_b                      3
#   the fifteen-term sum from 0.0 (the first addition is exact)               14
# 42 -- rounded up to a power of two.
ELEMENT_BAR_TET = 64


def _frac(a):
    return np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(a)


def measure(term):
    """The cells' area (triangles) or volume (tetrahedra), as the term holds it."""
    return term.area if term.cells.shape[1] == 3 else term.volume


def exact_element_matrices(term, v, coefficients=None):
    """Object array (n_cells, nv, nv) of ``Fraction``."""
    c = [Fraction(float(x)) for x in (term.coefficients if coefficients is None
                                      else coefficients)]
    nv = term.cells.shape[1]
    lam, wq, size = _frac(term.lam), _frac(term.wq), _frac(measure(term))
    v = _frac(np.asarray(v, dtype=np.float64))
    E = np.empty((len(term.cells), nv, nv), dtype=object)
    for e, nodes in enumerate(term.cells):
        wg = []
        for q in range(len(wq)):
            s = sum((lam[q, k] * v[nodes[k]] for k in range(nv)), Fraction(0))
            wg.append(wq[q] * size[e] * sum((ck * s ** k for k, ck in enumerate(c)), Fraction(0)))
        for a in range(nv):
            for b in range(nv):
                E[e, a, b] = sum((wg[q] * lam[q, a] * lam[q, b] for q in range(len(wq))),
                                 Fraction(0))
    return E


def scales(term, v, coefficients=None):
    """``S[e, a, b] = sum_q wq_q |cell_e| (sum_k |c_k| (sum_c lam_qc |v_c|)^k) lam_qa lam_qb``."""
    c = np.abs(term.coefficients if coefficients is None else coefficients)
    s = np.abs(np.asarray(v, dtype=np.float64))[term.cells] @ np.abs(term.lam).T     # (ne, nq)
    g = sum(ck * s ** k for k, ck in enumerate(c))
    return np.einsum("eq,qa,qb->eab", np.abs(term.W) * g, np.abs(term.lam), np.abs(term.lam))


# ------------------------------------------------------------ shared by the CPU and the GPU file
BOXES = {"cube": (2, 2, 2, 2.0, 2.0, 2.0), "flat": (3, 2, 2, 3.0, 1.0, 0.5)}
ITERATES = ("normal", "decades", "zero_level")
COEFFICIENTS = [(2.0, 0.0, 0.5), (2.0, 0.0, 1.5), (1.25, -0.75, 0.5, -2.0, 0.375)]

_EXACT = {}


def iterate(kind, disc, n_t=3, seed=0):
    """The three iterate kinds of ``tests/test_gpu_reaction_kernels.py`` (its ``_iterate``)."""
    rng = np.random.default_rng(seed + ITERATES.index(kind))
    v = rng.standard_normal((n_t, disc.n_dofs))
    if kind == "decades":
        v = np.sign(v) * 10.0 ** rng.uniform(-6.0, 6.0, size=v.shape)
    elif kind == "zero_level":
        v[1] = 0.0
    return v


def exact_elements(box_name, kind, c, seed):
    """Exact element matrices and scales per level of ``iterate(kind, ...)`` on a box, computed
    once per (box, iterate, coefficients) and shared: callers do not modify them."""
    key = (box_name, kind, c, seed)
    if key not in _EXACT:
        from control_amd import fem
        disc = fem.box_p1(*BOXES[box_name])
        term = fem.ReactionTerm(disc, c)
        _EXACT[key] = [(exact_element_matrices(term, w), scales(term, w))
                       for w in iterate(kind, disc, seed=seed)]
    return _EXACT[key]
