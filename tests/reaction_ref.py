"""The reaction element matrices of ``fem.ReactionTerm`` in rational arithmetic.

``E[a][b] = sum_q wq_q area_e g(s_q) lam_qa lam_qb`` with ``s_q = sum_c lam_qc v_c`` and
``g(s) = sum_k c_k s^k``: the quadrature sum of the term's statement, evaluated exactly from its
float tables (``wq``, ``area``, ``lam``), the coefficients and the nodal values, all taken as the
rationals they are.  ``scales`` is the same sum with every coefficient, nodal value and term
replaced by its absolute value: the magnitude ``S`` a rounding error is measured against.
Imported like ``common``.
"""
from fractions import Fraction

import numpy as np

from relin_ref import U, worst_ratio  # noqa: F401  (re-exported)

# Roundings on the path from the tables and the nodal values to one element entry, as
# fem.ReactionTerm and the device kernel evaluate it, to first order and relative to S:
#   W_eq = wq_q area_e                                                        1
#   s_q: every term lam v passes its product and at most two additions: an error of 3 u sum
#        lam |v|, which the power s^k carries k times: degree 4                12
#   Horner: the leading coefficient passes 4 products and 4 additions          8
#   the scalings W g, (W g) lam_a and ((W g) lam_a) lam_b                      3
#   the seven-term sum from 0.0 (the first addition is exact)                  6
# 30 -- rounded up to a power of two.
ELEMENT_BAR = 32


def _frac(a):
    return np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(a)


def exact_element_matrices(term, v, coefficients=None):
    """Object array (n_cells, 3, 3) of ``Fraction``."""
    c = [Fraction(float(x)) for x in (term.coefficients if coefficients is None
                                      else coefficients)]
    lam, wq, area = _frac(term.lam), _frac(term.wq), _frac(term.area)
    v = _frac(np.asarray(v, dtype=np.float64))
    E = np.empty((len(term.cells), 3, 3), dtype=object)
    for e, nodes in enumerate(term.cells):
        wg = []
        for q in range(len(wq)):
            s = sum((lam[q, k] * v[nodes[k]] for k in range(3)), Fraction(0))
            wg.append(wq[q] * area[e] * sum((ck * s ** k for k, ck in enumerate(c)), Fraction(0)))
        for a in range(3):
            for b in range(3):
                E[e, a, b] = sum((wg[q] * lam[q, a] * lam[q, b] for q in range(len(wq))),
                                 Fraction(0))
    return E


def scales(term, v, coefficients=None):
    """``S[e, a, b] = sum_q wq_q area_e (sum_k |c_k| (sum_c lam_qc |v_c|)^k) lam_qa lam_qb``."""
    c = np.abs(term.coefficients if coefficients is None else coefficients)
    s = np.abs(np.asarray(v, dtype=np.float64))[term.cells] @ np.abs(term.lam).T     # (ne, nq)
    g = sum(ck * s ** k for k, ck in enumerate(c))
    return np.einsum("eq,qa,qb->eab", np.abs(term.W) * g, np.abs(term.lam), np.abs(term.lam))


# ---------------------------------------------------------------- the problem the loops are run on
KAT_SP = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 500,
          "relative_tolerance": 1.0e-14, "absolute_tolerance": 1.0e-14,
          "monitor_convergence": False}


def reaction_heat_control(CN, declared=True, n=8, n_t=5, coefficients=(2.0, 0.0, 0.5), **kw):
    """``_reaction_heat_control`` of ``tests/test_control_driver.py`` restated: the instationary
    version of the reference's non-linear reaction problem, ``grad-grad + (2 + 0.5 v_old^2) mass``,
    with the forward operator declared as a ``fem.ReactionTerm`` or as that file's callable."""
    from control_amd import fem
    from control_amd.control import Instationary
    disc = fem.unit_square_p1(n)

    def forward(v_old, t):
        return disc.K + disc.weighted_mass(
            lambda lam, cells: 2.0 + 0.5 * (v_old[cells] @ lam.T) ** 2)

    def v_d(X, t):
        return (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.exp(X[:, 0])
    op = fem.ReactionTerm(disc, coefficients) if declared else forward
    kw.setdefault("beta", 1.0e-2)
    return Instationary(disc, op, desired_state=v_d, CN=CN, n_t=n_t, time_interval=(0.0, 1.0),
                        **kw)
