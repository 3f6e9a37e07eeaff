"""The exact reference of the convection element matrices (``tests/relin_ref.py``, no GPU)
checked against ``fem.py``: the precomputed integrals against the Radon-rule sum over the tables
(degree-5 exactness), and the host element matrices against the exact ones."""
from fractions import Fraction

import numpy as np
import pytest

import common
import relin_ref
import test_relinearise_plan as host_path
from control_amd import fem

U = relin_ref.U
# Roundings on a path from the tables and the wind to one element entry, as fem.py and the device
# kernel evaluate it: the table entries of W, phi (twice) and gphi (4 x ~3: constants of the rule,
# barycentric products, the Jacobian), the six-term interpolation of the wind (6), the two-term
# advection (3), the two scalings W phi and (W phi) adv (2) and the seven-term accumulation (7):
# about 27 -- rounded up to a power of two.
ELEMENT_BAR = 32
# The tables alone (no wind, exact summation): W = (constant of the rule: a square root, a
# difference, a quotient) x 2A / 2, two values of phi (lam_q: square root, sum, quotient; then a
# product and a difference) and gphi (d phi / d lam: two; grad lam: the 3 x 3 inverse; their
# three-term sum): 3 + 2 x 5 + 3 -- rounded up to a power of two.
TABLE_BAR = 16


def _frac(a):
    return np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(a)


def test_tensor_is_the_radon_sum_of_the_tables():
    """(a) 2A sum_k T[c][a][b][k] d lam_k / d x_d = sum_q W_eq phi_qc phi_qa gphi_eqbd, and the
    pressure analogue, with the table entries summed exactly."""
    th = fem.rectangle_p2p1(3, 2, 3.0, 1.0)
    e = th.elem
    W, phi, gphi, lam = _frac(e["W"]), _frac(e["phi"]), _frac(e["gphi"]), _frac(e["lam"])
    worst = worst_p = 0.0
    for el, nodes in enumerate(e["V"]):
        A2, g = relin_ref.triangle_geometry(th.coords_v[nodes[:3]])
        for c in range(6):
            for a in range(6):
                wpp = [W[el, q] * phi[q, c] * phi[q, a] for q in range(7)]
                for b in range(6):
                    for d in range(2):
                        terms = [wpp[q] * gphi[el, q, b, d] for q in range(7)]
                        exact = A2 * sum(relin_ref.T[c][a][b][k] * g[k][d] for k in range(3))
                        scale = sum(abs(t) for t in terms)
                        err = abs(sum(terms) - exact)
                        assert scale > 0 or err == 0
                        if err:
                            worst = max(worst, float(err / (Fraction(U) * scale)))
            for a in range(3):
                terms = [W[el, q] * phi[q, c] * lam[q, a] for q in range(7)]
                err = abs(sum(terms) - A2 * relin_ref.PL[c][a])
                worst_p = max(worst_p, float(err / (Fraction(U) * sum(abs(t) for t in terms))))
    print(f"tables against the exact integrals: worst error {worst:.2f} u (velocity), "
          f"{worst_p:.2f} u (pressure) of the absolute sums")
    assert worst <= TABLE_BAR and worst_p <= TABLE_BAR


@pytest.mark.parametrize("nx,ny,lx,ly", [(2, 2, 2.0, 2.0), (4, 4, 2.0, 2.0), (3, 2, 3.0, 1.0)])
def test_host_element_matrices_are_exact_to_the_bar(nx, ny, lx, ly):
    """(b) fem.py's element matrices lie within ``32 u S`` of the exact ones."""
    th = fem.rectangle_p2p1(nx, ny, lx, ly)
    rng = np.random.default_rng(common.SEED + nx)
    for scale in (1.0, 0.1):
        w = scale * rng.standard_normal(th.n_v)
        Nv, Np = host_path._element_matrices(th, w)
        Xv, Xp = relin_ref.mesh_element_matrices(th, w)
        Sv, Sp = relin_ref.scales(th.elem, th.n_v // 2, w)
        rv, rp = relin_ref.worst_ratio(Nv, Xv, Sv), relin_ref.worst_ratio(Np, Xp, Sp)
        print(f"{nx}x{ny} wind x {scale}: worst err / (u S) = {rv:.2f} (velocity), {rp:.2f} "
              f"(pressure)")
        assert rv <= ELEMENT_BAR and rp <= ELEMENT_BAR


def test_zero_wind_and_linearity():
    """The reference itself: zero for a zero wind, the form annihilates constants (the basis sums
    to one: rows of N sum to zero over b), and it is linear in the wind."""
    xy = np.array([[0.25, 0.5], [1.5, 0.75], [0.5, 2.0]])
    rng = np.random.default_rng(common.SEED)
    w1, w2 = rng.standard_normal((2, 6)), rng.standard_normal((2, 6))
    z = np.zeros(6)
    Nv0, Np0 = relin_ref.element_matrices(xy, z, z)
    assert all(x == 0 for row in Nv0 for x in row) and all(x == 0 for row in Np0 for x in row)
    Cm, Cp = relin_ref.element_matrices(xy, *w1)
    assert any(x != 0 for row in Cm for x in row)
    for a in range(6):
        assert sum(Cm[a]) == 0
    for a in range(3):
        assert sum(Cp[a]) == 0
    # dyadic data: the sum of two winds is exact
    w3 = np.round(w1 * 64) / 64
    w4 = np.round(w2 * 64) / 64
    A, Ap = relin_ref.element_matrices(xy, *w3)
    B, Bp = relin_ref.element_matrices(xy, *w4)
    Cm, Cp = relin_ref.element_matrices(xy, *(w3 + w4))
    assert all(A[a][b] + B[a][b] == Cm[a][b] for a in range(6) for b in range(6))
    assert all(Ap[a][b] + Bp[a][b] == Cp[a][b] for a in range(3) for b in range(3))
