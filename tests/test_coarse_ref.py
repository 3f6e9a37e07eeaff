"""The host references of the coarse set-up and correction kernels (``tests/coarse_ref.py``, no
GPU) checked against ``fractions.Fraction`` arithmetic and closed forms, before
``tests/test_gpu_coarse_kernels.py`` holds the device to them."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_ref as ref
import structures as st


def _fraction_triple(At, P):
    A = ref.to_fractions(sp.csr_matrix(At).toarray())
    Q = ref.to_fractions(sp.csr_matrix(P).toarray())
    return Q.T @ (A @ Q)


# --------------------------------------------------------------------------- Galerkin matrices
def test_longdouble_carries_a_64_bit_significand():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("integer", [True, False])
def test_galerkin_exact_against_fractions(integer):
    """40 x 40, 7 coarse functions: integer data is reproduced exactly (and equals the float64
    SciPy product); real data lies within 2^-60 G of the exact product."""
    A = st.banded(40, 7, seed=1, integer=integer)
    P = st.banded(40, 3, seed=2, integer=integer, ncols=7)
    if integer:
        P = P * 0.125
    E, G = ref.galerkin_exact(A, P)
    exact = _fraction_triple(A, P)
    Gx = _fraction_triple(abs(A), abs(P))
    assert G.shape == (7, 7) and (G > 0).any()
    for i in range(7):
        for k in range(7):
            assert abs(Fraction(float(G[i, k])) - Gx[i, k]) <= Fraction(2) ** -50 * Gx[i, k]
            err = abs(Fraction(float(E[i, k].astype(np.float64))) +
                      Fraction(float((E[i, k] - E[i, k].astype(np.float64)).astype(np.float64))) -
                      exact[i, k])
            if integer:
                assert err == 0
                assert float(E[i, k]) == (P.T @ A @ P).toarray()[i, k]
            else:
                assert err <= Fraction(2) ** -60 * Gx[i, k]


def test_galerkin_depth_counts_the_chains():
    d = ref.galerkin_depth(7, [1, 256, 257, 289, 513])
    assert d.tolist() == [7 + 1 + 10, 7 + 1 + 10, 7 + 2 + 10, 7 + 2 + 10, 7 + 3 + 10]
    assert ref.reduce_depth([1, 256, 257, 324]).tolist() == [9, 9, 10, 10]


# ------------------------------------------------------------------------------- inverses
@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_restatements_against_fraction_elimination(n):
    """Both forms against the exact inverse at n <= 12, within the classical bound
    ``n cond u`` on an entry relative to the largest one."""
    for name in ref.REAL_FAMILIES:
        A = ref.real_family(name, n)
        exact = ref.fraction_inverse(A)
        bar = 8 * n * np.linalg.cond(A) * ref.U * np.abs(exact).max()
        for f in (ref.gauss_jordan_unblocked, ref.gauss_jordan_f64):
            X, bad = f(A)
            assert bad == n and np.abs(X - exact).max() <= bar, (name, f.__name__)
        assert np.abs(ref.gauss_jordan_f64(A, panel=3)[0] - exact).max() <= bar


@pytest.mark.parametrize("n", [31, 32, 33, 65, 100])
def test_blocked_form_equals_the_unblocked_one(n):
    """The same pivots and the same eliminations, summed in another order: the two forms differ by
    round-off alone, and a panel of any width gives the same."""
    for name in ref.REAL_FAMILIES:
        A = ref.real_family(name, n)
        U1, bad1 = ref.gauss_jordan_unblocked(A)
        bar = 8 * n * np.linalg.cond(A) * ref.U * np.abs(U1).max()
        for panel in (32, 7):
            B1, bad2 = ref.gauss_jordan_f64(A, panel=panel)
            assert bad1 == bad2 == n
            assert np.abs(B1 - U1).max() <= bar, (name, panel)


def test_restatements_flag_the_smallest_column_below_the_threshold():
    for f in (ref.gauss_jordan_unblocked, ref.gauss_jordan_f64):
        d = np.ones(40)
        d[17] = 2.0 ** -43
        assert f(np.diag(d))[1] == 40
        d[17] = 2.0 ** -44
        d[33] = 0.0
        assert f(np.diag(d))[1] == 17


@pytest.mark.parametrize("name", sorted(ref.EXACT_FAMILIES))
def test_exact_families_in_fractions(name):
    """n = 70 (three panels) in ``Fraction``: every value either form computes -- every partial sum
    of the panel products in the device's order included -- is a short dyadic number, so float64
    commits no rounding, fused or not, and the result is the closed form."""
    A, X = ref.EXACT_FAMILIES[name](70)
    seen = [0]

    def check(v):
        seen[0] += np.size(v)
        assert ref.short_dyadic(v)
    for f in (ref.gauss_jordan_unblocked, ref.gauss_jordan_f64):
        got, bad = f(ref.to_fractions(A), check=check)
        assert bad == 70 and np.array_equal(got.astype(np.float64), X)
    assert seen[0] > 70 * 140


@pytest.mark.parametrize("name", sorted(ref.EXACT_FAMILIES))
def test_exact_families_at_1100_in_float64(name):
    A, X = ref.EXACT_FAMILIES[name](1100)
    assert np.array_equal(A @ X, np.eye(1100))
    for f in (ref.gauss_jordan_unblocked, ref.gauss_jordan_f64):
        got, bad = f(A)
        assert bad == 1100 and np.array_equal(got, X), f.__name__


def test_unit_bidiagonal_ties_and_never_underflows():
    A, X = ref.unit_bidiagonal(1100)
    s = np.diag(A, -1)
    assert set(np.unique(np.abs(s))) == {0.0, 0.5, 1.0} and (np.abs(s) == 1.0).sum() > 100
    runs = np.diff(np.flatnonzero(np.r_[0.0, s, 0.0] == 0.0))
    assert runs.max() <= 40
    assert np.abs(X[X != 0]).min() >= 2.0 ** -39


@pytest.mark.parametrize("n", [33, 70, 1100])
def test_tie_blocks_need_the_tie_rule(n):
    """With equal magnitudes taking the LARGEST row the restatements miss the closed form: the
    family tells the two rules apart, which the other exact families do not."""
    A, X = ref.tie_blocks(n)
    for f in (ref.gauss_jordan_unblocked, ref.gauss_jordan_f64):
        assert np.array_equal(f(A)[0], X)
        wrong, bad = f(A, tie_smallest=False)
        assert bad == n and not np.array_equal(wrong, X)
        assert np.abs(wrong - X).max() < 1e-14
    for name in ("permuted_scaling", "unit_bidiagonal"):
        A, X = ref.EXACT_FAMILIES[name](n)
        assert np.array_equal(ref.gauss_jordan_f64(A, tie_smallest=False)[0], X)


@pytest.mark.parametrize("n", [33, 65, 300])
def test_refinement_has_converged(n):
    """The last refinement step moves no column by more than 2^-60 of its largest entry, and the
    result agrees with the exact inverse where that is known."""
    for name in ref.REAL_FAMILIES:
        A = ref.real_family(name, n)
        cols = ref.sample_columns(n)
        X, changes = ref.inverse_columns(A, cols)
        assert changes[-1] <= 2.0 ** -60, (name, changes)
    for name, fam in ref.EXACT_FAMILIES.items():
        A, exact = fam(n)
        cols = ref.sample_columns(n)
        X, changes = ref.inverse_columns(A, cols)
        assert changes[-1] <= 2.0 ** -60 and ref.distance(exact, cols, X) == 0.0, name


def test_refinement_has_converged_at_the_benchmark_size():
    A = ref.real_family("normal", 1089)
    cols = ref.sample_columns(1089)
    assert {0, 1, 31, 32, 33, 1023, 1024, 1025, 1088} <= set(cols.tolist())
    X, changes = ref.inverse_columns(A, cols)
    assert changes[-1] <= 2.0 ** -60, changes
    # the reference is far closer to either float64 inverse than they are to each other
    d, rho = ref.cpu_measures(A, cols, X)
    assert 0 < d < 1e-10 and 0 < rho < 1e-10


def test_refinement_against_fraction_inverse():
    A = ref.real_family("normal", 12)
    cols = np.arange(12)
    X, changes = ref.inverse_columns(A, cols)
    exact = ref.fraction_inverse(A)             # correctly rounded entries of the exact inverse
    assert np.array_equal(X.astype(np.float64), exact)


def test_reference_ratio_is_at_most_one():
    """What the GPU test asks of the device, asked of the restatement itself."""
    for name in ref.REAL_FAMILIES:
        A = ref.real_family(name, 300)
        cols = ref.sample_columns(300)
        X, _ = ref.inverse_columns(A, cols)
        d, rho = ref.cpu_measures(A, cols, X)
        gj = ref.gauss_jordan_f64(A)[0]
        assert ref.distance(gj, cols, X) <= d and ref.residual(A, gj) <= rho


# ------------------------------------------------------------------------ correction stages
def test_stage_ok_is_exact_on_integers_and_bounds_a_float64_product():
    A = st.banded(300, 9, seed=3, integer=True)
    x = np.random.default_rng(4).integers(-8, 9, size=300).astype(np.float64)
    plus = np.random.default_rng(5).integers(-8, 9, size=300).astype(np.float64)
    assert ref.stage_ok(A @ x, A, x) == (0.0, True)
    assert ref.stage_ok(A @ x + plus, A, x, plus=plus) == (0.0, True)
    B = st.with_values(A, seed=6)
    y = np.random.default_rng(7).standard_normal(300)
    ratio, _ = ref.stage_ok(B @ y + plus, B, y, plus=plus)
    assert ratio <= 1.0
    wrong = B @ y + plus
    wrong[17] += 64 * ref.U * (abs(B) @ np.abs(y))[17]
    assert ref.stage_ok(wrong, B, y, plus=plus)[0] > 1.0
    # a depth in place of the row's entries tightens the bar
    assert ref.stage_ok(wrong, B, y, terms=np.full(300, 2), plus=plus)[0] > \
        ref.stage_ok(wrong, B, y, plus=plus)[0]
