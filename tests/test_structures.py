"""CPU checks of tests/structures.py: every generator gives the row and slice widths the
dispatch tests rely on, and the exact references are exact."""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import structures as st


@pytest.mark.parametrize("nrows", st.ROW_COUNTS)
@pytest.mark.parametrize("w", [1, 2, 7, 8, 9, 15, 16])
def test_banded_uniform_widths(nrows, w):
    w = min(w, nrows)
    A = st.banded(nrows, w, seed=nrows + w)
    assert st.width_histogram(A) == {w: nrows}
    assert A.has_sorted_indices and A.shape == (nrows, nrows)
    assert all(np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0) for r in range(nrows))
    assert st.padding_fraction(A) == 0.0
    assert np.all(st.slice_widths(A) == w)
    assert len(st.slice_widths(A)) == -(-nrows // 128)


def test_banded_integer_values_hold_explicit_zeros_and_empty_rows():
    w = np.array([0, 3, 0, 5, 1] * 40)
    A = st.banded(len(w), w, seed=1, integer=True)
    assert st.width_histogram(A) == {0: 80, 1: 40, 3: 40, 5: 40}
    assert np.all(A.data == np.round(A.data)) and np.abs(A.data).max() <= 4
    assert np.count_nonzero(A.data == 0) > 0          # stored zeros stay stored
    B = st.with_values(A, seed=2)
    assert np.array_equal(B.indices, A.indices) and B.nnz == A.nnz


def test_rectangular_banded():
    A = st.banded(300, 7, seed=3, ncols=40)
    assert A.shape == (300, 40) and st.width_histogram(A) == {7: 300}
    assert A.indices.max() < 40


def test_switch_mixtures():
    sw = st.mixture({4: 0.2, 9: 0.3, 12: 0.2, 19: 0.2, 25: 0.1}, 20)
    A = st.banded(len(sw) * 128, st.slice_row_widths(sw), seed=4)
    assert sorted(set(st.slice_widths(A).tolist())) == [4, 9, 12, 19, 25]
    slots = {w: w * np.count_nonzero(sw == w) for w in set(sw.tolist())}
    share_25 = slots[25] / sum(slots.values())
    assert 0.05 < share_25 < 0.2
    # ragged rows inside a slice: the slice width is its widest row
    rw = st.slice_row_widths([24, 38, 5], seed=5, ragged=True)
    A = st.banded(len(rw), rw, seed=5)
    assert st.slice_widths(A).tolist() == [24, 38, 5]
    assert len(st.width_histogram(A)) > 10


@pytest.mark.parametrize("width", [5, 9, 15])
def test_near_uniform_straddles_the_padding_limit(width):
    under, over = st.near_uniform(width, False), st.near_uniform(width, True)
    assert st.padding_fraction_of(under) <= st.PAD_LIMIT < st.padding_fraction_of(over)
    assert np.count_nonzero(over != width) == np.count_nonzero(under != width) + 1
    # the library's integer test (system.cpp): (uniform - stored) * 100 <= 3 * stored
    for sw, ok in ((under, True), (over, False)):
        stored = int(sw.sum())
        assert ((width * len(sw) - stored) * 100 <= 3 * stored) == ok
    A = st.banded(len(under) * 128, st.slice_row_widths(under), seed=6)
    assert st.padding_fraction(A) == st.padding_fraction_of(under)


@pytest.mark.parametrize("n", [4, 12])
def test_q1_square(n):
    sd = st.q1_square(n)
    N = (n + 1) ** 2
    assert sd.n_dofs == N and sd.coords.shape == (N, 2)
    assert st.width_histogram(sd.M) == {4: 4, 6: 4 * (n - 1), 9: (n - 1) ** 2}
    assert np.array_equal(sd.M.indptr, sd.K.indptr) and np.array_equal(sd.M.indices, sd.K.indices)
    assert len(sd.boundary) == 4 * n
    # Q1 mass integrates 1 to the area, stiffness annihilates constants and x
    assert math.isclose(sd.M.sum(), 1.0, rel_tol=1e-14)
    inner = np.setdiff1d(np.arange(N), sd.boundary)
    assert np.abs(sd.K @ np.ones(N)).max() < 1e-12
    assert np.abs(sd.K @ sd.coords[:, 0])[inner].max() < 1e-12 * n
    assert abs(sd.coords[:, 0] @ sd.M @ sd.coords[:, 1] - 0.25) < 1e-14
    assert (abs(sd.K - sd.K.T)).max() == 0


@pytest.mark.parametrize("n", [4, 40])
def test_fd5_square(n):
    sd = st.fd5_square(n)
    N = (n + 1) ** 2
    assert st.width_histogram(sd.M) == {1: N}
    assert st.width_histogram(sd.K) == {3: 4, 4: 4 * (n - 1), 5: (n - 1) ** 2}
    # a last slice of top-boundary rows is narrower: padded (uniform width 5 for the kernels)
    assert st.slice_widths(sd.K).max() == 5 and st.padding_fraction(sd.K) <= st.PAD_LIMIT
    assert np.allclose(sd.M.diagonal(), 1.0 / n**2)
    assert np.abs(sd.K @ np.ones(N))[np.setdiff1d(np.arange(N), sd.boundary)].max() == 0


def test_two_prod_is_error_free():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(1000) * 1e3, rng.standard_normal(1000) * 1e-3
    p, e = st.two_prod(a, b)
    for i in range(0, 1000, 37):
        assert Fraction(p[i]) + Fraction(e[i]) == Fraction(a[i]) * Fraction(b[i])


def test_matvec_exact_is_correctly_rounded():
    A = st.banded(300, st.slice_row_widths([9, 38, 0], nrows=300, ragged=True), seed=8)
    # cancellation: exact results far smaller than the terms
    x = np.random.default_rng(9).standard_normal(300) * np.logspace(-8, 8, 300)
    y, absum, k = st.matvec_exact(A, x)
    for r in range(0, 300, 7):
        s = slice(A.indptr[r], A.indptr[r + 1])
        exact = sum((Fraction(v) * Fraction(x[c]) for v, c in zip(A.data[s], A.indices[s])),
                    Fraction(0))
        assert y[r] == float(exact)
    assert np.array_equal(k, st.row_widths(A))
    assert np.allclose(absum, abs(A) @ np.abs(x))
    # SciPy's product lies within the bound, and exactly equal on integer data
    assert st.componentwise_ok(A @ x, y, absum, k) <= 1.0
    Ai = st.banded(300, 15, seed=10, integer=True)
    xi = np.random.default_rng(11).integers(-8, 9, 300).astype(np.float64)
    assert np.array_equal(st.matvec_exact(Ai, xi)[0], Ai @ xi)


def test_rows_exact_sums_terms():
    A, B = st.banded(200, 7, seed=12), st.banded(200, 5, seed=13, ncols=64)
    x, z = np.random.default_rng(14).standard_normal(200), np.random.default_rng(15).standard_normal(64)
    y, absum, k = st.rows_exact([(A, x), (B, z)], 200)
    ref = sp.hstack([A, B]).tocsr()
    y2, absum2, k2 = st.matvec_exact(ref, np.r_[x, z])
    assert np.array_equal(y, y2) and np.array_equal(k, k2) and np.allclose(absum, absum2)
