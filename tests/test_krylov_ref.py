"""The host references of the Krylov vector kernels (``tests/krylov_ref.py``, no GPU) checked
against ``fractions.Fraction`` arithmetic, and the reduction tree they describe held against the
rounding-error bound that ``tests/test_gpu_krylov_kernels.py`` asks of the device."""
import math
from fractions import Fraction

import numpy as np
import pytest

import krylov_ref as ref


def _fraction_dot(w, v):
    return float(sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, v)))


def _cancelling(n, seed):
    """``<w, v> = 3 * 2^-40`` exactly, from products of size ``2^60`` that cancel in pairs: the
    float64 sum loses every digit in most orders."""
    rng = np.random.default_rng([ref.SEED, n, seed])
    half = (n - 3) // 2
    a = np.ldexp(rng.integers(2 ** 52, 2 ** 53, size=half).astype(np.float64), -22)
    b = np.ldexp(rng.integers(2 ** 52, 2 ** 53, size=half).astype(np.float64), -22)
    w = np.concatenate([a, -a, np.full(n - 2 * half, 2.0 ** -20)])
    v = np.concatenate([b, b, np.full(n - 2 * half, 2.0 ** -20 * 3 / (n - 2 * half))])
    perm = rng.permutation(n)
    return w[perm], v[perm]


@pytest.mark.parametrize("n", [1, 2, 3, 17, 300])
def test_exact_dots_round_the_exact_value(n):
    w, V = ref.real_data(n, 3, 1)
    got = ref.exact_dots(w, V)
    for i in range(3):
        assert got[i] == _fraction_dot(w, V[i])
    w, V = ref.int_data(n, 2, 1)
    assert np.array_equal(ref.exact_dots(w, V), (V.astype(np.int64) @ w.astype(np.int64)))


@pytest.mark.parametrize("n", [15, 299, 300])
def test_exact_dots_on_cancelling_data(n):
    w, v = _cancelling(n, 0)
    want = _fraction_dot(w, v)
    assert want == 3 * 2.0 ** -40
    assert ref.exact_dots(w, [v])[0] == want
    if n >= 299:     # (fifteen terms may cancel by luck)
        assert abs(float(np.dot(w, v)) - want) > 0.5 * abs(want)


def test_two_product_is_error_free():
    rng = np.random.default_rng([ref.SEED, 7])
    a = rng.standard_normal(200) * np.exp2(rng.integers(-20, 21, size=200))
    b = rng.standard_normal(200) * np.exp2(rng.integers(-20, 21, size=200))
    p, e = ref.two_product(a, b)
    for k in range(200):
        assert Fraction(float(p[k])) + Fraction(float(e[k])) == Fraction(float(a[k])) * Fraction(float(b[k]))


def test_fma_rounds_once():
    x = 1.0 + 2.0 ** -52
    # x^2 = 1 + 2^-51 + 2^-104: the product rounds to 1 + 2^-51, a fused operation keeps the rest
    assert x * x - (1.0 + 2.0 ** -51) == 0.0
    assert ref.fma(x, x, -(1.0 + 2.0 ** -51)) == 2.0 ** -104
    assert ref.fma(3.0, 5.0, 7.0) == 22.0
    # two roundings land on a tie and go to even; one rounding sees the excess and goes up
    b = 2.0 ** -53 * (1.0 - 2.0 ** -53)
    assert x * b == 2.0 ** -53 and x * b + 1.0 == 1.0
    assert ref.fma(x, b, 1.0) == 1.0 + 2.0 ** -52
    rng = np.random.default_rng([ref.SEED, 8])
    a, b, c = (rng.standard_normal(300) * np.exp2(rng.integers(-20, 21, size=300)) for _ in range(3))
    p, e = ref.two_product(a, b)
    for k in range(300):
        want = float(Fraction(float(p[k])) + Fraction(float(e[k])) + Fraction(float(c[k])))
        assert ref.fma(a[k], b[k], c[k]) == want
        if hasattr(math, "fma"):
            assert ref.fma(a[k], b[k], c[k]) == math.fma(a[k], b[k], c[k])
    # the array form the tree walk uses agrees wherever the result is representable
    assert np.array_equal(ref._fma_np(p, np.ones(300), -p), np.zeros(300))
    assert np.array_equal(ref._fma_np(a, b, -p), e)


@pytest.mark.parametrize("nv", [1, 8, 9, 17])
def test_maxpy_exact_is_the_documented_chain(nv):
    w, V = ref.int_data(37, nv, 2, amp=64)
    coef = np.arange(1, nv + 1, dtype=np.float64) * np.where(np.arange(nv) % 2, -1.0, 1.0)
    want = w.astype(np.int64) - coef.astype(np.int64) @ V.astype(np.int64)
    assert np.array_equal(ref.maxpy_exact(w, V, coef, -1.0), want)
    # real data: the chain written out with the scalar fma, and grouping that matters
    w, V = ref.real_data(5, nv, 2)
    coef = ref.exact_dots(w, V)
    got = ref.maxpy_exact(w, V, coef, -1.0)
    for p in range(5):
        x = w[p]
        for g in range(0, nv, 8):
            a = 0.0
            for i in range(g, min(g + 8, nv)):
                a = ref.fma(coef[i], V[i][p], a)
            x = ref.fma(-1.0, a, x)
        assert got[p] == x


def test_constants_of_the_reduction():
    assert [ref.chunk(n) for n in (1, 2048, 2049, 2420, 524288, 524289, 1536001)] == \
        [2, 2, 4, 4, 512, 514, 1502]
    assert ref.chunk(8_450_000) == 16 * 512 + 60        # sixteen full trips and a ragged one
    assert [ref.stride(n) for n in (1, 32, 33, 2421)] == [32, 32, 64, 2432]
    # 2 fmas per trip + shuffle tree 6 + wave results 3 + stage-2 chain 4 + stage-2 tree 8
    assert ref.dot_depth(2420) == 2 + 21 and ref.dot_depth(524288) == 2 + 21
    assert ref.dot_depth(524289) == 4 + 21 and ref.dot_depth(1536001) == 6 + 21
    assert ref.dot_depth(8_450_000) == 2 * 17 + 21
    assert ref.gamma(1) == pytest.approx(2.0 ** -53, rel=1e-15)


INT_SIZES = [1, 2, 3, 2047, 2048, 2049, 2421, 65537, 524287, 524288, 524289]


@pytest.mark.parametrize("n", INT_SIZES)
def test_tree_is_exact_on_integer_data(n):
    w, V = ref.int_data(n, 2, 0)
    assert np.array_equal(ref.tree_dots(w, V), V.astype(np.int64) @ w.astype(np.int64))


@pytest.mark.parametrize("n,nv", [(3, 9), (2049, 9), (2421, 9), (65537, 9), (1536001, 2)])
def test_tree_stays_inside_the_bound_on_the_real_inputs(n, nv):
    """The conditions of the GPU test, met by float64 arithmetic in the device's order: each inner
    product within ``gamma(dot_depth(n) + 1) sum |w_p v_p|`` of the rounded exact one, and the
    projected vector of ``real_data`` far smaller than ``w``."""
    w, V = ref.real_data(n, nv, 0)
    exact, scale = ref.exact_dots(w, V), ref.abs_dots(w, V)
    got = ref.tree_dots(w, V)
    bound = ref.gamma(ref.dot_depth(n) + 1) * scale
    assert np.all(scale > 0) and np.all(np.abs(got - exact) <= bound)
    if n >= nv:
        assert np.linalg.norm(w - exact @ V) < 1e-6 * np.linalg.norm(w)
    if n <= 2421:
        w_out = ref.maxpy_exact(w, V, got, -1.0)
        sq = ref.tree_dots(w_out, [w_out])[0]
        sq_exact = ref.exact_dots(w_out, [w_out])[0]
        assert abs(sq - sq_exact) <= ref.gamma(ref.dot_depth(n) + 1) * sq_exact


def test_orth_amp_keeps_the_integer_step_exact():
    for n, nv in [(3, 9), (2421, 30), (65537, 9)]:
        amp = ref.orth_amp(n, nv, 0)
        w, V = ref.int_data(n, nv, 0, amp)
        assert np.all(np.abs(V) <= amp) and np.all(V != 0) and np.all(V == np.round(V))
        h, w_out, sq = ref.int_orthogonalise(w, V)
        assert sq is not None and sq < 2 ** 53
        assert sq == sum(int(x) ** 2 for x in w_out)
        assert np.array_equal(ref.maxpy_exact(w, V, h.astype(np.float64), -1.0)
                              if n <= 2421 else w_out, w_out)
