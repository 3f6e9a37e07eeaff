"""The host references of ``tests/blockops_ref.py`` checked on the CPU: against the oracle's
transforms and ``ConstantNullspace``, by their own algebra (inverse of the transform, splitting at
every cut, SELL round trip, the vectorised fused multiply-add against ``Fraction``), and -- so that
each assertion of ``tests/test_gpu_block_kernels.py`` is known to be able to fail -- that a reference
perturbed the way a wrong kernel would be is rejected by the comparison the GPU tests use."""
import numpy as np
import pytest

import blockops_ref as ref
from oracle import kkt_oracle as ko

KINDS = (1, 2, 3, 4)
ORACLE_T = {1: ko.apply_T_1, 2: ko.apply_T_2, 3: ko.apply_T_1_inv, 4: ko.apply_T_2_inv}
INVERSE = {1: 3, 2: 4, 3: 1, 4: 2}


def halos(kind, h):
    """``(lo, hi)`` with ``h`` on the side the transform reads."""
    return (None, h) if kind in (1, 3) else (h, None)


# ------------------------------------------------------------------------- the transforms
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 2, 5))
def test_transforms_match_the_oracle(kind, n):
    x = ref.real_data((n, 7), kind)
    assert ref.same_bits(ref.time_transform(kind, x), ORACLE_T[kind](x))
    # a halo is one more level of the oracle's transform
    h = ref.real_data(7, 10 + kind)
    lo, hi = halos(kind, h)
    # (the oracle's inverses leave the level they start from as it is: appended there, `h` is the
    # neighbour's finished value)
    after = kind in (1, 3)
    want = ORACLE_T[kind](np.vstack([x, h[None]]) if after else np.vstack([h[None], x]))
    want = want[:-1] if after else want[1:]
    assert ref.same_bits(ref.time_transform(kind, x, lo, hi), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_halo", (False, True))
def test_inverse_undoes_the_transform_on_integer_data(kind, with_halo):
    x = ref.int_data((6, 9), kind)
    lo, hi = halos(kind, ref.int_data(9, 20 + kind)) if with_halo else (None, None)
    y = ref.time_transform(kind, x, lo, hi)
    assert not ref.same_bits(y, x)
    assert ref.same_bits(ref.time_transform(INVERSE[kind], y, lo, hi), x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_halo", (False, True))
def test_pieces_with_the_right_halo_reproduce_the_whole(kind, with_halo):
    x = ref.real_data((6, 5), 30 + kind)
    lo, hi = halos(kind, ref.real_data(5, 40 + kind)) if with_halo else (None, None)
    y = ref.time_transform(kind, x, lo, hi)
    for cut in range(1, 6):
        (lo_a, hi_a), (lo_b, hi_b) = ref.split_halos(kind, x, y, cut, lo, hi)
        assert ref.same_bits(ref.time_transform(kind, x[:cut], lo_a, hi_a), y[:cut]), cut
        assert ref.same_bits(ref.time_transform(kind, x[cut:], lo_b, hi_b), y[cut:]), cut


def test_fused_form_and_mask_blocks():
    t, xin = ref.real_data((3, 6), 1), ref.real_data((3, 6), 2)
    m = np.zeros((3, 6), dtype=bool)
    m[0, 0] = m[1, 5] = m[2, 2] = True
    alpha = np.array([2.0, -3.0, 0.5])
    for kind in (1, 2):
        y = ref.time_transform_mask(kind, t, xin, [m[0], None, m[2]], alpha)
        plain = ref.time_transform(kind, t)
        assert y[0, 0] == 2.0 * xin[0, 0] and y[2, 2] == 0.5 * xin[2, 2]
        keep = ~m
        keep[1] = True
        assert ref.same_bits(y[keep], plain[keep])
    y = ref.mask_blocks(t, xin, [m[0], None, m[2]], alpha)
    assert y[0, 0] == 2.0 * xin[0, 0] and y[1, 5] == t[1, 5]
    y = ref.mask_blocks(t, None, list(m), alpha)
    assert ref.same_bits(y[m], np.zeros(3)) and ref.same_bits(y[~m], t[~m])


# -------------------------------------------------------------------------------- the sums
@pytest.mark.parametrize("nx", (1, 2, 255, 256, 257, 2049, 16385))
def test_ordered_sum(nx):
    x = ref.int_data(nx, 3)
    assert ref.ordered_sum(x) == ref.exact_sum(x) == float(x.astype(np.int64).sum())
    x = ref.real_data(nx, 4)
    err = abs(ref.ordered_sum(x) - ref.exact_sum(x))
    assert err <= ref.gamma(ref.sum_depth(nx) + 1) * ref.exact_sum(np.abs(x))
    assert ref.sum_depth(256) == 9 and ref.sum_depth(257) == 10
    # the order matters on such data: the reversed vector sums to other bits at some size
    if nx == 16385:
        assert ref.ordered_sum(x) != ref.ordered_sum(x[::-1].copy())


def test_constant_nullspace_against_the_oracle():
    """Power-of-two lengths and integer data: the mean and every shift are exact, so the oracle's
    ``alpha * sum / size`` and the kernels' ``c * sum`` with ``c = alpha / size`` agree in bits."""
    nx, alpha = 64, 0.5
    jobs = [(3, nx, -1.0 / nx, 1.0 / nx, alpha / nx)]
    y0 = 64.0 * ref.int_data(200, 5)
    b = 64.0 * ref.int_data(200, 6)
    ns = ko.ConstantNullspace(alpha=alpha)
    for second in (0, 1, 2):
        want = y0.copy()
        seg = want[3:3 + nx]
        if second == 0:
            ns.lhs_left(seg)
        elif second == 1:
            ns.lhs_left(seg)
            ns.pc_extended_correct_soln(seg, b[3:3 + nx])
        else:
            ns.lhs_left(seg)
            ns.extended_correct_lhs(b[3:3 + nx], seg)
        sa = ref.const_jobs_sums(y0, jobs)
        sb = ref.const_jobs_sums(b, jobs)
        rounded, fused = ref.shift_candidates(y0, y0, jobs, sa, second, sb)
        assert ref.same_bits(rounded, want) and ref.same_bits(fused, want), second
        assert ref.same_bits(rounded[:3], y0[:3]) and ref.same_bits(rounded[3 + nx:], y0[3 + nx:])


def test_vectorised_fma_is_the_exact_one():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    b = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    c = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    c[:1000] = -(a[:1000] * b[:1000]) * (1 + rng.integers(-4, 5, 1000) * 2.0 ** -52)  # cancellation
    # ties: a b + c exactly half way between two float64, with a small product deciding
    a[1000:1500] = 1.0 + rng.integers(1, 2 ** 20, 500) * 2.0 ** -52
    b[1000:1500] = 2.0 ** -54 * rng.choice([-1.0, 1.0, 3.0, -3.0], 500)
    c[1000:1500] = (1.0 + rng.integers(0, 2 ** 30, 500) * 2.0 ** -52) * rng.choice([-1.0, 1.0], 500)
    got = ref.fma_np(a, b, c)
    want = np.array([ref.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert ref.same_bits(got, want)
    # and it is not the two-rounding result
    assert np.count_nonzero(got != a * b + c) > 400
    # scalars broadcast
    assert ref.same_bits(ref.fma_np(a[0], b[0], c[:5]), [ref.fma(a[0], b[0], z) for z in c[:5]])


# ------------------------------------------------------------------------- the value arrays
def test_value_array_references():
    csr = np.array([1.5, -2.0, 3.0])
    assert ref.same_bits(ref.csr_to_sell(csr, [2, -1, 0, 0]), [3.0, 0.0, 1.5, 1.5])
    assert ref.same_bits(ref.mask_columns([1.0, -2.0, 3.0], [0, 1, 0], [1, 0]), [0.0, -2.0, 0.0])
    assert ref.vals_differ([0.0], [-0.0]) == 1 and ref.vals_differ([np.nan], [np.nan]) == 0
    assert ref.vals_differ([1.0], [1.0], flag=1) == 1
    a = np.array([4.0, 1.0, 3.0, 7.0])            # [[4, 1], [3, 7]]
    h, sk, flag = ref.vals_sym_skew(a, [0, 2, 1, 3])
    assert ref.same_bits(h, [4.0, 2.0, 2.0, 7.0]) and ref.same_bits(sk, [0.0, -1.0, 1.0, 0.0])
    assert flag == 1
    assert ref.vals_sym_skew([4.0, 0.0, 3.0, 7.0], [0, 2, 1, 3])[2] == 0      # a zero on one side
    # the threshold is relative to |x| + |y|
    assert ref.vals_sym_skew([1.0, ref.apart(1.0, 2e-12)], [1, 0])[2] == 1
    assert ref.vals_sym_skew([1.0, ref.apart(1.0, 0.5e-12)], [1, 0])[2] == 0
    assert abs(abs(ref.apart(-3.0, 2e-12) + 3.0) / (3.0 + abs(ref.apart(-3.0, 2e-12))) / 2e-12 - 1) < 1e-3
    h, sk, flag = ref.vals_sym_skew([5.0, -0.0], [-1, -1])
    assert ref.same_bits(h, [5.0, -0.0]) and ref.same_bits(sk, [0.0, 0.0]) and flag == 0
    indptr, indices, _ = ref.random_csr(9, 0)
    # (random_csr is not symmetric: symmetrise the pattern)
    pairs = {(r, int(c)) for r in range(9) for c in indices[indptr[r]:indptr[r + 1]]}
    pairs |= {(c, r) for r, c in pairs}
    rows = [sorted(c for r2, c in pairs if r2 == r) for r in range(9)]
    ip = np.cumsum([0] + [len(r) for r in rows])
    ix = np.array([c for r in rows for c in r])
    t = ref.transpose_map(ip, ix)
    assert np.array_equal(t[t], np.arange(len(ix)))
    for r in range(9):
        for p in range(ip[r], ip[r + 1]):
            q = t[p]
            assert ix[q] == r and ip[ix[p]] <= q < ip[ix[p] + 1]


@pytest.mark.parametrize("R", (1, 2))
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("nrows", (1, 65, 130))
def test_sell_builder_round_trips(R, permuted, nrows):
    indptr, indices, data = ref.random_csr(nrows, R, no_diag=(nrows // 2,))
    C = 64 * R
    perm = None
    extra = None
    if permuted:
        nslices = -(-nrows // C) + 1                 # a slice of padding rows more than needed
        rng = np.random.default_rng(nrows)
        perm = np.full(nslices * C, -1)
        perm[rng.permutation(nslices * C)[:nrows]] = rng.permutation(nrows)
        extra = np.arange(nslices) % 2               # padding entries in every second slice
    S = ref.build_sell(indptr, indices, data, R, perm, extra)
    assert len(S["col"]) == S["slice_off"][-1] * C == len(S["vals"])
    ip, ix, d = ref.sell_to_csr(S)
    assert np.array_equal(ip, indptr) and np.array_equal(ix, indices) and ref.same_bits(d, data)
    dinv = ref.extract_dinv(S)
    for r in range(nrows):
        cols = indices[indptr[r]:indptr[r + 1]].tolist()
        if r in cols:
            assert dinv[r] == 1.0 / data[indptr[r] + cols.index(r)]


# ------------------------------------------------- the perturbations the GPU tests must reject
def test_a_halo_from_the_wrong_side_is_rejected():
    x, h = ref.int_data((3, 4), 50), ref.int_data(4, 51)
    for kind in KINDS:
        lo, hi = halos(kind, h)
        good = ref.time_transform(kind, x, lo, hi)
        # the halo applied at the other end of the levels: what `lo > 0` for `hi < mf` would do
        flipped = ref.time_transform(kind, x[::-1], lo, hi)[::-1]
        assert not ref.same_bits(good, flipped), kind
        # and a halo that is there but ignored
        assert not ref.same_bits(good, ref.time_transform(kind, x)), kind


def test_an_inverse_that_reads_the_original_neighbour_is_rejected():
    x = ref.int_data((4, 4), 52)
    wrong3 = x.copy()
    wrong3[:-1] -= x[1:]
    wrong4 = x.copy()
    wrong4[1:] -= x[:-1]
    assert not ref.same_bits(ref.time_transform(3, x), wrong3)
    assert not ref.same_bits(ref.time_transform(4, x), wrong4)
    # ... also at a cut: the halo must be the updated level
    y = ref.time_transform(3, x)
    assert not ref.same_bits(ref.time_transform(3, x[:2], None, x[2]), y[:2])
    assert ref.same_bits(ref.time_transform(3, x[:2], None, y[2]), y[:2])


@pytest.mark.parametrize("nx", (2, 257, 2049))
def test_a_sum_without_its_last_element_is_rejected(nx):
    x = ref.int_data(nx, 53)
    assert ref.ordered_sum(x[:-1]) != ref.ordered_sum(x)
    x = ref.real_data(nx, 54, binades=1)
    short, full = ref.ordered_sum(x[:-1]), ref.ordered_sum(x)
    assert short != full
    # the bound of the real-data test separates them as well
    bound = ref.gamma(ref.sum_depth(nx) + 1) * ref.exact_sum(np.abs(x))
    assert abs(short - ref.exact_sum(x)) > bound


def test_a_contracted_vals_axpy_is_rejected():
    a, b = ref.real_data(4096, 55), ref.real_data(4096, 56)
    for c in (-0.5, 1.0 / 3.0):
        two, one = ref.vals_axpy(a, c, b), ref.vals_axpy_fused(a, c, b)
        share = np.count_nonzero(bits_differ(two, one)) / 4096
        assert (share > 0.05) == (c != -0.5), (c, share)   # a power of two: the product is exact
        if c != -0.5:
            assert not ref.same_bits(two, one)
    # without `a` the two agree except in the sign of a zero product
    assert ref.same_bits(ref.vals_axpy(None, 1.0 / 3.0, b), ref.vals_axpy_fused(None, 1.0 / 3.0, b))
    assert ref.same_bits(ref.vals_axpy(None, 0.0, -b), np.zeros(4096))


def bits_differ(a, b):
    return ref.bits(a) != ref.bits(b)


def test_a_negative_zero_for_a_masked_entry_is_rejected():
    x = ref.int_data((1, 4), 57)
    m = np.array([True, False, False, True])
    good = ref.mask_blocks(x, None, [m], [3.0])
    wrong = good.copy()
    wrong[0, 3] = -0.0
    assert np.array_equal(good, wrong) and not ref.same_bits(good, wrong)
    assert not np.signbit(good[0, 0]) and not np.signbit(good[0, 3])


def test_a_sell_position_with_r_and_64_swapped_is_rejected():
    indptr, indices, data = ref.random_csr(130, 9)
    S = ref.build_sell(indptr, indices, data, 2)
    good = ref.extract_dinv(S)
    wrong = ref.extract_dinv(S, position=ref.sell_position_swapped)
    assert not ref.same_bits(good, wrong)
    # (for R = 1 the two formulas are the same one)
    S1 = ref.build_sell(indptr, indices, data, 1)
    assert ref.same_bits(ref.extract_dinv(S1), ref.extract_dinv(S1, position=ref.sell_position_swapped))
