"""``tests/spectrum_kernels_ref.py`` held against plain Python before a GPU sees it: the stage-2
scalars against hand-written cases in Python floats (IEEE doubles), ``fma_array`` against
``Fraction`` on ties, near-ties, zeros of both signs, subnormals and non-finite operands, the
updates against element-by-element loops, the vectorised fingerprint against one in Python
integers, and -- for every array, position and bit the GPU tests flip -- that the flip changes the
folded fingerprint of the reference itself, so that no GPU assertion rests on a collision the
reference would share.  No GPU, no library."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blockops_ref
import krylov_ref
import spectrum_kernels_ref as ref


def test_constants_and_sizes():
    assert ref.batch_stride(1) == 34 and ref.batch_stride(2) == 34 and ref.batch_stride(3) == 36
    assert all(ref.batch_stride(n) % 2 == 0 and ref.batch_stride(n) >= n + 32 for n in range(1, 300))
    assert ref.UPDATE_TRIP == 65536 and ref.SPLIT_TRIP == 131072
    assert ref.FP_N == (1, 255, 256, 257, 2048, 2049, 131073, 600001)
    assert [ref.fingerprint_blocks(n) for n in ref.FP_N] == [1, 1, 1, 1, 1, 2, 64, 64]
    assert ref.fingerprint_blocks(131072) == 64 and ref.fingerprint_blocks(129025) == 64
    assert ref.fingerprint_blocks(129024) == 63


def test_same_takes_nans_for_equal_and_nothing_else():
    nan2 = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
    assert ref.same([1.0, np.nan], [1.0, nan2]) and ref.same(-np.nan, np.nan)
    assert not ref.same([0.0], [-0.0]) and not ref.same([1.0], [np.nextafter(1.0, 2.0)])
    assert not ref.same([np.nan, 1.0], [1.0, np.nan]) and not ref.same([1.0], [1.0, 1.0])


# ------------------------------------------------------------------------------ stage 2
def _state(B=3, max_steps=4):
    s = ref.new_state(B, max_steps)
    s["active"][1] = 0
    return s


def _unchanged(a, b, b_idx, B, skip=()):
    """Every field of matrix b_idx equal in states a and b, but the named ones."""
    for k in a:
        if k in skip:
            continue
        cols = a[k].reshape(-1, B)[:, b_idx] if k in ("alpha", "beta") else a[k][b_idx]
        cols2 = b[k].reshape(-1, B)[:, b_idx] if k in ("alpha", "beta") else b[k][b_idx]
        assert ref.same(np.asarray(cols, dtype=np.float64), np.asarray(cols2, dtype=np.float64)), k


def test_stage2_lanczos_scalars():
    B, ms = 3, 4
    s0 = _state(B, ms)
    s0["rz"][:] = [3.0, 5.0, 1e-3]
    # START: rz = dot; stops unless positive and finite -- rz is written either way
    s = ref.stage2(s0, [7.0, 9.0, -2.0], ref.START, 0, ms)
    assert list(s["rz"]) == [7.0, 5.0, -2.0] and list(s["active"]) == [1, 0, 0]
    _unchanged(s0, s, 0, B, skip=("rz",)), _unchanged(s0, s, 1, B), _unchanged(s0, s, 2, B, skip=("rz", "active"))
    for bad in (0.0, -0.0, math.inf, math.nan):
        s = ref.stage2(s0, [bad, 1.0, 1.0], ref.START, 0, ms)
        assert s["active"][0] == 0 and ref.same(s["rz"][0], bad)
    # PAP: alpha = rz / dot at [na B + b]
    s = ref.stage2(s0, [7.0, 9.0, 0.0], ref.PAP, 0, ms)
    assert s["alpha"][0 * B + 0] == 3.0 / 7.0 and s["coef"][0] == 3.0 / 7.0 and s["na"][0] == 1
    assert s["active"][2] == 0
    _unchanged(s0, s, 1, B), _unchanged(s0, s, 2, B, skip=("active",))
    assert np.count_nonzero(s["alpha"] != s0["alpha"]) == 1
    s1 = ref.copy_state(s0)
    s1["na"][:] = [ms - 1, 0, ms]
    s = ref.stage2(s1, [7.0, 9.0, 2.0], ref.PAP, 0, ms)
    assert s["alpha"][(ms - 1) * B + 0] == 3.0 / 7.0 and list(s["na"]) == [ms, 0, ms + 1]
    assert s["coef"][2] == 1e-3 / 2.0 and np.count_nonzero(s["alpha"] != s1["alpha"]) == 1
    for bad in (0.0, -1.0, math.inf, math.nan):
        s = ref.stage2(s0, [bad, 1.0, 1.0], ref.PAP, 0, ms)
        assert s["active"][0] == 0
        _unchanged(s0, s, 0, B, skip=("active",))
    # RZ: beta = dot / rz, rz = dot; the residual is gone at dot <= 1e-28 rz
    thr = 1e-28 * 3.0
    s = ref.stage2(s0, [thr, 1.0, 4e-3], ref.RZ, 0, ms)
    assert s["active"][0] == 0 and s["beta"][2] == 4e-3 / 1e-3 and s["rz"][2] == 4e-3 and s["nb"][2] == 1
    _unchanged(s0, s, 0, B, skip=("active",))
    up = np.nextafter(thr, 1.0)
    s = ref.stage2(s0, [up, 1.0, 1.0], ref.RZ, 0, ms)
    assert s["active"][0] == 1 and s["beta"][0] == up / 3.0 and s["rz"][0] == up and s["coef"][0] == up / 3.0
    s1["nb"][:] = [ms, 0, ms - 1]
    s = ref.stage2(s1, [6.0, 1.0, 1.0], ref.RZ, 0, ms)
    assert list(s["nb"]) == [ms + 1, 0, ms] and s["beta"][(ms - 1) * B + 2] == 1.0 / 1e-3
    assert np.count_nonzero(s["beta"] != s1["beta"]) == 1 and s["rz"][0] == 6.0 and s["coef"][0] == 2.0


def test_stage2_power_scalars():
    B, ms = 3, 1
    s0 = _state(B, ms)
    s0["last"][:] = [2.0, 2.0, 1.0]
    s = ref.stage2(s0, [9.0, 9.0, 0.0], ref.NORM0, 0, ms)
    assert s["coef"][0] == 1.0 / 3.0 and list(s["active"]) == [1, 0, 0]
    _unchanged(s0, s, 0, B, skip=("coef",)), _unchanged(s0, s, 2, B, skip=("active",))
    for bad in (-1.0, math.inf, math.nan):
        assert ref.stage2(s0, [bad, 1.0, 1.0], ref.NORM0, 0, ms)["active"][0] == 0
    # NORM: mu2 and na always; settled from step 8 on
    for k, settles in ((7, False), (8, True)):
        s = ref.stage2(s0, [4.0, 1.0, 4.2], ref.NORM, k, ms)
        assert s["mu2"][0] == 2.0 and s["na"][0] == k + 1 and s["na"][2] == k + 1
        assert bool(s["active"][0]) == (not settles) and s["active"][2] == 1
        assert s["last"][2] == math.sqrt(4.2) and s["coef"][2] == 1.0 / math.sqrt(4.2)
        if settles:
            _unchanged(s0, s, 0, B, skip=("active", "mu2", "na"))
        else:
            assert s["last"][0] == 2.0 and s["coef"][0] == 0.5
    # the boundary of the 0.5 % rule between two neighbours: nv = 1 + m 2^-20, last = 1
    nv = [1.0 + m * 2.0 ** -20 for m in (5269, 5270)]
    assert [ref.power_settled(8, v, 1.0) for v in nv] == [True, False]
    assert [ref.power_settled(7, v, 1.0) for v in nv] == [False, False]
    assert all(math.sqrt(v * v) == v and Fraction(v * v) == Fraction(v) ** 2 for v in nv)
    s = ref.stage2(s0, [-4.0, 1.0, math.inf], ref.NORM, 3, ms)
    assert np.isnan(s["mu2"][0]) and s["mu2"][2] == math.inf and list(s["active"]) == [0, 0, 0]
    assert list(s["na"]) == [4, 0, 4]


# ------------------------------------------------------------------------------ updates
def _fma_inputs():
    rng = np.random.default_rng(5)
    a, b, c = (blockops_ref.real_data(4000, s) for s in (51, 52, 53))
    c[:1000] = -(a[:1000] * b[:1000])                               # cancellation to the last bits
    c[1000:1200] = np.nextafter(c[1000:1200], np.inf)
    spec = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1e300, -1e300,
                     1.7976931348623157e308, math.inf, -math.inf, math.nan, 1.0, -1.0, 0.5, 3.0])
    A, Bm, Cm = (v.ravel() for v in np.meshgrid(spec, spec, spec, indexing="ij"))
    ties = (1.0 + 2.0 ** -52 * rng.integers(0, 8, 300), 1.0 + 2.0 ** -52 * rng.integers(0, 8, 300),
            2.0 ** -53 * rng.integers(-8, 8, 300))
    return (np.concatenate([a, A, ties[0]]), np.concatenate([b, Bm, ties[1]]),
            np.concatenate([c, Cm, ties[2]]))


def test_fma_array_has_one_rounding():
    a, b, c = _fma_inputs()
    got = ref.fma_array(a, b, c)
    want = np.array([ref.fma_scalar(x, y, z) for x, y, z in zip(a, b, c)])
    assert ref.same(got, want)
    # the scalar against Fraction on finite data, as krylov_ref.fma does it
    fin = np.flatnonzero(np.isfinite(a) & np.isfinite(b) & np.isfinite(c))[:6000]
    for i in fin:
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        if abs(exact) < Fraction(2) ** 1023 and exact != 0:
            assert want[i] == krylov_ref.fma(a[i], b[i], c[i]), i
    assert ref.fma_scalar(1e308, 10.0, -math.inf) == -math.inf
    assert math.isnan(ref.fma_scalar(0.0, math.inf, 1.0)) and math.isnan(ref.fma_scalar(1.0, 1.0, math.nan))
    assert math.isnan(ref.fma_scalar(math.inf, 1.0, -math.inf))
    assert ref.fma_scalar(1e308, 10.0, 0.0) == math.inf and ref.fma_scalar(-1e308, 10.0, 1e308) == -math.inf
    # (the product alone overflows, the sum does not)
    assert ref.fma_scalar(1.5e308, 1.125, -1e308) == float(Fraction(1.5e308) * Fraction(1.125) - Fraction(1e308))
    z = [ref.fma_scalar(*t) for t in ((-0.0, 1.0, -0.0), (0.0, 1.0, -0.0), (-0.0, -1.0, -0.0),
                                      (3.0, 2.0, -6.0), (0.0, -5.0, 0.0), (5e-324, 0.25, -0.0))]
    assert [math.copysign(1.0, v) for v in z] == [-1.0, 1.0, 1.0, 1.0, 1.0, 1.0] and not any(z)
    assert ref.fma_scalar(-5e-324, 0.25, -0.0) == 0.0 and math.copysign(1.0, ref.fma_scalar(-5e-324, 0.25, 0.0)) < 0
    # ties in the subnormals go to even: 1.5 and 2.5 units both give 2
    assert ref.fma_scalar(5e-324, 0.5, 5e-324) == 1e-323 and ref.fma_scalar(5e-324, 0.5, 1e-323) == 1e-323
    assert ref.fma_scalar(5e-324, 0.25, 5e-324) == 5e-324 and ref.fma_scalar(5e-324, 0.75, 1e-323) == 1.5e-323


@pytest.mark.parametrize("kind", (ref.UPD_R, ref.UPD_P, ref.UPD_SCALE, ref.UPD_COPY))
def test_update_forms(kind):
    B, n = 3, 300
    stride = ref.batch_stride(n)
    v = ref.special_values(blockops_ref.real_data((B, stride), 61), 1)
    x = ref.special_values(blockops_ref.real_data((B, stride), 62), 2)
    x[2, 5], x[2, 6] = math.nan, math.inf
    active = np.array([1, 0, 1], dtype=np.uint32)
    for coef in ([1.0 / 3.0, 9.0, -2.5], [0.0, 9.0, -0.0]):
        got = ref.update(kind, v, x, coef, active, n)
        assert blockops_ref.same_bits(got[1], v[1]) and blockops_ref.same_bits(got[:, n:], v[:, n:])
        for b in (0, 2):
            c = coef[b]
            for p in range(n):
                with np.errstate(all="ignore"):
                    cv = float(np.float64(c) * v[b, p])
                want = {ref.UPD_R: lambda: ref.fma_scalar(-c, x[b, p], v[b, p]),
                        ref.UPD_P: lambda: ref.fma_scalar(1.0, x[b, p], cv),
                        ref.UPD_SCALE: lambda: ref.fma_scalar(0.0, x[b, p], cv),
                        ref.UPD_COPY: lambda: x[b, p]}[kind]()
                assert ref.same(got[b, p], want), (b, p, c)
        if kind == ref.UPD_SCALE:       # 0 NaN and 0 inf: the second vector's NaN keeps its way
            assert np.isnan(got[2, 5]) and np.isnan(got[2, 6])
        if kind == ref.UPD_COPY:
            assert blockops_ref.same_bits(got[0, :n], x[0, :n])
    assert ref.axpby_coefficients(ref.UPD_R, 0.25) == (-0.25, 1.0)
    assert ref.axpby_coefficients(ref.UPD_P, 0.25) == (1.0, 0.25)
    assert ref.axpby_coefficients(ref.UPD_SCALE, 0.25) == (0.0, 0.25)


# -------------------------------------------------------------------------- fingerprint
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 2048, 2049, 4100, 9000))
def test_fingerprint_equals_the_scalar_restatement(n):
    a = ref.special_values(blockops_ref.real_data(n, 71), 3)
    words, folded = ref.fingerprint(a)
    swords, sfolded = ref.fingerprint_scalar(a)
    assert len(words) == ref.fingerprint_blocks(n) and np.array_equal(words, swords)
    assert folded == sfolded == ref.fold(words) and 0 <= folded < 2 ** 64


def test_last_share_position():
    for n in (1, 2, 255, 256, 257, 2048, 2049, 2305, 4100, 131073, 140000, 600001):
        nb = ref.fingerprint_blocks(n)
        seen = [p for p in range(n) if (p % (nb * ref.THREADS)) // ref.THREADS == nb - 1]
        assert ref.last_share_position(n) == (max(seen) if seen else n - 1), n


@pytest.mark.parametrize("nmat", ref.FP_NMAT)
@pytest.mark.parametrize("n", ref.FP_N)
def test_every_flip_of_the_gpu_tests_changes_the_reference_fingerprint(n, nmat):
    a = ref.fingerprint_arrays(n, nmat)
    folds = [ref.fingerprint(a[m])[1] for m in range(nmat)]
    assert len(set(folds)) == nmat                        # distinct candidates, distinct fingerprints
    m = nmat - 1
    for pos in ref.fingerprint_positions(n):
        for kind in ref.BIT_KINDS:
            base, other = ref.flip(a[m], pos, kind)
            assert np.count_nonzero(base.view(np.uint64) != other.view(np.uint64)) == 1
            assert bin(int(base.view(np.uint64)[pos] ^ other.view(np.uint64)[pos])).count("1") == 1
            wb, fb = ref.fingerprint(base)
            wo, fo = ref.fingerprint(other)
            assert fb != fo, (pos, kind)
            assert np.count_nonzero(wb != wo) == 1       # one workgroup's word


def test_positions_reach_both_trips():
    assert ref.pair_positions(1) == [0]
    assert ref.pair_positions(65536) == [0, 32768, 65535]
    assert ref.pair_positions(65537) == [0, 32768, 65535, 65536]
    assert ref.pair_positions(200001) == [0, 65535, 65536, 100000, 200000]
    assert ref.fingerprint_positions(1) == [0]
    assert set(ref.fingerprint_positions(600001)) >= {0, 255, 256, 600000}
