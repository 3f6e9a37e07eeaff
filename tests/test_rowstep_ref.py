"""``tests/rowstep_ref.py`` and the data of ``tests/rowstep_cases.py`` on the host, before a GPU sees
them: the vectorised fma is the exact one; the unfused candidate is the NumPy oracle's step; every
candidate lies inside the bound; the real-data sets of every GPU launch separate every two
candidates on at least 5 % of the unmasked outputs (with production's ``cy = 1`` or ``ca = -1``
candidates coincide, which is why the sets use other coefficients); and the comparison the GPU test
makes rejects each of seven perturbations."""
import dataclasses
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import rowstep_cases as rc
import rowstep_ref as ref
import structures as st
from oracle import kkt_oracle as ko

SEPARATION = 0.05


def test_fma_np_is_the_exact_fma():
    rng = np.random.default_rng(ref.SEED)
    a = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    b = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    c = rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))
    c[:1000] = -(a[:1000] * b[:1000])                 # cancellation: the product's error is the result
    c[1000:1200] = 0.0
    a[1100:1300] = 0.0
    c[1250:1300] = -0.0
    # ties: a b = 1 + 2^-52 + 2^-104 exactly halfway and just off it
    a[3000:3004] = [1 + 2.0 ** -26, 1 + 2.0 ** -26, 3.0, 3.0]
    b[3000:3004] = [1 + 2.0 ** -26, 1 - 2.0 ** -26, 2.0 ** -54, 2.0 ** -54]
    c[3000:3004] = [2.0 ** -53, -2.0 ** -53, 1.0, 1 + 2.0 ** -52]
    got = ref.fma_np(a, b, c)
    want = np.array([ref.fma(x, y, z) for x, y, z in zip(a, b, c)])
    nz = want != 0.0
    assert ref.same_bits(got[nz], want[nz])
    assert np.all(got[~nz] == 0.0)
    # signed zeros as IEEE 754 has them
    z = ref.fma_np(np.array([0.0, -0.0, 0.0, 2.0]), np.array([1.0, 1.0, -1.0, 1.0]),
                   np.array([0.0, -0.0, -0.0, -2.0]))
    assert list(np.signbit(z)) == [False, True, True, False]


def test_unfused_candidate_is_the_oracle_step_on_integer_data():
    n = 300
    A = st.banded(n, 7, seed=1, integer=True)
    dinv, b, x0 = ref.pow2_vec(n, 1), ref.int_vec(n, 2), ref.int_vec(n, 3)
    emin, emax = 0.5, 15.5                                         # scale = 2 / 16
    p1 = ko.chebyshev_jacobi_from(A, dinv, b, x0, emin, emax, 1)
    op1 = ref.Op("cheb", [(A, x0)], dinv=dinv, b=b, pk=x0, c2=1.0, c3=2.0 / (emax + emin))
    assert ref.same_bits(ref.run(op1, "uu")[0], p1)
    p2 = ko.chebyshev_jacobi_from(A, dinv, b, x0, emin, emax, 2)
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    mu = 1.0 / alpha
    omega = (2.0 / alpha) * mu / (2.0 * mu * mu - 1.0)
    op2 = ref.Op("cheb", [(A, p1)], dinv=dinv, b=b, pk=p1, pkm1=x0, c1=1.0 - omega, c2=omega,
                 c3=scale * omega)
    assert ref.same_bits(ref.run(op2, "uu")[0], p2)
    # ... and the zero-guess solve: first step (no matrix), then one three-term step
    q2 = ko.chebyshev_jacobi(A, dinv, b, emin, emax, 2)
    q1 = ref.run(ref.Op("cheb", dinv=dinv, b=b, c3=scale), "uu")[0]
    op = ref.Op("cheb", [(A, q1)], dinv=dinv, b=b, pk=q1, pkm1=np.zeros(n), c1=1.0 - omega,
                c2=omega, c3=scale * omega)
    assert ref.same_bits(ref.run(op, "uu")[0], q2)


def test_unfused_lin_candidate_is_the_numpy_expression_on_integer_data():
    """The level update ``b - U x`` and the products ``y = ca A x (+ cz z)`` as the oracle's drivers
    write them (``kkt_oracle.pc_instationary_BE``: ``rhs - blk @ u``), and ``y2`` as the first step of
    ``chebyshev_jacobi`` on the updated right-hand side."""
    n = 300
    A, B = st.banded(n, 7, seed=1, integer=True), None
    B = st.with_values(A, 5, integer=True)
    x, w, yin, z = (ref.int_vec(n, k) for k in (4, 5, 6, 7))
    dinv = ref.pow2_vec(n, 2)
    emin, emax = 0.5, 15.5
    op = ref.Op("lin", [(A, x), (B, w)], ca=-1.0, cy=1.0, yin=yin, y2=True, dinv=dinv,
                c3=2.0 / (emax + emin))
    y, y2 = ref.run(op, "uu")
    want = yin - (A @ x + B @ w)
    assert ref.same_bits(y, want)
    assert ref.same_bits(y2, ko.chebyshev_jacobi(A, dinv, want, emin, emax, 1))
    # non-dyadic coefficients: the plain NumPy expression, left to right
    op = ref.Op("lin", [(A, x)], ca=-0.37, cy=0.77, cz=0.43, yin=yin, z=z)
    assert ref.same_bits(ref.run(op, "uu")[0], (-0.37 * (A @ x) + 0.77 * yin) + 0.43 * z)
    # masked rows: the exact zero of the bc-assembled matrix, and y2 from it
    m = ref.row_mask(n)
    op = ref.Op("lin", [(A, x)], ca=-1.0, cy=1.0, yin=yin, y2=True, dinv=dinv, c3=0.125, mask=m)
    y, y2 = ref.run(op, "uu")
    assert ref.same_bits(y, np.where(m, 0.0, yin - A @ x)) and ref.same_bits(y2, 0.125 * (dinv * y))


# ---- the data of the GPU launches
def _launches(kind):
    for sname, n, makers in rc.cases():
        A, _ = rc.structure(sname, n)
        mats = rc.matrices(A, kind)
        for mk in makers:
            L = mk(kind)
            yield L, rc.ref_ops(L, mats)


@pytest.fixture(scope="module")
def real_launches():
    return list(_launches("real"))


def test_every_data_set_separates_the_candidates_inside_the_bound(real_launches):
    worst_sep, worst_ratio, pairs = 1.0, 0.0, 0
    for L, ops in real_launches:
        for k, op in enumerate(ops):
            acc = ref.accumulate(op)
            un = np.ones(op.n, bool) if op.mask is None else ~op.mask
            outs = {c: ref.run(op, c, acc) for c in ref.candidates(op)}
            tri, tri2 = ref.exact(op)
            for c, (y, y2) in outs.items():
                r = ref.bound_ratio(y, tri, un)
                if y2 is not None:
                    r = max(r, ref.bound_ratio(y2, tri2, un))
                worst_ratio = max(worst_ratio, r)
                assert r <= 1.0, (L.name, k, c, r)
            if not un.any():           # (one row, and that one masked: no unmasked output)
                continue
            for c, d in itertools.combinations(outs, 2):
                sep = ref.differ(outs[c][0], outs[d][0])[un].mean()
                worst_sep = min(worst_sep, sep)
                pairs += 1
                assert sep >= SEPARATION, (L.name, k, op.operands(), c, d, sep)
    assert pairs > 500
    print(f"smallest separation {worst_sep:.3f}, largest error / bound {worst_ratio:.3f}")


def test_integer_sets_make_every_candidate_coincide():
    for L, ops in itertools.islice(_launches("int"), 0, None, 7):
        for op in ops:
            acc = ref.accumulate(op)
            outs = [ref.run(op, c, acc) for c in ref.candidates(op)]
            for y, y2 in outs[1:]:
                assert ref.same_bits(y, outs[0][0])
                assert y2 is None or ref.same_bits(y2, outs[0][1])


def test_production_coefficients_do_not_separate():
    n = 3000
    A = st.banded(n, 7, seed=2)
    x, yin, z = (ref.real_vec(n, k) for k in (1, 2, 3))
    op = ref.Op("lin", [(A, x)], ca=-0.37, cy=1.0, cz=0.43, yin=yin, z=z)
    assert ref.same_bits(ref.run(op, "uu")[0], ref.run(op, "fu")[0])          # cy = 1
    op = ref.Op("lin", [(A, x)], ca=-1.0, cy=0.77, cz=0.43, yin=yin, z=z)
    assert ref.same_bits(ref.run(op, "uu")[0], ref.run(op, "gu")[0])          # ca = -1
    op = ref.Op("lin", [(A, x)], ca=-0.37, cy=0.77, cz=0.43, yin=yin, z=z)
    outs = [ref.run(op, c)[0] for c in ref.candidates(op)]
    for u, v in itertools.combinations(outs, 2):
        assert 0.13 <= ref.differ(u, v).mean() <= 0.5


# ---- each comparison can fail
@pytest.fixture(scope="module")
def middle():
    """A middle Chebyshev step and a two-term level update on a ragged structure."""
    n = 513
    A, _ = rc.structure("ragged", n)
    mats = rc.matrices(A, "real")
    L = rc.rows_launch("perturb", n, "real")
    ops = rc.ref_ops(L, mats)
    return A, mats, L, ops


def _accepted(op, y, y2=None):
    return ref.matching(op, y, y2)


def test_neighbouring_candidate_is_rejected(middle):
    _, _, _, ops = middle
    for op in ops:
        cands = ref.candidates(op)
        for c in cands:
            y, y2 = ref.run(op, c)
            assert _accepted(op, y, y2) == [c]


def test_dropped_slot_swapped_operands_and_terms_are_rejected(middle):
    _, _, L, ops = middle
    cheb = ops[11]                                   # pk and pkm1
    assert cheb.pk is not None and cheb.pkm1 is not None
    for c in ref.candidates(cheb):
        assert not _accepted(cheb, ref.run(cheb, c, ref.accumulate(cheb, drop_last=True))[0])
        sw = dataclasses.replace(cheb, pk=cheb.pkm1, pkm1=cheb.pk)
        assert not _accepted(cheb, ref.run(sw, c, ref.accumulate(cheb))[0])
    lin = ops[4]                                     # two terms
    assert len(lin.terms) == 2
    sw = dataclasses.replace(lin, terms=lin.terms[::-1])
    for c in ref.candidates(lin):
        y, y2 = ref.run(sw, c)
        assert not _accepted(lin, y, y2)


def test_negative_zero_on_a_masked_row_is_rejected(middle):
    _, _, _, ops = middle
    for op in (ops[3], ops[11]):
        y, y2 = ref.run(op, "uu")
        r = int(np.flatnonzero(op.mask)[-1])
        assert y[r] == 0.0 and not np.signbit(y[r])
        y = y.copy()
        y[r] = -0.0
        assert not _accepted(op, y, y2)


def test_post_factor_of_the_next_level_is_rejected():
    n = 257
    A, _ = rc.structure("w9", n)
    mats = rc.matrices(A, "real")
    L = rc.il_launch("post", n, "real", "last")
    ops = rc.ref_ops(L, mats)
    for l in range(len(ops) - 1):
        wrong = dataclasses.replace(ops[l], post1=ops[l + 1].post1)
        for c in ref.candidates(ops[l]):
            assert not _accepted(ops[l], ref.run(wrong, c)[0])


def test_swapped_sell_position_is_rejected(middle):
    A, mats, _, ops = middle
    n = A.shape[0]
    sw = st.slice_widths(A)
    off = np.r_[0, np.cumsum(sw)]
    w = np.diff(A.indptr)
    # the value array as stored, read back through the right and through the exchanged layout
    M = mats[1]
    stored = np.zeros(off[-1] * 128)
    for r in range(n):
        for k in range(w[r]):
            stored[ref.sell_index(r, k, off)] = M.data[A.indptr[r] + k]
    right = np.array([stored[ref.sell_index(r, k, off)] for r in range(n) for k in range(w[r])])
    wrong = np.array([stored[ref.sell_index_swapped(r, k, off)] for r in range(n)
                      for k in range(w[r])])
    assert np.array_equal(right, M.data)
    op = ops[1]                                       # y = ca A x with block 1
    assert op.terms[0][0] is mats[1]
    Mw = sp.csr_matrix((wrong, A.indices, A.indptr), shape=A.shape)
    bad = dataclasses.replace(op, terms=[(Mw, op.terms[0][1])])
    assert not _accepted(op, ref.run(bad, "uu")[0])
