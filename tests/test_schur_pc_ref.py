"""The extended-precision definition of the Schur preconditioner (tests/schur_pc_ref.py): against
plain facts, against the float64 oracle on every case of tests/schur_pc_cases.py, and against
seeded misreadings.  No GPU.

* facts: ``r_k(0) = 1``; ``|r_k| <= 1 / T_k(d / a)`` on the interval; with a degree at which
  ``r_k < 1e-30`` on the spectrum ``Q(A) b`` is ``A^-1 b`` and ``L^-1 g`` solves the block
  bidiagonal system with the matrices themselves on the diagonal;
* every case: the reference agrees with itself across 50 and 70 digits to 1e-18, with the fixture
  ``tests/golden/schur_pc_definition.npz`` exactly, and the oracle is within ``d_case <= 1e-13`` of
  it per output block (largest measured: 2.8e-14, backward Euler on the convection operators
  with ``b_0`` on one level; random inputs: 2.2e-14 Crank-Nicolson n_t = 4 two-grid, backward
  Euler at most 3.4e-15).  The device test's bar is built on ``d_case``, so this cap keeps it tight;
* impulses: output blocks that are exactly zero in the reference are ``+0.0`` in the oracle,
  boundary rows carry the input bit for bit;
* every seeded misreading moves the comparison above the cap.
"""
import mpmath as mp
import numpy as np
import pytest

import schur_pc_cases as sc
import schur_pc_ref as ref

CAP = 1e-13


# ------------------------------------------------------------------------------ plain facts
ELLIPSES = [(0.07, 2.1, 0.0), (0.25, 2.0, 0.0), (0.07, 2.1, 0.3), (0.25, 2.0, 1.5)]


@pytest.mark.parametrize("emin,emax,eimag", ELLIPSES)
def test_residual_polynomial_is_one_at_zero(emin, emax, eimag):
    with mp.workdps(ref.DPS):
        for k in (0, 1, 2, 3, 8, 20):
            r = ref.residual_polynomial(k, mp.mpf(0), emin, emax, eimag)
            assert r == 1 and mp.im(r) == 0, (k, r)


@pytest.mark.parametrize("emin,emax", [(0.07, 2.1), (0.25, 2.0), (0.05, 2.1)])
def test_residual_polynomial_is_bounded_on_the_interval(emin, emax):
    """``max |r_k| = 1 / T_k(d / a)`` on ``[emin, emax]``, attained at both ends."""
    with mp.workdps(ref.DPS):
        d, a = (mp.mpf(emax) + mp.mpf(emin)) / 2, (mp.mpf(emax) - mp.mpf(emin)) / 2
        for k in (1, 2, 3, 6, 20):
            bound = 1 / ref.chebyshev_T(k, d / a)
            lams = [mp.mpf(emin) + (mp.mpf(emax) - mp.mpf(emin)) * j / 200 for j in range(201)]
            vals = [abs(ref.residual_polynomial(k, lam, emin, emax)) for lam in lams]
            assert max(vals) <= bound * (1 + mp.mpf(10) ** -40), (k, max(vals), bound)
            assert abs(vals[0] - bound) <= bound * mp.mpf(10) ** -40
            assert abs(vals[-1] - bound) <= bound * mp.mpf(10) ** -40
            # ... and outside the interval, towards 0, it grows to 1
            assert abs(ref.residual_polynomial(k, mp.mpf(emin) / 2, emin, emax)) > bound


def _degree_for(emin, emax, target):
    with mp.workdps(ref.DPS):
        d, a = (mp.mpf(emax) + mp.mpf(emin)) / 2, (mp.mpf(emax) - mp.mpf(emin)) / 2
        k = 1
        while 1 / ref.chebyshev_T(k, d / a) >= target:
            k += 1
        return k


def test_high_degree_sub_solves_are_the_inverses():
    """An interval that brackets the spectrum of every ``D^-1 A`` and a degree with
    ``1 / T_k(d / a) < 1e-30``: the sub-solves are the inverses, so the forward stage ``w`` of
    backward Euler solves ``(blockdiag(A_i) + P_bc N) w = g`` with the level matrices themselves."""
    c = sc.case("BE", 4, 6)
    p = sc.problem(c)
    M, b10, nodes = p["sd"].M.toarray(), p["blocks"][2], p["nodes"]
    free = np.setdiff1d(np.arange(M.shape[0]), nodes)
    s = p["tau"] / p["beta"] ** 0.5
    lo, hi = np.inf, 0.0
    for i, ci in enumerate((0.0, s, s, sc.EPSILON ** 0.5 * s)):
        A = (b10[(i, i)].toarray() + ci * M)[np.ix_(free, free)]
        ev = np.linalg.eigvals(A / np.diag(A)[:, None]).real
        lo, hi = min(lo, ev.min()), max(hi, ev.max())
    emin, emax = 0.9 * lo, 1.1 * hi
    k = _degree_for(emin, emax, mp.mpf(10) ** -30)
    R = sc.reference(c)
    R._schur = dict(its=k, emin=emin, emax=emax, eimag=0.0)
    rng = np.random.default_rng(3)
    with mp.workdps(ref.DPS):
        # one sub-solve: Q(A) b = A^-1 b
        A = R.shifted(2, 1, 1, R.tau / mp.sqrt(R.beta), True)
        b = R.P_bc(ref.vec(rng.standard_normal(R.nx)))
        x = R.Q(A, b, R.schur("forward", 1))
        res = [u - v for u, v in zip(A.matvec(x), b)]
        assert ref._amax(res) <= mp.mpf(10) ** -28 * ref._amax(b), (k, ref._amax(res))
        # the forward stage
        g = [R.P_bc(ref.vec(rng.standard_normal(R.nx))) for _ in range(R.m)]
        sq = mp.sqrt(R.eps)
        shifts = [mp.mpf(0), R.tau / mp.sqrt(R.beta), R.tau / mp.sqrt(R.beta),
                  sq * R.tau / mp.sqrt(R.beta)]
        w = R.bidiagonal_inverse(
            lambda i, rhs: R.Q(R.shifted(2, i, i, shifts[i], True), rhs, R.schur("forward", i)),
            lambda i, j: R.raw(2, i, j), g, lower=True)
        for i in range(R.m):
            lhs = R.shifted(2, i, i, shifts[i], True).matvec(w[i])
            if i >= 1:
                lhs = [u + v for u, v in zip(lhs, R.P_bc(R.raw(2, i, i - 1).matvec(w[i - 1])))]
            res = [u - v for u, v in zip(lhs, g[i])]
            assert ref._amax(res) <= mp.mpf(10) ** -28 * ref._amax(g[i]), (i, k)


def test_transform_inverses():
    rng = np.random.default_rng(5)
    with mp.workdps(ref.DPS):
        x = [ref.vec(rng.standard_normal(3)) for _ in range(5)]
        R = ref.Reference
        assert R.T1(R.T1_inv(x)) == x and R.T2(R.T2_inv(x)) == x
        assert R.T1(x)[0] == [a + b for a, b in zip(x[0], x[1])] and R.T1(x)[4] == x[4]
        assert R.T2(x)[4] == [a + b for a, b in zip(x[4], x[3])] and R.T2(x)[0] == x[0]


# ------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_oracle_is_close_to_the_definition(c):
    x = sc.inputs(c)["random"]
    x0, x1 = sc.split(c, x)
    own, (u0, u1), imag = ref.self_distance(lambda dps: sc.reference(c, dps=dps), x0, x1)
    (h0, l0), (h1, l1) = ref.to_pairs(u0), ref.to_pairs(u1)
    g0, gl0, g1, gl1, d_gold = sc.golden_reference(c, "random")
    d = sc.distance(c, sc.oracle_apply(c, x), h0, l0, h1, l1)
    print(f"definition {sc.case_id(c)}: d_case {d:.2e} self {own:.1e} imag {float(imag):.1e}")
    assert own <= 1e-18, own
    assert imag <= mp.mpf(10) ** -40, imag
    # the fixture holds this reference and this distance
    assert np.array_equal(h0, g0) and np.array_equal(h1, g1)
    assert np.array_equal(l0.astype(np.float32), gl0.astype(np.float32))
    assert np.array_equal(l1.astype(np.float32), gl1.astype(np.float32))
    # (the oracle inverts its coarse matrices with LAPACK: its last bits may differ by platform)
    assert abs(d - d_gold) <= 0.5 * max(d, d_gold), (d, d_gold)
    assert d <= CAP and d_gold <= CAP, (sc.case_id(c), d, d_gold)


IMPULSE_CASES = [c for c in sc.CASES if c["impulses"]]


@pytest.mark.parametrize("c", IMPULSE_CASES, ids=sc.case_id)
def test_impulses_through_the_oracle(c):
    p = sc.problem(c)
    zero_blocks = 0
    for name, x in sc.inputs(c).items():
        gold = sc.golden_reference(c, name)
        y = sc.oracle_apply(c, x)
        d = sc.distance(c, y, *gold[:4])
        print(f"definition {sc.case_id(c)} {name}: d_case {d:.2e} (fixture {gold[4]:.2e})")
        assert d <= CAP and gold[4] <= CAP, (name, d, gold[4])
        assert abs(d - gold[4]) <= 0.5 * max(d, gold[4]), (name, d, gold[4])
        assert sc.zero_blocks_are_plus_zero(c, y, *gold[:4]), name
        zero_blocks += sum(int(not h.any()) for hi in (gold[0], gold[2]) for h in hi)
        assert np.array_equal(sc.split(c, y)[:, :, p["nodes"]], sc.split(c, x)[:, :, p["nodes"]])
    assert zero_blocks >= 2 * p["m"]      # (the boundary-node impulses alone leave 2 (2 m - 1))


def test_impulse_references_are_the_fixture():
    """The fixture's impulse references recomputed (one case per sweep kind)."""
    for c in (IMPULSE_CASES[0], next(c for c in IMPULSE_CASES if c["kind"] == "CN")):
        R = sc.reference(c)
        for name, x in sc.inputs(c).items():
            if name == "random":
                continue
            u0, u1 = R.apply(*sc.split(c, x))
            gold = sc.golden_reference(c, name)
            assert np.array_equal(ref.to_pairs(u0)[0], gold[0]), name
            assert np.array_equal(ref.to_pairs(u1)[0], gold[2]), name


# ------------------------------------------------------------------------------ misreadings
def _find(**kw):
    for c in sc.CASES:
        if all(c[k] == v for k, v in kw.items()):
            return c
    raise KeyError(kw)


WRONG = [("eps_first", dict(kind="BE", n_t=4, schur=6, coarse=0, disc="p1", td=False, beta=1e-2)),
         ("no_sqrt_eps", dict(kind="BE", n_t=4, schur=6, coarse=0, disc="p1", td=False, beta=1e-2)),
         ("no_sqrt_eps", dict(kind="BE", n_t=5, schur=6, coarse=0, disc="p1", beta=1e-4)),
         ("swap_T", dict(kind="CN", n_t=4, schur=6, coarse=0, disc="p1", td=False, beta=1e-2)),
         ("degree_minus_1", dict(kind="BE", n_t=5, schur=3, coarse=0, disc="p1", td=False)),
         ("degree_minus_1", dict(kind="CN", n_t=6, schur=6, coarse=0, disc="p1", td=False,
                                 beta=1e-2)),
         ("degree_minus_1", dict(kind="stationary", schur=1)),
         ("restart_from_zero", dict(kind="BE", n_t=4, schur=4, coarse=1, disc="p1")),
         ("restart_from_zero", dict(kind="CN", n_t=6, schur=2, coarse=2)),
         ("bc_not_passed", dict(kind="BE", n_t=4, schur=6, coarse=0, disc="p1", td=False,
                                beta=1e-2)),
         ("bc_not_passed", dict(kind="stationary", schur=6))]


@pytest.mark.parametrize("wrong,sel", WRONG, ids=[f"{w}-{i}" for i, (w, _) in enumerate(WRONG)])
def test_wrong_reference_is_rejected(wrong, sel):
    """The misreading seeded into the reference: the oracle is far from it."""
    c = _find(**sel)
    x = sc.inputs(c)["random"]
    u0, u1 = sc.reference(c, wrong=wrong).apply(*sc.split(c, x))
    d = sc.distance(c, sc.oracle_apply(c, x), *ref.to_pairs(u0), *ref.to_pairs(u1))
    print(f"definition {sc.case_id(c)} wrong {wrong}: distance {d:.2e}")
    assert d > 1e3 * CAP, (wrong, d)


@pytest.mark.parametrize("eimag", [0.3, 1.5])
def test_wrong_first_ellipse_step_is_rejected(eimag, monkeypatch):
    """The misreading seeded into the oracle: 1/4 in place of 1/2 in the first ellipse step."""
    from oracle import kkt_oracle as ko
    c = _find(kind="BE", schur=6, disc="conv", eimag=eimag)

    def quarter(emin, emax, eimag, its):
        d, a = 0.5 * (emax + emin), 0.5 * (emax - emin)
        c2 = a * a - eimag * eimag
        out, alpha = [], 1.0 / d
        for _ in range(1, its):
            alpha = 1.0 / (d - 0.25 * c2 * alpha)
            out.append((-(d * alpha - 1.0), d * alpha, alpha))
        return out

    x = sc.inputs(c)["random"]
    gold = sc.golden_reference(c, "random")
    assert sc.distance(c, sc.oracle_apply(c, x), *gold[:4]) <= CAP
    monkeypatch.setattr(ko, "chebyshev_ellipse_coefficients", quarter)
    d = sc.distance(c, sc.oracle_apply(c, x), *gold[:4])
    print(f"definition {sc.case_id(c)} wrong quarter: distance {d:.2e}")
    assert d > 1e3 * CAP, d


def test_wrong_input_is_rejected():
    """A reference of another input (one entry moved by one part in 1e9) is told apart."""
    c = sc.CASES[0]
    x = sc.inputs(c)["random"].copy()
    gold = sc.golden_reference(c, "random")
    x[8] *= 1.0 + 1e-9          # (a free node of the first level)
    assert sc.distance(c, sc.oracle_apply(c, x), *gold[:4]) > CAP
