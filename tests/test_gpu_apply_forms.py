"""Every form of the operator apply against exact references (run with -m gpu on an MI355X).

The apply picks its kernel per launch from the slice widths of the block structures
(kernels.hip launch_rowops; system.cpp finalize): the fixed-width kernel of width 1..16, the
shared-values kernel for groups of block rows with equal structure (widths 1..8), the
width-switched kernel in three shapes for ragged structures, and the slot loop.  Each case
builds a structure for one of them (tests/structures.py), asserts through
``MultiBlockSystem.apply_forms`` that the launch ran that form, and checks the product:

- integer data: every product and partial sum is exact in fp64, in any order, so ``mult`` must
  equal the oracle's product bit for bit -- a missed term, a padded slot read as a value, a wrong
  segment, row permutation or mask cannot hide behind a tolerance;
- real data: row by row against a correctly rounded reference (error-free products, ``fsum``),
  |y_i - y*_i| <= (k_i + 2) u (|A||x|)_i + u |y*_i| with k_i the stored entries of the row;
- every layout option must leave the result bit-identical (each row keeps its fma chain).
"""
import numpy as np
import pytest

import structures as st
from control_amd.multiblock import (ConstantNullspace, DirichletBCNullspace, FullNullspace,
                                    MultiBlockSystem, NoneNullspace)

pytestmark = pytest.mark.gpu

SWITCH, SWITCH_1WAVE, SWITCH_NARROW, SLOT_LOOP = -2, -3, -4, -1
ALPHA = 2.5
M = 3                                    # time levels per variable


# --------------------------------------------------------------------------- systems
class Case:
    """A two-variable block system on given structures: per variable a square level pattern
    (diagonal block and one time neighbour, as in the BE / CN stencils) and the coupling blocks
    between the variables (rectangular when nx0 != nx1)."""

    def __init__(self, name, S0, S1=None, C=None, D=None, form=None):
        self.name, self.S0 = name, S0
        self.S1 = S0 if S1 is None else S1
        self.C = S0 if C is None else C              # nx0 x nx1
        self.D = S0 if D is None else D              # nx1 x nx0
        self.form = form                             # what apply_forms must report

    def blocks(self, seed, integer):
        v = lambda A, k: st.with_values(A, seed * 16 + k, integer)   # noqa: E731
        A, A2, E, E2 = v(self.S0, 0), v(self.S0, 1), v(self.S1, 2), v(self.S1, 3)
        C, D = v(self.C, 4), v(self.D, 5)
        keys = [(i, j) for i in range(M) for j in range(M)]
        b00 = {k: A if k[0] == k[1] else A2 if k[1] == k[0] - 1 else None for k in keys}
        b01 = {k: C if k[0] == k[1] else None for k in keys}
        b10 = {k: D if k[0] == k[1] else None for k in keys}
        b11 = {k: E if k[0] == k[1] else E2 if k[1] == k[0] + 1 else None for k in keys}
        return b00, b01, b10, b11

    @property
    def nx(self):
        return self.S0.shape[0], self.S1.shape[0]

    def nullspaces(self, rich):
        nx0, nx1 = self.nx
        bc0 = np.arange(0, nx0, 5, dtype=np.int32)
        bc1 = np.arange(1, nx1, 7, dtype=np.int32)
        ns0 = [DirichletBCNullspace(bc0, alpha=ALPHA) for _ in range(M)]
        ns1 = [DirichletBCNullspace(bc1, alpha=ALPHA) for _ in range(M)]
        if rich:
            # ConstantNullspace where the mean is exact (a power-of-two length), FullNullspace
            ns0[1] = NoneNullspace()
            ns1[2] = FullNullspace()
            if nx1 & (nx1 - 1) == 0:
                ns1[0] = ConstantNullspace(alpha=ALPHA)
        return ns0, ns1

    def gpu(self, blocks, layout, options=None, share=True, rich=True):
        ns0, ns1 = self.nullspaces(rich)
        kw = dict(sub_n_blocks_00_0=1, sub_n_blocks_11_0=2) if layout == "CN_split" else {}
        return MultiBlockSystem(*self.nx, *blocks, n_blocks_00=M, n_blocks_11=M,
                                nullspace_0=ns0, nullspace_1=ns1, CN=layout != "BE",
                                options=options, share_values=share, **kw)

    def oracle(self, blocks, layout, rich=True):
        from oracle import kkt_oracle as ko

        def conv(ns):
            if isinstance(ns, DirichletBCNullspace):
                return ko.DirichletBCNullspace(ns._nodes, alpha=ns._alpha)
            if isinstance(ns, ConstantNullspace):
                return ko.ConstantNullspace(alpha=ns._alpha)
            if isinstance(ns, FullNullspace):
                return ko.FullNullspace()
            return ko.NoneNullspace()
        ns0, ns1 = self.nullspaces(rich)
        kw = dict(sub_n_blocks_00_0=1, sub_n_blocks_11_0=2) if layout == "CN_split" else {}
        return ko.OracleSystem(*self.nx, *blocks, n_blocks_00=M, n_blocks_11=M,
                               nullspace_0=[conv(n) for n in ns0],
                               nullspace_1=[conv(n) for n in ns1], CN=layout != "BE", **kw)


def same(name, S, form):
    return Case(name, S, form=form)


def uniform(w, nrows=129):
    w = min(w, nrows)
    return st.banded(nrows, w, seed=100 + w)


def sliced(slice_widths, seed, ragged=False, nrows=None):
    rw = st.slice_row_widths(slice_widths, nrows=nrows, seed=seed, ragged=ragged)
    return st.banded(len(rw), rw, seed=seed)


def cases():
    """The structure families; ``form`` = (R, uniform_w) every launch with blocks must report
    with default options and values shared between the time levels (None: not one form)."""
    out = []
    for w in range(1, 17):
        out.append(same(f"W{w}", uniform(w), (2, w)))
    # ragged: most slots in the unrolled widths, narrow on average -> four-wave switch
    out.append(same("switch", sliced(st.mixture({4: .15, 5: .15, 7: .2, 9: .3, 12: .1, 25: .1}, 24,
                                                seed=1), seed=1), (2, SWITCH)))
    # ... wide on average -> one wave per workgroup; every unrolled width, 24 and 38 (two
    # segments), and a generic width inside the switch
    out.append(same("switch_1wave", sliced(list(st.SWITCH_WIDTHS) + [40, 24, 38, 19, 24, 38],
                                           seed=2), (2, SWITCH_1WAVE)))
    # ... at most 7 wide -> the narrow switch (3..7 unrolled, 1 and 2 generic)
    out.append(same("switch_narrow", sliced([1, 2, 3, 4, 5, 6, 7, 7, 5, 3], seed=3),
                    (2, SWITCH_NARROW)))
    # ... mostly widths the switch does not unroll -> the slot loop
    out.append(same("slot_loop", sliced([25, 40, 25, 3, 40, 25, 11, 40], seed=4), (2, SLOT_LOOP)))
    # ragged rows inside slices (P2 / Q2-like): row-sorted storage
    out.append(same("sorted", sliced([19, 9, 38, 19, 9, 24, 15, 19, 9, 19], seed=5, ragged=True),
                    None))
    # near-uniform: padded to the fixed width just under the 3 % limit, not just over it
    out.append(same("pad_under", sliced(st.near_uniform(9, False), seed=6), (2, 9)))
    out.append(same("pad_over", sliced(st.near_uniform(9, True), seed=7), None))
    # rectangular couplings (Stokes-like shapes: 9 / 19 levels, 4 / 7 couplings)
    n0, n1 = 5 * 128 + 17, 256
    out.append(Case("rect", S0=sliced([9, 19, 19, 9, 19, 9], seed=8, nrows=n0),
                    S1=st.banded(n1, 7, seed=9),
                    C=st.banded(n0, st.slice_row_widths([4, 7, 4, 4, 7, 4], nrows=n0), seed=10,
                                ncols=n1),
                    D=st.banded(n1, 38, seed=11, ncols=n0)))
    return out


CASES = {c.name: c for c in cases()}


def forms_of(g):
    return g.apply_forms()


def int_vector(n, seed):
    return np.random.default_rng(seed).integers(-8, 9, n).astype(np.float64)


def check_form(case, g, share=True, rich=True):
    f = forms_of(g)
    assert len(f) == g.info()["apply_launches"] >= 1
    if case.form is not None:
        R, w = case.form
        live = [r for r in f if r["uniform_w"] != 0]
        assert live and all((r["R"], r["uniform_w"]) == (R, w) for r in live), (case.name, f)
        # groups need block rows of equal structure, masks included: the Dirichlet-only systems
        # have them (the interior rows of a variable); the mixed nullspaces leave too few
        if not rich:
            grouped = share and 1 <= w <= 8
            assert all((r["groups"] > 0) == grouped for r in live), (case.name, f)
    if case.name == "sorted":
        assert any(r["sorted"] for r in f) and all(r["uniform_w"] < 0 for r in f if r["sorted"])
    if case.name == "pad_over":
        assert all(r["uniform_w"] != 9 for r in f)
    return f


# ------------------------------------------------------------------------- integer-exact
@pytest.mark.parametrize("layout", ["BE", "CN", "CN_split"])
@pytest.mark.parametrize("name", list(CASES))
def test_integer_exact(name, layout):
    case = CASES[name]
    blocks = case.blocks(seed=1, integer=True)
    o = case.oracle(blocks, layout)
    x = int_vector(o.N, 3)
    ref = o.mult(x)             # exact: small integers and power-of-two means
    for share in (True, False):
        g = case.gpu(blocks, layout, share=share)
        check_form(case, g, share)
        y = g.mult(x)
        bad = np.flatnonzero(y != ref)
        assert bad.size == 0, (name, layout, share, bad[:10], y[bad[:5]], ref[bad[:5]])


@pytest.mark.parametrize("nrows", st.ROW_COUNTS)
@pytest.mark.parametrize("kind", ["W7", "W16", "W3_shared", "switch_1wave"])
def test_integer_exact_row_counts(kind, nrows):
    """Row counts around the slices: partial last slices, one row, one full slice."""
    if kind == "switch_1wave":
        # as many slices as the rows need, cycling through two-segment and one-segment widths
        sw = np.resize([24, 38, 19, 12], -(-nrows // 128))
        S = sliced(sw, seed=nrows, nrows=nrows) if nrows >= 38 else st.banded(nrows, nrows, 1)
        assert S.shape[0] == nrows
    else:
        S = uniform(int(kind[1:].split("_")[0]), nrows)
    case = same(f"{kind}_{nrows}", S, None)
    blocks = case.blocks(seed=2, integer=True)
    shared = kind.endswith("shared")
    o = case.oracle(blocks, "CN", rich=not shared)
    x = int_vector(o.N, 4)
    g = case.gpu(blocks, "CN", share=shared, rich=not shared)
    f = forms_of(g)
    w = min(S.shape[0], int(kind[1:].split("_")[0])) if kind[0] == "W" else None
    if w is not None:
        assert all(r["uniform_w"] == w for r in f)
        assert all((r["groups"] > 0) == shared for r in f)
    elif nrows > 128:
        assert all(r["uniform_w"] == SWITCH_1WAVE for r in f), f
    elif nrows >= 38:
        # one slice: a uniform width above 16, which no fixed-width kernel has -> the slot loop
        assert all(r["uniform_w"] == 24 for r in f), f
    assert np.array_equal(g.mult(x), o.mult(x))


# ---------------------------------------------------------------------- real data, per row
def exact_rows(case, blocks, layout, x):
    """Correctly rounded A x per row, (|A||x|)_i and k_i, for the Dirichlet-only system (the
    CN transforms sum two block rows: both rows' terms go into one fsum)."""
    nx0, nx1 = case.nx
    x0, x1 = x[:M * nx0].reshape(M, nx0), x[M * nx0:].reshape(M, nx1)
    ns0, ns1 = case.nullspaces(rich=False)
    xc0, xc1 = x0.copy(), x1.copy()
    for i in range(M):
        xc0[i, ns0[i]._nodes] = 0
        xc1[i, ns1[i]._nodes] = 0
    b00, b01, b10, b11 = blocks

    def terms(var, i):
        t = []
        for blk, xs in ((b00, xc0), (b01, xc1)) if var == 0 else ((b10, xc0), (b11, xc1)):
            t += [(A, xs[j]) for (r, j), A in blk.items() if r == i and A is not None]
        return t
    out = []
    for var, nx, ns, xv in ((0, nx0, ns0, x0), (1, nx1, ns1, x1)):
        for i in range(M):
            rows = [i]
            if layout == "CN":
                nb = i + 1 if var == 0 else i - 1         # T_1 on variable 0, T_2 on variable 1
                if 0 <= nb < M:
                    rows.append(nb)
            y, absum, k = st.rows_exact([t for r in rows for t in terms(var, r)], nx)
            y[ns[i]._nodes] = ALPHA * xv[i, ns[i]._nodes]
            absum[ns[i]._nodes] = 0
            out.append((y, absum, k))
    return [np.concatenate(a) for a in zip(*out)]


@pytest.mark.parametrize("layout", ["BE", "CN"])
@pytest.mark.parametrize("name", ["W1", "W5", "W8", "W9", "W16", "switch", "switch_1wave",
                                  "switch_narrow", "slot_loop", "sorted", "pad_under", "rect"])
def test_componentwise_real_data(name, layout):
    case = CASES[name]
    blocks = case.blocks(seed=3, integer=False)
    g = case.gpu(blocks, layout, rich=False)
    check_form(case, g, rich=False)
    x = np.random.default_rng(5).standard_normal(g.local_size) * np.exp(
        np.random.default_rng(6).uniform(-6, 6, g.local_size))
    y = g.mult(x)
    ref, absum, k = exact_rows(case, blocks, layout, x)
    worst = st.componentwise_ok(y, ref, absum, k)
    assert worst <= 1.0, (name, layout, worst)
    # masked rows are alpha x exactly
    masked = absum == 0
    assert np.array_equal(y[masked], ref[masked])


# --------------------------------------------------------------------- cross-form identity
TOGGLES = [{"sell_r": "1"}, {"sell_sort": "0"}, {"sell_sigma": "1"}, {"sell_sigma": "64"},
           {"ragged_switch": "0"}, {"ragged_xcd": "0"}, {"apply_xcd": "1"}, {"shared_rows": "0"}]


@pytest.mark.parametrize("layout", ["BE", "CN_split"])
@pytest.mark.parametrize("name", ["W2", "W7", "W8", "W11", "W16", "switch", "switch_1wave",
                                  "switch_narrow", "slot_loop", "sorted", "rect"])
def test_layout_options_are_bit_identical(name, layout):
    case = CASES[name]
    blocks = case.blocks(seed=4, integer=False)
    base = case.gpu(blocks, layout, rich=False)
    f0 = check_form(case, base, rich=False)
    x = np.random.default_rng(7).standard_normal(base.local_size)
    y0 = base.mult(x)
    for opt in TOGGLES:
        g = case.gpu(blocks, layout, options=opt, rich=False)
        f = forms_of(g)
        y = g.mult(x)
        assert np.array_equal(y, y0), (name, layout, opt, np.flatnonzero(y != y0)[:10])
        # ... and the option changed the form where it applies
        if "sell_r" in opt:
            assert all(r["R"] == 1 for r in f)
        if "shared_rows" in opt:
            assert all(r["groups"] == 0 for r in f)
        if "ragged_switch" in opt:
            assert all(r["uniform_w"] >= -1 for r in f)
        if opt == {"sell_sort": "0"}:
            assert not any(r["sorted"] for r in f)
        if "sell_sigma" in opt and any(r["sorted"] for r in f0):
            assert len(f) == len(f0)


# ------------------------------------------------------------------------ the whole table
def test_every_apply_form_is_reached():
    """Walk the dispatch table: every (R = 2) fixed width 1..16 unshared and 1..8 shared, the
    three switch shapes, the slot loop, row-sorted storage and R = 1 each ran for a case above
    -- and every unrolled switch width (with 24 and 38, the two-segment bodies) and a generic
    width sat in a slice of a switched launch."""
    reached = set()
    switch_slice_widths = set()
    for case in CASES.values():
        blocks = case.blocks(seed=5, integer=True)
        for share, opts in ((True, None), (False, None), (True, {"sell_r": "1"})):
            g = case.gpu(blocks, "BE", options=opts, share=share, rich=False)
            x = int_vector(g.local_size, 8)
            assert np.array_equal(g.mult(x), case.oracle(blocks, "BE", rich=False).mult(x)), \
                case.name
            for r in forms_of(g):
                w = r["uniform_w"]
                if r["R"] == 1:
                    reached.add(("R1",))
                elif r["groups"]:
                    reached.add(("shared", w))
                else:
                    reached.add(("fixed", w) if w > 0 else ("ragged", w))
                if r["sorted"]:
                    reached.add(("sorted",))
                if w in (SWITCH, SWITCH_1WAVE, SWITCH_NARROW):
                    for S in (case.S0, case.S1, case.C, case.D):
                        switch_slice_widths |= set(st.slice_widths(S).tolist())
    want = ({("fixed", w) for w in range(1, 17)} | {("shared", w) for w in range(1, 9)} |
            {("ragged", w) for w in (SWITCH, SWITCH_1WAVE, SWITCH_NARROW, SLOT_LOOP)} |
            {("R1",), ("sorted",)})
    assert not want - reached, sorted(want - reached)
    missing = set(st.SWITCH_WIDTHS + (1, 2, 3, 6) + (40,)) - switch_slice_widths
    assert not missing, sorted(missing)
