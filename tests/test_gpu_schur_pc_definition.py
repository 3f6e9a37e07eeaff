"""The block Schur preconditioner's application on the device against its definition in extended
precision (run with -m gpu on an MI355X).

Every kernel under the preconditioner is pinned one launch at a time, and every sweep form equals
plain launches bit for bit; what the launches add up to was held only to the float64 oracle, a
restatement by the same hand.  Here ``pc_apply`` is compared with ``tests/schur_pc_ref.py``: every
sub-solve as the Chebyshev residual polynomial of ``D^-1 A`` (no recurrence in the iterates, no
coefficient sequence), the application as a product of block matrices (no substitution loop).
Cases: ``tests/schur_pc_cases.py``; references and the oracle's own distance ``d_case`` from them:
``tests/golden/schur_pc_definition.npz``, checked on the host by ``tests/test_schur_pc_ref.py``.

For every case, on a fresh handle with default options and on one with ``persistent=0``:

* per output block ``|got_k - ref_k|_inf / |ref_k|_inf <= 8 max(d_case, u steps)`` with
  ``u = 1.1e-16`` and ``steps`` the dependent row steps on the longest path
  (``schur_pc_cases.steps``) -- the bar of the pressure-stage test, set by the reference and the
  oracle's distance from it, never by the device;
* ``pc_forms()``: the first handle ran sweep programs or tile launches (two-grid cases: the tile
  form with coarse corrections), the second plain launches; three ``short`` cases have no run the
  library fuses, there both handles run plain launches and the test asserts that too;
* boundary rows of the output are the input's, bit for bit;
* the two handles agree bit for bit, except where a two-grid level ran in the tile form (another
  summation order: both are held to the reference);
* impulse inputs: every output block that is exactly zero in the reference is ``+0.0``;
* estimated intervals (``ChebSpec(-1, 0, 0)``): the reference runs every sub-solve with the
  interval and degree that ``pc_solves()`` reports for it, so every level is pinned to its record.

Measured on an MI355X (gfx950): largest ``distance / max(d_case, u steps)`` per family, allowed 8:
stationary 0.19, BE 0.52, CN 1.66, ellipse 1.30, two-grid 1.74 in the tile form and in plain
launches, estimated intervals 1.03.  On these sizes the tile program has one tile and its two-grid
levels came out bit-equal to plain launches; the test does not ask for that.  The file takes 4 s.
"""
import numpy as np
import pytest

import schur_pc_cases as sc
import schur_pc_ref as ref

pytestmark = pytest.mark.gpu

PROGRAM, TILE_STEP, TILE_CHEB = 4, 5, 6          # pc_forms()["form"]
FUSED = (PROGRAM, TILE_STEP, TILE_CHEB)


def apply_both(c, xs):
    """Default options and plain launches, each on a fresh handle: outputs, forms and records."""
    g, pc = sc.gpu_handle(c)
    gp, pcp = sc.gpu_handle(c, options={"persistent": "0"})
    ys = {name: (g.pc_apply(x, pc), gp.pc_apply(x, pcp)) for name, x in xs.items()}
    for h in (g, gp):
        assert h.info()["program_fallbacks"] == 0, h.info()
    forms, plain_forms = g.pc_forms(), gp.pc_forms()
    assert gp.info()["sweep_form"] == 0 and not any(f["form"] in FUSED for f in plain_forms)
    # (``short`` cases: the library has no sweep program for them, both handles run plain launches)
    assert any(f["form"] in FUSED for f in forms) != c["short"], (sc.case_id(c), forms)
    tiled_two_grid = any(f["form"] == TILE_STEP and f["variant"] & 2 for f in forms)
    assert tiled_two_grid == bool(c["coarse"] and not c["short"]), (sc.case_id(c), forms)
    assert g.pc_solves() == gp.pc_solves()
    return ys, forms, tiled_two_grid, g.pc_solves()


def check(c, name, x, y, gold, bar, what):
    d = sc.distance(c, y, *gold)
    print(f"definition {sc.case_id(c)} [{sc.family(c)}] {name} {what}: distance {d:.2e} "
          f"bar {bar:.2e} ratio {d / bar * 8:.2f} of 8")
    assert d <= bar, (sc.case_id(c), name, what, d, bar)
    nodes = sc.problem(c)["nodes"]
    assert np.array_equal(sc.split(c, y)[:, :, nodes], sc.split(c, x)[:, :, nodes]), (name, what)
    assert sc.zero_blocks_are_plus_zero(c, y, *gold), (sc.case_id(c), name, what)


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_application_matches_its_definition(c):
    xs = sc.inputs(c)
    ys, forms, tiled_two_grid, solves = apply_both(c, xs)
    assert all(r["estimate"] == "given" and r["its"] == c["schur"] for r in solves), solves
    for name, x in xs.items():
        *gold, d_case = sc.golden_reference(c, name)
        bar = 8.0 * max(d_case, sc.U * sc.steps(c))
        y, yp = ys[name]
        check(c, name, x, y, gold, bar, "default")
        check(c, name, x, yp, gold, bar, "plain")
        if not tiled_two_grid:
            assert np.array_equal(y, yp), (sc.case_id(c), name, np.flatnonzero(y != yp)[:8])
        else:
            print(f"definition {sc.case_id(c)} {name}: two-grid levels in the tile form, "
                  f"bit-equal to plain launches: {np.array_equal(y, yp)}")


@pytest.mark.parametrize("c", sc.ESTIMATED, ids=sc.case_id)
def test_estimated_intervals_are_what_the_records_report(c):
    """No oracle here (it takes one interval for all levels): ``d_case`` is 0 and the bar
    ``8 u steps`` with the degree the records report."""
    xs = {"random": sc.inputs(c)["random"]}
    ys, forms, _, solves = apply_both(c, xs)
    m = sc.problem(c)["m"]
    assert len(solves) == 2 * m and all(r["estimate"] in ("lanczos", "shared") for r in solves)
    its = {r["its"] for r in solves}
    assert len(its) == 1 and min(its) >= 4, its
    if c["disc"] == "conv":
        assert all(r["eimag"] > 0.0 for r in solves)
    if not c["td"] and c["kind"] == "BE":
        assert len({(r["emin"], r["emax"]) for r in solves}) >= 3     # first, middle, last level
    x = xs["random"]
    u0, u1 = sc.reference(c, records=solves).apply(*sc.split(c, x))
    gold = (*ref.to_pairs(u0), *ref.to_pairs(u1))
    bar = 8.0 * sc.U * sc.steps(c, its=its.pop())
    y, yp = ys["random"]
    check(c, "random", x, y, gold, bar, "default")
    check(c, "random", x, yp, gold, bar, "plain")
    assert np.array_equal(y, yp)
    # the reference is sensitive to the records: the first level's interval on every level
    # moves it by far more than the bar
    first = dict(solves[0])
    wrong = [dict(r, emin=first["emin"], emax=first["emax"]) for r in solves]
    if wrong != solves:
        v0, v1 = sc.reference(c, records=wrong).apply(*sc.split(c, x))
        assert sc.distance(c, y, *ref.to_pairs(v0), *ref.to_pairs(v1)) > 100 * bar
