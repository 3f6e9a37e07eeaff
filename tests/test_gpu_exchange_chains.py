"""The local parts of a coarse exchange in the two-grid tile program (``pc_tile_sweep<...,
COARSE = true>``): coarse residual, owned products and prolongation read their indices and
operands in groups ahead of the add / fma chains, and lane 0's wave sum of the restriction and of
the products comes from register moves across lanes (run with -m gpu on an MI355X).

The chains themselves are those of ``tests/tile_level_ref.py``, so every case compares bit for bit
with it through ``kkt_debug_tile_levels`` (``test_gpu_tile_levels.run_hook_cases``).  What a case
is there for is a count -- terms per lane, rounds per thread, entries per list -- that decides
which groups are full, which are partly filled and where the general loops take over.  The
device's CU count sets the tiles, so each case reads its plan back and asserts that count:

  p1c10    P1 41^2, 10 coarse cells (121 functions), 64 threads: the coarse residual in two
           rounds with the second partly filled, tiles that own more rows of the inverse than
           they have waves, owned rows of 121 columns (lanes with 2 terms and with 1)
  p1c16    P1 65^2, 16 cells (289 functions), 64 and 256 threads: lanes with 5 and with 4 terms,
           5 and 2 rounds of the coarse residual
  p1r64 / p1r128   P1 160^2 and 192^2 with cells of 32 widths: restriction lists of more than 64
           and more than 128 entries (a lane with two and with three terms), n_t = 2
  p1_3d, p2v8      the existing shapes: rows of P with 8 entries, lists without rings,
           ``ew < n_coarse`` -- the general loops

and 20 applications in a row through ``kkt_pc_apply`` on the first shape against the plain
launches (the project's 1e-12 bar) and against themselves (bitwise).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import common
import test_gpu_tile_levels as lv
from test_gpu_coarse_polls import waves_system
from test_gpu_sweep_forms import per_block_err, problem

pytestmark = pytest.mark.gpu

NEW_SHAPES = {"p1c10": ("p1", 40, 10), "p1c16": ("p1", 64, 16),
              "p1r64": ("p1", 160, 5), "p1r128": ("p1", 192, 6)}
PLACEMENTS = [(2, 1), (1, 1), (0, 0)]    # (cache, rings)


@pytest.fixture
def shapes(monkeypatch):
    for name, spec in NEW_SHAPES.items():
        monkeypatch.setitem(lv.SHAPES, name, spec)
        monkeypatch.setitem(lv.WIDTH, name, 7)
        monkeypatch.setitem(lv.RINGS_BUILT, name, True)


def two_steps(monkeypatch):
    """``n_t`` = 2 for the settings made from here on (the large shapes; their names are used
    nowhere else, so the cached setting is theirs alone)."""
    monkeypatch.setattr(lv, "problem", lambda space, n, n_t=4, **kw: problem(space, n, n_t=2, **kw))


def counts(shape, plan):
    """What the exchange code meets on this plan: per coarse function the tiles that contribute a
    partial sum, the lengths of the restriction lists (own rows of a tile that touch a function),
    the entries per row of P, the rows of the inverse the first tile owns."""
    _, P, mask, _ = lv.setting(shape)
    P = sp.csr_matrix(P)
    pat = sp.csr_matrix((np.ones(len(P.data)), P.indices, P.indptr), shape=P.shape)
    per_tile = np.array([np.asarray(pat[own].sum(axis=0)).ravel() for own in plan["own"]])
    contributing = (per_tile > 0).sum(axis=0)
    lists = per_tile[per_tile > 0]
    p_rows = np.diff(P.indptr)[~mask]
    owned = -(-plan["n_coarse"] // plan["tiles"])
    return contributing, lists, p_rows, owned


def run(monkeypatch, shape, waves, depth, cache, rings, **kw):
    """``run_hook_cases`` on a handle with 64 * ``waves`` threads (0: the plan's own), then the
    plan and its counts."""
    base, made = (waves_system(waves) if waves else lv.tile_system), []

    def system(*a, **k):
        made.append(base(*a, **k))
        return made[-1]
    monkeypatch.setattr(lv, "tile_system", system)
    lv.run_hook_cases(shape, depth, cache, rings, **kw)
    g, = made
    plan = g.debug_tile_levels()
    assert plan["depth"] == depth and (not waves or plan["threads"] == 64 * waves)
    contributing, lists, p_rows, owned = counts(shape, plan)
    print(f"{shape} waves {waves} depth {depth} cache {cache} rings {rings}: {plan['tiles']} tiles x "
          f"{plan['threads']} threads, {plan['n_coarse']} functions, ew {plan['ew']}, tiles per "
          f"function {sorted(set(contributing.tolist()))}, longest list {lists.max()}, entries per "
          f"row of P {sorted(set(p_rows.tolist()))}, rows of the inverse per tile {owned}")
    return plan, contributing, lists, p_rows, owned


@pytest.mark.parametrize("cache,rings", PLACEMENTS)
@pytest.mark.parametrize("depth", [1, 3])
def test_two_rounds_short_rows_more_owned_rows_than_waves(monkeypatch, shapes, depth, cache, rings):
    plan, contributing, lists, p_rows, owned = run(monkeypatch, "p1c10", 1, depth, cache, rings,
                                                   its_list=(4, 5), cycles_list=(2, 3))
    T, nc = plan["threads"], plan["n_coarse"]
    assert T == 64 and nc == 121 and T < nc < 2 * T      # two rounds, the second partly filled
    assert owned > T // 64                                # more owned rows than waves
    assert plan["ew"] == nc and 64 < nc < 128             # lanes with 2 terms and with 1
    # in one plan: functions with 1, 2, 3 and 4 contributing tiles (and none, and more than the
    # unrolled four), rows of P with 1, 2 and 4 entries
    assert set(contributing.tolist()) >= {1, 2, 3, 4}, sorted(set(contributing.tolist()))
    assert set(p_rows.tolist()) >= {1, 2, 4}, sorted(set(p_rows.tolist()))


@pytest.mark.parametrize("waves", [1, 4])
def test_read_ahead_group_with_a_tail(monkeypatch, shapes, waves):
    plan, contributing, lists, p_rows, owned = run(monkeypatch, "p1c16", waves, 2, 2, 1,
                                                   its_list=(4,), cycles_list=(2,))
    T, nc = plan["threads"], plan["n_coarse"]
    assert nc == 289 and plan["ew"] == nc                 # lanes with 5 terms and with 4
    assert -(-nc // T) == (5 if waves == 1 else 2)        # rounds of the coarse residual
    assert set(p_rows.tolist()) >= {1, 2, 4}


@pytest.mark.parametrize("shape,longer_than", [("p1r64", 64), ("p1r128", 128)])
def test_long_restriction_lists(monkeypatch, shapes, shape, longer_than):
    two_steps(monkeypatch)
    plan, contributing, lists, p_rows, owned = run(monkeypatch, shape, 0, 2, 2, 1,
                                                   its_list=(4,), cycles_list=(2,))
    assert lists.max() > longer_than, lists.max()


@pytest.mark.parametrize("shape,cache,rings", [("p1_3d", 2, 0), ("p2v8", 2, 1)])
def test_general_loops(monkeypatch, shape, cache, rings):
    plan, contributing, lists, p_rows, owned = run(monkeypatch, shape, 0, 2, cache, rings,
                                                   its_list=(4,), cycles_list=(2,))
    if shape == "p1_3d":
        assert p_rows.max() == 8 and plan["rings"] == 0   # long rows of P, lists without rings
    else:
        assert plan["ew"] < plan["n_coarse"]


def test_twenty_applications_equal_the_plain_launches(shapes):
    """Twenty applications in a row (buffer alternation and tags across launches) on the two
    inputs the project's 1e-12 bar against the plain launches is stated for
    (``test_gpu_tile_levels.bars``: random, and sin sin, on which the correction is a large part
    of the result), taken in turn; every application equals bit for bit the earlier ones of its
    input.  (Not each result as the next input: that is a power iteration, whose vectors the bar
    does not cover -- the tile form and the plain launches, which associate the restriction sums
    differently, were 1.07e-12 apart at the twelfth, with the parent's kernel as with this one.)"""
    p, P, mask, smooth = lv.setting("p1c10")
    one = waves_system(1)(p, 3)
    plain = common.gpu_system(p, options={"persistent": "0"})
    pcs = [common.gpu_pc(p, lv.MASS, lv.SCHUR_B, coarse=(P, 2)) for _ in range(2)]
    m = p["m"]
    xs = [common.rng_vector(one.local_size),
          np.tile(np.where(mask, 0.0, smooth), 2 * m) * np.repeat(1.0 + 0.1 * np.arange(2 * m), len(mask))]
    first = [None, None]
    for k in range(20):
        y = one.pc_apply(xs[k % 2], pcs[0])
        if first[k % 2] is None:
            first[k % 2] = y
            e = per_block_err(p, y, plain.pc_apply(xs[k % 2], pcs[1]))
            print(f"input {k % 2}: tile against plain {e:.2e}")
            assert e < 1e-12, (k, e)
        assert np.array_equal(y, first[k % 2]), k                     # run to run
    assert one.info()["sweep_form"] == 3 and one.info()["program_fallbacks"] == 0
    assert plain.info()["sweep_form"] == 0
    assert one.debug_tile_levels()["threads"] == 64
