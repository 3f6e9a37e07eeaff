"""The polls of the two-grid tile program (``pc_tile_sweep<..., COARSE = true>``) in the slot
patterns that the small default plans never reach (run with -m gpu on an MI355X).

Every poll of a round -- the partial sums of the coarse all-gather, four slots per thread and
round, and the ring entries of a hand-off -- is issued before the round's one wait; a slot whose
granule has arrived is not requested again, and an arrived granule goes to LDS at once.  Which
slots of a thread are live depends on the workgroup size, so the option ``tile_waves`` sets it:

  tile_waves 1   64 threads: two rounds of the all-gather, the second one partly filled (threads
                 with 4, 2 and 1 live slots); at depth 3 -- only there, depth 1 has fewer ring
                 rows than threads -- both hand-off slots of a thread are live, and two row slots
  tile_waves 2   128 threads: one round, threads with 3 and with 2 live slots
  tile_waves 4   256 threads: threads with 2 and with 1 live slot
  tile_waves 16  the 1 024-thread variant itself: most threads without any slot
  tile_waves 12  on the P2 velocity shape: the 768-thread variant, rows of the coarse inverse
                 shorter than n_coarse

The device's CU count sets the tiles, so each case reads its plan back and asserts the pattern it
is there for.  Results are compared bit for bit with ``tests/tile_level_ref.py`` through
``kkt_debug_tile_levels`` (``test_gpu_tile_levels.run_hook_cases``: 4 and 5 sweeps, 2 and 3 cycles,
two coarse inverses, two right-hand sides, chained and solo levels), and 20 applications in a row
through ``kkt_pc_apply`` with the default plan's (buffer alternation and tags across launches).
Shape: P1 41^2 with 5 coarse cells (36 coarse functions), n_t = 4; references are computed once
and shared by the cases (they depend on the tiles, not on the threads).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import common
import test_gpu_tile_levels as lv

pytestmark = pytest.mark.gpu

CSL = 4                                  # slots per thread and round of the all-gather
PLACEMENTS = [(2, 1), (1, 1), (0, 0)]    # (cache, rings): cache 2 / 1 with rings, cache 0


def waves_system(waves):
    """``test_gpu_tile_levels.tile_system`` with the workgroup size set."""
    def system(p, depth=None, cache="auto", rings="1", rows="block", keep=False):
        opts = {"prog_mode": "tile", "tile_coarse_cache": str(cache), "coarse_rings": str(rings),
                "tile_coarse_rows": rows, "coarse_keep": "1" if keep else "0",
                "tile_waves": str(waves)}
        if depth:
            opts["tile_depth"] = str(depth)
        system.made.append(common.gpu_system(p, options=opts))
        return system.made[-1]
    system.made = []
    return system


def slot_pattern(shape, plan, depth):
    """What the poll code meets on this plan: live slots per thread in every round of the
    all-gather (a row per round), ring rows of the largest ring."""
    p, P, mask, _ = lv.setting(shape)
    T = plan["threads"]
    Pr = sp.csr_matrix(P)
    # a tile publishes one partial sum per coarse function its own rows touch
    nslots = sum(len(np.unique(Pr[own].indices)) for own in plan["own"])
    tid = np.arange(T)
    live = np.array([[np.sum(base + np.arange(CSL) * T + t < nslots) for t in tid]
                     for base in range(0, nslots, CSL * T)])
    # rings: rows within graph distance `depth` of the own rows, outside the mask
    A = lv.inputs_of(shape)["A"][0]
    G = sp.csr_matrix(abs(A) + abs(A).T)
    ring = 0
    for own in plan["own"]:
        cur = np.zeros(A.shape[0], bool)
        cur[own] = True
        for _ in range(depth):
            cur[G[np.flatnonzero(cur)].indices] = True
        cur[own] = False
        ring = max(ring, int((cur & ~mask).sum()))
        assert len(own) + int((cur & ~mask).sum()) < plan["nk_pad"], "the plan holds these rows"
    return nslots, live, ring


def run(monkeypatch, shape, waves, depth, cache, rings, **kw):
    system = waves_system(waves)
    monkeypatch.setattr(lv, "tile_system", system)
    lv.run_hook_cases(shape, depth, cache, rings, **kw)
    g, = system.made
    plan = g.debug_tile_levels()
    assert plan["threads"] == 64 * waves and plan["depth"] == depth
    nslots, live, ring = slot_pattern(shape, plan, depth)
    print(f"{shape} waves {waves} depth {depth}: {plan['tiles']} tiles x {plan['threads']} threads, "
          f"{plan['row_slots']} row slots, {nslots} slots in {len(live)} rounds, live per thread "
          f"{[sorted(set(r)) for r in live.tolist()]}, largest ring {ring}")
    return plan, nslots, live, ring


@pytest.mark.parametrize("cache,rings", PLACEMENTS)
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("waves", [1, 2, 4, 16])
def test_slot_patterns_equal_reference(monkeypatch, waves, depth, cache, rings):
    plan, nslots, live, ring = run(monkeypatch, "p1", waves, depth, cache, rings,
                                   its_list=(4, 5), cycles_list=(2, 3))
    T = plan["threads"]
    if waves == 1:
        # several rounds, the last one partly filled: full threads, and threads with fewer slots
        assert len(live) >= 2 and set(live[0]) == {CSL}
        assert len(set(live[-1])) >= 2 and live[-1].max() < CSL and live[-1].min() >= 1
        if depth == 3:
            assert ring > T and plan["row_slots"] >= 2       # both hand-off slots of a thread live
    elif waves == 2:
        assert len(live) == 1 and set(live[0]) == {2, 3}
    elif waves == 4:
        assert len(live) == 1 and set(live[0]) == {1, 2}
    else:
        assert len(live) == 1 and np.sum(live[0] == 0) > T // 2 and live[0].max() == 1
    if waves > 1:
        assert ring < T                                       # the second hand-off slot is dead


def test_live_slot_counts_are_all_met():
    """Between them the plans of ``tile_waves`` 1 and 2 have threads with 1, 2, 3 and 4 live slots
    (plans only: the launches are the cases above)."""
    p, P, _, _ = lv.setting("p1")
    met = set()
    for waves in (1, 2):
        g = waves_system(waves)(p, 3, 2, 1)
        g.pc_apply(common.rng_vector(g.local_size),
                   common.gpu_pc(p, lv.MASS, (lv.PC_ITS, 0.07, 2.1), coarse=(P, 1)))
        plan = g.debug_tile_levels()
        assert plan["threads"] == 64 * waves
        met |= set(slot_pattern("p1", plan, 3)[1].ravel().tolist())
    assert met >= {1, 2, 3, 4}, met


def test_768_thread_variant_with_short_rows(monkeypatch):
    plan, nslots, live, ring = run(monkeypatch, "p2v8", 12, 2, 2, 1,
                                   its_list=(4, 5), cycles_list=(2, 3))
    assert plan["threads"] == 768 and plan["W"] == 19 and plan["row_slots"] == 1
    assert 64 <= plan["ew"] < plan["n_coarse"]
    assert len(live) == 1 and live[0].min() == 0


def test_twenty_applications_equal_the_default_plan():
    p, P, _, _ = lv.setting("p1")
    one = waves_system(1)(p, 3)
    default = lv.tile_system(p)
    pcs = [common.gpu_pc(p, lv.MASS, lv.SCHUR_B, coarse=(P, 2)) for _ in range(2)]
    x = common.rng_vector(one.local_size)
    for k in range(20):
        y, y0 = one.pc_apply(x, pcs[0]), default.pc_apply(x, pcs[1])
        assert np.array_equal(y, y0), (k, common.rel_err(y, y0))
        # the next input: this result, brought back to the size of the first
        x = y * (np.linalg.norm(x) / np.linalg.norm(y))
    for g in (one, default):
        assert g.info()["sweep_form"] == 3 and g.info()["program_fallbacks"] == 0
    assert one.debug_tile_levels()["threads"] == 64
    assert default.debug_tile_levels()["threads"] != 64
