"""The pressure stage of ``StokesPC::run()`` -- everything after the nested velocity solve --
against an extended-precision reference, without the nested GMRES in the comparison.

Two facts about ``kkt_pc_apply`` on the outer handle separate the stage from the solve:

1. with a zero velocity right-hand side the nested solve leaves with ``u_0 = 0`` exactly (first
   residual norm 0), so the pressure output is the stage applied to ``-s2 b_1``;
2. with any right-hand side the velocity half of the output is the nested solve's ``u_0`` bit for
   bit on interior dofs (the post-correction only overwrites Dirichlet dofs, which are exactly 0
   inside), so it is read back, its boundary dofs are zeroed and it goes to the references as
   data: the ``B`` product sees a real ``u_0``.

References and cases: ``tests/stokes_stage_ref.py``.  A case passes when, on the pressure half,
``rel_err(gpu, extended) <= 8 max(d_case, eps its_total)`` with ``d_case`` the distance of the
float64 oracle stage from the extended one for the same ``u_0``, computed here at test time.

Measured on an MI355X (gfx950): largest ``d_case`` 2.0e-15 (backward Euler, 8-step ``K_p`` chain,
random input; the time-sharded run on two ranks the same), largest ratio
``rel_err(gpu, extended) / max(d_case, eps its_total)`` 0.90 (4-step ``K_p`` chain) against the
allowed 8; every other case is below 0.75, the 30-step chains below 0.15.  ``shared_rows``,
``no_graph``, ``pc_xcd`` and ``sell_r`` are all bit-identical.  ``shared_rows`` = "0" used to be
ignored by these chains (the four-blocks-per-thread form ran regardless); it is honoured now, so
the one-block-per-thread form of every step is what that comparison runs.
"""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import common
import stokes_stage_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def check(c, x, y, what):
    """One GPU output against the references for the ``u_0`` it carries."""
    p = ref.problem(c)
    u0 = ref.interior_u0(p, y)
    px, _, d = ref.references(c, x, u0)
    e = float(common.rel_err(ref.split(p, y)[1], px))
    ratio = e / max(d, ref.EPS * ref.its_total(c))
    print(f"stage {ref.case_id(c)} {what}: d_case {d:.2e} gpu {e:.2e} ratio {ratio:.2f}")
    assert e <= ref.bound(d, c), (ref.case_id(c), what, e, d, ratio)
    # the Dirichlet dofs of the velocity half are the post-correction's alpha b
    bv = p["th"].boundary_v
    assert np.array_equal(ref.split(p, y)[0][:, bv], ref.split(p, x)[0][:, bv])
    return u0


@pytest.mark.parametrize("c", ref.CASES, ids=ref.case_id)
def test_stage_matches_extended_reference(c):
    outer, gpc = ref.stage_gpu(c)
    x1, x2 = ref.inputs(c)
    u0 = check(c, x1, outer.pc_apply(x1, gpc), "zero_b0")
    assert not u0.any()                      # fact 1: the nested solve returned exactly 0
    u0 = check(c, x2, outer.pc_apply(x2, gpc), "random")
    assert np.all(np.abs(u0).max(axis=1) > 0)   # a real u_0 in every block


REPLAY = [ref.case(4, 3, False), ref.case(8, 3, True), ref.case(8, 3, False, two_grid=(2, 4))]


@pytest.mark.parametrize("c", REPLAY, ids=ref.case_id)
def test_graph_replay_reads_the_current_input(c):
    """Both chains are captured graphs here (8 or more steps).  The second application on one
    handle replays them and must match the reference of the SECOND input; the first input again
    gives the first result bit for bit."""
    outer, gpc = ref.stage_gpu(c)
    xa, xb = ref.inputs(c, seed=1)[1], ref.inputs(c, seed=2)[1]
    ya = outer.pc_apply(xa, gpc)
    yb = outer.pc_apply(xb, gpc)
    check(c, xa, ya, "first")
    check(c, xb, yb, "replayed")
    assert common.rel_err(yb, ya) > 0.1      # (the two inputs are unrelated)
    assert np.array_equal(outer.pc_apply(xa, gpc), ya)
    assert np.array_equal(outer.pc_apply(xb, gpc), yb)


OPTION_CASES = [ref.case(8, 3, False), ref.case(7, 2, True), ref.case(8, 3, True, two_grid=(2, 4))]
# ("sell_r" = "1" is bit-identical for the same kernels of the Schur preconditioner,
# tests/test_gpu_sweep_forms.py::test_plain_step_options_are_bit_identical: so it is here)
OPTIONS = [{"no_graph": "1"}, {"shared_rows": "0"}, {"pc_xcd": "0"}, {"sell_r": "1"}]


@pytest.mark.parametrize("c", OPTION_CASES, ids=ref.case_id)
def test_execution_options_are_bit_identical(c):
    """Plain launches for the captured graphs, one block per thread for four, dispatch order for
    the XCD order, SELL-64 for SELL-128: the same fma chains, the full output bit for bit."""
    outer, gpc = ref.stage_gpu(c)
    xs = ref.inputs(c)
    base = [outer.pc_apply(x, gpc) for x in xs]
    for opt in OPTIONS:
        o, g = ref.stage_gpu(c, options=opt)
        for x, y0, kind in zip(xs, base, ("zero_b0", "random")):
            y = o.pc_apply(x, g)
            assert np.array_equal(y, y0), (ref.case_id(c), opt, kind,
                                           np.flatnonzero(y != y0)[:8], common.rel_err(y, y0))


# ------------------------------------------------------------------------------ time shards
def launch(world, CN, target="run_rank_stokes_pressure_stage"):
    """As ``tests/test_gpu_sharded.py::launch``: one process per rank, duplex pipes between every
    pair, results through a queue whose ``get`` has a timeout."""
    ctx = mp.get_context("spawn")
    conns = [[None] * world for _ in range(world)]
    for a in range(world):
        for b in range(a + 1, world):
            ca, cb = ctx.Pipe(duplex=True)
            conns[a][b], conns[b][a] = ca, cb
    q = ctx.Queue()
    sys.path.insert(0, HERE)
    import sharded_worker
    procs = [ctx.Process(target=getattr(sharded_worker, target), args=(r, world, conns[r], q, CN))
             for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=240)
            assert status == "ok", f"rank {rank}: {payload}"
            res[rank] = payload
    finally:
        for pr in procs:
            pr.join(timeout=10)
            if pr.is_alive():
                pr.kill()
    return res


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_time_sharded_stage(world, CN):
    """Worlds 2 and 3 with one rank holding a single level (the Crank-Nicolson scans take their
    halo in and pass their only block on): every rank's shard of both input kinds against the
    one-rank extended reference under the same criterion.  With the zero velocity right-hand side
    every rank equals the one-rank GPU run on its rows bit for bit.  With the random one it
    cannot: the nested GMRES in front of the stage sums its inner products rank by rank, its u_0
    differs from the one-rank u_0 in the last bits and backward Euler amplifies that (1e-11 in
    the output) -- so the reference takes the sharded run's own u_0, gathered from the ranks,
    and the stage is held to the same bound."""
    res = launch(world, CN)
    assert sorted(res) == list(range(world))
    assert min(res[r]["levels"] for r in res) == 1
    for r in range(world):
        d = res[r]
        for kind in ("zero_b0", "random"):
            k = d[kind]
            print(f"stage sharded world {world} {'CN' if CN else 'BE'} rank {r} {kind}: "
                  f"d_case {k['d']:.2e} gpu {k['e']:.2e} ratio {k['ratio']:.2f} "
                  f"one-rank {k['e_one']:.1e}")
            assert k["e"] <= k["bound"], (r, kind, k)
            assert k["bitwise"] or kind == "random", (r, kind, k)
            assert k["e_one"] < (1e-7 if CN else 1e-4), (r, kind, k)   # tests/test_gpu_stokes.py
        assert d["u0_zero"], d
