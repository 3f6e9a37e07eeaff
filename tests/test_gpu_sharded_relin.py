"""Device re-linearisation on time-sharded solvers (``GpuLinearSolver(comm=..., relinearise="device")``,
DESIGN.md section 6.6): every rank keeps, assembles, evaluates and updates its own levels of the
Picard iterate in HBM.  2, 3 and 5 ranks (processes) share GPU 0 over the host-staged pipe
transport; with six unknown blocks they own 3, 2 and 2-or-1 of them -- a one-block shard has
both halo levels next to its only row.  Each rank compares itself with a one-rank plan in its own
process (tests/sharded_relin_worker.py); one launch per (world, scheme) serves the tests below."""
import multiprocessing as mp
import os
import queue
import sys

import pytest

from control_amd.dist import shard_range

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
M = 6                       # unknown blocks: n_t = 6 (BE), n_t = 7 (CN)
LIMIT = 240                 # seconds for all ranks of one launch


def launch(world, CN, target):
    """Spawn the ranks, collect one result each.  The first error or the time limit ends every
    rank (the others would wait in a pipe for the one that raised); nothing starts afterwards."""
    assert world <= 5
    ctx = mp.get_context("spawn")
    conns = [[None] * world for _ in range(world)]
    for a in range(world):
        for b in range(a + 1, world):
            conns[a][b], conns[b][a] = ctx.Pipe(duplex=True)
    q = ctx.Queue()
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import sharded_relin_worker
    procs = [ctx.Process(target=getattr(sharded_relin_worker, target),
                         args=(r, world, conns[r], CN, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res, failure = {}, None
    try:
        while len(res) < world and failure is None:
            try:
                rank, status, payload = q.get(timeout=LIMIT)
            except queue.Empty:
                failure = f"no result within {LIMIT} s (ranks done: {sorted(res)})"
                break
            if status == "ok":
                res[rank] = payload
            else:
                failure = f"rank {rank}: {payload}"
    finally:
        if failure is not None:
            for pr in procs:
                if pr.is_alive():
                    pr.kill()
        for pr in procs:
            pr.join(timeout=10)
            if pr.is_alive():
                pr.kill()
                pr.join()
    assert failure is None, failure
    return res


_cache = {}


def results(world, CN, target="run_rank_kernels"):
    key = (world, CN, target)
    if key not in _cache:
        try:
            _cache[key] = launch(world, CN, target)
        except BaseException as e:          # a failed launch is not repeated by the next test
            _cache[key] = e
    if isinstance(_cache[key], BaseException):
        raise _cache[key]
    return _cache[key]


def check(d, *keys):
    """Every flag of a rank's result holds (the message names those that do not)."""
    assert all(d[k] is True for k in keys), {k: d[k] for k in keys if d[k] is not True}


CASES = [(w, cn) for cn in (False, True) for w in (2, 3, 5)]
case = pytest.mark.parametrize("world,CN", CASES)


@case
def test_windows(world, CN):
    """``kkt_picard_window``: BE holds v [lo-1, hi), zeta [lo, hi], D [lo, hi) -- without level
    lo-1 on rank 0 and level hi on the last rank; CN holds [lo, hi] of all three, v_0 on rank 0
    and the zero level zeta_{n_t-1} on the last rank inside them."""
    res = results(world, CN)
    n_t = M + 1 if CN else M
    sizes = set()
    for r in range(world):
        d = res[r]
        lo, hi = shard_range(M, r, world)
        assert (d["lo"], d["hi"]) == (lo, hi)
        sizes.add(hi - lo)
        w = d["window"]
        assert w["blocks"] == (lo, hi)
        if CN:
            assert w["v"] == w["zeta"] == w["D"] == (lo, hi + 1), w
        else:
            assert w["v"] == (lo - 1 if r > 0 else 0, hi), w
            assert w["zeta"] == (lo, hi + 1 if r < world - 1 else hi), w
            assert w["D"] == (lo, hi), w
        assert d["window_one"] == {"v": (0, n_t), "zeta": (0, n_t), "D": (0, n_t), "blocks": (0, M)}
    assert res[0]["window"]["v"][0] == 0 and res[world - 1]["window"]["zeta"][1] == n_t
    assert sizes == {2: {3}, 3: {2}, 5: {1, 2}}[world]


@case
def test_assembly_is_rank_independent(world, CN):
    """Element matrices and D of every window level equal the one-rank plan's bit for bit -- CN's
    D_lo included, built from the halo v, which the rank's own host had as NaN."""
    res = results(world, CN)
    for r in range(world):
        d = res[r]
        check(d, "halo_poisoned", "halo_travelled", "asm_Ev", "asm_Ep", "asm_D2", "asm_Dp")


@case
def test_residual_and_right_hand_side_rows(world, CN):
    """The rank's rows of all four families equal the one-rank rows bit for bit (CN: with the
    neighbours' boundary rows in the time transforms); one norm on every rank.  Both norms are
    square roots of sums of the same N non-negative squares in different orders: each carries a
    relative error below (N - 1) u / 2, u = 2^-53, so they differ by less than N u."""
    res = results(world, CN)
    for rhs in (0, 1):
        for r in range(world):
            d = res[r]
            check(d, f"res{rhs}", f"res{rhs}_nonzero")
            assert d[f"norm{rhs}"] == res[0][f"norm{rhs}"]
            bound = d["n_entries"] * 2.0 ** -53 * d[f"norm{rhs}_one"]
            assert abs(d[f"norm{rhs}"] - d[f"norm{rhs}_one"]) <= bound, (
                d[f"norm{rhs}"], d[f"norm{rhs}_one"], bound)
    assert res[0]["norm0"] == res[0]["norm1"]          # the norm is the residual's in both modes


@case
def test_composition(world, CN):
    """Every owned linearised block of the three sharded handles equals the one-rank handle's;
    a recipe for another rank's row is an argument error that names the block."""
    res = results(world, CN)
    total = 0
    for r in range(world):
        d = res[r]
        check(d, "blocks_equal")
        assert d["n_blocks"] > 0
        total += d["n_blocks"]
        code, msg = d["foreign"]
        assert code == -1 and "block (" in msg and "not owned" in msg, d["foreign"]
    assert total == 3 * (2 * M if not CN else 4 * M - 2)      # every recipe on exactly one rank


@case
def test_update(world, CN):
    """A dyadic update moves the owned levels by exactly its blocks and is zeroed; zeta is zero
    on the Dirichlet dofs of the whole window; the halo slots change with the next exchange; the
    gathered iterate equals the one-rank plan's."""
    res = results(world, CN)
    for r in range(world):
        d = res[r]
        check(d, "update_owned", "update_changed", "u_zeroed", "zeta_bc_zero", "halo_stale",
              "halo_updated", "state_gathered")
        assert d["null_state"] == "ValueError", d["null_state"]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_device_loop_matches_one_rank(world, CN):
    """The loop with the iterate in HBM on a time shard against the same loop on one rank, at the
    bars of test_gpu_sharded.py's host-sharded loop (the sharded nested GMRES sums its inner
    products rank by rank); no block values cross from the host after the first build."""
    res = results(world, CN, "run_rank_loop")
    for r in range(world):
        d = res[r]
        print(world, CN, r, {k: d[k] for k in ("n", "n_ref", "e_norms", "e_v", "e_p", "its", "its_ref")})
        assert d["converged"] and d["n"] == d["n_ref"], (d["converged"], d["n"], d["n_ref"])
        assert d["e_norms"] < 1e-6 and d["e_v"] < 1e-6 and d["e_p"] < 1e-5, (
            d["e_norms"], d["e_v"], d["e_p"])
        assert d["uploads"] == 0, d["uploads"]
        assert d["hist"] == res[0]["hist"]


def test_refusals():
    """Registering the blocks of a time shard by pattern stays refused, and says so."""
    import common
    from control_amd import picard
    from control_amd.dist import CallbackComm
    pb = common.navier_stokes_problem(n=4, n_t=M)
    comm = CallbackComm(0, 2, None, None)
    with pytest.raises(ValueError, match="build='device' does not support time-sharded"):
        picard.GpuLinearSolver(pb, comm=comm, host_allreduce=lambda a, op: None,
                               relinearise="device", build="device")
    gls = picard.GpuLinearSolver(pb, comm=comm, host_allreduce=lambda a, op: None,
                                 relinearise="device")          # ... the device loop is not
    assert gls.relinearise == "device" and gls.dist is comm
