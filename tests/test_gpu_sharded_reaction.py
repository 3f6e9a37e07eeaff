"""The scalar Picard / Gauss-Newton loop on the device on time-sharded solvers
(``Instationary.non_linear_solve(device=True, comm=...)``): every rank
keeps, assembles, evaluates and updates its own levels of the iterate in HBM.  2, 3 and 5 ranks
(processes) share GPU 0 over the host-staged pipe transport; with six unknown blocks they own 3, 2
and 2-or-1 of them -- a one-block shard has both halo levels next to its only row.  Each rank
compares itself with a one-rank plan in its own process (tests/sharded_reaction_worker.py), on
``unit_square_p1(4)`` and ``box_p1(3, 3, 3)``; one launch per (world, scheme, target) serves the
tests below."""
import multiprocessing as mp
import os
import queue
import sys

import pytest

import reaction_shard_ref as sref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
M = sref.M_BLOCKS           # unknown blocks: n_t = 6 (BE), n_t = 7 (CN)
LIMIT = 240                 # seconds for all ranks of one launch
MESHES = ("triangles", "tetrahedra")


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
    import sharded_reaction_worker
    procs = [ctx.Process(target=getattr(sharded_reaction_worker, target),
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
    """``kkt_reaction_window`` equals ``shard_windows`` on every rank; the one-rank plan reports
    ``(0, n_t)`` throughout."""
    res = results(world, CN)
    n_t = M + 1 if CN else M
    sizes = set()
    for r in range(world):
        for mesh in MESHES:
            d = res[r][mesh]
            assert d["n_t"] == n_t
            assert d["window"] == sref.shard_windows(M, CN, r, world) == d["window_want"]
            assert d["window"]["blocks"] == sref.shard_range(M, r, world) == (d["lo"], d["hi"])
            assert d["window_one"] == {"v": (0, n_t), "zeta": (0, n_t), "D": (0, n_t),
                                       "blocks": (0, M)}
        sizes.add(res[r]["triangles"]["hi"] - res[r]["triangles"]["lo"])
    assert sizes == {2: {3}, 3: {2}, 5: {1, 2}}[world]


@case
def test_assembly_is_rank_independent(world, CN):
    """The halo levels were NaN in what the rank uploaded; after ``assemble()`` the windows of
    ``v`` and ``zeta`` equal the global state and the element matrices and ``D`` of every window
    level equal the one-rank plan's bit for bit -- CN's ``D_lo`` included, built from the halo
    ``v``.  Triangles and tetrahedra (Picard), and one case with Gauss-Newton coefficients."""
    res = results(world, CN)
    for r in range(world):
        for key in MESHES + ("newton",):
            check(res[r][key], "halo_poisoned", "halo_travelled", "asm_E", "asm_D",
                  "asm_nonlinear")


@case
def test_residual_and_right_hand_side_rows(world, CN):
    """The rank's rows of both families equal the one-rank rows bit for bit (CN: with the
    neighbours' boundary rows in the time transforms) and are not zero; one norm on every rank.
    Both norms are square roots of sums of the same N non-negative squares in different orders:
    each carries a relative error below (N - 1) u / 2, u = 2^-53, so they differ by less than
    N u (the bound of tests/test_gpu_sharded_relin.py)."""
    res = results(world, CN)
    for mesh in MESHES:
        for rhs in (0, 1):
            for r in range(world):
                d = res[r][mesh]
                check(d, f"res{rhs}", f"res{rhs}_nonzero")
                assert d[f"norm{rhs}"] == res[0][mesh][f"norm{rhs}"]
                bound = d["n_entries"] * 2.0 ** -53 * d[f"norm{rhs}_one"]
                print(mesh, world, CN, rhs, r, d[f"norm{rhs}"], d[f"norm{rhs}_one"], bound)
                assert abs(d[f"norm{rhs}"] - d[f"norm{rhs}_one"]) <= bound, (
                    d[f"norm{rhs}"], d[f"norm{rhs}_one"], bound)
        assert res[0][mesh]["norm0"] == res[0][mesh]["norm1"]   # the residual's in both modes
        assert res[0][mesh]["norm0"] > 0.0


@case
def test_composition(world, CN):
    """Every owned block of the full build list equals the one-rank handle's values; every recipe
    lies on exactly one rank; a recipe for another rank's row is an argument error that names the
    block, and nothing is written."""
    from control_amd.blocks import instationary_build_recipes
    res = results(world, CN)
    n_full = len(instationary_build_recipes(0.2, 1.0e-2, M + 1 if CN else M, CN)["inner"])
    assert n_full >= (8 * M - 12 if CN else 6 * M - 4)
    for mesh in MESHES:
        total = 0
        for r in range(world):
            d = res[r][mesh]
            check(d, "blocks_equal", "foreign_wrote_nothing", "default_recipes_owned")
            assert d["n_blocks"] == d["n_recipes"] > 0 and d["n_full"] == n_full
            total += d["n_blocks"]
            code, msg = d["foreign"]
            assert code == -1 and "block (" in msg and "not owned" in msg, d["foreign"]
        assert total == n_full


@case
def test_update(world, CN):
    """A dyadic update moves the owned levels by exactly its blocks and is zeroed; zeta is zero
    on the Dirichlet dofs of the whole window, v keeps its values there; the halo slots change
    with the next exchange; the gathered iterate equals the one-rank plan's."""
    res = results(world, CN)
    for r in range(world):
        for mesh in MESHES:
            check(res[r][mesh], "update_owned", "update_changed", "u_zeroed", "zeta_bc_zero",
                  "v_bc_kept", "halo_stale", "halo_updated", "state_gathered")


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_device_loop_matches_one_rank(world, CN):
    """The sharded loop against the one-rank device loop in the same process (BE and CN on
    triangles, BE on tetrahedra).  Linear iteration counts are printed, not asserted: the sharded
    GMRES sums its inner products rank by rank.

    Fields: the bar ``_compare_loops`` of the one-rank loop tests holds between two paths that
    differ only in rounding, ``1e-9 max(1, |ref|)``.  Measured on an MI355X: 5.9e-15 at worst.

    Norms: that bar is 1e-8 relative per norm, and the last norms of these loops (1e-10 of the
    first) miss it: measured 6.2e-6 (BE triangles), 3.1e-6 (tetrahedra) and 1.3e-6 (CN) relative
    at worst, with linear iteration counts that differ by up to 22 in a solve.  The same difference between the existing host-built sharded and one-rank
    solves at this size (the first linearised system, these solver parameters; the quantities of
    tests/test_gpu_sharded.py) is 4.1 relative on the residual histories and 3.1e-14 on the
    solutions; times ten for the outer steps that is a bar of 41 relative on the norms (DESIGN.md
    section 6.6a has both figures).  Asserted here is less than that allows, for every norm these
    loops can reach: ``|a - b| <= 1e-8 b + 2e-13 max(1, norm_0)``.  The second term is what the
    linear solves leave: each stops at a residual of ``1e-14 max(||b||, 1)`` (every solve here
    converges below its iteration limit, which is asserted), the next non-linear residual is that
    residual plus the quadratic remainder of the update, so two paths differ by at most the sum of
    their two residuals per step, ``2e-14 max(1, norm_0)``, and ten outer steps of a contracting
    iteration by at most ten times that.  Measured: 8.7e-15 ``max(1, norm_0)`` at worst, 3 % of
    the bound."""
    res = results(world, CN, "run_rank_loop")
    for mesh in ("triangles",) if CN else MESHES:
        for r in range(world):
            d = res[r][mesh]
            print(mesh, world, CN, r, {k: d[k] for k in ("n", "n_ref", "e_norms", "e_norms_abs",
                                                         "e_norms_bar", "e_v", "e_zeta", "its",
                                                         "its_ref")})
            assert d["n_ref"] - 1 > 4                  # a loop that stops at once tests nothing
            assert d["converged"] and d["n"] == d["n_ref"], (d["converged"], d["n"], d["n_ref"])
            assert max(d["its"] + d["its_ref"]) < d["max_its"]
            assert d["e_norms_bar"] <= 1.0, (d["e_norms"], d["e_norms_abs"])
            assert d["e_v"] <= 1e-9 and d["e_zeta"] <= 1e-9, (d["e_v"], d["e_zeta"])
            check(d, "bc_exact", "zeta_bc_zero")
            assert d["hist"] == res[0][mesh]["hist"]
            assert d["window"] == sref.shard_windows(M, CN, r, world)
