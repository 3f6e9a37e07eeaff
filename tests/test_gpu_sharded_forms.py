"""Every sweep form of the preconditioner on time shards, bit for bit against one rank (run with
-m gpu on an MI355X).

2, 3 and 5 ranks (processes) share GPU 0 over the host-staged pipe transport of
tests/test_gpu_sharded.py.  With explicit Chebyshev intervals and degrees no all-reduce enters
``SchurPC``: a shard runs the RowOps of one rank on the same operands, its neighbours' levels
arriving through the ``COMM`` steps of ``build_BE`` / ``build_CN`` (csrc/pc.cpp).  So every
rank's shard of an application must equal the one-rank plain-launch result bit for bit, in every
form that tests/test_gpu_sweep_forms.py, test_gpu_mass_tiles.py and test_gpu_coarse_rings.py
prove bit-identical on one rank.  Each handle is applied to two inputs and to the first one
again: the repeat goes through the cached program or graph and meets the halo buffers as the
second application left them, so a halo that no ``COMM`` step refreshed shows.

One ``launch()`` per case; the ranks loop over the option sets in-process
(tests/sharded_forms_worker.py) and never assert.  Each set reads back through ``info()`` and
``pc_forms()`` that the form it is named after ran, on every rank; what the library by design
does not run on a shard, or on a rank with few levels, is listed below with the line that
decides it, and the form that ran instead is asserted, still bit for bit.
"""
import functools

import pytest

import sharded_forms_worker as worker
import test_gpu_sharded as base

pytestmark = pytest.mark.gpu

PLAIN, FLAGS, DATAFLOW, TILE = 0, 1, 2, 3                     # info()["sweep_form"]
ROWS, SHARED, KERNARG, INTERLEAVED, PROGRAM, TILE_STEP, TILE_CHEB = range(7)   # pc_forms()["form"]

# Forms the library refuses on a shard by design: option -> (where, what runs instead).
REFUSED_ON_A_SHARD = {
    "lanes": ("csrc/pc.cpp:2083 (build_BE) `const bool lanes = use_lanes_ && !S_.sharded && "
              "(hi - lo) >= 16;`",
              "every step on the main lane; no interleaved levels either "
              "(pc.cpp:1918 emit_solves_interleaved `if (!S_.opts.interleave || S_.opts.lanes)`)"),
}
# Forms that batch the levels of a rank need four of them, sharded or not: a rank with fewer
# runs the batched solves as plain row steps with one op per level.
NEEDS_FOUR_LEVELS = {
    "interleaved": "csrc/pc.cpp:1982 (emit_solves) `if (m >= 4 && !first_done && its >= 2 && ...`",
    "shared": "csrc/kernels.hpp:88 launch_rowops_shared `serves R = 2 and at least four ops`",
    "mass_tile": "csrc/pc_lower.cpp (fuse_mass_tiles) replaces runs of ROWS_IL steps only",
}
# (world, m) -> levels per rank (kkt_shard_range)
LEVELS = {(2, 7): [4, 3], (5, 7): [2, 2, 1, 1, 1], (5, 5): [1, 1, 1, 1, 1], (3, 4): [2, 1, 1],
          (2, 2): [1, 1]}
HEAT_CASES = [(2, 7), (5, 7), (5, 5)]
# (2, 2): the narrowest case in which a tile launch without coarse levels (the mass solve of a
# one-level rank) comes before one with them -- see test_two_grid_forms_on_shards
COARSE_CASES = [(2, 7), (5, 5), (2, 2)]
SCHEMES = [False, True]


_cache = {}


def results(target, world, CN, **kw):
    """One launch per case, shared by the tests below; a failed launch is not repeated by the
    next test that asks for it."""
    key = (target, world, CN, tuple(sorted(kw.items())))
    if key not in _cache:
        try:
            _cache[key] = base.launch(world, CN, None,
                                      target=functools.partial(getattr(worker, target), CN=CN, **kw))
        except BaseException as e:
            _cache[key] = e
    if isinstance(_cache[key], BaseException):
        raise _cache[key]
    return _cache[key]


def kinds(rb):
    return {f["form"] for f in rb["forms"]}


def records(rb, form):
    return [f for f in rb["forms"] if f["form"] == form]


def show(label, r, d, name, rb):
    """One line per (rank, option set): measured before anything is asserted."""
    apps = rb.get("apps", [])
    print(f"{label} rank {r} ({d['levels']} levels from {d['lo']}) {name}: "
          f"same {[a['same'] for a in apps]} sweep_form {rb['info']['sweep_form']} "
          f"depth {rb['info']['sweep_depth']} rings {rb['info']['sweep_coarse_rings']} "
          f"falls {rb['info']['program_fallbacks']} forms "
          f"{sorted((f['form'], f['width'], f['slots'], f['count'], f['variant']) for f in rb['forms'])}")


def check_apps(label, r, d, name, apps):
    """All three applications equal the one-rank shard bit for bit; a difference is reported as
    (local block, row) of the first differing entries."""
    nx = d.get("nx") or d.get("nv")
    for k, a in enumerate(apps):
        where = [(i // nx, i % nx) for i in a["first"]]
        assert a["same"], (label, "rank", r, name, "application", k, "differs at (block, row)",
                           where, "entries", a["n_bad"], "rel. distance", a["dist"])


def check_heat_set(label, r, d, name, rb, width):
    """The form the option set is named after ran on this rank."""
    nl, info, k = d["levels"], rb["info"], kinds(rb)
    progs, tiles = records(rb, PROGRAM), records(rb, TILE_STEP)
    assert info["program_fallbacks"] == 0, (label, r, name, info)
    if name.startswith("plain"):
        assert info["sweep_form"] == PLAIN and not k & {PROGRAM, TILE_STEP, TILE_CHEB}, (label, r, name)
        assert all(f["lane"] == 0 for f in rb["forms"]), (label, r, name)      # REFUSED_ON_A_SHARD
    if name == "plain":
        assert (INTERLEAVED in k) == (nl >= 4), (label, r, nl, rb["forms"])    # NEEDS_FOUR_LEVELS
        assert KERNARG not in k
    elif name == "plain,kernarg_ops=1":
        assert KERNARG in k
    elif name == "plain,interleave=0":
        assert INTERLEAVED not in k and (SHARED in k) == (nl >= 4), (label, r, nl, rb["forms"])
    elif name == "plain,shared_rows=0":
        assert SHARED not in k
    elif name == "plain,sell_r=1":
        rows = [f for f in rb["forms"] if f["form"] in (ROWS, SHARED, KERNARG, INTERLEAVED)]
        assert rows and all(f["slots"] == 1 and f["form"] == ROWS for f in rows), rb["forms"]
    elif name == "plain,lanes=1":
        assert INTERLEAVED not in k
    elif name == "flags":
        assert info["sweep_form"] == FLAGS and progs and all(f["variant"] == 0 for f in progs), rb
    elif name in ("dataflow", "dataflow,prog_steps=0"):
        # fixed-width data-flow forms exist for widths 1..8 (kernels.hip row_program_g_available)
        assert 1 <= width <= 8
        assert info["sweep_form"] == DATAFLOW and progs and all(f["variant"] == 1 for f in progs), rb
    elif name == "w":
        assert info["sweep_form"] == DATAFLOW and progs and all(f["variant"] == 2 for f in progs), rb
    elif name.startswith("tile"):
        depth = int(name.split("=")[1])
        assert info["sweep_form"] == TILE and info["sweep_depth"] == depth and tiles, rb
        assert all(f["variant"] == 1 and f["width"] == width for f in tiles), tiles
        # one tile launch per sweep (a one-level rank: its mass solve, a single solve, as well) and
        # no row program: on a one-level rank the products between the sweeps are single-block
        # steps of the sweeps' runs (rank 0: in front of the forward level; the last rank: between
        # the sweeps), which fuse_programs (csrc/pc_lower.cpp) must not let take the levels with them
        assert not progs and sum(f["n"] for f in tiles) == 2 + (nl == 1), (label, r, name, rb["forms"])
        assert all((f["count"], f["slots"]) == (info["sweep_threads"], info["sweep_row_slots"])
                   for f in tiles), (tiles, info)
    elif name.startswith("mass_tiles"):
        cheb = records(rb, TILE_CHEB)
        if nl >= 4:
            # degree 8 at 3 steps per launch: launches of 3, 3 and 2 steps for every solve
            counts = rb["cheb_counts"]
            assert cheb and INTERLEAVED not in k, rb["forms"]
            assert counts == [3, 3, 2] * (len(counts) // 3), counts
        else:
            assert not cheb and INTERLEAVED not in k, rb["forms"]              # NEEDS_FOUR_LEVELS


def check_heat_case(label, res, world, m, options, width):
    assert sorted(res) == list(range(world))
    assert [res[r]["levels"] for r in range(world)] == LEVELS[(world, m)]
    for r in range(world):
        d = res[r]
        assert d["inputs_differ"] and list(d["sets"]) == [n for n, _ in options]
        for name, rb in d["sets"].items():
            show(label, r, d, name, rb)
    for r in range(world):
        d = res[r]
        for name, rb in d["sets"].items():
            check_apps(label, r, d, name, rb["apps"])
            check_heat_set(label, r, d, name, rb, width)


# --------------------------------------------------------------------- 1. heat control, P1
@pytest.mark.parametrize("CN", SCHEMES, ids=["BE", "CN"])
@pytest.mark.parametrize("world,m", HEAT_CASES)
def test_heat_forms_on_shards_equal_one_rank(world, m, CN):
    """41 x 41 P1 (1 681 nodes, rows of 7), mass (8, 0.5, 2.0), Schur (6, 0.05, 2.1).  Shards of
    4 + 3 levels (the only rank with an interleaved group and with mass tiles), of 2, 2, 1, 1, 1
    (one-level ranks in the middle and at the end: ``blk(., hi-1)`` is ``blk(., lo)``) and of one
    level each (rank 0 is level 0 alone, the last rank the epsilon level alone)."""
    label = f"heat world {world} m {m} {'CN' if CN else 'BE'}"
    check_heat_case(label, results("run_heat_forms", world, CN, m=m), world, m,
                    worker.HEAT_OPTIONS, 7)


def test_ragged_structure_on_shards_equals_one_rank():
    """13 x 13 Q2 nodes, rows of 9 / 15 / 25 entries: the interleaved and shared-matrix kernels for
    any width, and the row program the ragged structure gets, on shards of 4 + 3 levels."""
    res = results("run_heat_forms", 2, False, m=7, space="q2", n=6)
    check_heat_case("heat q2 world 2 m 7 BE", res, 2, 7, worker.Q2_OPTIONS, 0)
    for r in range(2):
        rb = res[r]["sets"]["auto"]
        assert rb["info"]["sweep_form"] in (FLAGS, DATAFLOW, TILE), rb["info"]
        assert records(rb, PROGRAM) or records(rb, TILE_STEP)
        assert rb["info"]["program_fallbacks"] == 0


def test_every_form_met_a_shard():
    """The union over the cases above: plain launches, the interleaved kernels of both kinds
    (fixed width <= 8 and any width), the counter program, both data-flow programs, the tile
    program and the mass tiles each ran on some rank, with all three applications bit-equal to
    one rank.  Only the entries of REFUSED_ON_A_SHARD are exempt."""
    reached = set()
    runs = [results("run_heat_forms", w, CN, m=m) for w, m in HEAT_CASES for CN in SCHEMES]
    runs.append(results("run_heat_forms", 2, False, m=7, space="q2", n=6))
    for res in runs:
        for d in res.values():
            for name, rb in d["sets"].items():
                if not all(a["same"] for a in rb["apps"]) or rb["info"]["program_fallbacks"]:
                    continue
                if name == "plain" and rb["info"]["sweep_form"] == PLAIN:
                    reached.add("plain")
                for f in rb["forms"]:
                    if f["form"] == INTERLEAVED:
                        reached.add(("interleaved", "fixed" if 1 <= f["width"] <= 8 else "any"))
                    elif f["form"] == PROGRAM:
                        reached.add(("program", f["variant"]))
                    elif f["form"] == TILE_STEP:
                        reached.add("tile")
                    elif f["form"] == TILE_CHEB:
                        reached.add("mass_tile")
                    if f["lane"] == 1:
                        reached.add("lanes")
    want = {"plain", ("interleaved", "fixed"), ("interleaved", "any"), ("program", 0),
            ("program", 1), ("program", 2), "tile", "mass_tile"}
    assert not want - reached, sorted(want - reached, key=str)
    assert not reached & set(REFUSED_ON_A_SHARD), reached


# ------------------------------------------------------------- 2. two-grid sub-solves on shards
PLAN = ("sweep_tiles", "sweep_threads", "sweep_depth", "sweep_row_slots")


@pytest.mark.parametrize("CN", SCHEMES, ids=["BE", "CN"])
@pytest.mark.parametrize("world,m", COARSE_CASES)
def test_two_grid_forms_on_shards(world, m, CN):
    """Same mesh, coarse space of 5 x 5 cells, 1 and 2 cycles, Schur (6, 0.07, 2.1).  Sharded
    plain launches equal one-rank plain launches bit for bit (the plain form sums the coarse
    residual row by row whatever the sharding).  The sharded tile program in the ring form equals
    the one with the hand-off after the correction bit for bit (the criterion of
    test_gpu_coarse_rings.py).  Against one-rank plain launches the tile program is held to the
    per-block 1e-12 of test_gpu_sweep_forms.py::tile_family: it sums the coarse residual from
    the tiles' partial sums in tile order.  Where a rank's tile plan is
    the one-rank tile handle's (tiles, threads, depth, row slots), its shard also equals the
    one-rank TILE run bit for bit: that condition was met by every handle of every case on the
    MI355X these tests were written on (52 tiles x 512 threads, depth 6, one row slot: the plan
    follows from the spatial structure, the sweep count and the CU count, none of which a shard
    changes).

    Ranks with ONE level (worlds 5 / 5 and 2 / 2) found two things in csrc/pc.cpp.  Their mass
    solve is a single solve and becomes a tile launch without coarse levels, the first of the
    application; the granule buffers of the coarse exchanges were zeroed only by a FIRST launch
    that had coarse levels (launch_tile_sweep, `if (h_coarse)`), so from the second application
    on the two-grid launches met the tags of the application before and read its partial sums:
    relative errors of 0.4 to 14 in the second and third application, the first one correct --
    fixed by PcStep::clear_coarse.  And the products between the sweeps have one op there, so
    they joined the run of single-block steps of a sweep level wherever no hand-off separates
    them (rank 0: in front of the forward level; the last rank: between the sweeps), and
    fuse_tile_run refused the whole run: those levels ran as plain launches (as a data-flow row
    program without coarse space) and the shard could not equal the one-rank tile run --
    fuse_programs now gives every stretch of levels inside such a run its tile launch."""
    label = f"two-grid world {world} m {m} {'CN' if CN else 'BE'}"
    res = results("run_coarse_forms", world, CN, m=m)
    assert [res[r]["levels"] for r in range(world)] == LEVELS[(world, m)]
    met = []
    for r in range(world):
        d = res[r]
        for cycles in (1, 2):
            c = d["cycles"][cycles]
            for name in ("plain", "rings=1", "rings=0"):
                show(f"{label} cycles {cycles}", r, d, name, c[name])
            print(f"{label} cycles {cycles} rank {r}: tile against one-rank plain "
                  f"{c['rings=1']['err_plain']}, against one-rank tile "
                  f"{[a['dist'] for a in c['rings=1']['one_tile']]}; one-rank plan "
                  f"{[c['one_tile']['info'][k] for k in PLAN]}")
    for r in range(world):
        d = res[r]
        for cycles in (1, 2):
            c = d["cycles"][cycles]
            lab = f"{label} cycles {cycles}"
            check_apps(lab, r, d, "plain", c["plain"]["apps"])
            assert c["plain"]["info"]["sweep_form"] == PLAIN
            assert c["one_tile"]["info"]["sweep_form"] == TILE
            check_apps(lab, r, d, "rings=1 against rings=0", c["rings_equal"])
            for rings in (1, 0):
                rb = c[f"rings={rings}"]
                tiles = records(rb, TILE_STEP)
                assert rb["info"]["sweep_form"] == TILE and rb["info"]["program_fallbacks"] == 0, rb
                # one two-grid tile launch per sweep, on every rank; a one-level rank's mass solve
                # is a tile launch without coarse levels in front of them
                assert not records(rb, PROGRAM)
                assert sum(f["n"] for f in tiles if f["variant"] & 2) == 2, (lab, r, rb["forms"])
                assert sum(f["n"] for f in tiles if not f["variant"] & 2) == (d["levels"] == 1)
                assert rb["info"]["sweep_coarse_rings"] == rings, rb["info"]
                assert max(rb["err_plain"]) < 1e-12, (lab, r, rings, rb["err_plain"])
                same_plan = all(rb["info"][k] == c["one_tile"]["info"][k] for k in PLAN)
                met.append(same_plan)
                if same_plan:
                    check_apps(lab, r, d, f"rings={rings} against the one-rank tile program",
                               rb["one_tile"])
    print(f"{label}: tile plan equal to the one-rank plan in {sum(met)} of {len(met)} handles")


# -------------------------------------- 3. Stokes control, the places without a nested Krylov loop
@pytest.mark.parametrize("CN", SCHEMES, ids=["BE", "CN"])
def test_stokes_operator_and_velocity_preconditioner_on_shards(CN):
    """P2-P1 on a 4 x 4 mesh, three ranks with 2, 1 and 1 of m = 4 levels (n_t = 4 with backward
    Euler, 5 with Crank-Nicolson).  The outer operator -- sharded by two block families, with
    rectangular B blocks, the constant nullspace and Crank-Nicolson's sub-block split -- and the
    velocity preconditioner alone (``inner`` and ``inner_pc`` of ``stokes_gpu``: vector P2,
    row-sorted rows of 9 / 19) equal one rank bit for bit on every shard.  The full ``StokesPC``
    application contains a nested GMRES whose inner products are summed rank by rank: it is not
    bit-comparable and stays at its tolerance in tests/test_gpu_sharded.py and
    tests/test_gpu_stokes_pressure_stage.py."""
    label = f"stokes world 3 {'CN' if CN else 'BE'}"
    res = results("run_stokes_forms", 3, CN)
    assert [res[r]["levels"] for r in range(3)] == LEVELS[(3, 4)] and res[0]["m"] == 4
    for r in range(3):
        for name, rb in res[r]["velocity"].items():
            show(label, r, res[r], name, rb)
    for r in range(3):
        d = res[r]
        assert d["outer_inputs_differ"]
        for k, a in enumerate(d["outer"]):
            assert a["same"], (label, "rank", r, "outer.mult, application", k, a)
        for name, rb in d["velocity"].items():
            check_apps(label, r, d, "velocity " + name, rb["apps"])
            info = rb["info"]
            assert info["program_fallbacks"] == 0
            # the shard runs the form one rank runs under the same options
            assert info["sweep_form"] == rb["one_rank_form"], (label, r, name, info)
            progs = records(rb, PROGRAM)
            if name == "plain":
                assert info["sweep_form"] == PLAIN and not progs and not records(rb, TILE_STEP)
            elif name == "flags":
                assert info["sweep_form"] == FLAGS and progs and all(f["variant"] == 0 for f in progs)
            else:
                # auto: tile where a variant fits, else a row program
                assert info["sweep_form"] in (FLAGS, DATAFLOW, TILE), info
                assert progs or records(rb, TILE_STEP)
