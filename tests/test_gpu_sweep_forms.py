"""Every form of the preconditioner's time sweeps, on every level structure it serves (run with
-m gpu on an MI355X).

The sweeps of the heat-control preconditioner run as plain launches (``persistent=0``), as a
persistent row program (counter form ``prog_mode=flags``, data-flow form, data-flow form for any
width ``prog_mode=w``) or as the tile program (``tile_kernels.hip``: one kernel variant per row
width 5 / 7 / 9 / 15 / 19, row slots per thread, threads per workgroup, level update fused or not,
coarse corrections or not).  Every form performs the same arithmetic in the same order, so each
must equal plain launches bit for bit, and so must every execution option of the plain steps.
Each case asserts through ``info()`` and ``pc_forms()`` that it ran the form it is named after
and that no program fell back; plain launches are compared with the CPU oracle per output block.
Chebyshev intervals are explicit: no spectrum estimate enters.
"""
import numpy as np
import pytest

import common
import structures as st
from control_amd.blocks import instationary_blocks
from control_amd.coarse import multilinear_coarse_space
from control_amd.fem import (SpatialDiscretisation, rectangle_p2p1, unit_cube_p1, unit_square_p1,
                             unit_square_q2)

pytestmark = pytest.mark.gpu

PLAIN, FLAGS, DATAFLOW, TILE = 0, 1, 2, 3                     # info()["sweep_form"]
ROWS, SHARED, KERNARG, INTERLEAVED, PROGRAM, TILE_STEP = range(6)   # pc_forms()["form"]
MASS = (8, 0.5, 2.0)
SCHUR = (16, 0.05, 2.1)


def spatial(space, n):
    if space == "fd5":
        # the preconditioner keeps mass and level matrices on one structure: the lumped mass is
        # stored on the 5-point structure, explicit zeros off the diagonal
        sd = st.fd5_square(n)
        M = sd.K.copy()
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        M.data[:] = np.where(M.indices == rows, sd.M.diagonal()[rows], 0.0)
        sd.M = M
        return sd
    if space == "q1":
        return st.q1_square(n)
    if space == "p2v":                      # the velocity blocks of P2-P1 Taylor-Hood
        th = rectangle_p2p1(n, n, 1.0, 1.0)
        return SpatialDiscretisation(M=th.M_v, K=th.K_v, coords=np.vstack([th.coords_v] * 2),
                                     boundary=th.boundary_v, name="p2v")
    return {"p1": unit_square_p1, "p1_3d": unit_cube_p1, "q2": unit_square_q2}[space](n)


def problem(space, n, n_t=4, CN=False, beta=1e-2):
    sd = spatial(space, n)
    tau = 2.0 / (n_t - 1.0)
    b00, b01, b10, b11, m = instationary_blocks(sd.M, sd.K, tau, beta, n_t, CN, share=True)
    return dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=sd.boundary)


def coarse_of(p, cells=4):
    return multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells), 1


def run(p, options=None, coarse=None, schur=SCHUR, x=None):
    g = common.gpu_system(p, options=options)
    if x is None:
        x = common.rng_vector(g.local_size)
    y = g.pc_apply(x, common.gpu_pc(p, MASS, schur, coarse=coarse))
    info = g.info()
    assert info["program_fallbacks"] == 0, (options, info)
    return y, info, g.pc_forms(), x


def per_block_err(p, y, ref):
    """Relative error of the v part and of the zeta part, each against its own norm."""
    h = len(ref) // 2
    return max(common.rel_err(y[:h], ref[:h]), common.rel_err(y[h:], ref[h:]))


def oracle_ref(p, x, coarse=None, schur=SCHUR):
    o = common.oracle_system(p)
    return o.pc_apply(common.oracle_pc(p, MASS, schur, coarse=coarse), x)


# -------------------------------------------------------------- structures x row programs
# (space, n): level rows 5 (fd5), 9 (q1), 7 (P1), 15 (P1 3-D), 9/15/25 (Q2, row-sorted),
# 9/19 (P2 velocity, row-sorted)
STRUCTURES = [("fd5", 40), ("q1", 24), ("p1", 24), ("p1_3d", 8), ("q2", 10), ("p2v", 8)]
PROGRAM_MODES = [("flags", {"prog_mode": "flags"}), ("dataflow", {"prog_mode": "dataflow"}),
                 ("w", {"prog_mode": "w"}), ("auto", {})]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("space,n", STRUCTURES)
def test_program_forms_match_plain_launches_and_oracle(space, n, CN):
    p = problem(space, n, CN=CN)
    plain, info, forms, x = run(p, {"persistent": "0"})
    assert info["sweep_form"] == PLAIN
    assert not any(f["form"] in (PROGRAM, TILE_STEP) for f in forms)
    assert per_block_err(p, plain, oracle_ref(p, x)) < 1e-10
    seen = {}
    for name, opts in PROGRAM_MODES:
        y, info, forms, _ = run(p, opts, x=x)
        assert np.array_equal(y, plain), (space, name)
        progs = [f for f in forms if f["form"] == PROGRAM]
        tiles = [f for f in forms if f["form"] == TILE_STEP]
        seen[name] = (info["sweep_form"], sorted({f["variant"] for f in progs}))
        if name == "flags":
            assert info["sweep_form"] == FLAGS and progs and all(f["variant"] == 0 for f in progs)
        elif name == "w":
            assert info["sweep_form"] == DATAFLOW and progs and all(f["variant"] == 2 for f in progs)
        elif name == "dataflow":
            # the data-flow program has fixed-width forms for widths 1..8 (kernels.hip
            # row_program_g_available); wider and ragged structures get the counter form
            w = p_width(forms)
            if 1 <= w <= 8:
                assert info["sweep_form"] == DATAFLOW and progs
                assert all(f["variant"] == 1 for f in progs), forms
            else:
                assert info["sweep_form"] == FLAGS and progs
                assert all(f["variant"] == 0 for f in progs), forms
        else:
            # auto: tile where a variant fits, else data-flow, else counters (ragged Q2)
            assert info["sweep_form"] in (FLAGS, DATAFLOW, TILE) and (progs or tiles)
            if space == "q2":
                assert info["sweep_form"] == FLAGS
    # ... and without compact STEP records
    y, info, _, _ = run(p, {"prog_mode": "dataflow", "prog_steps": "0"}, x=x)
    assert np.array_equal(y, plain) and info["sweep_form"] == seen["dataflow"][0]


def p_width(forms):
    return max(f["width"] for f in forms if f["form"] in (ROWS, KERNARG, PROGRAM))


# ------------------------------------------------------------ execution options of plain steps
# "lanes" needs 16 or more time levels, in chunks of at least 4 (pc.cpp build_BE)
PLAIN_TOGGLES = [{"kernarg_ops": "1"}, {"interleave": "0"}, {"lanes": "1"},
                 {"lanes": "1", "lane_chunks": "2"}, {"lanes": "1", "lane_chunks": "3"},
                 {"shared_rows": "0"}, {"pc_xcd": "0"}, {"no_graph": "1"}, {"sell_r": "1"}]
PLAIN_SPACES = [("fd5", 24), ("q1", 16), ("p1_3d", 6), ("q2", 6)]
_PLAIN_FORMS = {}


def plain_step_forms(space, n, CN):
    """pc_forms records of every toggle of PLAIN_TOGGLES (each checked bit for bit against the
    default plain launches), by toggle."""
    key = (space, n, CN)
    if key in _PLAIN_FORMS:
        return _PLAIN_FORMS[key]
    p = problem(space, n, n_t=16, CN=CN)
    base = {"persistent": "0"}
    plain, _, forms0, x = run(p, base)
    out = {"": forms0}
    for opt in PLAIN_TOGGLES:
        y, info, forms, _ = run(p, {**base, **opt}, x=x)
        assert info["sweep_form"] == PLAIN
        assert np.array_equal(y, plain), (space, opt, np.flatnonzero(y != plain)[:8])
        out[",".join(f"{k}={v}" for k, v in opt.items())] = forms
    _PLAIN_FORMS.clear()
    _PLAIN_FORMS[key] = out
    return out


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("space,n", PLAIN_SPACES)
def test_plain_step_options_are_bit_identical(space, n, CN):
    by_opt = plain_step_forms(space, n, CN)
    kinds0 = {f["form"] for f in by_opt[""]}
    assert INTERLEAVED in kinds0 and KERNARG not in kinds0
    for name, forms in by_opt.items():
        kinds = {f["form"] for f in forms}
        if "kernarg_ops" in name:
            assert KERNARG in kinds
        if "interleave=0" in name:
            # the mass solves: one shared-matrix launch serves four levels
            assert INTERLEAVED not in kinds and SHARED in kinds
        if "lanes" in name and not CN:
            # the side lane serves the BE sweep (pc.cpp build_BE); CN has no lane form
            assert INTERLEAVED not in kinds and any(f["lane"] == 1 for f in forms)
        if "shared_rows" in name:
            assert SHARED not in kinds
        if "sell_r" in name:
            # the interleaved and shared-matrix kernels read the R = 2 layout only
            rows = [f for f in forms if f["form"] in (ROWS, SHARED, KERNARG, INTERLEAVED)]
            assert rows and all(f["slots"] == 1 and f["form"] == ROWS for f in rows)


# --------------------------------------------------------------------------- tile variants
# Every variant the tile dispatch holds (tile_kernels.hip pick_tile / pick_tile_coarse), as
# (W, row slots, threads, level update fused, coarse corrections).  A 768-thread plan of widths
# 5 / 7 / 9 / 15 runs the one-slot 1 024-thread kernel with 768 threads: listed as such.
def tile_table():
    t = set()
    for W in (5, 7, 9):
        for co in (False, True):
            t |= {(W, s, 512, True, co) for s in (1, 2, 3)}
            t |= {(W, 1, 1024, True, co), (W, 1, 768, True, co)}
    for fused in (True, False):
        t |= {(15, 1, 1024, fused, False), (15, 1, 768, fused, False), (15, 1, 512, fused, False),
              (15, 2, 512, fused, False), (19, 1, 512, fused, False), (19, 2, 512, fused, False),
              (19, 1, 768, fused, False)}
    t |= {(15, 1, 1024, True, True), (15, 1, 768, True, True), (15, 1, 512, True, True),
          (15, 2, 512, True, True), (19, 1, 512, True, True), (19, 2, 512, True, True),
          (19, 1, 768, True, True)}
    return t


# (space, n, coarse cells or 0, unfused): the hand-off depth sets how many rows a tile computes,
# so a sweep over depths walks the row-slot counts at moderate mesh sizes; the plan's tiles
# follow the device's CU count, so what each depth gives is read back, not assumed.
TILE_FAMILIES = [("fd5", 160, 0, False), ("fd5", 160, 6, False),
                 ("q1", 160, 0, False), ("q1", 160, 6, False),
                 ("p1", 160, 0, False), ("p1", 160, 6, False),
                 ("p1_3d", 24, 0, False), ("p1_3d", 24, 0, True), ("p1_3d", 24, 4, False),
                 ("p2v", 24, 0, False), ("p2v", 24, 0, True), ("p2v", 24, 4, False)]
TILE_WAVES = (8, 12, 16)
TILE_DEPTHS = (1, 2, 3, 4, 6, 8, 10, 12, 14, 16)
_TILE_RUNS = {}
caches = {}      # (space, cells) -> the placements of the coarse tables its plans took


def tile_variant(forms):
    t = [f for f in forms if f["form"] == TILE_STEP]
    return {(f["width"], f["slots"], f["count"], bool(f["variant"] & 1), bool(f["variant"] & 2))
            for f in t}


def tile_family(space, n, cells, unfused):
    """Run every (waves, depth) of the family; check each tile plan against plain launches and
    against info(); return the variants the records name."""
    key = (space, n, cells, unfused)
    if key in _TILE_RUNS:
        return _TILE_RUNS[key]
    p = problem(space, n, CN=False)
    co = coarse_of(p, cells) if cells else None
    schur = (8, 2.1 / 30, 2.1) if co else SCHUR
    plain, _, _, x = run(p, {"persistent": "0"}, coarse=co, schur=schur)
    reached = set()
    for waves in TILE_WAVES:
        for depth in TILE_DEPTHS:
            opts = {"prog_mode": "tile", "tile_waves": str(waves), "tile_depth": str(depth)}
            if unfused:
                opts["tile_unfused"] = "1"
            y, info, forms, _ = run(p, opts, coarse=co, schur=schur, x=x)
            if info["sweep_form"] != TILE:
                continue            # no variant for this plan: another form ran (checked above)
            v = tile_variant(forms)
            assert len(v) >= 1 and info["sweep_depth"] == depth
            assert all((t[2], t[1]) == (info["sweep_threads"], info["sweep_row_slots"]) and
                       t[4] == (co is not None) for t in v), (v, info)
            # where the coarse tables of the plan live (auto: the first placement that fits)
            cache, ew = info["sweep_coarse_cache"], info["sweep_coarse_ew"]
            if co is None:
                assert (cache, ew, info["sweep_coarse_rings"]) == (0, 0, 0)
                assert np.array_equal(y, plain), (space, opts, np.flatnonzero(y != plain)[:8])
            else:
                nc = co[0].shape[1]
                assert cache in (0, 1, 2) and ew >= min(nc, 64), info
                assert info["sweep_coarse_rings"] <= (cache >= 1), info   # rings need the lists on chip
                caches.setdefault((space, cells), set()).add(cache)
                # by design not bit for bit: the tile program sums the coarse residual from the
                # tiles' partial sums in tile order, the plain launches row by row (DESIGN.md
                # section 6); the bar of test_gpu_coarse.py::
                # test_coarse_tile_program_soak_and_sharded_equivalents
                assert per_block_err(p, y, plain) < 1e-12, (space, opts, per_block_err(p, y, plain))
            reached |= v
    if co is not None:
        print(f"{space} cells {cells}: sweep_coarse_cache of the plans {sorted(caches[(space, cells)])}")
        assert 2 in caches[(space, cells)]       # the shallow plans fit everything on chip
    _TILE_RUNS[key] = reached
    return reached


@pytest.mark.parametrize("space,n,cells,unfused", TILE_FAMILIES,
                         ids=[f"{f[0]}-c{f[2]}-{'u' if f[3] else 'f'}" for f in TILE_FAMILIES])
def test_tile_plans_match_plain_launches(space, n, cells, unfused):
    reached = tile_family(space, n, cells, unfused)
    assert reached and reached <= tile_table(), sorted(reached - tile_table())


@pytest.mark.parametrize("space,n,cells", [("fd5", 24, 4), ("q1", 16, 4), ("p1", 16, 4),
                                           ("p1_3d", 6, 3), ("p2v", 6, 3)])
def test_two_grid_plain_launches_against_oracle(space, n, cells):
    for CN in (False, True):
        p = problem(space, n, CN=CN)
        co = coarse_of(p, cells)
        schur = (8, 2.1 / 30, 2.1)
        y, info, _, x = run(p, {"persistent": "0"}, coarse=co, schur=schur)
        assert per_block_err(p, y, oracle_ref(p, x, co, schur)) < 1e-10


# ------------------------------------------------------------------------ the whole table
def test_every_sweep_form_is_reached():
    """Walk the sweep dispatch through pc_forms(): every tile variant of tile_table(), every row
    program (counters, data-flow fixed width, data-flow any width), and every plain-step form --
    row steps, shared-matrix steps of a fixed width (<= 8) and of any width, kernel-argument
    steps, interleaved levels of both kernels (width <= 8 and wider), the side lane -- must have
    run in one of the cases above.  Fails if any was not reached."""
    tiles = set()
    for fam in TILE_FAMILIES:
        tiles |= tile_family(*fam)
    assert not tile_table() - tiles, sorted(tile_table() - tiles)

    reached = set()
    for space, n in PLAIN_SPACES:
        for forms in plain_step_forms(space, n, False).values():
            for f in forms:
                if f["form"] in (SHARED, INTERLEAVED):
                    reached.add((f["form"], "fixed" if 1 <= f["width"] <= 8 else "any"))
                elif f["form"] in (ROWS, KERNARG):
                    reached.add((f["form"], f["slots"]))
                if f["lane"] == 1:
                    reached.add(("lane",))
    for space, n in (("fd5", 40), ("q1", 24)):
        p = problem(space, n)
        for opts in ({"prog_mode": "flags"}, {"prog_mode": "dataflow"}, {"prog_mode": "w"}):
            _, _, forms, _ = run(p, opts)
            reached |= {(PROGRAM, f["variant"]) for f in forms if f["form"] == PROGRAM}
    want = ({(SHARED, "fixed"), (SHARED, "any"), (INTERLEAVED, "fixed"), (INTERLEAVED, "any"),
             (ROWS, 2), (ROWS, 1), (KERNARG, 2), ("lane",)} |
            {(PROGRAM, v) for v in (0, 1, 2)})
    assert not want - reached, sorted(want - reached, key=str)
