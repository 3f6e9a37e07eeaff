"""Option ``pc_alias``: the Schur preconditioner reads value arrays that its twin search proved
equal bit for bit from one array (csrc/pc.cpp, ``collect_matrices``; run with -m gpu on an MI355X).

Mode G (``share=False``) keeps one device copy per time block.  For a time-invariant operator
those copies hold the same bits; with ``pc_alias=1`` (the default) the formed level matrices, their
Jacobi diagonals and the stored blocks the updates multiply with are then one array per class, and
``pc_alias=0`` is the program with one array per level.  Aliasing changes which address a value is
read from and nothing else, so the contract is equality of bits: one ``pc_apply`` with
``pc_alias=1`` equals ``pc_alias=0`` in every form the suite switches between, and, where every
level is equal, mode G equals mode S.

Which arrays a level reads is asserted through ``pc_alias()`` (``kkt_debug_pc_alias``) against the
classes counted on the host from the blocks' bytes: a comparison that took a near-twin (one block
scaled by 1 + 2^-30, or -0.0 for +0.0 in one entry) for a twin would read another level's matrix.

Shapes: small meshes (625 to 729 rows) on which the default form is the tile program on two tiles
or more -- 19 to 22 tiles, asserted from ``info()`` -- and n_t = 6; the whole file runs in 6 s.
"""
import copy
import functools

import numpy as np
import pytest

import common
import pc_alias_worker as worker
import test_gpu_sharded as base
from control_amd.blocks import instationary_blocks, stationary_blocks
from control_amd.coarse import multilinear_coarse_space
from control_amd.fem import unit_cube_p1, unit_square_p1, unit_square_p2
from control_amd.multiblock import ChebSpec, CoarseSpace, MultiBlockSystem, SchurPC

pytestmark = pytest.mark.gpu

TILE = 3
Q01, Q10 = 1, 2
N_T = 6
MASS = (8, 0.5, 2.0)
TWO_GRID = (4, 2.1 / 30, 2.1)          # 4 sweeps per cycle
PLAIN_SWEEPS = (-1, 0.0, 0.0)         # intervals and degree estimated: the twin search runs
NEAR = 1.0 + 2.0 ** -30
SPACES = {"p1": (unit_square_p1, 24, 4), "p1_3d": (unit_cube_p1, 8, 3), "p2": (unit_square_p2, 12, 4)}
# kind -> (CN, two-grid cycles, tile depth)
KINDS = {"BE-2g-d2": (False, 2, 2), "BE-2g-d4": (False, 2, 4), "CN-2g-d2": (True, 2, 2),
         "CN-2g-d4": (True, 2, 4), "BE-plain": (False, 0, 0)}
FORMS = [("default", {}), ("plain", {"persistent": "0"}), ("flags", {"prog_mode": "flags"}),
         ("dataflow", {"prog_mode": "dataflow"}), ("w", {"prog_mode": "w"})]
PATTERNS = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def spatial(space):
    make, n, cells = SPACES[space]
    sd = make(n)
    return sd, multilinear_coarse_space(sd.coords, sd.boundary, cells=cells)


def problem(space, CN, share=False):
    sd, _ = spatial(space)
    tau = 2.0 / (N_T - 1.0)
    b00, b01, b10, b11, m = instationary_blocks(sd.M, sd.K, tau, 1e-2, N_T, CN, share=share)
    return dict(sd=sd, tau=tau, beta=1e-2, n_t=N_T, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=sd.boundary)


def middle(p):
    return p["m"] // 2


def near_twin(A):
    B = A.copy()
    B.data = B.data * NEAR
    return B


def with_pattern(p, pattern):
    """(b) the diagonal block of the middle level scaled by 1 + 2^-30; (c) its sub-diagonal block
    alone; (d) one entry of every sub-diagonal block +0.0, of the middle one -0.0."""
    p = dict(p, blocks=tuple(dict(b) for b in p["blocks"]))
    b10, L = p["blocks"][2], middle(p)
    if pattern == "b":
        b10[(L, L)] = near_twin(b10[(L, L)])
    elif pattern == "c":
        b10[(L, L - 1)] = near_twin(b10[(L, L - 1)])
    elif pattern == "d":
        for i in range(1, p["m"]):
            A = b10[(i, i - 1)].copy()
            A.data[A.nnz // 2] = -0.0 if i == L else 0.0
            b10[(i, i - 1)] = A
    return p


def pc_of(p, space, kind):
    _, cycles, _ = KINDS[kind]
    co = (spatial(space)[1], cycles) if cycles else None
    return common.gpu_pc(p, MASS, TWO_GRID if cycles else PLAIN_SWEEPS, coarse=co)


def options(kind, form, alias):
    o = dict(form, pc_alias=str(alias))
    if KINDS[kind][2]:
        o["tile_depth"] = str(KINDS[kind][2])
    return o


def labels(keys):
    """Classes numbered in order of first appearance; -1 for no array."""
    seen = {}
    return [-1 if k is None or k == -1 else seen.setdefault(k, len(seen)) for k in keys]


def sweeps_of(solves):
    out = {}
    for k, s in enumerate(solves):
        out.setdefault(s["sweep"], []).append(k)
    return out


def expected_classes(p, solves):
    """Per sub-solve, from the blocks' bytes on the host: (shift, level block) and the update's
    block.  Both sweeps of BE multiply with -M, so the update's key is the bytes alone."""
    b01, b10 = p["blocks"][1], p["blocks"][2]
    mat, upd = [], []
    for s in solves:
        i, fwd = s["level"], s["sweep"] == "forward"
        D = (b10 if fwd else b01)[(i, i)]
        U = (b10.get((i, i - 1)) if i >= 1 else None) if fwd else \
            (b01.get((i, i + 1)) if i + 1 < p["m"] else None)
        mat.append((float(s["c"]).hex(), D.data.tobytes()))
        upd.append(None if U is None else U.data.tobytes())
    return mat, upd


def check_partition(p, g, alias, what):
    """With pc_alias=1 the arrays a sweep's levels read are the host's classes; with 0 every level
    reads arrays of its own."""
    solves, recs = g.pc_solves(), g.pc_alias()
    assert len(solves) == len(recs) == 2 * p["m"], what
    mat, upd = expected_classes(p, solves)
    for sweep, idx in sweeps_of(solves).items():
        got_m = labels([recs[k]["matrix"] for k in idx])
        got_d = labels([recs[k]["dinv"] for k in idx])
        got_u = labels([recs[k]["update"] for k in idx])
        if alias:
            want_m, want_u = labels([mat[k] for k in idx]), labels([upd[k] for k in idx])
        else:
            want_m = list(range(len(idx)))
            want_u = labels([None if upd[k] is None else k for k in idx])
        print(f"{what} pc_alias={alias} {sweep}: matrix {got_m} dinv {got_d} update {got_u}")
        assert got_m == want_m and got_d == want_m, (what, alias, sweep, got_m, got_d, want_m)
        # (CN backward: the update's matrix is a formed one, formed once per class of its block)
        assert got_u == want_u, (what, alias, sweep, got_u, want_u)
    return solves, recs


def apply_pair(p, space, kind, form, x):
    """One application with pc_alias 0 and 1 on fresh handles: (y0, y1, g0, g1)."""
    out = []
    for alias in (0, 1):
        g = common.gpu_system(p, options=options(kind, form, alias))
        out.append((g.pc_apply(x, pc_of(p, space, kind)), g))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def check_forms(p, space, kind, pattern):
    """Bit-equality of pc_alias 1 and 0 in every form; returns the default form's handles."""
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    keep = None
    for name, form in FORMS:
        y0, y1, g0, g1 = apply_pair(p, space, kind, form, x)
        i0, i1 = g0.info(), g1.info()
        what = (space, kind, pattern, name)
        print(f"{what}: sweep_form {i0['sweep_form']} / {i1['sweep_form']} tiles {i1['sweep_tiles']} "
              f"fallbacks {i0['program_fallbacks']} / {i1['program_fallbacks']} "
              f"differing entries {int(np.count_nonzero(y0 != y1))}")
        assert np.array_equal(y1, y0), what
        assert i1["program_fallbacks"] == i0["program_fallbacks"], what
        assert i1["sweep_form"] == i0["sweep_form"], what
        if name == "default":
            assert i1["sweep_form"] == TILE and i1["sweep_tiles"] >= 2, (what, i1)
            assert i1["program_fallbacks"] == 0, what
            keep = (x, y1, g0, g1)
        else:
            g0.close()
            g1.close()
    return keep


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_aliased_levels_equal_own_copies(kind, pattern):
    p = with_pattern(problem("p1", KINDS[kind][0]), pattern)
    x, y1, g0, g1 = check_forms(p, "p1", kind, pattern)
    what = ("p1", kind, pattern)
    check_partition(p, g0, 0, what)
    solves, recs = check_partition(p, g1, 1, what)
    m, L = p["m"], middle(p)
    fwd = [recs[k] for k, s in enumerate(solves) if s["sweep"] == "forward"]
    fm, fu = labels([r["matrix"] for r in fwd]), labels([r["update"] for r in fwd])
    if not p["CN"]:
        # BE: the first level (no shift), the interior class, the last level (its own shift)
        interior = [0] + [1] * (m - 2) + [2]
        if pattern == "b":
            interior[L] = 2
            interior[-1] = 3
        assert fm == interior, (what, fm)
    else:
        assert fm == ([0] * m if pattern != "b" else [0] * L + [1] + [0] * (m - L - 1)), (what, fm)
    if pattern in ("a", "b"):
        assert fu == [-1] + [0] * (m - 1), (what, fu)
    else:
        # (c), (d): the middle level's update is an array of its own, its neighbours share
        assert fu == [-1] + [0] * (L - 1) + [1] + [0] * (m - L - 1), (what, fu)
    st0, st1 = g0.spectrum_stats(), g1.spectrum_stats()
    print(f"{what}: spectrum_stats pc_alias=0 {st0}\n{what}: spectrum_stats pc_alias=1 {st1}")
    assert st1["fallbacks"] == st0["fallbacks"] == 0 and st1["matrices"] == st0["matrices"], what
    if pattern == "a":
        assert st1["twin_syncs"] <= st0["twin_syncs"] and st1["syncs"] <= st0["syncs"], (st0, st1)
        assert st1["alias_blocks"] > 0 and st1["aliased"] > 0 and st0["aliased"] == 0, (st0, st1)
        # mode G with all levels equal: mode S's result and mode S's launches
        ps = problem("p1", p["CN"], share=True)
        gs = common.gpu_system(ps, options=options(kind, {}, 1))
        ys = gs.pc_apply(x, pc_of(ps, "p1", kind))
        assert np.array_equal(y1, ys), what
        assert g1.pc_forms() == gs.pc_forms(), (what, g1.pc_forms(), gs.pc_forms())
        assert gs.info()["sweep_tiles"] == g1.info()["sweep_tiles"]


def test_against_the_oracle():
    """BE, two-grid, all levels equal, mode G: the aliased program against
    ``oracle.pc_instationary_BE`` at the bar of tests/test_gpu_parity.py for that comparison."""
    kind = "BE-2g-d2"
    p = problem("p1", False)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    g = common.gpu_system(p, options=options(kind, {"persistent": "0"}, 1))
    y = g.pc_apply(x, pc_of(p, "p1", kind))
    co = (spatial("p1")[1], KINDS[kind][1])
    ref = common.oracle_system(p).pc_apply(common.oracle_pc(p, MASS, TWO_GRID, coarse=co), x)
    err = common.rel_err(y, ref)
    print(f"pc_alias=1 against the oracle: {err:.2e}; aliased {g.spectrum_stats()['aliased']}")
    assert g.spectrum_stats()["aliased"] > 0
    assert err < 1e-10


@pytest.mark.parametrize("kind", ["BE-2g-d2", "CN-2g-d2", "BE-plain"])
def test_classes_follow_value_updates(kind):
    """(e) all levels equal; kkt_update_block_values makes the middle diagonal block a near-twin;
    a second update makes it equal again.  Every rebuild proves its classes anew."""
    CN = KINDS[kind][0]
    p = problem("p1", CN)
    pb = with_pattern(p, "b")
    L = middle(p)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    for name, form in FORMS[:2]:
        gs = [common.gpu_system(p, options=options(kind, form, alias)) for alias in (0, 1)]
        pcs = [pc_of(p, "p1", kind) for _ in gs]
        for stage, cur in (("equal", p), ("near-twin", pb), ("equal again", p)):
            if stage != "equal":
                for g in gs:
                    g.update_block_values(Q10, L, L, cur["blocks"][2][(L, L)])
            y0, y1 = (g.pc_apply(x, pc) for g, pc in zip(gs, pcs))
            what = (kind, name, stage)
            print(f"{what}: differing entries {int(np.count_nonzero(y0 != y1))}")
            assert np.array_equal(y1, y0), what
            check_partition(cur, gs[0], 0, what)
            check_partition(cur, gs[1], 1, what)
            assert gs[1].info()["program_fallbacks"] == 0, what
        for g in gs:
            g.close()


@pytest.mark.parametrize("space", ["p1_3d", "p2"])
def test_other_structures(space):
    """P1 tetrahedra (rows of 15) and P2 triangles (ragged rows): BE two-grid, (a) and (b)."""
    kind = "BE-2g-d2"
    for pattern in ("a", "b"):
        p = with_pattern(problem(space, False), pattern)
        _, _, g0, g1 = check_forms(p, space, kind, pattern)
        check_partition(p, g0, 0, (space, kind, pattern))
        check_partition(p, g1, 1, (space, kind, pattern))


def test_stationary():
    """The stationary kind: two sub-solves, one product with D_v; nothing to share in mode G but
    the two sub-solve matrices where D_v is symmetric."""
    sd, P = spatial("p1")
    blocks = stationary_blocks(sd.M, sd.K, 1e-2)
    x = common.rng_vector(2 * sd.n_dofs)
    for coarse in (None, CoarseSpace(P, 2)):
        ys, recs = [], []
        for alias in (0, 1):
            g = MultiBlockSystem(sd.n_dofs, sd.n_dofs, *copy.deepcopy(blocks),
                                 options={"pc_alias": str(alias)})
            sch = ChebSpec(*(TWO_GRID if coarse else PLAIN_SWEEPS))
            if coarse:
                sch.coarse = coarse
            pc = SchurPC(kind="stationary", M=sd.M, beta=1e-2, bc_nodes=sd.boundary,
                         mass=ChebSpec(*MASS), schur=sch)
            ys.append(g.pc_apply(x, pc))
            recs.append(g.pc_alias())
            assert g.info()["program_fallbacks"] == 0 and len(recs[-1]) == 2
        print(f"stationary coarse {coarse is not None}: records {recs}")
        assert np.array_equal(ys[0], ys[1])
        assert all(r["update"] == -1 for r in recs[0] + recs[1])
        assert recs[0][0]["matrix"] != recs[0][1]["matrix"]


def test_time_shards():
    """Two ranks on one device: each rank aliases among its own levels and its shard of two
    applications equals its pc_alias=0 shard bit for bit."""
    res = base.launch(2, False, None, target=functools.partial(worker.run_alias, CN=False, m=N_T))
    for r, d in sorted(res.items()):
        r0, r1 = d["runs"]["0"], d["runs"]["1"]
        print(f"rank {r} ({d['levels']} levels from {d['lo']}): form {r1['form']} "
              f"aliased {r1['stats']['aliased']} matrix ids {[a['matrix'] for a in r1['alias']]}")
        assert r1["y"] == r0["y"], r
        assert r0["falls"] == r1["falls"] == 0 and r0["form"] == r1["form"]
        assert len(r1["alias"]) == 2 * d["levels"]
        assert r1["stats"]["aliased"] > 0 and r0["stats"]["aliased"] == 0
        assert len({a["matrix"] for a in r1["alias"]}) < len({a["matrix"] for a in r0["alias"]})
