"""The two-grid levels of the tile program (``pc_tile_sweep<..., COARSE = true>``, tables from
``SchurPC::build_tile_coarse``) bit for bit, in every placement of its tables (run with -m gpu on
an MI355X).

a. ``kkt_debug_tile_levels`` -- one launch of the program on host data, on the handle's own plan
   and tables -- against ``tests/tile_level_ref.py``, a NumPy restatement written from the
   definitions that ``tests/test_tile_level_ref.py`` holds to the CPU emulation of the scheme and
   to the recurrence in extended precision.  Every placement is forced by the options
   ``tile_coarse_cache`` / ``coarse_rings`` / ``tile_coarse_rows`` and read back from the hook; a
   forced placement that did not run fails the case.
b. The placements against each other through ``kkt_pc_apply``: every combination of the three
   options equals the default run bit for bit; the default run is held to the project's bars for
   this form (1e-12 per block against plain launches, 1e-10 against the oracle), on a random and
   on a smooth input -- on the smooth one the correction is a large part of the result.
c. After ``update_block_values`` the tile form with block rows of the coarse inverse equals the
   form with full rows and a fresh handle on the new values.

The device's CU count sets the tiles, so everything about the plan is read back, not assumed.
Shapes: P1 41^2 (W 7), fd5 41^2 (W 5), q1 25^2 (W 9), p1_3d 9^3 (W 15, lists without rings), p2v
n = 8 (W 19, two components), coarse spaces of 4 or 5 cells; n_t = 4.  With 4 cells the two
components of p2v have 25 coarse functions each and the row length of the inverse, which starts
at 64, is not below n_coarse = 50: ``p2v8`` is the same mesh with 8 cells (162 coarse functions,
rows of 98), the shape on which ``ew < n_coarse``.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import common
import tile_level_ref as tl
from control_amd import _lib
from control_amd.coarse import multilinear_coarse_space
from test_gpu_sweep_forms import per_block_err, problem

pytestmark = pytest.mark.gpu

G, PAD = _lib.BLOCK_GUARD, _lib.KRYLOV_PAD
Q00, Q10 = 0, 2
MASS = (8, 0.5, 2.0)
PC_ITS = 5
SHAPES = {"p1": ("p1", 40, 5), "fd5": ("fd5", 40, 5), "q1": ("q1", 24, 4), "p1_3d": ("p1_3d", 8, 4),
          "p2v": ("p2v", 8, 4), "p2v8": ("p2v", 8, 8)}
WIDTH = {"p1": 7, "fd5": 5, "q1": 9, "p1_3d": 15, "p2v": 19, "p2v8": 19}
RINGS_BUILT = {s: s != "p1_3d" for s in SHAPES}       # rows of P with at most 4 entries
PLACEMENTS = [(2, 1), (2, 0), (1, 1), (1, 0), (0, 0)]   # (cache, rings): rings need the lists on chip
# every legal placement of every shape (lists without rings have no ring form)
LEGAL = [(s, c, r) for s in SHAPES for c, r in PLACEMENTS if RINGS_BUILT[s] or not r]


def canon(A):
    A = sp.csr_matrix(A)
    return A if A.has_sorted_indices else A.sorted_indices()


@functools.lru_cache(maxsize=None)
def setting(shape, CN=False):
    space, n, cells = SHAPES[shape]
    p = problem(space, n, n_t=4, CN=CN, beta=1e-4)
    P = canon(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells))
    nx = p["sd"].n_dofs
    mask = np.zeros(nx, bool)
    mask[np.asarray(p["nodes"])] = True
    X = np.asarray(p["sd"].coords)
    smooth = np.prod(np.sin(np.pi * X), axis=1)
    return p, P, mask, smooth


def tile_system(p, depth=None, cache="auto", rings="1", rows="block", keep=False):
    opts = {"prog_mode": "tile", "tile_coarse_cache": str(cache), "coarse_rings": str(rings),
            "tile_coarse_rows": rows, "coarse_keep": "1" if keep else "0"}
    if depth:
        opts["tile_depth"] = str(depth)
    return common.gpu_system(p, options=opts)


def expect_placement(info, shape, cache, rings, rows, nc, ranges=None):
    assert info["sweep_form"] == 3 and info["program_fallbacks"] == 0, info
    if cache != "auto":
        assert info["sweep_coarse_cache"] == int(cache), (info, cache)
    lists_on_chip = info["sweep_coarse_cache"] >= 1
    assert info["sweep_coarse_rings"] == int(str(rings) == "1" and RINGS_BUILT[shape] and lists_on_chip)
    if rows == "full":
        assert info["sweep_coarse_ew"] == nc
    elif ranges is not None:
        assert info["sweep_coarse_ew"] == max(64, int((ranges[1] - ranges[0]).max()))


# ------------------------------------------------------------------ a. hook against reference
def hook_inputs(shape):
    """Level data that does not depend on the handle: two matrices of the level pattern (blocks
    (Q10, 0, 0) = tau K + M and (Q00, 0, 0) = tau M), the update (Q10, 1, 0) = -M, right-hand sides
    (random / sin sin), coefficient tables and a synthetic coarse matrix per level matrix."""
    p, P, mask, smooth = setting(shape)
    n, nc = P.shape
    b00, _, b10, _ = p["blocks"]
    A = [canon(b10[(0, 0)]), canon(b00[(0, 0)])]
    Um = canon(b10[(1, 0)])
    rng = np.random.default_rng([common.SEED, n, nc])
    dinv = [np.where(mask, 1.0, 1.0 / a.diagonal()) for a in A]
    rhs = {"random": [rng.standard_normal(n) for _ in range(3)],
           "smooth": [(1.0 + 0.25 * l) * smooth for l in range(3)]}
    coef = {its: [np.column_stack([0.1 * rng.uniform(-1, 1, its), 1.0 + 0.1 * rng.uniform(-1, 1, its),
                                   0.4 + 0.1 * rng.uniform(-1, 1, its)]) for _ in range(2)]
            for its in (4, 5)}
    # dense inside the diagonal blocks of P^T A P, entries over nine binades with both signs
    # (a wrong column order then changes the sum), exact zeros outside; scaled by 2^-10 so that
    # the "corrections" of this non-inverse keep the iterates of three cycles of moderate size
    lo, hi = tl.inverse_ranges(A[0], P)
    synth = []
    for _ in range(2):
        E = np.zeros((nc, nc))
        for j in range(nc):
            cols = np.flatnonzero((hi == hi[j]) & (lo == lo[j]))
            E[j, cols] = (rng.choice([-1.0, 1.0], len(cols)) * np.exp2(rng.integers(-14, -5, len(cols)))
                          * (1.0 + rng.random(len(cols))))
        synth.append(E)
    return dict(A=A, U=Um, dinv=dinv, rhs=rhs, coef=coef, synth=synth, ranges=(lo, hi))


_INPUTS, _REFS = {}, {}


def inputs_of(shape):
    if shape not in _INPUTS:
        _INPUTS.clear()            # one shape's data at a time
        _REFS.clear()
        _INPUTS[shape] = hook_inputs(shape)
    return _INPUTS[shape]


def level_specs(shape, its, einv, kind):
    """The chain of three levels: solo on A0 / E0, chained on A1 / E1 (matrix and inverse change:
    the kernel reloads both), chained on A1 / E1 again (it keeps both)."""
    d = inputs_of(shape)
    b, c = d["rhs"][kind], d["coef"][its]
    lev = [dict(A=d["A"][0], block=(Q10, 0, 0), dinv=d["dinv"][0], b=b[0], coef=c[0], einv=einv[0],
                p1_scale=0.7, post1=0.9, post2=1.1),
           dict(A=d["A"][1], block=(Q00, 0, 0), dinv=d["dinv"][1], b=b[1], coef=c[1], einv=einv[1],
                p1_scale=0.6, post1=1.2, post2=0.8, U=d["U"], update=(Q10, 1, 0), ca=-1.0, cy=1.0,
                bout=True),
           dict(A=d["A"][1], block=(Q00, 0, 0), dinv=d["dinv"][1], b=b[2], coef=c[1], einv=einv[1],
                p1_scale=0.6, post1=1.0, post2=1.0, U=d["U"], update=(Q10, 1, 0), ca=0.5, cy=-1.0,
                bout=True)]
    return lev


def reference(shape, its, cycles, ekind, einv, kind, own, rows):
    key = (shape, its, cycles, ekind, kind, rows,
           hash(b"".join(np.asarray(o, np.int32).tobytes() + b"|" for o in own)),
           hash(b"".join(np.asarray(e).tobytes() for e in einv)))
    if key not in _REFS:
        _, P, mask, _ = setting(shape)
        _REFS[key] = tl.run(level_specs(shape, its, einv, kind), mask, P, own, its, cycles, rows=rows)
    return _REFS[key]


def check_launch(g, shape, res, ref, mask, what):
    n = len(mask)
    assert res["inputs_changed"] == 0, what
    for l, (x, b) in enumerate(ref):
        out = res["out"][l]
        assert np.all(out[:G] == PAD) and np.all(out[G + n:] == PAD), (what, l)
        bad = np.flatnonzero(tl.rr.differ(out[G:G + n], x))
        assert bad.size == 0, (what, "level", l, "rows", bad[:8], out[G + bad[:4]], x[bad[:4]])
        if res["bout"][l] is not None:
            bo = res["bout"][l]
            assert np.all(bo[:G] == PAD) and np.all(bo[G + n:] == PAD), (what, l)
            assert not tl.rr.differ(bo[G:G + n], b).any(), (what, "bout of level", l)


def run_hook_cases(shape, depth, cache, rings, rows="block", its_list=(4, 5), cycles_list=(1, 2, 3)):
    p, P, mask, _ = setting(shape)
    n, nc = P.shape
    d = inputs_of(shape)
    g = tile_system(p, depth, cache, rings, rows, keep=True)
    x = common.rng_vector(g.local_size)
    pc = common.gpu_pc(p, MASS, (PC_ITS, 0.07, 2.1), coarse=(P, 1))
    y0 = g.pc_apply(x, pc)
    launches = 0
    ranges = d["ranges"] if rows == "block" else tl.inverse_ranges(d["A"][0], P, "full")
    expect_placement(g.info(), shape, cache, rings, rows, nc, ranges)
    # the level matrices as the library stores them are the reference's CSR arrays, wherever an
    # entry can matter: outside the rows and columns of the mask (masked rows are not computed,
    # masked columns multiply an exact zero -- in the kernel and in the reference)
    for blk, A in (((Q10, 0, 0), d["A"][0]), ((Q00, 0, 0), d["A"][1]), ((Q10, 1, 0), d["U"])):
        live = ~(np.repeat(mask, np.diff(A.indptr)) | mask[A.indices])
        stored = g.block_values(*blk)[0]
        assert live.sum() > n and np.array_equal(stored[live], A.data[live]), blk
    own_inv = g.coarse_inverses()
    own_e = [np.ascontiguousarray(own_inv[0]), np.ascontiguousarray(0.5 * own_inv[-1])]
    if rows == "full":
        # whole rows: a matrix without any zero shows a column that is left out
        rng = np.random.default_rng([common.SEED, nc, 7])
        einvs = {"dense": [np.exp2(-10.0) * rng.uniform(0.5, 1.0, (nc, nc)) * rng.choice([-1.0, 1.0], (nc, nc))
                           for _ in range(2)]}
    else:
        einvs = {"own": own_e, "synthetic": d["synth"]}
    plan = g.debug_tile_levels()
    assert (plan["cache"], plan["rings"], plan["ew"]) == \
        (g.info()["sweep_coarse_cache"], g.info()["sweep_coarse_rings"], g.info()["sweep_coarse_ew"])
    assert plan["cache"] == int(cache) and plan["depth"] == depth and plan["W"] == WIDTH[shape]
    assert plan["rings"] == int(str(rings) == "1" and RINGS_BUILT[shape] and int(cache) >= 1)
    assert plan["nrows"] == n and plan["n_coarse"] == nc and plan["tiles"] == g.info()["sweep_tiles"]
    owned = np.sort(np.concatenate(plan["own"]))
    assert np.array_equal(owned, np.flatnonzero(~mask)), "the tiles own every row outside the mask once"
    for its in its_list:
        for cycles in cycles_list:
            for ekind, einv in einvs.items():
                for kind in ("random", "smooth"):
                    lev = level_specs(shape, its, einv, kind)
                    ref = reference(shape, its, cycles, ekind, einv, kind, plan["own"], rows)
                    what = (shape, depth, cache, rings, rows, its, cycles, ekind, kind)
                    chain = g.debug_tile_levels(lev, its, cycles)
                    for k in ("cache", "rings", "ew", "depth", "tiles", "threads"):
                        assert chain[k] == plan[k]
                    check_launch(g, shape, chain, ref, mask, what + ("chain",))
                    solo = g.debug_tile_levels(lev[:1], its, cycles)
                    launches += 2
                    check_launch(g, shape, solo, ref[:1], mask, what + ("solo",))
    # the production program still runs, and as before
    assert np.array_equal(g.pc_apply(x, pc), y0) and g.info()["program_fallbacks"] == 0
    print(f"{shape} depth {depth} cache {plan['cache']} rings {plan['rings']} ew {plan['ew']} rows {rows}: "
          f"{plan['tiles']} tiles x {plan['threads']} threads, {launches} launches, "
          f"{len(_REFS)} references held")


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("shape,cache,rings", LEGAL)
def test_hook_equals_reference_in_every_placement(shape, cache, rings, depth):
    run_hook_cases(shape, depth, cache, rings)


@pytest.mark.parametrize("cache", [2, 1, 0])
@pytest.mark.parametrize("shape", ["p2v", "p2v8", "p1"])
def test_hook_equals_reference_with_full_rows(shape, cache):
    """The fall-back assignment e_lo = 0, e_hi = n_coarse, ew = n_coarse, with a matrix that has
    no zero at all."""
    run_hook_cases(shape, 2, cache, 1, rows="full", its_list=(4,), cycles_list=(2,))


def test_hook_rejects_what_it_cannot_run():
    shape = "p2v8"
    p, P, mask, _ = setting(shape)
    n, nc = P.shape
    d = inputs_of(shape)
    g = tile_system(p, 2, 2, 1)
    with pytest.raises(_lib.KktError) as e:
        g.debug_tile_levels()
    assert e.value.code == -3                        # KKT_ERR_STATE: nothing built yet
    g.pc_apply(common.rng_vector(g.local_size), common.gpu_pc(p, MASS, (PC_ITS, 0.07, 2.1), coarse=(P, 1)))
    assert g.info()["sweep_coarse_ew"] < nc
    lev = level_specs(shape, 4, d["synth"], "random")
    dense = np.ones((nc, nc))
    for bad in ([dict(lev[0], einv=dense)],                          # outside the blocks
                [dict(lev[0], block=(Q10, 3, 0))],                   # not stored
                [lev[1]],                                            # chained first level
                [dict(lev[0], bout=True)]):                          # bout on a solo level
        with pytest.raises(_lib.KktError) as e:
            g.debug_tile_levels(bad, 4, 1)
        assert e.value.code == -1, bad
    with pytest.raises(_lib.KktError) as e:
        g.debug_tile_levels(lev[:1], 4, 0)                           # no cycle
    assert e.value.code == -1
    # nothing was launched by any of these, and the program is as it was
    ok = g.debug_tile_levels(lev[:1], 4, 1)
    assert ok["inputs_changed"] == 0 and g.info()["program_fallbacks"] == 0
    # ... and a handle without a two-grid tile program
    h = common.gpu_system(p, options={"persistent": "0"})
    h.pc_apply(common.rng_vector(h.local_size), common.gpu_pc(p, MASS, (PC_ITS, 0.07, 2.1), coarse=(P, 1)))
    with pytest.raises(_lib.KktError) as e:
        h.debug_tile_levels()
    assert e.value.code == -3


# ---------------------------------------------------- b. placements against each other
SCHUR_B = (6, 0.07, 2.1)


@functools.lru_cache(maxsize=None)
def bars(shape, CN):
    """Inputs (random, sin sin), the default tile run on each, held to the project's bars: 1e-12
    per block against the plain launches, 1e-10 against the oracle."""
    p, P, mask, smooth = setting(shape, CN)
    m, nx = p["m"], p["sd"].n_dofs
    xs = {"random": common.rng_vector(2 * m * nx),
          "smooth": np.tile(np.where(mask, 0.0, smooth), 2 * m) * np.repeat(1.0 + 0.1 * np.arange(2 * m), nx)}
    pc_tile, pc_plain = (common.gpu_pc(p, MASS, SCHUR_B, coarse=(P, 2)) for _ in range(2))
    g = tile_system(p)
    plain = common.gpu_system(p, options={"persistent": "0"})
    osys, opc = common.oracle_system(p), common.oracle_pc(p, MASS, SCHUR_B, coarse=(P, 2))
    ys = {}
    for kind, x in xs.items():
        ys[kind] = g.pc_apply(x, pc_tile)
        e_plain = per_block_err(p, ys[kind], plain.pc_apply(x, pc_plain))
        e_oracle = per_block_err(p, ys[kind], osys.pc_apply(opc, x))
        print(f"{shape} CN={CN} {kind}: tile against plain {e_plain:.2e}, against the oracle {e_oracle:.2e}")
        assert e_plain < 1e-12, (shape, CN, kind, e_plain)
        assert e_oracle < 1e-10, (shape, CN, kind, e_oracle)
    assert plain.info()["sweep_form"] == 0
    expect_placement(g.info(), shape, "auto", 1, "block", P.shape[1])
    return xs, ys


@pytest.mark.parametrize("rows", ["block", "full"])
@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_placements_equal_the_default_run(shape, CN, rows):
    p, P, mask, _ = setting(shape, CN)
    xs, ys = bars(shape, CN)
    lo, hi = tl.inverse_ranges(canon(p["blocks"][2][(0, 0)]), P, rows)
    for cache in ("auto", 2, 1, 0):
        for rings in (1, 0):
            g = tile_system(p, None, cache, rings, rows)
            pc = common.gpu_pc(p, MASS, SCHUR_B, coarse=(P, 2))
            for kind in ("random", "smooth", "random"):          # xa, xb, xa
                y = g.pc_apply(xs[kind], pc)
                assert np.array_equal(y, ys[kind]), (shape, CN, rows, cache, rings, kind,
                                                     common.rel_err(y, ys[kind]))
            expect_placement(g.info(), shape, cache, rings, rows, P.shape[1], (lo, hi))


# ------------------------------------------------------------------------------ c. rebuild
def _p2v_pair():
    p, P, _, _ = setting("p2v8")
    # the same structure, other Schur matrices: the diagonal doubled (not a multiple of the old
    # matrix -- to a scaling of L the product (L + c M)^-1 L of the sweeps is nearly blind)
    new = canon(p["blocks"][2][(0, 0)]).copy()
    diagonal = new.indices == np.repeat(np.arange(new.shape[0]), np.diff(new.indptr))
    new.data = np.where(diagonal, 2.0 * new.data, new.data)
    q10 = {k: (new if k[0] == k[1] else v) for k, v in p["blocks"][2].items()}
    return p, P, q10


def _convection_pair():
    from test_gpu_multigrid_drivers import _two_component_convection_problem
    p, P = _two_component_convection_problem(n=24)
    q, _ = _two_component_convection_problem(n=24, scale=2.0)
    q10 = dict(p["blocks"][2])
    for i in range(p["n_t"]):
        q10[(i, i)] = q["blocks"][2][(i, i)]
    return p, canon(P), q10


@pytest.mark.parametrize("pair", [_p2v_pair, _convection_pair], ids=["p2v8", "convection"])
def test_rebuilt_block_rows_equal_full_rows_and_a_fresh_handle(pair):
    """The ranges of the rows of the coarse inverse are made once per handle; the inverses are
    formed again with every ``update_block_values``.  Were a new inverse non-zero outside the old
    ranges, the block rows would leave terms out that the full rows and a fresh handle keep."""
    p, P, q10 = pair()
    nc = P.shape[1]
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    schur = (6, 0.07, 2.1)
    lo, hi = tl.inverse_ranges(canon(p["blocks"][2][(0, 0)]), P)
    assert (hi - lo).min() < nc                  # block rows leave columns out
    ew = {"block": max(64, int((hi - lo).max())), "full": nc}
    before, after = {}, {}
    for rows in ("block", "full"):
        g = tile_system(p, rows=rows)
        pc = common.gpu_pc(p, MASS, schur, coarse=(P, 2))
        before[rows] = g.pc_apply(x, pc)
        assert g.info()["sweep_form"] == 3
        assert g.info()["sweep_coarse_ew"] == ew[rows], g.info()
        for i in range(p["m"]):
            g.update_block_values(Q10, i, i, q10[(i, i)])
        after[rows] = g.pc_apply(x, pc)
        assert g.info()["sweep_form"] == 3 and g.info()["program_fallbacks"] == 0
        assert g.info()["sweep_coarse_ew"] == ew[rows], g.info()
    fresh_p = dict(p, blocks=(p["blocks"][0], p["blocks"][1], q10, p["blocks"][3]))
    gf = tile_system(fresh_p)
    fresh = gf.pc_apply(x, common.gpu_pc(fresh_p, MASS, schur, coarse=(P, 2)))
    assert gf.info()["sweep_form"] == 3 and gf.info()["sweep_coarse_ew"] == ew["block"]
    assert np.array_equal(before["block"], before["full"])
    # the new values are in use: a change far above round-off (it is small on the P2 shape, where
    # the mass term of the Schur matrices dominates: 6e-7)
    assert common.rel_err(after["block"], before["block"]) > 1e-10
    assert np.array_equal(after["block"], after["full"])
    assert np.array_equal(after["block"], fresh)
