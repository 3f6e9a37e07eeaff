"""What the registers of the level matrix hold at a level boundary of the two-grid tile program
(``pc_tile_sweep<..., COARSE = true>``), bit for bit (run with -m gpu on an MI355X).

At the end of a level the values of the NEXT level's update matrix are requested into the registers
of the level matrix, in front of the hand-off; after the hand-off they are multiplied, the level's
own matrix is requested into the same registers and is waited for only behind the first coarse
exchange.  A key says which array the registers hold.  The chains here are the boundaries at which
that bookkeeping can go wrong and which the three-level chain of ``tests/test_gpu_tile_levels.py``
does not reach:

``alternating``   a solo level and five chained ones whose level matrix alternates A1 / A0: both
                  matrices are requested again at every boundary;
``same_block``    a level whose update block IS its level block (one stored array: the values
                  requested for the update serve as the level matrix), then a level on another
                  matrix;
``same_matrix``   two consecutive levels on one level matrix with different update blocks
                  (``update_block_values`` gives the stored (Q10, 2, 1) values of its own first);
``no_update``     a level without an update behind chained ones (the hook accepts it), and a
                  chained level behind that.

Every chain is launched whole and with its first level alone, through ``kkt_debug_tile_levels``, and
compared with ``tests/tile_level_ref.py``.  ``its`` = 1 with one cycle makes the first sweep the
last one: the level matrix is needed right behind the exchange.  ``tile_waves`` picks the
1 024-thread (128 registers; 768 threads for W = 19) and the 512-thread instantiations; threads,
width and depth are read back from the hook.  Shapes: the smallest of ``test_gpu_tile_levels``.
"""
import numpy as np
import pytest

import common
import tile_level_ref as tl
from test_gpu_tile_levels import (MASS, PC_ITS, Q00, Q10, WIDTH, canon, check_launch, inputs_of,
                                  setting)

pytestmark = pytest.mark.gpu

SHAPE_WAVES = [("p1", 16), ("p1", 8), ("fd5", 16), ("fd5", 8), ("q1", 16), ("q1", 8),
               ("p1_3d", 16), ("p1_3d", 8), ("p2v", 12), ("p2v", 8)]
DEPTHS = [1, 2, 4]
# (its, cycles): every value of its in {1, 4, 5} and of cycles in {1, 2, 3}; (1, 1): one sweep in all
RUNS = [(1, 1), (4, 2), (5, 3), (1, 3)]
CHAINS = ["alternating", "same_block", "same_matrix", "no_update"]
U2_BLOCK = (Q10, 2, 1)

_DATA, _REFS = {}, {}


def fetch_inputs(shape):
    """Per shape: the matrices of ``test_gpu_tile_levels.hook_inputs``, a second update matrix on the
    structure of the first, six right-hand sides and coefficient tables for ``its`` = 1, 4, 5."""
    if shape not in _DATA:
        _DATA.clear()
        _REFS.clear()
        d = inputs_of(shape)
        n = d["A"][0].shape[0]
        rng = np.random.default_rng([common.SEED, n, 41])
        U2 = d["U"].copy()
        U2.data = d["U"].data * (1.0 + 0.5 * rng.random(len(U2.data)))
        coef = {its: [np.column_stack([0.1 * rng.uniform(-1, 1, its), 1.0 + 0.1 * rng.uniform(-1, 1, its),
                                       0.4 + 0.1 * rng.uniform(-1, 1, its)]) for _ in range(2)]
                for its in (1, 4, 5)}
        _DATA[shape] = dict(d, U2=canon(U2), rhs6=[rng.standard_normal(n) for _ in range(6)], coef3=coef)
    return _DATA[shape]


def chain_specs(shape, chain, its):
    d = fetch_inputs(shape)
    A, E, dinv, b, c = d["A"], d["synth"], d["dinv"], d["rhs6"], d["coef3"][its]
    blocks = [(Q10, 0, 0), (Q00, 0, 0)]

    def level(l, k, update=None, **kw):
        L = dict(A=A[k], block=blocks[k], dinv=dinv[k], b=b[l], coef=c[k], einv=E[k],
                 p1_scale=0.7 - 0.05 * l, post1=0.9 + 0.1 * l, post2=1.1 - 0.1 * l)
        if update is not None:
            U, blk = update
            L.update(U=U, update=blk, ca=(-1.0, 0.5)[l % 2], cy=(1.0, -1.0, 0.75)[l % 3], bout=True)
        return dict(L, **kw)
    U1, U2 = (d["U"], (Q10, 1, 0)), (d["U2"], U2_BLOCK)
    if chain == "alternating":
        return [level(0, 0)] + [level(l, l % 2, U1 if l % 2 else U2) for l in range(1, 6)]
    if chain == "same_block":
        return [level(0, 0), level(1, 1, (A[1], blocks[1])), level(2, 0, U1)]
    if chain == "same_matrix":
        return [level(0, 0), level(1, 1, U1), level(2, 1, U2)]
    if chain == "no_update":
        return [level(0, 0), level(1, 1, U1), level(2, 0), level(3, 1, U2)]
    raise ValueError(chain)


def reference(shape, chain, its, cycles, own):
    key = (shape, chain, its, cycles,
           hash(b"".join(np.asarray(o, np.int32).tobytes() + b"|" for o in own)))
    if key not in _REFS:
        _, P, mask, _ = setting(shape)
        _REFS[key] = tl.run(chain_specs(shape, chain, its), mask, P, own, its, cycles)
    return _REFS[key]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape,waves", SHAPE_WAVES)
def test_level_boundaries_equal_reference(shape, waves, depth):
    p, P, mask, _ = setting(shape)
    n, nc = P.shape
    d = fetch_inputs(shape)
    g = common.gpu_system(p, options={"prog_mode": "tile", "tile_depth": str(depth),
                                      "tile_waves": str(waves), "coarse_keep": "1"})
    # the stored (Q10, i, i - 1) blocks are one matrix on this problem: (Q10, 2, 1) gets its own
    g.update_block_values(*U2_BLOCK, d["U2"])
    x = common.rng_vector(g.local_size)
    pc = common.gpu_pc(p, MASS, (PC_ITS, 0.07, 2.1), coarse=(P, 1))
    y0 = g.pc_apply(x, pc)
    assert g.info()["sweep_form"] == 3 and g.info()["program_fallbacks"] == 0, g.info()
    for blk, A in (((Q10, 0, 0), d["A"][0]), ((Q00, 0, 0), d["A"][1]), ((Q10, 1, 0), d["U"]),
                   (U2_BLOCK, d["U2"])):
        live = ~(np.repeat(mask, np.diff(A.indptr)) | mask[A.indices])
        assert np.array_equal(g.block_values(*blk)[0][live], A.data[live]), blk
    plan = g.debug_tile_levels()
    assert (plan["threads"], plan["W"], plan["depth"]) == (64 * waves, WIDTH[shape], depth), plan
    assert plan["nrows"] == n and plan["n_coarse"] == nc
    launches = 0
    for its, cycles in RUNS:
        for chain in CHAINS:
            lev = chain_specs(shape, chain, its)
            ref = reference(shape, chain, its, cycles, plan["own"])
            what = (shape, waves, depth, chain, its, cycles)
            whole = g.debug_tile_levels(lev, its, cycles)
            for k in ("threads", "W", "depth", "tiles", "cache", "rings"):
                assert whole[k] == plan[k], (what, k)
            check_launch(g, shape, whole, ref, mask, what + ("chain",))
            first = g.debug_tile_levels(lev[:1], its, cycles)
            check_launch(g, shape, first, ref[:1], mask, what + ("first level alone",))
            launches += 2
    # the production program still runs, and as before
    assert np.array_equal(g.pc_apply(x, pc), y0) and g.info()["program_fallbacks"] == 0
    print(f"{shape} waves {waves} depth {depth}: {plan['tiles']} tiles x {plan['threads']} threads, "
          f"cache {plan['cache']} rings {plan['rings']}, {launches} launches, {len(_REFS)} references held")
