"""The batched mass solves on tiles where a workgroup serves several level groups, and the
tile-order copy of the matrix values the tile kernel reads (``mass_tile_kernels.hip``).  Run with
-m gpu on an MI355X.

The kernel reads its tile's global rows once per launch into LDS and uses that copy for the loads
and stores of every level group; a group's record (right-hand sides, outputs, factors) comes by
scalar loads per group.  A problem of test size has one level group per workgroup by default, so
the cases set ``mass_tile_levels``: a workgroup then serves ceil(levels / 4) groups, g,
g + grid_y, ... of the ceil(m / 4) groups of a solve on m levels.  Per (row, level) the kernel
performs the fma chain of the single-step interleaved kernel, so every case equals ``mass_tiles=0``
(one launch per step) bit for bit.

A kernel that fetched a workgroup's next level group under the steps of the current one was tried
with this change and not kept: profiles/mass_tile_pipe.md.
"""
import ctypes as C

import numpy as np
import pytest

import common
from test_gpu_mass_tiles import (ONE_TILE, SCHUR, TILE_CHEB, apply, check_launches, degrees, problem)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [6, 10, 14, 16])   # 6, 10, 14: the last group has fewer than four levels
@pytest.mark.parametrize("space", ["fd5", "p1", "q1"])
def test_one_two_and_three_groups_per_workgroup(space, n_t, CN):
    """41^2 nodes in tiles of 64 and 200 own rows, 4, 8 and 12 levels per workgroup.  With three
    groups of a solve and two per workgroup (n_t 10, 8 levels) the workgroups of a tile run two
    groups and one; with four groups and three per workgroup (n_t 14 and 16, 12 levels) grid_y is 2
    and both run two."""
    p = problem(space, 40, n_t, CN)
    K, its = 3, 7
    y0, f0, x, _ = apply(p, its, {"mass_tiles": "0"})
    for rows in (64, 200):
        for levels in (4, 8, 12):
            y, forms, _, _ = apply(p, its, {"mass_tile_depth": str(K), "mass_tile_rows": str(rows),
                                            "mass_tile_levels": str(levels)}, x)
            bad = np.flatnonzero(y != y0)
            assert bad.size == 0, (space, n_t, CN, rows, levels, bad[:8])
            assert not np.signbit(y[y == 0.0]).any()            # Dirichlet rows: +0.0
            check_launches(forms, f0, its, K)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_every_depth_and_degree_with_two_groups_per_workgroup(K):
    """A last launch of one step, 0, 1 and 2 steps done in front of a launch (K = 1, 2), K larger
    than the solve: two groups per workgroup on three groups of a solve."""
    p = problem("p1", 40, 10, True)
    x = None
    for its in degrees(K):
        y0, f0, x, _ = apply(p, its, {"mass_tiles": "0"}, x)
        y, forms, _, _ = apply(p, its, {"mass_tile_depth": str(K), "mass_tile_rows": "200",
                                        "mass_tile_levels": "8"}, x)
        assert np.array_equal(y, y0), (K, its)
        if its >= 2:
            check_launches(forms, f0, its, K)
        else:
            # a one-step solve is no interleaved solve: nothing to replace
            assert not any(f["form"] == TILE_CHEB for f in forms)


@pytest.mark.parametrize("n,K", [(32, 1), (32, 2), (40, 3)])
def test_one_tile_holds_the_mesh(n, K):
    """33^2 and 41^2 nodes in one tile (961 and 1 521 free rows: the row table in LDS is as long
    as the iterates), two groups per workgroup."""
    p = problem("p1", n, 16, False)
    its = 5
    y0, f0, x, _ = apply(p, its, {"mass_tiles": "0"})
    y, forms, _, _ = apply(p, its, {"mass_tile_depth": str(K), "mass_tile_rows": str(ONE_TILE),
                                    "mass_tile_levels": "8"}, x)
    assert np.array_equal(y, y0)
    check_launches(forms, f0, its, K)


@pytest.mark.parametrize("no_graph", ["0", "1"])
def test_repeated_applications_through_the_graph(no_graph):
    """97^2 nodes x 12 levels, two groups per workgroup: a second application with another input,
    then 20 alternating ones, each bit for bit what single-step launches give."""
    p = problem("p1", 96, 12, False)
    its = 10
    g0 = common.gpu_system(p, options={"persistent": "0"})
    g1 = common.gpu_system(p, options={"no_graph": no_graph, "mass_tile_depth": "4",
                                       "mass_tile_rows": "512", "mass_tile_levels": "8"})
    pc0 = common.gpu_pc(p, (its, 0.5, 2.0), SCHUR)
    pc1 = common.gpu_pc(p, (its, 0.5, 2.0), SCHUR)
    xa, xb = common.rng_vector(g0.local_size), 3.0 * common.rng_vector(g0.local_size)[::-1].copy()
    ya, yb = g0.pc_apply(xa, pc0), g0.pc_apply(xb, pc0)
    assert not np.array_equal(ya, yb)
    assert np.array_equal(g1.pc_apply(xa, pc1), ya)
    assert np.array_equal(g1.pc_apply(xb, pc1), yb)
    tiles = [f for f in g1.pc_forms() if f["form"] == TILE_CHEB]
    assert tiles and [f["count"] for f in tiles[:3]] == [4, 4, 2]
    for k in range(20):
        x, y = (xa, ya) if k % 2 else (xb, yb)
        assert np.array_equal(g1.pc_apply(x, pc1), y), k
    assert g1.info()["program_fallbacks"] == 0


@pytest.mark.parametrize("rows", [200, ONE_TILE])
def test_tile_order_copy_of_the_matrix_values(rows):
    """What the kernel reads instead of vals[gpos]: the same numbers, +0.0 in the padding."""
    p = problem("p1", 40, 8, False)
    _, forms, _, g = apply(p, 6, {"mass_tile_depth": "3", "mass_tile_rows": str(rows)})
    assert any(f["form"] == TILE_CHEB for f in forms)
    hook = g._lib.kkt_debug_mass_tile_values
    n, nv = C.c_int64(0), C.c_int64(0)
    assert hook(g._h, C.byref(n), C.byref(nv), None, None, None) == 0
    copy, gpos, vals = np.full(n.value, np.nan), np.zeros(n.value, dtype=np.int32), np.zeros(nv.value)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert hook(g._h, None, None, copy.ctypes.data_as(f64), gpos.ctypes.data_as(i32),
                vals.ctypes.data_as(f64)) == 0
    assert n.value > 0 and (gpos < 0).any() and (gpos >= 0).any() and gpos.max() < nv.value
    expect = np.where(gpos >= 0, vals[np.maximum(gpos, 0)], 0.0)
    assert np.array_equal(copy.view(np.uint64), expect.view(np.uint64))
    assert not np.signbit(copy[gpos < 0]).any()


def test_the_hook_reports_a_handle_without_the_form():
    p = problem("p1", 40, 8, False)
    _, forms, _, g = apply(p, 6, {"mass_tiles": "0"})
    assert not any(f["form"] == TILE_CHEB for f in forms)
    n = C.c_int64(0)
    assert g._lib.kkt_debug_mass_tile_values(g._h, C.byref(n), None, None, None, None) != 0
