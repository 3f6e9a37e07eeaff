"""The batched mass solves as several Chebyshev steps per launch out of LDS
(``mass_tile_kernels.hip``, form 6 of ``pc_forms()``), run with -m gpu on an MI355X.

The form performs per (row, level) the fma chain of the single-step interleaved kernel, so every
case must equal ``mass_tiles=0`` and ``persistent=0`` bit for bit, whatever the tile size, the
steps per launch K and the degree of the solve -- K does not divide it, it is smaller than K, a
last launch of one step.  Each case reads back that the form ran, with ceil(its / K) launches per
solve whose step counts add up to the degree.  Chebyshev intervals are explicit.
"""
import numpy as np
import pytest

import common
import structures as st
from control_amd.blocks import instationary_blocks
from control_amd.fem import (SpatialDiscretisation, rectangle_p2p1, unit_cube_p1, unit_square_p1)

pytestmark = pytest.mark.gpu

INTERLEAVED, TILE_CHEB = 3, 6                     # pc_forms()["form"]
SCHUR = (6, 0.05, 2.1)
ONE_TILE = 65536                                  # own rows per tile: more than the mesh has


def spatial(space, n):
    if space == "fd5":
        # mass and level matrices share one structure: the lumped mass on the 5-point structure
        sd = st.fd5_square(n)
        M = sd.K.copy()
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        M.data[:] = np.where(M.indices == rows, sd.M.diagonal()[rows], 0.0)
        sd.M = M
        return sd
    if space == "q1":
        return st.q1_square(n)
    if space == "p2v":
        th = rectangle_p2p1(n, n, 1.0, 1.0)
        return SpatialDiscretisation(M=th.M_v, K=th.K_v, coords=np.vstack([th.coords_v] * 2),
                                     boundary=th.boundary_v, name="p2v")
    return {"p1": unit_square_p1, "p1_3d": unit_cube_p1}[space](n)


def problem(space, n, n_t, CN, beta=1e-2):
    sd = spatial(space, n)
    tau = 2.0 / (n_t - 1.0)
    b00, b01, b10, b11, m = instationary_blocks(sd.M, sd.K, tau, beta, n_t, CN, share=True)
    return dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=sd.boundary)


def apply(p, its, options, x=None):
    g = common.gpu_system(p, options=options)
    if x is None:
        x = common.rng_vector(g.local_size)
    y = g.pc_apply(x, common.gpu_pc(p, (its, 0.5, 2.0), SCHUR))
    assert g.info()["program_fallbacks"] == 0, options
    return y, g.pc_forms(), x, g


def degrees(K):
    return sorted({2, 3, K, K + 1, 2 * K - 1, 2 * K, 20})


def check_launches(forms, ref_forms, its, K):
    """Every run of `its` interleaved steps of the reference became ceil(its / K) launches."""
    tiles = [f for f in forms if f["form"] == TILE_CHEB]
    solves = sum(f["form"] == INTERLEAVED for f in ref_forms) // its
    assert solves >= 1 and not any(f["form"] == INTERLEAVED for f in forms)
    per = -(-its // K)
    assert len(tiles) == solves * per, (its, K, len(tiles), solves)
    counts = [f["count"] for f in tiles]
    one = [K] * (its // K) + ([its % K] if its % K else [])
    assert counts == one * solves, (its, K, counts)
    assert all(f["variant"] in (256, 512) and f["slots"] >= 1 for f in tiles)


# own rows per tile: several tiles with rings of the full depth (41^2 nodes: 1 521 free rows are 24
# tiles of 64, 8 of 200), and one tile that holds the whole mesh
ROWS = (64, 200, ONE_TILE)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [6, 16])      # 6: a level group with fewer than four levels
@pytest.mark.parametrize("space", ["fd5", "p1", "q1"])
def test_every_depth_and_degree_equals_single_step_launches(space, n_t, CN):
    p = problem(space, 40, n_t, CN)
    ref, x = {}, None
    case = 0
    for K in (1, 2, 3, 4, 5):
        for its in degrees(K):
            if its not in ref:
                y0, f0, x, _ = apply(p, its, {"mass_tiles": "0"}, x)
                y1, f1, _, _ = apply(p, its, {"persistent": "0"}, x)
                assert not any(f["form"] == TILE_CHEB for f in f0 + f1)
                assert np.array_equal(y0, y1)
                ref[its] = (y0, f0)
            rows = ROWS[case % len(ROWS)]
            case += 1
            y, forms, _, _ = apply(p, its, {"mass_tile_depth": str(K), "mass_tile_rows": str(rows)}, x)
            bad = np.flatnonzero(y != ref[its][0])
            assert bad.size == 0, (space, n_t, CN, K, its, rows, bad[:8])
            assert not np.signbit(y[y == 0.0]).any()            # Dirichlet rows: +0.0
            if its >= 2:
                check_launches(forms, ref[its][1], its, K)
            else:
                # a one-step solve is no interleaved solve: nothing to replace
                assert not any(f["form"] == TILE_CHEB for f in forms)


@pytest.mark.parametrize("space", ["fd5", "p1", "q1"])
def test_every_tile_size_at_every_depth(space):
    """The (tile size, K) pairs the rotation above leaves out, at one degree that K never divides
    evenly except K = 1."""
    p = problem(space, 40, 6, False)
    its = 7
    y0, f0, x, _ = apply(p, its, {"mass_tiles": "0"})
    for K in (1, 2, 3, 4, 5):
        for rows in ROWS:
            y, forms, _, _ = apply(p, its, {"mass_tile_depth": str(K), "mass_tile_rows": str(rows)}, x)
            assert np.array_equal(y, y0), (space, K, rows)
            check_launches(forms, f0, its, K)


@pytest.mark.parametrize("CN", [False, True])
def test_where_the_form_is_off_nothing_changes(CN):
    p = problem("p1", 40, 16, CN)
    its = 8
    on = {"mass_tile_depth": "3", "mass_tile_rows": "200"}
    y_on, forms, x, _ = apply(p, its, on)
    assert any(f["form"] == TILE_CHEB for f in forms)
    for off in ({"persistent": "0"}, {"lanes": "1"}, {"sell_r": "1"}, {"mass_tiles": "0"}):
        y, forms, _, _ = apply(p, its, {**on, **off}, x)
        assert not any(f["form"] == TILE_CHEB for f in forms), off
        assert np.array_equal(y, y_on), off


@pytest.mark.parametrize("no_graph", ["0", "1"])
def test_repeated_applications_through_the_graph(no_graph):
    """97^2 nodes x 8 levels: a second application with another input, then 20 repeated ones, each
    bit for bit what single-step launches give -- through the captured graph and without it."""
    p = problem("p1", 96, 8, False)
    its = 10
    g0 = common.gpu_system(p, options={"persistent": "0"})
    g1 = common.gpu_system(p, options={"no_graph": no_graph, "mass_tile_depth": "4",
                                       "mass_tile_rows": "512"})
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


@pytest.mark.parametrize("space,n", [("p1_3d", 8), ("p2v", 8)])
def test_widths_without_a_variant_keep_the_interleaved_form(space, n):
    p = problem(space, n, 8, False)
    its = 6
    y0, _, x, _ = apply(p, its, {"persistent": "0"})
    y, forms, _, _ = apply(p, its, {"mass_tile_depth": "2", "mass_tile_rows": "64"}, x)
    assert np.array_equal(y, y0)
    assert any(f["form"] == INTERLEAVED for f in forms)
    assert not any(f["form"] == TILE_CHEB for f in forms)
