"""Two-grid tile sweeps in the ring form (option "coarse_rings", kkt_info.sweep_coarse_rings): a
tile prolongs a coarse correction onto its ring rows itself instead of fetching them in a
hand-off after the correction.  A ring row's fma chain is its owner's, so the form with the
hand-off ("coarse_rings" = "0") is the reference, bit for bit; the oracle's restatement
(oracle.kkt_oracle.coarse_chebyshev) to the bar of tests/test_gpu_coarse.py.  The scheme itself
(credit, hand-off counts, no stale ring entry) is emulated on the CPU in
tests/test_tile_coarse_plan.py."""
import functools

import numpy as np
import pytest

import common
from control_amd.coarse import multilinear_coarse_space

pytestmark = pytest.mark.gpu

MASS = (20, 0.5, 2.0)
ITS = (4, 6, 8)


@functools.lru_cache(maxsize=None)
def _problem(CN):
    p = common.heat_problem(n=40, n_t=6, CN=CN, beta=1e-4)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=5)
    osys = common.oracle_system(p)
    return p, P, osys, common.rng_vector(osys.N)


@functools.lru_cache(maxsize=None)
def _oracle(CN, its, cycles):
    p, P, osys, x = _problem(CN)
    y = osys.pc_apply(common.oracle_pc(p, MASS, (its, 0.07, 2.1), coarse=(P, cycles)), x)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("cycles", [1, 2, 3])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_ring_form_equals_the_handoff_form_and_the_oracle(CN, cycles, depth):
    """41^2 rows in 52 tiles, sweep counts that the depth divides and that it does not (the
    hand-off in front of a later cycle's residual is today's in the first case, new in the
    second)."""
    p, P, _, x = _problem(CN)
    sys = {r: common.gpu_system(p, options={"prog_mode": "tile", "tile_depth": str(depth),
                                            "coarse_rings": r}) for r in ("1", "0")}
    for its in ITS:
        pc = {r: common.gpu_pc(p, MASS, (its, 0.07, 2.1), coarse=(P, cycles)) for r in sys}
        y = {r: sys[r].pc_apply(x, pc[r]) for r in sys}
        info = {r: sys[r].info() for r in sys}
        assert info["1"]["sweep_form"] == 3 and info["0"]["sweep_form"] == 3, (its, info)
        assert info["1"]["sweep_depth"] == depth
        assert info["1"]["sweep_coarse_rings"] == 1 and info["0"]["sweep_coarse_rings"] == 0
        # (41^2 in 52 tiles: the lists and the owned rows of the coarse inverse fit on chip)
        assert info["1"]["sweep_coarse_cache"] == 2 and info["0"]["sweep_coarse_cache"] == 2
        assert info["1"]["program_fallbacks"] == 0 and info["0"]["program_fallbacks"] == 0
        assert np.array_equal(y["1"], y["0"]), (its, common.rel_err(y["1"], y["0"]))
        assert common.rel_err(y["1"], _oracle(CN, its, cycles)) < 1e-10, its


@pytest.mark.parametrize("CN", [False, True])
def test_stokes_velocity_sub_solves_in_ring_form(CN):
    """The shape of tests/test_gpu_coarse.py::test_stokes_velocity_sub_solves_in_two_grid_form
    (vector P2, a copy of the coarse functions per component)."""
    p = common.stokes_problem(n=8, n_t=5 if CN else 4, CN=CN)
    th = p["th"]
    P = multilinear_coarse_space(np.vstack([th.coords_v, th.coords_v]), th.boundary_v, cells=4)
    specs = dict(common.STOKES_SPECS, schur=(6, 0.07, 2.2))
    y, rings, forms = {}, {}, {}
    for r in ("1", "0"):
        outer, gpc = common.stokes_gpu(p, specs, coarse=(P, 1), options={"coarse_rings": r})
        x = common.rng_vector(outer.info()["n_local"])
        y[r] = outer.pc_apply(x, gpc)
        inf = gpc.inner.info()
        rings[r], forms[r] = inf["sweep_coarse_rings"], inf["sweep_form"]
        assert inf["program_fallbacks"] == 0
        assert inf["sweep_coarse_cache"] == (2 if inf["sweep_form"] == 3 else 0), inf
    assert rings["0"] == 0
    assert forms["1"] == forms["0"]
    # the velocity block's rows of P have at most 4 entries and its lists fit on chip: wherever
    # the two-grid levels run as a tile program, they run in the ring form
    assert rings["1"] == (1 if forms["1"] == 3 else 0), (rings, forms)
    assert np.array_equal(y["1"], y["0"])


def test_ring_form_repeats_itself():
    """20 applications at 97^2 x 8, 2 cycles: each equals the first bit for bit, no fall-back."""
    p = common.heat_problem(n=96, n_t=8, beta=1e-4)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=12)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    g = common.gpu_system(p, options={"prog_mode": "tile"})
    pc = common.gpu_pc(p, MASS, (6, 0.07, 2.1), coarse=(P, 2))
    y0 = g.pc_apply(x, pc)
    assert g.info()["sweep_form"] == 3 and g.info()["sweep_coarse_rings"] == 1
    assert g.info()["sweep_coarse_cache"] == 2
    for _ in range(19):
        assert np.array_equal(g.pc_apply(x, pc), y0)
    assert g.info()["program_fallbacks"] == 0
