"""kkt_set_option: every documented key and value is accepted; an unknown key, or a value
outside a key's list (include/kkt.h), is refused with an error that names the key and leaves
the handle's options as they were."""
import numpy as np
import pytest

import common
from control_amd._lib import KktError

pytestmark = pytest.mark.gpu

MASS = (20, 0.5, 2.0)
SCHUR = (12, 0.08, 2.1)   # beta = 1e-2 on the 10x10 mesh (test_gpu_parity.py)

SWITCHES = ("sell_sort", "shared_rows", "ragged_switch", "ragged_xcd", "apply_xcd", "pc_xcd",
            "interleave", "kernarg_ops", "no_graph", "persistent", "prog_steps", "tile_unfused",
            "lanes", "coarse_keep", "coarse_blocks", "stage_timers", "verbose", "stamps")
DOCUMENTED = ([(k, v) for k in SWITCHES for v in ("0", "1")]
              + [("sell_r", "1"), ("sell_r", "2")]
              + [("sell_sigma", str(v)) for v in range(1, 65)]
              + [("prog_mode", v) for v in ("auto", "tile", "dataflow", "flags", "w")]
              + [("prog_waves", str(v)) for v in range(1, 9)]
              + [("tile_depth", str(v)) for v in range(1, 17)]
              + [("tile_waves", str(v)) for v in range(1, 17)]
              + [("coarse_setup", v) for v in ("batched", "columns")]
              + [(k, v) for k in ("lane_chunks", "tile_poll_delay", "debug_drop_handoff")
                 for v in ("-1", "0", "3", "48")])
REJECTED = [("lanes", "2"), ("prog_mode", "tiles"), ("tile_waves", "17"), ("tile_depth", "x"),
            ("sell_r", "3"), ("persistent", "yes"), ("verbose", ""), ("prog_mode", "t"),
            ("prog_waves", "0"), ("tile_waves", "0"), ("tile_depth", "17"), ("sell_sigma", "65"),
            ("coarse_setup", "column"), ("lane_chunks", "4x"), ("tile_poll_delay", " 24"),
            ("debug_drop_handoff", "")]


def test_documented_values_are_accepted():
    p = common.heat_problem(n=6, n_t=4)
    g = common.gpu_system(p)
    for key, value in DOCUMENTED:
        g.set_option(key, value)


def test_rejected_values_name_the_key_and_change_nothing():
    p = common.heat_problem(n=10, n_t=10, CN=True, beta=1e-2)
    g = common.gpu_system(p, options={"persistent": "0"})
    with pytest.raises(KktError, match="unknown option: no_such_key"):
        g.set_option("no_such_key", "1")
    for key, value in REJECTED:
        with pytest.raises(KktError, match=f"option {key}: ") as e:
            g.set_option(key, value)
        assert e.value.code == -1                 # KKT_ERR_ARG

    # the handle solves as a fresh one with the same options does, and as the oracle does
    osys = common.oracle_system(p)
    m, nx = p["m"], p["sd"].n_dofs
    b = osys.mult(common.rng_vector(2 * m * nx)).reshape(2 * m, nx)
    sp = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 300,
          "relative_tolerance": 1e-9, "absolute_tolerance": 0.0,
          "monitor_convergence": False, "preconditioner": True}

    def solve(sys, pc):
        u0, u1 = np.zeros((m, nx)), np.zeros((m, nx))
        r = sys.solve(u0, u1, b[:m].copy(), b[m:].copy(), solver_parameters=sp, pc_fn=pc)
        return r, np.vstack([u0, u1])

    r, u = solve(g, common.gpu_pc(p, MASS, SCHUR))
    assert g.info()["sweep_form"] == 0            # still "persistent" = "0"
    r_fresh, u_fresh = solve(common.gpu_system(p, options={"persistent": "0"}),
                             common.gpu_pc(p, MASS, SCHUR))
    assert r.reason > 0 and r.its == r_fresh.its and np.array_equal(u, u_fresh)
    ro, uo = solve(osys, common.oracle_pc(p, MASS, SCHUR))
    assert ro.reason > 0 and common.rel_err(u, uo) < 1e-6
