"""`bench.py` on one GPU: a plain run prints the headline line and nothing it does not need; --full
adds the side measurements around the same timed steps, which compute the same iterate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SIDE_LEGS = ("roofline", "roofline_sweeps", "stages", "cpu_baseline", "config4")


def _bench(*args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "4", "--warmup", "1"] + list(args),
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _dumped(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_and_full_heat_runs(tmp_path):
    # (the default 256^2 x 64 system: on small ones the SpMV streams from cache and its roofline
    # fraction is no fraction of the HBM peak; the 64^3 x 128 leg is left out)
    args = ["--cpu-its", "2", "--no-config4"]
    plain = _bench(*args, "--dump-outputs", str(tmp_path / "plain"))
    for k in HEADLINE:
        assert k in plain, k
    assert plain["steps"] == 4 and plain["warmup"] == 1 and plain["value"] > 0
    assert plain["unit"] == "Krylov iterations/s" and plain["higher_is_better"] is True
    assert abs(plain["ms_per_step"] - 1e3 / plain["value"]) < 1e-9 * plain["ms_per_step"]
    assert not set(SIDE_LEGS) & set(plain), sorted(plain)
    assert not {"time_to_solution", "pc_apply_ms", "kkt_apply_ms"} & set(plain["config"])
    assert plain["config"]["sweeps"]["program_fallbacks"] == 0

    full = _bench(*args, "--full", "--dump-outputs", str(tmp_path / "full"))
    assert full["metric"] == plain["metric"]
    assert full["config"]["workload"] == plain["config"]["workload"]
    assert 0 < full["roofline"]["frac"] <= 1 and full["stages"]["krylov_iteration_ms"]["sum"] > 0
    assert full["config"]["time_to_solution"]["converged"] and full["config"]["pc_apply_ms"] > 0
    assert full["cpu_baseline"]["value"] > 0 and "config4" not in full

    # the side legs do not touch the timed solve: same iterate, same residual
    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert sorted(a) == sorted(b)
    assert a["iterations"][0] == b["iterations"][0] == 4
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-10, atol=0, err_msg=k)


def test_plain_and_full_stokes_runs():
    small = ["--workload", "stokes2d", "--n", "16", "--n_t", "8"]
    plain = _bench(*small)
    for k in HEADLINE:
        assert k in plain, k
    assert not {"roofline", "stages"} & set(plain) and "time_to_solution" not in plain["config"]
    full = _bench(*small, "--full")
    assert full["config"]["time_to_solution"]["iterations"] > 0
    assert full["stages"]["krylov_iteration_ms"]["preconditioner"] > 0 and "roofline" in full
