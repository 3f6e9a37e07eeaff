"""`bench.py --dump-outputs DIR`: what the files hold, their size bound, and that the sample of a
large iterate is the same from run to run (no GPU: the writer is called with host arrays)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_iterate_written_whole(tmp_path):
    u = np.random.default_rng(1).standard_normal(10_000)
    bench.dump_outputs(str(tmp_path), 0, 1, u, 7, 0.25)
    got = _read(tmp_path)
    assert set(got) == {"u", "u_block_norms", "residual_norm", "iterations"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["u"], u)
    assert got["iterations"].tolist() == [7.0] and got["residual_norm"].tolist() == [0.25]
    assert got["u_block_norms"].shape == (4096,)
    assert np.isclose(np.sum(got["u_block_norms"] ** 2), np.sum(u ** 2))


def test_large_iterate_sampled_within_budget_and_reproducible(tmp_path):
    # the size of the default heat2d iterate (2 n_t 257^2): 67.6 MB of float64 in full
    n = 2 * 64 * 257 ** 2
    u = np.arange(n, dtype=np.float64) * 0.5
    runs = []
    for r in ("a", "b"):
        d = tmp_path / r
        bench.dump_outputs(str(d), 0, 1, u, 50, 1.0)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
        runs.append(_read(d))
    a, b = runs
    assert "u" not in a and a["u_sample"].size == bench.DUMP_SAMPLE < n // 2
    idx = a["u_sample_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["u_sample"], u[idx])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_ranks_write_their_own_shards(tmp_path):
    u = np.ones(100)
    for r in range(2):
        bench.dump_outputs(str(tmp_path), r, 2, u * (r + 1), 3, 0.5)
    got = _read(tmp_path)
    assert np.array_equal(got["u.rank1"], 2 * u) and np.array_equal(got["u.rank0"], u)


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr
