"""Spectrum estimates of one preconditioner build, one matrix at a time against lock-step batches:
heat control on n^2 P1 x n_t levels (BE, every level its own operator K + 0.1 i M), Chebyshev
intervals estimated by the library (``ChebSpec(-1, 0, 0)``), no coarse space.  Per batch size and
repetition one JSON line with the build's wall time (first preconditioner application of a fresh
handle) and ``spectrum_stats()``; then one line of medians per batch size."""
import argparse, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
from control_amd import problems

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--n_t", type=int, default=64)
ap.add_argument("--batches", default="0,8,32,128")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

p = problems.heat_problem(n=a.n, n_t=a.n_t, beta=1e-4, time_dependent=True)
batches = [int(b) for b in a.batches.split(",")]
runs = {b: [] for b in batches}
for rep in range(-1, a.reps):                      # rep -1: warm process, not recorded
    for b in batches:
        g = problems.gpu_system(p, options={"spectrum_batch": str(b)})
        x = problems.rng_vector(g.local_size)
        t0 = time.perf_counter()
        g.pc_apply(x, problems.gpu_pc(p, (20, 0.5, 2.0), (-1, 0.0, 0.0)))
        r = dict(build_s=round(time.perf_counter() - t0, 4), **g.spectrum_stats())
        g.close()
        if rep >= 0:
            runs[b].append(r)
            print(json.dumps(dict(spectrum_batch=b, rep=rep, n=a.n, n_t=a.n_t, **r)), flush=True)
for b in batches:
    med = {k: statistics.median(r[k] for r in runs[b]) for k in runs[b][0]}
    print(json.dumps(dict(spectrum_batch=b, median_of=a.reps, **med)), flush=True)
