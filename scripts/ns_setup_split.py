"""Navier-Stokes control at BASELINE configs[4] size (P2-P1 128 x 128, n_t = 64, nu = 1/100,
Multigrid) on one GPU: the set-up before the first linearised solve, itemised, for
``GpuLinearSolver(build="host")`` and ``build="device"``.  One JSON line per build and
repetition, then one line of medians per build.

Items (seconds; the library calls are timed where the Python mirror makes them):
host_assembly (pb.D_v / pb.D_p of every level), host_blocks
(instationary_incompressible_blocks), host_plan (RelinearisationPlan), upload (kkt_add_block and
kkt_add_block_structure, with the bytes they carry), finalize (kkt_finalize), plan_compose
(kkt_set_relinearisation, kkt_picard_state, kkt_relinearise_device), pc_setup (kkt_set_pc_*),
first_pc_apply (the preconditioner's lazy part) and other (the rest of the build call).
A commit without the ``build`` keyword measures the host build only."""
import argparse, gc, inspect, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, R + "/tests")
import numpy as np
import common
from control_amd import _lib, picard, relinearise

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--n_t", type=int, default=64)
ap.add_argument("--nu", type=float, default=1.0 / 100.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--builds", default="host,device")
a = ap.parse_args()

lib = _lib.load()
acc, seen = {}, set()
GROUP = {"kkt_add_block": "upload", "kkt_add_block_structure": "upload",
         "kkt_finalize": "finalize", "kkt_set_relinearisation": "plan_compose",
         "kkt_picard_state": "plan_compose", "kkt_relinearise_device": "plan_compose",
         "kkt_set_pc_schur": "pc_setup", "kkt_set_pc_stokes": "pc_setup"}


def timed(name, fn):
    def call(*args):
        t0 = time.perf_counter()
        rc = fn(*args)
        acc[GROUP[name]] = acc.get(GROUP[name], 0.0) + time.perf_counter() - t0
        if name.startswith("kkt_add_block"):
            # what crosses to the GPU: values of a block whose share id the handle has not seen,
            # index arrays once per handle and structure (the library keeps one copy of each)
            h, nrows, indptr = args[0].value, args[4], args[6]
            nnz = int(indptr[nrows])
            sid = args[9] if name == "kkt_add_block" else None
            if name == "kkt_add_block" and (sid < 0 or (h, sid) not in seen):
                seen.add((h, sid))
                acc["bytes_uploaded"] = acc.get("bytes_uploaded", 0) + 8 * nnz
            if (h, nrows, nnz) not in seen:
                seen.add((h, nrows, nnz))
                acc["bytes_uploaded"] = acc.get("bytes_uploaded", 0) + 4 * (nrows + 1) + 4 * nnz
        return rc
    return call


for name in GROUP:
    if hasattr(lib, name):
        setattr(lib, name, timed(name, getattr(lib, name)))
plan_init = relinearise.RelinearisationPlan.__init__


def timed_plan_init(self, pb):
    t0 = time.perf_counter()
    plan_init(self, pb)
    acc["host_plan"] = acc.get("host_plan", 0.0) + time.perf_counter() - t0


relinearise.RelinearisationPlan.__init__ = timed_plan_init
has_build = "build" in inspect.signature(picard.GpuLinearSolver.__init__).parameters
builds = [b for b in a.builds.split(",") if b == "host" or has_build]
sp = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)


def one(pb, build):
    """One set-up; returns its items."""
    acc.clear()
    seen.clear()
    n_t, th = pb.n_t, pb.disc
    m = n_t - 1 if pb.CN else n_t
    state = (pb.v_d.copy(), np.zeros((n_t, th.n_v)), np.zeros((m, th.n_p)),
             np.zeros((m, th.n_p)))
    kw = dict(build=build) if has_build else {}
    ls = picard.GpuLinearSolver(pb, solver_parameters=sp, Multigrid=True, relinearise="device",
                                **kw)
    t0 = time.perf_counter()
    if build == "host":
        D = [pb.D_v(x) for x in state[0]]
        Dp = [pb.D_p(x) for x in state[0]]
        t1 = time.perf_counter()
        bl = ls._blocks(D, Dp)
        t2 = time.perf_counter()
        ls._build(bl)
        acc["host_assembly"], acc["host_blocks"] = t1 - t0, t2 - t1
    else:
        ls._build_device(*state)
    ls.outer._set_pc(ls.pc)
    t3 = time.perf_counter()
    x = np.random.default_rng(common.SEED).standard_normal(ls.outer.local_size)
    ls.outer.pc_apply(x, ls.pc)
    t4 = time.perf_counter()
    out = {k: round(v, 4) if isinstance(v, float) else v for k, v in acc.items()}
    out["setup_s"] = round(t3 - t0, 4)
    out["first_pc_apply"] = round(t4 - t3, 4)
    out["other"] = round(t3 - t0 - sum(v for k, v in acc.items() if k != "bytes_uploaded"), 4)
    st = ls.inner.spectrum_stats()      # the velocity sub-solves' estimates (KKT_SPECTRUM_BATCH)
    out["spectrum_ms"], out["spectrum_batch_bytes"] = round(st["ms"], 1), st["batch_bytes"]
    out["coarse_ms"] = round(ls.inner.coarse_setup_stats()["ms"], 1)
    out["device_value_bytes"] = sum(s.info()["bytes_device_values"]
                                    for s in (ls.outer, ls.inner, ls.comm))
    del ls
    gc.collect()
    return out


one(common.navier_stokes_problem(n=8, n_t=4, nu=a.nu), builds[0])      # warm process
pb = common.navier_stokes_problem(n=a.n, n_t=a.n_t, nu=a.nu)
runs = {b: [] for b in builds}
for rep in range(a.reps):
    for b in builds:                      # both builds interleaved in one session
        r = one(pb, b)
        runs[b].append(r)
        print(json.dumps(dict(build=b, rep=rep, n=a.n, n_t=a.n_t, **r)), flush=True)
for b in builds:
    keys = sorted({k for r in runs[b] for k in r})
    med = {k: statistics.median(r.get(k, 0) for r in runs[b]) for k in keys}
    print(json.dumps(dict(build=b, median_of=a.reps, n=a.n, n_t=a.n_t, **med)), flush=True)
