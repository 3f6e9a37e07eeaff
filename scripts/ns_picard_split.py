"""Navier-Stokes control at BASELINE configs[4] size (P2-P1 128 x 128, n_t = 64, nu = 1/100,
Multigrid) on one GPU: wall time of a Picard iteration outside the linearised solve, host
re-linearisation against the device path.  One JSON line per path."""
import argparse, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, R + "/tests")
import common
from control_amd import picard

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--n_t", type=int, default=64)
ap.add_argument("--nu", type=float, default=1.0 / 100.0)
ap.add_argument("--its", type=int, default=2, help="Picard iterations")
ap.add_argument("--paths", default="device,host")
ap.add_argument("--build", default="host", help="first build of the device path: host | device")
a = ap.parse_args()
pb = common.navier_stokes_problem(n=a.n, n_t=a.n_t, nu=a.nu)
sp = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)
for path in a.paths.split(","):
    kw = dict(build=a.build) if path == "device" else {}
    ls = picard.GpuLinearSolver(pb, solver_parameters=sp, Multigrid=True, relinearise=path, **kw)
    t0 = time.perf_counter()
    out = picard.incompressible_non_linear_solve(pb, ls, max_non_linear_iter=a.its,
                                                 relative_non_linear_tol=1e-12,
                                                 device=path == "device",
                                                 print_error_non_linear=False)
    t1 = time.perf_counter()
    st = ls.solve_times
    # between two solves: update, residual, re-assembly and re-upload of the blocks
    between = [st[k][0] - st[k - 1][1] for k in range(1, len(st))]
    print(json.dumps(dict(path=path, build=kw.get("build", "host"), n=a.n, n_t=a.n_t, nu=a.nu, total_s=round(t1 - t0, 3),
                          before_first_solve_s=round(st[0][0] - t0, 3),
                          outside_solve_s=[round(x, 4) for x in between],
                          after_last_solve_s=round(t1 - st[-1][1], 4),
                          solve_s=[round(e - s, 3) for s, e in st],
                          linear_iterations=out["linear_iterations"],
                          norms=out["norms"])), flush=True)
    del ls
