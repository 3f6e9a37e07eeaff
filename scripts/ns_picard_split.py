"""Navier-Stokes control at BASELINE configs[4] size (P2-P1 128 x 128, n_t = 64, nu = 1/100,
Multigrid) on one GPU: wall time of a Picard iteration outside the linearised solve, host
re-linearisation against the device path.  One JSON line per path.

``--element q2q1 --multigrid 0``: the same problem on ``fem.rectangle_q2q1`` with plain sweeps and
the reference's Q2 / Q1 mass intervals (``profiles/ns_picard_q2q1.md``).  ``--split_pc 1`` forces
the preconditioner's set-up or rebuild in front of every solve by one preconditioner application
and reports it on its own (``pc_setup_s``, with the spectrum estimates' share as the library
reports it); it is then part of "outside the solve"."""
import argparse, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, R + "/tests")
import numpy as np
import common
from control_amd import fem, multiblock, picard

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--n_t", type=int, default=64)
ap.add_argument("--nu", type=float, default=1.0 / 100.0)
ap.add_argument("--its", type=int, default=2, help="Picard iterations")
ap.add_argument("--paths", default="device,host")
ap.add_argument("--build", default="host", help="first build of the device path: host | device")
ap.add_argument("--element", default="p2p1", choices=["p2p1", "q2q1"])
ap.add_argument("--multigrid", type=int, default=1, help="1: two-grid sub-solves")
ap.add_argument("--split_pc", type=int, default=0)
a = ap.parse_args()
pb = common.navier_stokes_problem(n=a.n if a.element == "p2p1" else 1, n_t=a.n_t, nu=a.nu)
specs = {}
if a.element == "q2q1":      # the same data on the quadrilateral mesh
    th = fem.rectangle_q2q1(a.n, a.n, 2.0, 2.0)
    X, Y = th.coords_v[:, 0], th.coords_v[:, 1]
    shape = np.concatenate([np.sin(0.5 * np.pi * X) ** 2 * np.sin(np.pi * Y),
                            -np.sin(np.pi * X) * np.sin(0.5 * np.pi * Y) ** 2])
    v_d = np.stack([np.cos(0.5 * np.pi * i * pb.tau) * shape for i in range(a.n_t)])
    pb = picard.NavierStokesControl(disc=th, nu=a.nu, beta=pb.beta, n_t=a.n_t, T=pb.T, v_d=v_d,
                                    f=np.zeros((a.n_t, th.n_v)), CN=False)
    specs = dict(mass=(20, 0.25, 1.5625), mp=(20, 0.25, 2.25))
pc_setup = []                # (seconds, spectrum estimates ms) in front of every solve


def _forced(method):
    def solve(self, *args, **kw):
        t = time.perf_counter()
        self.pc_apply(np.zeros(self.local_size), kw["pc_fn"])    # set-up or rebuild, then a sync
        pc_setup.append((time.perf_counter() - t, kw["pc_fn"].inner.spectrum_stats()["ms"]))
        return method(self, *args, **kw)
    return solve


if a.split_pc:
    multiblock.MultiBlockSystem.solve = _forced(multiblock.MultiBlockSystem.solve)
    multiblock.MultiBlockSystem.solve_device = _forced(multiblock.MultiBlockSystem.solve_device)
sp = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)
for path in a.paths.split(","):
    kw = dict(build=a.build) if path == "device" else {}
    ls = picard.GpuLinearSolver(pb, solver_parameters=sp, Multigrid=bool(a.multigrid),
                                relinearise=path, **specs, **kw)
    pc_setup.clear()
    t0 = time.perf_counter()
    out = picard.incompressible_non_linear_solve(pb, ls, max_non_linear_iter=a.its,
                                                 relative_non_linear_tol=1e-12,
                                                 device=path == "device",
                                                 print_error_non_linear=False)
    t1 = time.perf_counter()
    st = ls.solve_times
    # between two solves: update, residual, re-assembly and re-upload of the blocks
    between = [st[k][0] - st[k - 1][1] for k in range(1, len(st))]
    print(json.dumps(dict(path=path, build=kw.get("build", "host"), element=a.element,
                          multigrid=a.multigrid, n=a.n, n_t=a.n_t, nu=a.nu,
                          n_v=pb.disc.n_v, n_p=pb.disc.n_p, total_s=round(t1 - t0, 3),
                          pc_setup_s=[round(x[0], 4) for x in pc_setup],
                          spectrum_ms=[round(x[1], 1) for x in pc_setup],
                          before_first_solve_s=round(st[0][0] - t0, 3),
                          outside_solve_s=[round(x, 4) for x in between],
                          after_last_solve_s=round(t1 - st[-1][1], 4),
                          solve_s=[round(e - s, 3) for s, e in st],
                          linear_iterations=out["linear_iterations"],
                          norms=out["norms"])), flush=True)
    del ls
