"""Stationary reaction-diffusion control (P1, g(v) = 2 + 0.5 v^2, Picard) on one GPU: wall time of a
Picard iteration outside the linearised solve, the host loop of ``Stationary.non_linear_solve``
against ``non_linear_solve(device=True)``, on ``unit_square_p1(n)`` (``--mesh square``, the record
of ``profiles/stationary_picard.md`` is ``--n 1024``: 1 050 625 nodes) or ``box_p1(n, n, n)``
(``--mesh cube``).  Both paths run in one process, alternating, after one warm-up iteration each.
One JSON line per loop.

"Outside the solve" is what lies between the end of one linearised solve and the start of the
next, by a host clock around work that ends in a synchronise: update, assembly, residual, blocks
and system construction (host) or composition (device), and the preconditioner's set-up or
rebuild (``pc_setup_s``; of it ``spectrum_ms`` for the sub-solve spectrum estimates and
``coarse_ms`` for the coarse set-up, as the library reports them) -- which both paths pay, would
otherwise do inside the solve call, and which is therefore forced here, in front of the solve, by
one preconditioner application."""
import argparse, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
from control_amd import fem, multiblock
from control_amd.control import GpuBackend, Stationary

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", choices=("square", "cube"), default="square")
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--beta", type=float, default=1.0e-2)
ap.add_argument("--amplitude", type=float, default=8.0, help="of the desired state")
ap.add_argument("--its", type=int, default=6, help="max_non_linear_iter")
ap.add_argument("--rtol", type=float, default=1.0e-10)
ap.add_argument("--repeats", type=int, default=1, help="measured loops per path")
ap.add_argument("--multigrid", type=int, default=0,
                help="1: two-grid sub-solves (the 33^2 / 9^3 coarse space is too coarse for GMRES(10) "
                     "to converge in 50 iterations on the 1024^2 mesh)")
ap.add_argument("--max_linear", type=int, default=200, help="GMRES(10) iterations per solve")
a = ap.parse_args()

t_mesh = time.perf_counter()
disc = fem.box_p1(a.n, a.n, a.n) if a.mesh == "cube" else fem.unit_square_p1(a.n)
term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
t_mesh = time.perf_counter() - t_mesh
# the interval of the mass solves: Wathen's bounds for P1 triangles / P1 tetrahedra
MASS = (0.5, 2.5) if a.mesh == "cube" else None


def v_d(X):
    return a.amplitude * np.prod(np.sin(np.pi * X), axis=1) * np.exp(X[:, 0])


def control():
    return Stationary(disc, term, desired_state=v_d, beta=a.beta)


# (solve start, solve end, preconditioner set-up in front of it) of every linearised solve of the
# running loop
marks = []


def _timed(method):
    def solve(self, *args, **kw):
        tp = time.perf_counter()
        self._set_pc(kw.get("pc_fn"))
        x = np.zeros(self.local_size)
        self.pc_apply(x, kw.get("pc_fn"))        # set-up or rebuild happens here, then a sync
        t0 = time.perf_counter()
        split = (self.spectrum_stats()["ms"], self.coarse_setup_stats()["ms"])
        out = method(self, *args, **kw)          # returns after the host has read the result
        marks.append((t0, time.perf_counter(), t0 - tp) + split + (out.getIterationNumber(),))
        return out
    return solve


multiblock.MultiBlockSystem.solve = _timed(multiblock.MultiBlockSystem.solve)
multiblock.MultiBlockSystem.solve_device = _timed(multiblock.MultiBlockSystem.solve_device)


def loop(device, its):
    ctl = control()
    marks.clear()
    t0 = time.perf_counter()
    sp = {"linear_solver": "gmres", "gmres_restart": 10, "maximum_iterations": a.max_linear,
          "relative_tolerance": 1.0e-6, "absolute_tolerance": 0.0, "monitor_convergence": False}
    norms = ctl.non_linear_solve(max_non_linear_iter=its, relative_non_linear_tol=a.rtol,
                                 absolute_non_linear_tol=0.0, lambda_v_bounds=MASS,
                                 solver_parameters=sp,
                                 backend=GpuBackend(), Multigrid=bool(a.multigrid), device=device)
    t1 = time.perf_counter()
    outside = [marks[k][0] - marks[k - 1][1] for k in range(1, len(marks))]
    return dict(path="device" if device else "host", mesh=a.mesh, n=a.n, nodes=disc.n_dofs,
                cells=len(disc.cells), mesh_and_term_s=round(t_mesh, 2),
                total_s=round(t1 - t0, 3),
                picard_iterations=len(norms) - 1,
                before_first_solve_s=round(marks[0][0] - t0, 3),
                outside_solve_s=[round(x, 4) for x in outside],
                outside_solve_median_s=round(statistics.median(outside), 4) if outside else None,
                after_last_solve_s=round(t1 - marks[-1][1], 4),
                pc_setup_s=[round(m[2], 4) for m in marks],
                spectrum_ms=[round(m[3], 1) for m in marks],
                coarse_ms=[round(m[4], 1) for m in marks],
                solve_s=[round(m[1] - m[0], 3) for m in marks],
                linear_iterations=[m[5] for m in marks],
                norms=norms)


for device in (False, True):                     # warm-up: one iteration each
    loop(device, 1)
print(f"warm: {disc.n_dofs} nodes, {len(disc.cells)} cells", file=sys.stderr, flush=True)
for _ in range(a.repeats):
    for device in (False, True):
        print(json.dumps(loop(device, a.its)), flush=True)
