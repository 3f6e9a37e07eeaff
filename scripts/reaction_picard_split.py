"""Reaction-diffusion control (256^2 P1 x 64 levels, BE, g(v) = 2 + 0.5 v^2, beta = 1e-4, [0, 2]) on
one GPU -- or, with ``--mesh cube``, the same problem on P1 tetrahedra (``box_p1(n, n, n)``; the
record of ``profiles/reaction_picard_3d.md`` is ``--mesh cube --n 32 --n_t 32``) or, with
``--mesh p2``, on P2 triangles (``unit_square_p2(n)``; ``profiles/reaction_picard_p2.md`` is
``--mesh p2 --n 128 --n_t 32``) or, with ``--mesh q2``, on Q2 quadrilaterals
(``rectangle_q2(n, n)``; ``profiles/reaction_picard_q2.md`` is ``--mesh q2 --n 128 --n_t 32
--multigrid 0``) --: wall time of
a Picard iteration outside the linearised solve, the host loop against
``non_linear_solve(device=True)``.  Both paths run in one process, alternating, after one warm-up
iteration each.  One JSON line per loop.

"Outside the solve" is what lies between the end of one linearised solve and the start of the
next (``pc_setup_s``; of it ``spectrum_ms`` for the sub-solve spectrum estimates and ``coarse_ms``
for the coarse set-up, as the library reports them -- KKT_SPECTRUM_BATCH=0 measures the
one-matrix estimates), by a host clock around work that ends in a synchronise: update, assembly, residual, blocks
and system construction (host) or composition (device), and the preconditioner's set-up or
rebuild -- which both paths would otherwise do inside the solve call and which is therefore forced
here, in front of the solve, by one preconditioner application."""
import argparse, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
from control_amd import fem, multiblock
from control_amd.control import GpuBackend, Instationary

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", choices=("square", "cube", "p2", "q2"), default="square")
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--n_t", type=int, default=64)
ap.add_argument("--beta", type=float, default=1.0e-4)
ap.add_argument("--its", type=int, default=10, help="max_non_linear_iter")
ap.add_argument("--rtol", type=float, default=1.0e-5)
ap.add_argument("--repeats", type=int, default=1, help="measured loops per path")
ap.add_argument("--multigrid", type=int, default=1)
a = ap.parse_args()

disc = {"cube": lambda: fem.box_p1(a.n, a.n, a.n), "p2": lambda: fem.unit_square_p2(a.n),
        "q2": lambda: fem.rectangle_q2(a.n, a.n),
        "square": lambda: fem.unit_square_p1(a.n)}[a.mesh]()
# the interval of the mass solves: Wathen's bounds for P1 triangles / P1 tetrahedra, the
# reference's intervals for P2 triangles and for Q2
MASS = {"cube": (0.5, 2.5), "p2": (0.3924, 2.0598), "q2": (0.25, 1.5625),
        "square": None}[a.mesh]


def v_d(X, t):
    bump = np.prod(np.sin(np.pi * X), axis=1) if a.mesh == "cube" else (
        np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]))
    return (1.0 + t) * bump * np.exp(X[:, 0])


def control():
    return Instationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d,
                        beta=a.beta, CN=False, n_t=a.n_t, time_interval=(0.0, 2.0))


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
        marks.append((t0, time.perf_counter(), t0 - tp) + split)
        return out
    return solve


multiblock.MultiBlockSystem.solve = _timed(multiblock.MultiBlockSystem.solve)
multiblock.MultiBlockSystem.solve_device = _timed(multiblock.MultiBlockSystem.solve_device)


def loop(device, its):
    ctl = control()
    marks.clear()
    t0 = time.perf_counter()
    norms = ctl.non_linear_solve(max_non_linear_iter=its, relative_non_linear_tol=a.rtol,
                                 lambda_v_bounds=MASS,
                                 backend=GpuBackend(), Multigrid=bool(a.multigrid), device=device)
    t1 = time.perf_counter()
    outside = [marks[k][0] - marks[k - 1][1] for k in range(1, len(marks))]
    return dict(path="device" if device else "host", mesh=a.mesh, n=a.n, n_t=a.n_t,
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
                norms=norms)


for device in (False, True):                     # warm-up: one iteration each
    loop(device, 1)
for _ in range(a.repeats):
    for device in (False, True):
        print(json.dumps(loop(device, a.its)), flush=True)
