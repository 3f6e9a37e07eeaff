"""Stationary Navier-Stokes control (P2-P1, Picard) on one GPU: wall time of a Picard iteration
outside the linearised solve, the host loop of ``Stationary.incompressible_non_linear_solve``
against ``incompressible_non_linear_solve(device=True)``, on ``rectangle_p2p1(n, n, 2, 2)`` (the
record of ``profiles/stationary_ns_picard.md`` is ``--n 128``, the spatial size of BASELINE
configs[2], and ``--n 256``).  Both paths run in one process, alternating, after one warm-up
iteration each.  One JSON line per loop.

"Outside the solve" is what lies between the end of one linearised solve and the start of the
next, by a host clock around work that ends in a synchronise, split into

* ``assembly_s``: ``D_v`` / ``D_p`` (host: ``construct_D_v`` twice -- once for the residual, once
  for the solve -- and ``term.pressure``; device: the element and gather kernels);
* ``residual_s``: the rows and their norm (device; on the host path the residual is what is left
  of the interval after the named pieces, ``other_s``, with the update and the field copies);
* ``composition_s``: the blocks (host: ``stationary_incompressible_blocks`` and
  ``stationary_blocks``; device: the composition kernels on the three handles);
* ``systems_s``: ``MultiBlockSystem`` construction (host: three per iteration; device: none);
* ``pc_setup_s``: the preconditioner's set-up (host: from nothing) or rebuild (device) -- which
  both paths would otherwise do inside the solve call and which is therefore forced here, in
  front of the solve, by one preconditioner application; of it ``spectrum_ms`` / ``coarse_ms``
  as the library reports them for the velocity sub-solves (the inner handle)."""
import argparse, collections, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
from control_amd import control, fem, multiblock, relinearise
from control_amd.control import GpuBackend, Stationary

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--nu", type=float, default=1.0)
ap.add_argument("--beta", type=float, default=1.0e-2)
ap.add_argument("--its", type=int, default=4, help="max_non_linear_iter")
ap.add_argument("--rtol", type=float, default=1.0e-12)
ap.add_argument("--repeats", type=int, default=2, help="measured loops per path")
ap.add_argument("--multigrid", type=int, default=1, help="1: two-grid sub-solves")
ap.add_argument("--max_linear", type=int, default=200, help="FGMRES(10) iterations per solve")
ap.add_argument("--perturb_ulps", type=int, default=0,
                help="k > 0: one more host loop with D_v and D_p scaled by 1 + k 2^-52 -- how far "
                     "a change in the last place of the operator moves the loop's iteration counts")
ap.add_argument("--element", default="p2p1", choices=["p2p1", "q2q1"],
                help="q2q1: fem.rectangle_q2q1 with the reference's Q2 / Q1 mass intervals "
                     "(profiles/ns_picard_q2q1.md)")
a = ap.parse_args()

t_mesh = time.perf_counter()
th = (fem.rectangle_q2q1 if a.element == "q2q1" else fem.rectangle_p2p1)(a.n, a.n, 2.0, 2.0)
bounds = (dict(lambda_v_bounds=(0.25, 1.5625), lambda_p_bounds=(0.25, 2.25))
          if a.element == "q2q1" else {})
term = fem.ConvectionTerm(th, a.nu)
t_mesh = time.perf_counter() - t_mesh


def v_d(X):
    return np.concatenate([np.sin(0.5 * np.pi * X[:, 0]) ** 2 * np.sin(np.pi * X[:, 1]),
                           -np.sin(np.pi * X[:, 0]) * np.sin(0.5 * np.pi * X[:, 1]) ** 2])


acc = collections.defaultdict(float)     # seconds per piece since the last solve ended
# (solve start, solve end, the pieces in front of it, spectrum ms, coarse ms, linear iterations)
marks = []


def _sync(system):
    system._ck(system._lib.kkt_sync(system.handle))


def _piece(name, fn, sync=None):
    def timed(*args, **kw):
        t = time.perf_counter()
        out = fn(*args, **kw)
        if sync is not None:
            sync(*args)
        acc[name] += time.perf_counter() - t
        return out
    return timed


def _timed_solve(method):
    def solve(self, *args, **kw):
        pc = kw.get("pc_fn")
        tp = time.perf_counter()
        self.pc_apply(np.zeros(self.local_size), pc)   # set-up or rebuild happens here, then a sync
        t0 = time.perf_counter()
        pieces = dict(acc, pc_setup=t0 - tp)
        stats = (pc.inner.spectrum_stats()["ms"], pc.inner.coarse_setup_stats()["ms"])
        out = method(self, *args, **kw)          # returns after the host has read the result
        marks.append((t0, time.perf_counter(), pieces) + stats + (out.getIterationNumber(),))
        acc.clear()
        return out
    return solve


scale = [1.0]                            # of the host path's D_v and D_p (--perturb_ulps)


def _scaled(fn):
    def operator(*args):
        A = fn(*args)
        A.data *= scale[0]
        return A
    return operator


fem.ConvectionTerm.__call__ = _scaled(fem.ConvectionTerm.__call__)
fem.ConvectionTerm.pressure = _scaled(fem.ConvectionTerm.pressure)
# host path
Stationary.construct_D_v = _piece("assembly", Stationary.construct_D_v)
fem.ConvectionTerm.pressure = _piece("assembly", fem.ConvectionTerm.pressure)
control.stationary_incompressible_blocks = _piece("composition",
                                                  control.stationary_incompressible_blocks)
control.stationary_blocks = _piece("composition", control.stationary_blocks)
multiblock.MultiBlockSystem.__init__ = _piece("systems", multiblock.MultiBlockSystem.__init__)
# device path: every piece ends in a synchronise of the handle it ran on
D = relinearise.DeviceRelinearisation
D.assemble = _piece("assembly", D.assemble, lambda dev: _sync(dev.outer))
D.residual = _piece("residual", D.residual, lambda dev, *_: _sync(dev.outer))
D.update = _piece("update", D.update, lambda dev, *_: _sync(dev.outer))
D.relinearise = _piece("composition", D.relinearise, lambda dev, system, *_: _sync(system))
multiblock.MultiBlockSystem.solve = _timed_solve(multiblock.MultiBlockSystem.solve)
multiblock.MultiBlockSystem.solve_device = _timed_solve(multiblock.MultiBlockSystem.solve_device)


def loop(device, its):
    ctl = Stationary(th, term, desired_state=v_d, beta=a.beta)
    marks.clear()
    acc.clear()
    sp = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": a.max_linear,
          "relative_tolerance": 1.0e-6, "absolute_tolerance": 0.0, "monitor_convergence": False}
    t0 = time.perf_counter()
    norms = ctl.incompressible_non_linear_solve(
        solver_parameters=sp, max_non_linear_iter=its, relative_non_linear_tol=a.rtol,
        absolute_non_linear_tol=0.0, backend=GpuBackend(), Multigrid=bool(a.multigrid),
        device=device, **bounds)
    t1 = time.perf_counter()
    between = range(1, len(marks))
    outside = [marks[k][0] - marks[k - 1][1] for k in between]
    names = ("assembly", "residual", "update", "composition", "systems", "pc_setup")
    split = {n + "_s": [round(marks[k][2].get(n, 0.0), 4) for k in between] for n in names}
    split["other_s"] = [round(outside[k - 1] - sum(marks[k][2].values()), 4) for k in between]
    return dict(path="device" if device else "host", element=a.element, operator_scale=scale[0], n=a.n, n_v=th.n_v, n_p=th.n_p,
                multigrid=a.multigrid, nu=a.nu, mesh_and_term_s=round(t_mesh, 2),
                total_s=round(t1 - t0, 3), picard_iterations=len(norms) - 1,
                before_first_solve_s=round(marks[0][0] - t0, 3),
                outside_solve_s=[round(x, 4) for x in outside],
                outside_solve_median_s=round(statistics.median(outside), 4) if outside else None,
                **split,
                spectrum_ms=[round(m[3], 1) for m in marks],
                coarse_ms=[round(m[4], 1) for m in marks],
                solve_s=[round(m[1] - m[0], 3) for m in marks],
                linear_iterations=[m[5] for m in marks], norms=norms)


for device in (False, True):                     # warm-up: one iteration each
    loop(device, 1)
print(f"warm: n_v = {th.n_v}, n_p = {th.n_p}", file=sys.stderr, flush=True)
for _ in range(a.repeats):
    for device in (False, True):
        print(json.dumps(loop(device, a.its)), flush=True)
if a.perturb_ulps > 0:
    scale[0] = 1.0 + a.perturb_ulps * 2.0 ** -52
    print(json.dumps(loop(False, a.its)), flush=True)
