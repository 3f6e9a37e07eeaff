"""Anderson acceleration of the device Picard loops on one GPU: plain against ``anderson`` in
1, 2, 3, 5, the depths taken in turn within one process (``profiles/anderson_picard.md``).

``--problem scalar``: reaction-diffusion control on ``unit_square_p2(n)`` x ``n_t`` levels, BE,
g(v) = 2 + 0.5 v^2 (the case of ``profiles/reaction_picard_p2.md``), non-linear rtol 1e-5 and 1e-9,
at most ``--its`` Picard iterations (absolute tolerance 0: the relative one decides).
``--problem ns``: Navier-Stokes control on ``rectangle_q2q1(n, n)`` x ``n_t``, nu = 1/100
(``profiles/ns_picard_q2q1.md``), rtol 1e-5.
``--problem kernels``: the mixer's three kernels alone on vectors of ``--len`` doubles, timed by
HIP events (option ``stage_timers``), with the bytes each must move and the fraction of
``--copy_rate`` (TB/s) that gives.

One JSON line per loop; ``--out FILE`` appends the rows as a Markdown table."""
import argparse, ctypes as C, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, R + "/tests")
import numpy as np
import scipy.sparse as sp

ap = argparse.ArgumentParser()
ap.add_argument("--problem", choices=("scalar", "ns", "kernels"), default="scalar")
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--n_t", type=int, default=32)
ap.add_argument("--its", type=int, default=30, help="max_non_linear_iter")
ap.add_argument("--rtols", default="1e-5,1e-9")
ap.add_argument("--depths", default="0,1,2,3,5")
ap.add_argument("--len", type=int, default=2 * 32 * 66049)
ap.add_argument("--copy_rate", type=float, default=6.3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
depths = [int(d) for d in a.depths.split(",")]
rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def scalar():
    from control_amd import fem
    from control_amd.control import GpuBackend, Instationary
    disc = fem.unit_square_p2(a.n)

    def v_d(X, t):
        return (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.exp(X[:, 0])

    def loop(depth, rtol, its):
        ctl = Instationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d,
                           beta=1.0e-4, CN=False, n_t=a.n_t, time_interval=(0.0, 2.0))
        t0 = time.perf_counter()
        norms = ctl.non_linear_solve(max_non_linear_iter=its, relative_non_linear_tol=rtol,
                                     absolute_non_linear_tol=0.0,
                                     lambda_v_bounds=(0.3924, 2.0598), backend=GpuBackend(),
                                     Multigrid=False, device=True, anderson=depth)
        t1 = time.perf_counter()
        info = ctl.non_linear_info
        return dict(problem="scalar", n=a.n, n_t=a.n_t, rtol=rtol, anderson=depth,
                    picard_iterations=len(norms) - 1, converged=bool(norms[-1] <= rtol * norms[0]),
                    last_over_first=norms[-1] / norms[0],
                    linear_iterations=info["linear_iterations"], total_s=round(t1 - t0, 3),
                    history_bytes=(2 * depth + 1) * 8 * 2 * a.n_t * disc.n_dofs if depth else 0,
                    mixer=info.get("anderson"))
    loop(0, 1.0e-5, 1)                           # warm-up
    for rtol in [float(x) for x in a.rtols.split(",")]:
        for depth in depths:
            emit(loop(depth, rtol, a.its))


def ns():
    import common
    from control_amd import fem, picard
    pb = common.navier_stokes_problem(n=1, n_t=a.n_t, nu=1.0 / 100.0)
    th = fem.rectangle_q2q1(a.n, a.n, 2.0, 2.0)
    X, Y = th.coords_v[:, 0], th.coords_v[:, 1]
    shape = np.concatenate([np.sin(0.5 * np.pi * X) ** 2 * np.sin(np.pi * Y),
                            -np.sin(np.pi * X) * np.sin(0.5 * np.pi * Y) ** 2])
    v_d = np.stack([np.cos(0.5 * np.pi * i * pb.tau) * shape for i in range(a.n_t)])
    pb = picard.NavierStokesControl(disc=th, nu=1.0 / 100.0, beta=pb.beta, n_t=a.n_t, T=pb.T,
                                    v_d=v_d, f=np.zeros((a.n_t, th.n_v)), CN=False)
    sp_ = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)
    n_local = 2 * a.n_t * (th.n_v + th.n_p)
    for rtol in [float(x) for x in a.rtols.split(",")]:
        for depth in depths:
            ls = picard.GpuLinearSolver(pb, solver_parameters=sp_, Multigrid=False,
                                        relinearise="device", mass=(20, 0.25, 1.5625),
                                        mp=(20, 0.25, 2.25))
            t0 = time.perf_counter()
            out = picard.incompressible_non_linear_solve(
                pb, ls, max_non_linear_iter=a.its, relative_non_linear_tol=rtol,
                absolute_non_linear_tol=0.0, device=True,
                print_error_non_linear=False, anderson=depth)
            t1 = time.perf_counter()
            emit(dict(problem="ns", n=a.n, n_t=a.n_t, rtol=rtol, anderson=depth,
                      picard_iterations=len(out["norms"]) - 1, converged=out["converged"],
                      last_over_first=out["norms"][-1] / out["norms"][0],
                      linear_iterations=out["linear_iterations"], total_s=round(t1 - t0, 3),
                      solve_s=[round(e - s, 3) for s, e in ls.solve_times],
                      history_bytes=(2 * depth + 1) * 8 * n_local if depth else 0,
                      mixer=out.get("anderson")))
            del ls


def kernels():
    from control_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0
    assert lib.kkt_set_option(h, b"stage_timers", b"1") == 0
    nx = a.len // 2
    assert lib.kkt_set_layout(h, 1, 1, nx, a.len - nx, 0, -1, -1) == 0
    for q, n in ((0, nx), (3, a.len - nx)):
        A = sp.identity(n, format="csr")
        ip, ix, va = _lib.i32(A.indptr), _lib.i32(A.indices), _lib.f64(A.data)
        assert lib.kkt_add_block(h, q, 0, 0, n, n, ip[1], ix[1], va[1], -1) == 0
    assert lib.kkt_finalize(h) == 0
    n = lib.kkt_local_size(h)
    d_u = C.c_void_p()
    assert lib.kkt_vec_alloc(h, C.byref(d_u)) == 0
    rng = np.random.default_rng(7)
    for depth in [d for d in depths if d]:
        assert lib.kkt_anderson_set(h, depth, 1.0, 1.0e7) == 0
        times = []
        for k in range(depth + 6):
            f = np.ascontiguousarray(0.7 ** k * rng.standard_normal(n))
            assert lib.kkt_vec_upload(h, d_u, f.ctypes.data_as(_lib.c_f64p)) == 0
            info = _lib.AndersonInfo()
            assert lib.kkt_anderson_step(h, d_u, C.byref(info)) == 0
            if info.columns == depth:
                times.append((info.push_ms, info.gram_ms, info.mix_ms))
        ms = np.median(np.array(times), axis=0)
        moved = np.array([4, depth + 1, 2 * depth + 3]) * 8.0 * n      # push, gram, mix
        emit(dict(problem="kernels", len=n, anderson=depth, calls=len(times),
                  push_ms=round(ms[0], 4), gram_ms=round(ms[1], 4), mix_ms=round(ms[2], 4),
                  push_bytes=int(moved[0]), gram_bytes=int(moved[1]), mix_bytes=int(moved[2]),
                  fraction_of_copy_rate=[round(float(b / (t * 1e-3) / (a.copy_rate * 1e12)), 3)
                                         for b, t in zip(moved, ms)],
                  history_bytes=(2 * depth + 1) * 8 * n))
    lib.kkt_vec_free(h, d_u)
    lib.kkt_destroy(h)


{"scalar": scalar, "ns": ns, "kernels": kernels}[a.problem]()
if a.out and rows:
    keys = [k for k in rows[0] if k not in ("mixer", "solve_s", "problem")]
    with open(a.out, "a") as fh:
        fh.write("\n| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
        for r in rows:
            fh.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
