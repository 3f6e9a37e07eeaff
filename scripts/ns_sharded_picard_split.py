"""Navier-Stokes control at BASELINE configs[4] size (P2-P1 128 x 128, n_t = 64, nu = 1/100,
Multigrid), time-sharded over --ranks processes that share ONE GPU (host-staged gloo transport):
wall time of a Picard iteration outside the linearised solve, the host-sharded loop (every rank
re-linearises the whole iterate on the host) against the device loop on time shards (every rank
its own levels, in HBM).  What scripts/ns_picard_split.py measures on one rank.  One JSON line per
path from every rank, with the per-rank bytes of the re-linearisation plan's level arrays."""
import argparse, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, R + "/tests")


def plan_bytes(dev):
    """Bytes of the plan's arrays that scale with the time levels held (window sizes)."""
    P, th = dev.plan, dev.pb.disc
    w = {k: b - a for k, (a, b) in dev.window.items()}
    ne = len(P.V)
    return 8 * (w["D"] * (ne * 45 + P.K2.nnz + P.Kp.nnz) + (w["v"] + w["zeta"]) * th.n_v
                + 2 * w["blocks"] * (th.n_p + th.n_v))


def rank_main(rank, world, a, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import common
    from control_amd import picard
    from control_amd.dist import CallbackComm, GlooTransport
    pb = common.navier_stokes_problem(n=a.n, n_t=a.n_t, nu=a.nu)
    sp = dict(common.NS_SOLVER_PARAMETERS, relative_tolerance=1.0e-6, maximum_iterations=200)
    tr = GlooTransport(rank, world)
    for path in a.paths.split(","):
        comm = CallbackComm(rank, world, tr.allreduce, tr.sendrecv)
        ls = picard.GpuLinearSolver(pb, solver_parameters=sp, Multigrid=True, relinearise=path,
                                    comm=comm if world > 1 else None, host_allreduce=tr.allreduce)
        t0 = time.perf_counter()
        out = picard.incompressible_non_linear_solve(pb, ls, max_non_linear_iter=a.its,
                                                     relative_non_linear_tol=1e-12,
                                                     device=path == "device",
                                                     print_error_non_linear=False)
        t1 = time.perf_counter()
        st = ls.solve_times
        line = dict(path=path, rank=rank, world=world, n=a.n, n_t=a.n_t, nu=a.nu,
                    total_s=round(t1 - t0, 3), before_first_solve_s=round(st[0][0] - t0, 3),
                    outside_solve_s=[round(st[k][0] - st[k - 1][1], 4) for k in range(1, len(st))],
                    after_last_solve_s=round(t1 - st[-1][1], 4),
                    solve_s=[round(e - s, 3) for s, e in st],
                    linear_iterations=out["linear_iterations"], norms=out["norms"])
        if path == "device":
            dev = ls.device_plan()
            line.update(window=dev.window, plan_level_bytes=plan_bytes(dev))
        print(json.dumps(line), flush=True)
        del ls


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--n_t", type=int, default=64)
    ap.add_argument("--nu", type=float, default=1.0 / 100.0)
    ap.add_argument("--its", type=int, default=2, help="Picard iterations")
    ap.add_argument("--paths", default="device,host")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--port", type=int, default=29541)
    a = ap.parse_args()
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=rank_main, args=(r, a.ranks, a, a.port)) for r in range(a.ranks)]
    for p in procs:
        p.start()
    codes = []
    for p in procs:
        p.join()
        codes.append(p.exitcode)
    sys.exit(0 if all(c == 0 for c in codes) else 1)
