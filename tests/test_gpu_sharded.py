"""Time-sharded path on one GPU box: 2, 3 and 5 ranks (processes; 5 leaves a one-level shard) share GPU 0, hand-offs go
through the host-staged callback transport.  The RCCL transport differs only in
``csrc/comm.cpp``'s RcclComm methods; halo pattern, pipelined sweeps and reductions are
the code exercised here."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, CN, ksp, target="run_rank", timeout=240):
    ctx = mp.get_context("spawn")
    # conns[r][q]: rank r's end of the duplex pipe to rank q
    conns = [[None] * world for _ in range(world)]
    for a in range(world):
        for b in range(a + 1, world):
            ca, cb = ctx.Pipe(duplex=True)
            conns[a][b], conns[b][a] = ca, cb
    q = ctx.Queue()
    sys.path.insert(0, HERE)
    import sharded_worker
    if callable(target):
        # a worker of another module (picklable: a module-level function or a partial of one)
        procs = [ctx.Process(target=target, args=(r, world, conns[r], q)) for r in range(world)]
    elif target == "run_rank":
        procs = [ctx.Process(target=sharded_worker.run_rank, args=(r, world, conns[r], CN, ksp, q))
                 for r in range(world)]
    else:
        procs = [ctx.Process(target=getattr(sharded_worker, target), args=(r, world, conns[r], q))
                 for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=timeout)
            assert status == "ok", f"rank {rank}: {payload}"
            res[rank] = payload
    finally:
        for pr in procs:
            pr.join(timeout=10)
            if pr.is_alive():
                pr.kill()
    return res


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("CN", [False, True])
def test_sharded_matches_oracle(world, CN):
    res = launch(world, CN, "fgmres")
    for r in range(world):
        d = res[r]
        assert d["e_op"] < 1e-13, d
        assert d["op_bitwise"], d
        assert d["e_pc"] < 1e-10, d
        assert abs(d["its_g"] - d["its_o"]) <= (0 if CN else 1), d
        assert d["e_u"] < (1e-6 if CN else 1e-5), d
        if CN:
            assert d["e_h"] < 1e-6, d
    # every rank saw the same residual history (deterministic reductions)
    for r in range(1, world):
        assert res[r]["hist"] == res[0]["hist"]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_stokes_matches_oracle(world, CN):
    """Time-sharded StokesPC (SURVEY 8f-1 on several GPUs; BASELINE configs[2] and [4] name the
    multi-GPU split), backward Euler and Crank-Nicolson (time transforms with halo blocks on the
    four block families of the outer operator, pipelined scans in the preconditioner): operator,
    one preconditioner application and a manufactured solve of every rank's shard against the
    single-rank oracle."""
    res = launch(world, CN, "fgmres", target="run_rank_stokes_cn" if CN else "run_rank_stokes")
    for r in range(world):
        d = res[r]
        assert d["e_op"] < 1e-13, d
        assert d["e_pc"] < 1e-4, d
        assert d["reason"] > 0 and d["e_u0"] < 1e-6 and d["e_u1"] < 1e-5, d
    for r in range(1, world):
        assert res[r]["hist"] == res[0]["hist"]


@pytest.mark.parametrize("CN", [False, True])
def test_sharded_picard_loop_matches_one_rank(CN):
    """Navier-Stokes control (BASELINE configs[4]: Picard loop on 8 GPUs) with the
    linearised solves time-sharded over two ranks: same number of Picard iterations, residual
    history and fields as the loop on one rank, identical on both ranks."""
    res = launch(2, CN, "fgmres", target="run_rank_picard_cn" if CN else "run_rank_picard")
    for r in range(2):
        d = res[r]
        assert d["converged"] and d["n"] == d["n_ref"], d
        assert d["e_norms"] < 1e-6 and d["e_v"] < 1e-6 and d["e_p"] < 1e-5, d
    assert res[0]["hist"] == res[1]["hist"]


def test_sweep_program_timeout_on_one_rank_is_agreed_by_all():
    """A time-out of a persistent sweep program on one rank only (drop hook on rank 0): every rank
    falls back to plain launches in the same iteration and restarts; iteration counts equal,
    results equal to the plain-launch run bit for bit, one fall-back counted on BOTH ranks -- in a
    solve and in a single kkt_pc_apply."""
    res = launch(2, False, "gmres", target="run_rank_timeout")
    for r in range(2):
        d = res[r]
        assert d["its"] == [8, 8], d
        assert d["falls"] == [0, 1], d            # plain run: none; program run: one, on both ranks
        assert d["forms"] == [0, 0], d            # what runs after the fall-back: plain launches
        assert d["same"] and d["pc_same"] and d["pc_falls"] == 1, d


def test_sharded_two_grid_sub_solves():
    """Two-grid sub-solves on a time shard (every rank runs its levels' cycles in its own tile
    program, hand-offs between ranks as before): preconditioner against the oracle, solve against
    the one-rank GPU run (same iteration count)."""
    res = launch(2, False, "gmres", target="run_rank_coarse")
    for r in range(2):
        d = res[r]
        assert d["e_pc"] < 1e-10 and d["its"] == d["its_one"] and d["e_u"] < 1e-6, d


def test_rccl_transport_single_rank():
    """RCCL is loaded, a communicator is created and the collectives used by bench.py
    (barrier = all-reduce of one double, max) run -- world size 1, the only RCCL shape a
    one-GPU box can execute; the multi-rank data path is the one tested above."""
    import ctypes as C
    import common
    from control_amd import _lib
    p = common.heat_problem(n=6, n_t=4)
    gsys = common.gpu_system(p)
    lib, h = gsys._lib, gsys.handle
    uid = C.create_string_buffer(128)
    assert lib.kkt_comm_unique_id(uid) == 0, lib.kkt_last_error(None)
    assert lib.kkt_comm_init_rccl(h, uid) == 0, lib.kkt_last_error(h)
    assert lib.kkt_comm_barrier(h) == 0, lib.kkt_last_error(h)
    v = C.c_double(3.25)
    assert lib.kkt_comm_max(h, C.byref(v)) == 0, lib.kkt_last_error(h)
    assert v.value == 3.25


def _bench_two_ranks(cmd_prefix, extra=()):
    import json
    import subprocess
    root = os.path.dirname(HERE)
    env = dict(os.environ, KKT_DEVICE="0", PYTHONUNBUFFERED="1")
    for k in ("KKT_TRANSPORT", "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    # --full: the assertions below read the side legs (time to solution, stages, config4)
    cmd = cmd_prefix + [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup",
                        "1", "--full", "--no-cpu-baseline"] + list(extra)
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


def test_bench_two_ranks_on_one_gpu_falls_back_to_gloo():
    """``bench.py --gpus 2`` exactly as the driver launches it (torch.distributed.run, one process
    per rank), both ranks on GPU 0 (``KKT_DEVICE=0``, the rehearsal): RCCL refuses two ranks on
    one device, the ranks agree to fall back to the host-staged gloo transport
    (control_amd.dist.RcclOrGloo), the sharded solve converges in the single-GPU iteration count
    and the line says what ran, stage by stage."""
    line, err = _bench_two_ranks([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                  "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                  "--master-port", "29533"], ["--no-config4"])
    assert line["n_gpus"] == 2 and line["steps"] == 4
    assert line["config"]["transport"].startswith("gloo"), line["config"]["transport"]
    tts = line["config"]["time_to_solution"]
    assert tts["converged"] and tts["iterations"] == 17      # as on one GPU (profiles/r03)
    assert "RCCL transport not usable" in err
    st = line["stages"]
    it = st["krylov_iteration_ms"]
    assert it["preconditioner"] > it["operator"] > 0 and it["allreduce"] > 0, it
    pcs = st["preconditioner_application_ms"]
    assert pcs["time_sweeps"] > 0 and pcs["handoff_steps"] > 0 and pcs["rank_handoffs"] > 0, pcs
    # (two ranks on ONE GPU: their 256-workgroup sweep kernels can end up half resident each; the
    # residency check at kernel entry then abandons one launch and that rank -- and with it, by
    # agreement, every rank -- continues with plain launches.  On distinct GPUs this cannot happen;
    # here it may, and then the line must say so)
    falls = line["config"]["sweeps"]["program_fallbacks"]
    assert falls in (0, 1) and (falls == 0 or "warning" in line["config"]), line["config"]


def test_bench_self_launch_two_ranks_with_the_sharded_config4_and_stokes_legs():
    """Plain ``python bench.py --gpus 2`` -- no launcher: the parent spawns the two ranks as fresh
    children and relays rank 0's line -- including the side leg on BASELINE configs[3] (64^3 x 128)
    time-sharded over the ranks; and ``--workload stokes2d`` sharded the same way (a small
    instance)."""
    line, _ = _bench_two_ranks([sys.executable])
    assert line["n_gpus"] == 2 and line["config"]["transport"].startswith("gloo")
    assert line["config"]["time_to_solution"]["iterations"] == 17
    c4 = line["config4"]
    assert "error" not in c4, c4
    assert c4["n_gpus"] == 2 and c4["config"]["unknowns"] == 70304000
    assert c4["config"]["time_to_solution"]["converged"]
    assert c4["stages"]["preconditioner_application_ms"]["handoff_steps"] > 0
    line, _ = _bench_two_ranks([sys.executable], ["--workload", "stokes2d", "--n", "16", "--n_t", "8"])
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["stages"]["krylov_iteration_ms"]["preconditioner"] > 0
