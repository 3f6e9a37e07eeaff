"""One rank of the stopping-rule table on time shards (tests/test_gpu_krylov_stopping_sharded.py
and tests/test_sharded_stop_worker_cpu.py spawn one process per rank through
``test_gpu_sharded.launch``; the ranks share GPU 0 over the host-staged pipe transport).

A rank goes through the whole list ``krylov_stop_cases.layer_cases()`` in-process with a
``ShardBackend``.  Its ``solve`` passes the rank's time levels of the guess and the right-hand
side to an *engine*, wraps the table's global callback preconditioner as a local one, and then
gathers the iterate, and every rank's (reason, count, history), to all ranks over the same pipes.
The gathers move bytes (each byte as a double, so the sum over the ranks' zero-padded buffers is
exact for every bit pattern, NaNs and signed zeros included).  The ``Result`` a check sees is
therefore the same on every rank: an ``assert`` of the table fails on all ranks at the same place
or on none, and the ranks stay in step for the next case.  Ranks whose reasons, counts or
histories differ in any bit make the solve itself fail, on every rank, with the values.

Engines: ``GpuEngine`` solves on a sharded ``MultiBlockSystem`` (``PointerEngine``: on vectors of
the handle, ``kkt_solve_device``).  ``OracleEngine`` proves the harness without a GPU: every rank
gathers the full vectors from the ranks' levels, solves the whole system with the oracle -- the
preconditioner being every rank's local wrapper in turn -- and keeps its own levels.

A worker never asserts and never leaves the loop alone: a failed check is recorded with its
message and the parent asserts.
"""
import copy
import time
import traceback

import numpy as np


def levels_of(m, rank, world):
    """``kkt_shard_range``: the first ``m % world`` ranks own one level more."""
    base, rem = divmod(m, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (rank < rem)


def local_pc(s, fn, lo, hi):
    """The table's global callback on the levels ``lo..hi`` of one rank: the local rows are put
    into zero ``(m, nx)`` arrays, the global function is called, the same rows are taken out.
    The table's preconditioners act row by row, so this is exact."""
    if fn is None:
        return None

    def pc(u_0, u_1, b_0, b_1):
        B0, B1 = np.zeros((s.m, s.nx)), np.zeros((s.m, s.nx))
        U0, U1 = np.zeros((s.m, s.nx)), np.zeros((s.m, s.nx))
        B0[lo:hi], B1[lo:hi] = b_0, b_1
        fn(U0, U1, B0, B1)
        u_0[:], u_1[:] = U0[lo:hi], U1[lo:hi]
    return pc


class Gather:
    """All-gathers over ``PipeTransport.allreduce``, exact for any bytes."""

    def __init__(self, rank, world, tr):
        self.rank, self.world, self.tr = rank, world, tr

    def numbers(self, row):
        """One row of small integers per rank -> the ``(world, len(row))`` table."""
        buf = np.zeros((self.world, len(row)))
        buf[self.rank] = row
        self.tr.allreduce(buf, 0)
        return buf

    def payloads(self, payload, length):
        """``payload`` (bytes, at most ``length``) of every rank, each padded to ``length``."""
        buf = np.zeros((self.world, length))
        buf[self.rank, :len(payload)] = np.frombuffer(payload, dtype=np.uint8)
        self.tr.allreduce(buf, 0)
        return [buf[r].astype(np.uint8).tobytes() for r in range(self.world)]

    def levels(self, s, lo, hi, v_0, v_1):
        """The full vector from every rank's levels of the two variables."""
        full = np.zeros(s.N)
        F0, F1 = s.split(full)
        F0[lo:hi], F1[lo:hi] = v_0, v_1
        # (a rank's rows are zero bytes in every other rank's buffer)
        buf = np.frombuffer(full.tobytes(), dtype=np.uint8).astype(np.float64)
        self.tr.allreduce(buf, 0)
        return np.frombuffer(buf.astype(np.uint8).tobytes(), dtype=np.float64).copy()


class ShardBackend:
    """A backend of ``krylov_stop_cases`` on one rank of a time shard."""

    def __init__(self, rank, world, tr, engine, name="shard"):
        self.rank, self.world, self.engine, self.name = rank, world, engine, name
        self.tr, self.gather = tr, Gather(rank, world, tr)

    def pointer(self):
        return ShardBackend(self.rank, self.world, self.tr, self.engine.pointer(), self.name)

    def handle(self, s, diagonal=False):
        return self.engine.handle(s, diagonal)

    def solve(self, h, s, spec, pc="id", x0=None, b=None):
        import krylov_stop_cases as kc
        lo, hi = levels_of(s.m, self.rank, self.world)
        x = np.array(s.guesses["zero"] if x0 is None else x0, dtype=np.float64)
        rhs = np.array(s.b if b is None else b, dtype=np.float64)
        (X0, X1), (B0, B1) = s.split(x), s.split(rhs)
        u_0, u_1 = X0[lo:hi].copy(), X1[lo:hi].copy()
        err, out = None, (0, 0, np.zeros(0), -1)
        try:
            out = self.engine.solve(h, s, spec, kc.make_pc(s, pc), lo, hi, u_0, u_1,
                                    B0[lo:hi].copy(), B1[lo:hi].copy())
        except RuntimeError as e:           # "Solver failed to converge" of the Python layer
            err = e
        reason, its, hist, ops = out
        meta = self.gather.numbers([err is not None, reason, its, len(hist), ops])
        raised = meta[:, 0]
        if raised.all():
            raise err
        assert not raised.any(), ("some ranks raised, some returned", raised.tolist(), repr(err))
        length = 8 * int(meta[:, 3].max())
        hists = [np.frombuffer(p, dtype=np.float64)[:int(n)]
                 for p, n in zip(self.gather.payloads(hist.tobytes(), length), meta[:, 3])]
        full = self.gather.levels(s, lo, hi, u_0, u_1)
        # across ranks: reasons, counts and histories are identical in every bit
        same = all(np.array_equal(meta[r], meta[0]) and hists[r].tobytes() == hists[0].tobytes()
                   for r in range(1, self.world))
        assert same, ("the ranks differ", meta[:, 1:4].tolist(), [h_.tolist() for h_ in hists])
        return kc.Result(int(meta[0, 1]), int(meta[0, 2]), hists[0].copy(), full, int(meta[0, 4]))


class GpuEngine:
    def __init__(self, rank, world, tr):
        self.rank, self.world, self.tr = rank, world, tr

    def pointer(self):
        return PointerEngine(self.rank, self.world, self.tr)

    def handle(self, s, diagonal):
        from control_amd.dist import CallbackComm, shard_range
        from control_amd.multiblock import MultiBlockSystem
        assert shard_range(s.m, self.rank, self.world) == levels_of(s.m, self.rank, self.world)
        comm = CallbackComm(self.rank, self.world, self.tr.allreduce, self.tr.sendrecv)
        return MultiBlockSystem(s.nx, s.nx, *(s.diag_blocks() if diagonal else s.blocks()),
                                n_blocks_00=s.m, n_blocks_11=s.m, comm=comm)

    def solve(self, h, s, spec, fn, lo, hi, u_0, u_1, b_0, b_1):
        r = h.solve(u_0, u_1, b_0, b_1, solver_parameters=spec.parameters(),
                    pc_fn=local_pc(s, fn, lo, hi))
        return (int(r.reason), int(r.its), np.array(r.history, dtype=np.float64),
                int(r.info["last_op_applies"]))


class PointerEngine(GpuEngine):
    """The same solves through ``kkt_solve_device`` on local vectors of the handle."""

    def solve(self, h, s, spec, fn, lo, hi, u_0, u_1, b_0, b_1):
        import ctypes as C
        lib, f64p = h._lib, C.POINTER(C.c_double)
        x = np.ascontiguousarray(np.concatenate([u_0.ravel(), u_1.ravel()]))
        b = np.ascontiguousarray(np.concatenate([b_0.ravel(), b_1.ravel()]))
        assert x.size == h.local_size
        d_b, d_u = C.c_void_p(), C.c_void_p()
        h._ck(lib.kkt_vec_alloc(h.handle, C.byref(d_b)))
        h._ck(lib.kkt_vec_alloc(h.handle, C.byref(d_u)))
        try:
            h._ck(lib.kkt_vec_upload(h.handle, d_b, b.ctypes.data_as(f64p)))
            h._ck(lib.kkt_vec_upload(h.handle, d_u, x.ctypes.data_as(f64p)))
            r = h.solve_device(d_b, d_u, solver_parameters=spec.parameters(),
                               pc_fn=local_pc(s, fn, lo, hi))
            h._ck(lib.kkt_vec_download(h.handle, d_u, x.ctypes.data_as(f64p)))
        finally:
            lib.kkt_vec_free(h.handle, d_b)
            lib.kkt_vec_free(h.handle, d_u)
        u_0[:], u_1[:] = x[:u_0.size].reshape(u_0.shape), x[u_0.size:].reshape(u_1.shape)
        return (int(r.reason), int(r.its), np.array(r.history, dtype=np.float64),
                int(r.info["last_op_applies"]))


class OracleEngine:
    """Every rank solves the whole system with the oracle, behind the same slicing, callback
    wrapping and gathering."""

    def __init__(self, rank, world, tr):
        import krylov_stop_cases as kc
        self.rank, self.world, self.tr = rank, world, tr
        self.gather, self.oracle = Gather(rank, world, tr), kc.OracleBackend()

    def pointer(self):
        return self

    def handle(self, s, diagonal):
        return self.oracle.handle(s, diagonal)

    def solve(self, h, s, spec, fn, lo, hi, u_0, u_1, b_0, b_1):
        x = self.gather.levels(s, lo, hi, u_0, u_1)
        b = self.gather.levels(s, lo, hi, b_0, b_1)
        ranges = [levels_of(s.m, q, self.world) for q in range(self.world)]
        # one copy of the callback per rank, as the ranks of a shard have: a callback that counts
        # its applications counts them on each rank
        pcs = [local_pc(s, copy.deepcopy(fn), lo_q, hi_q) for lo_q, hi_q in ranges]

        def every_rank(U0, U1, B0, B1):
            for pc, (lo_q, hi_q) in zip(pcs, ranges):
                pc(U0[lo_q:hi_q], U1[lo_q:hi_q], B0[lo_q:hi_q], B1[lo_q:hi_q])
        with np.errstate(all="ignore"):
            r = h.solve(*s.split(x), *s.split(b), solver_parameters=spec.parameters(),
                        pc_fn=None if fn is None else every_rank)
        (X0, X1) = s.split(x)
        u_0[:], u_1[:] = X0[lo:hi], X1[lo:hi]
        return int(r.reason), int(r.its), np.array(r.history, dtype=np.float64), -1


ENGINES = {"gpu": GpuEngine, "oracle": OracleEngine}
SEEDED = ("seeded-wrong-expectation", "check_seeded_wrong", (), {})


def check_seeded_wrong(backend):
    """A copy of one step count of case A with a wrong expectation: four steps asked for, five
    expected.  Only the CPU harness test runs it, to see a failing assert reported by every rank."""
    import krylov_stop_cases as kc
    s = kc.system("L5")
    res = backend.solve(backend.handle(s), s, kc.Spec("left", restart=3, max_it=4), "diag")
    assert (res.reason, res.its) == (kc.ref.DIVERGED_ITS, 5), ("seeded", res.reason, res.its)
    return [res]


def run_cases(rank, world, conns, out_q, engine="gpu", seeded_after=None, bits=False, only=None,
              trajectories=None):
    """The whole case list on this rank (``only``: the cases whose id starts with one of these
    prefixes).  ``seeded_after``: put the seeded wrong case behind that many cases.  ``bits``:
    also report every result in full, for a bitwise comparison.  ``trajectories``: the 60-digit
    reference as the parent computed it (``krylov_stop_cases.layer_trajectories``), so that not
    every rank computes it again."""
    try:
        import pytest
        import krylov_stop_cases as kc
        from control_amd.dist import PipeTransport
        t_start = time.perf_counter()
        kc.preload_trajectories(trajectories or {})
        tr = PipeTransport(rank, world, conns)
        backend = ShardBackend(rank, world, tr, ENGINES[engine](rank, world, tr))
        cases = [c for c in kc.layer_cases() if only is None or c[0].startswith(tuple(only))]
        if seeded_after is not None:
            cases.insert(seeded_after, SEEDED)
        records = {}
        for case in cases:
            rec = dict(status="ok", message="", results=[], seconds=0.0)
            t0 = time.perf_counter()
            try:
                out = (check_seeded_wrong(backend) if case is SEEDED
                       else kc.run_case(backend, case))
                rec["results"] = [(r.reason, r.its, len(r.history)) for r in out]
                if bits:
                    rec["bits"] = [(r.reason, r.its, r.history.tobytes(), r.x.tobytes())
                                   for r in out]
            except (AssertionError, RuntimeError, pytest.fail.Exception):
                # (pytest.fail.Exception: pytest.raises in a check that met no exception)
                # the same on every rank (see ShardBackend.solve): all go on to the next case
                rec["status"], rec["message"] = "failed", traceback.format_exc()[-2000:]
            rec["seconds"] = time.perf_counter() - t0
            records[case[0]] = rec
        out_q.put((rank, "ok", dict(records=records, order=[c[0] for c in cases],
                                    worst=kc.WORST.get(backend.name),
                                    seconds=time.perf_counter() - t_start)))
    except Exception as e:   # report instead of hanging the other ranks' pipes
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))
