"""One rank of the batched-spectrum case on time shards (tests/test_gpu_spectrum_batch.py spawns
one process per rank; all share GPU 0 over the host-staged pipe transport of
tests/test_gpu_sharded.py).  Every rank builds the same handles in the same order -- first with
``spectrum_batch`` 0, then with each batch size -- so the all-reduce of the derived degree pairs
up.  A worker never asserts: it reports the records, the statistics and the bits of one
preconditioner application through the queue.
"""
from sharded_forms_worker import Shard, _report

MASS = (20, 0.5, 2.0)
AUTO = (-1, 0.0, 0.0)
BATCHES = (0, 1, 3, 64)


def run_spectrum_batch(rank, world, conns, out_q, CN=False, m=7, n=16):
    def work():
        import common
        p = common.heat_problem(n=n, n_t=m + 1 if CN else m, CN=CN, beta=1e-4, time_dependent=True)
        s = Shard(rank, world, conns, p)
        x = s.shard(s.xs[0])
        out = dict(levels=s.hi - s.lo, runs={})
        for nb in BATCHES:
            g = common.gpu_system(p, comm=s.comm(), options={"spectrum_batch": str(nb)})
            y = g.pc_apply(x, common.gpu_pc(p, MASS, AUTO))
            out["runs"][nb] = dict(solves=g.pc_solves(), mats=g.pc_matrices(), stats=g.spectrum_stats(),
                                   y=y.tobytes())
            g.close()
        return out
    _report(out_q, rank, work)
