"""One rank of the time-shard case of tests/test_gpu_pc_alias.py (one process per rank, all on GPU 0
over the host-staged pipe transport of tests/test_gpu_sharded.py).  Every rank builds a handle with
``pc_alias`` 0 and one with 1 on mode-G copies of a time-invariant operator and reports the bits of
two applications of each, the arrays its levels read and the statistics.  A worker never asserts.
"""
from sharded_forms_worker import Shard, _report

MASS = (8, 0.5, 2.0)
SCHUR = (4, 2.1 / 30, 2.1)


def run_alias(rank, world, conns, out_q, CN=False, m=6, n=24, cells=4):
    def work():
        import common
        from control_amd.coarse import multilinear_coarse_space
        p = common.heat_problem(n=n, n_t=m + 1 if CN else m, CN=CN, beta=1e-2, share=False)
        co = (multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells), 2)
        s = Shard(rank, world, conns, p)
        out = dict(levels=s.hi - s.lo, lo=s.lo, runs={})
        for alias in ("0", "1"):
            g = common.gpu_system(p, comm=s.comm(), options={"pc_alias": alias})
            pc = common.gpu_pc(p, MASS, SCHUR, coarse=co)
            ys = [g.pc_apply(s.shard(x), pc) for x in s.xs]
            inf = g.info()
            out["runs"][alias] = dict(y=[y.tobytes() for y in ys], alias=g.pc_alias(),
                                      solves=g.pc_solves(), stats=g.spectrum_stats(),
                                      falls=int(inf["program_fallbacks"]),
                                      form=int(inf["sweep_form"]))
            g.close()
        return out
    _report(out_q, rank, work)
