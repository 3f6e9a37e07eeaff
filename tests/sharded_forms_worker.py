"""One rank of the sweep-form cases on time shards (tests/test_gpu_sharded_forms.py spawns one
process per rank; all share GPU 0 over the host-staged pipe transport).

Without reductions a shard runs the same RowOps on the same operands as one rank, so every rank
compares its shard of a preconditioner application with the one-rank plain-launch result it
computes itself, bit for bit.  A worker never asserts: it reports booleans, distances and
read-backs through the queue and the parent asserts -- a rank that raised in the middle of an
application would leave its neighbours in a pipe read.  Every rank builds the same handles and
applies them in the same order, so the ranks' hand-offs pair up.
"""
import numpy as np

MASS = (8, 0.5, 2.0)
SCHUR = (6, 0.05, 2.1)
SCHUR_COARSE = (6, 0.07, 2.1)
INFO_KEYS = ("sweep_form", "program_fallbacks", "sweep_tiles", "sweep_threads", "sweep_depth",
             "sweep_row_slots", "sweep_coarse_rings")
PLAIN = {"persistent": "0"}

# name -> options of the sharded handle (part 1 of the test module)
HEAT_OPTIONS = [
    ("plain", PLAIN),
    ("plain,no_graph=1", dict(PLAIN, no_graph="1")),
    ("plain,kernarg_ops=1", dict(PLAIN, kernarg_ops="1")),
    ("plain,interleave=0", dict(PLAIN, interleave="0")),
    ("plain,shared_rows=0", dict(PLAIN, shared_rows="0")),
    ("plain,sell_r=1", dict(PLAIN, sell_r="1")),
    ("plain,pc_xcd=0", dict(PLAIN, pc_xcd="0")),
    ("plain,lanes=1", dict(PLAIN, lanes="1")),
    ("flags", {"prog_mode": "flags"}),
    ("dataflow", {"prog_mode": "dataflow"}),
    ("w", {"prog_mode": "w"}),
    ("dataflow,prog_steps=0", {"prog_mode": "dataflow", "prog_steps": "0"}),
    ("tile,depth=1", {"prog_mode": "tile", "tile_depth": "1"}),
    ("tile,depth=2", {"prog_mode": "tile", "tile_depth": "2"}),
    ("tile,depth=3", {"prog_mode": "tile", "tile_depth": "3"}),
    ("mass_tiles,rows=64", {"mass_tile_depth": "3", "mass_tile_rows": "64"}),
    ("mass_tiles,rows=65536", {"mass_tile_depth": "3", "mass_tile_rows": "65536"}),
]
# the ragged Q2 structure (rows of 9 / 15 / 25 entries): the interleaved kernel for any width
Q2_OPTIONS = [("plain", PLAIN), ("plain,interleave=0", dict(PLAIN, interleave="0")),
              ("auto", {})]
VELOCITY_OPTIONS = [("plain", PLAIN), ("auto", {}), ("flags", {"prog_mode": "flags"})]


def inputs(n):
    import common
    return common.rng_vector(n), 3.0 * common.rng_vector(n)[::-1].copy()


def compare(y, ref):
    """Bit-equality, the first differing indices and the relative distance."""
    import common
    bad = np.flatnonzero(y != ref)
    return dict(same=bool(bad.size == 0), first=bad[:8].tolist(), n_bad=int(bad.size),
                dist=float(common.rel_err(y, ref)))


def per_block_err(y, ref):
    """tests/test_gpu_sweep_forms.py::per_block_err: the v part and the zeta part, each against
    its own norm."""
    import common
    h = len(ref) // 2
    return float(max(common.rel_err(y[:h], ref[:h]), common.rel_err(y[h:], ref[h:])))


def read_back(g):
    """info() and pc_forms() of a handle: the fields the parent asserts on, the distinct records
    with their multiplicities, and the step counts of the mass-tile launches in replay order."""
    inf = g.info()
    forms = g.pc_forms()
    keys = ("form", "width", "slots", "lane", "count", "variant")
    distinct = {}
    for f in forms:
        t = tuple(f[k] for k in keys)
        distinct[t] = distinct.get(t, 0) + 1
    return dict(info={k: int(inf[k]) for k in INFO_KEYS},
                forms=[dict(zip(keys, t), n=n) for t, n in sorted(distinct.items())],
                cheb_counts=[f["count"] for f in forms if f["form"] == 6])


class Shard:
    """Problem, transport and the one-rank reference of one rank."""

    def __init__(self, rank, world, conns, p):
        from control_amd.dist import PipeTransport, shard_range
        self.rank, self.world, self.p = rank, world, p
        self.m, self.nx = p["m"], p["sd"].n_dofs
        self.lo, self.hi = shard_range(self.m, rank, world)
        self.tr = PipeTransport(rank, world, conns)
        self.xs = inputs(2 * self.m * self.nx)

    def comm(self):
        from control_amd.dist import CallbackComm
        return CallbackComm(self.rank, self.world, self.tr.allreduce, self.tr.sendrecv)

    def shard(self, v):   # global flat -> this rank's [v_lo.. | zeta_lo..]
        V = np.asarray(v).reshape(2 * self.m, self.nx)
        return np.concatenate([V[self.lo:self.hi].ravel(),
                               V[self.m + self.lo:self.m + self.hi].ravel()])

    def one_rank(self, options, mass, schur, coarse=None):
        """Both inputs through a one-rank handle: (shards of the results, read-back)."""
        import common
        g = common.gpu_system(self.p, options=options)
        pc = common.gpu_pc(self.p, mass, schur, coarse=coarse)
        ys = [self.shard(g.pc_apply(x, pc)) for x in self.xs]
        return ys, read_back(g)

    def sharded(self, options, mass, schur, coarse=None):
        """shard(xa), shard(xb), shard(xa) through ONE sharded handle and ONE descriptor: the
        repeat runs the cached program or graph with the halos the second application left."""
        import common
        g = common.gpu_system(self.p, comm=self.comm(), options=options)
        pc = common.gpu_pc(self.p, mass, schur, coarse=coarse)
        xa, xb = (self.shard(x) for x in self.xs)
        ys = [g.pc_apply(x, pc) for x in (xa, xb, xa)]
        return ys, read_back(g)


def _report(out_q, rank, fn):
    try:
        out_q.put((rank, "ok", fn()))
    except Exception as e:   # report instead of hanging the other ranks' pipes
        import traceback
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))


def run_heat_forms(rank, world, conns, out_q, CN=False, m=7, space="p1", n=40, names=None):
    """Part 1: every option set of HEAT_OPTIONS (Q2_OPTIONS for space "q2") whose name is in
    `names` (None: all) on this rank's shard, three applications each."""
    def work():
        import common
        p = common.heat_problem(space=space, n=n, n_t=m + 1 if CN else m, CN=CN, beta=1e-2)
        s = Shard(rank, world, conns, p)
        ref, _ = s.one_rank(PLAIN, MASS, SCHUR)
        out = dict(levels=s.hi - s.lo, lo=s.lo, nx=s.nx, m=p["m"],
                   inputs_differ=not np.array_equal(ref[0], ref[1]), sets={})
        for name, opts in (Q2_OPTIONS if space == "q2" else HEAT_OPTIONS):
            if names is not None and name not in names:
                continue
            ys, rb = s.sharded(opts, MASS, SCHUR)
            rb["apps"] = [compare(y, ref[k]) for y, k in zip(ys, (0, 1, 0))]
            out["sets"][name] = rb
        return out
    _report(out_q, rank, work)


def run_coarse_forms(rank, world, conns, out_q, CN=False, m=7):
    """Part 2: two-grid sub-solves, 1 and 2 cycles -- sharded plain launches against one-rank
    plain launches, the sharded tile program with and without rings against each other, against
    the one-rank plain launches and against the one-rank tile program."""
    def work():
        import common
        from control_amd.coarse import multilinear_coarse_space
        p = common.heat_problem(n=40, n_t=m + 1 if CN else m, CN=CN, beta=1e-2)
        s = Shard(rank, world, conns, p)
        P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=5)
        out = dict(levels=s.hi - s.lo, lo=s.lo, nx=s.nx, cycles={})
        for cycles in (1, 2):
            co = (P, cycles)
            ref, _ = s.one_rank(PLAIN, MASS, SCHUR_COARSE, co)
            one_tile, one_rb = s.one_rank({"prog_mode": "tile"}, MASS, SCHUR_COARSE, co)
            d = dict(one_tile=one_rb)
            ys, rb = s.sharded(PLAIN, MASS, SCHUR_COARSE, co)
            rb["apps"] = [compare(y, ref[k]) for y, k in zip(ys, (0, 1, 0))]
            d["plain"] = rb
            tiles = {}
            for rings in ("1", "0"):
                tiles[rings], rb = s.sharded({"prog_mode": "tile", "coarse_rings": rings}, MASS,
                                             SCHUR_COARSE, co)
                rb["err_plain"] = [per_block_err(y, ref[k]) for y, k in zip(tiles[rings], (0, 1, 0))]
                rb["one_tile"] = [compare(y, one_tile[k]) for y, k in zip(tiles[rings], (0, 1, 0))]
                d["rings=" + rings] = rb
            d["rings_equal"] = [compare(a, b) for a, b in zip(tiles["1"], tiles["0"])]
            out["cycles"][cycles] = d
        return out
    _report(out_q, rank, work)


def run_stokes_forms(rank, world, conns, out_q, CN=False):
    """Part 3: the sharded outer operator of Stokes control and the velocity preconditioner alone
    (the `inner` system and `inner_pc` of stokes_gpu), each against one rank."""
    def work():
        import common
        from control_amd.dist import CallbackComm, PipeTransport, shard_range
        p = common.stokes_problem(n=4, n_t=5 if CN else 4, CN=CN)
        th, m = p["th"], p["m"]
        nv, np_ = th.n_v, th.n_p
        lo, hi = shard_range(m, rank, world)
        tr = PipeTransport(rank, world, conns)
        pick = list(range(lo, hi)) + list(range(m + lo, m + hi))

        def shard_outer(v):   # global [2m velocity blocks | 2m pressure blocks] -> local
            v = np.asarray(v)
            v0 = v[:2 * m * nv].reshape(2 * m, nv)
            v1 = v[2 * m * nv:].reshape(2 * m, np_)
            return np.concatenate([v0[pick].ravel(), v1[pick].ravel()])

        def shard_inner(v):
            return np.asarray(v).reshape(2 * m, nv)[pick].ravel()

        def gpu(options, sharded):
            comm = CallbackComm(rank, world, tr.allreduce, tr.sendrecv) if sharded else None
            return common.stokes_gpu(p, options=options, comm=comm)

        out = dict(levels=hi - lo, lo=lo, nv=nv, m=m)
        # outer operator, default options on both sides
        one, _ = gpu(None, False)
        xs = inputs(2 * m * (nv + np_))
        ref = [shard_outer(one.mult(x)) for x in xs]
        outer, _ = gpu(None, True)
        xa, xb = (shard_outer(x) for x in xs)
        out["outer"] = [compare(outer.mult(x), ref[k]) for x, k in zip((xa, xb, xa), (0, 1, 0))]
        out["outer_inputs_differ"] = not np.array_equal(ref[0], ref[1])
        # velocity preconditioner
        vs = inputs(2 * m * nv)
        _, gpc1 = gpu(PLAIN, False)
        vref = [shard_inner(gpc1.inner.pc_apply(x, gpc1.inner_pc)) for x in vs]
        out["velocity"] = {}
        for name, opts in VELOCITY_OPTIONS:
            _, g1 = gpu(opts, False)            # what one rank runs under these options
            g1.inner.pc_apply(vs[0], g1.inner_pc)
            _, gs = gpu(opts, True)
            va, vb = (shard_inner(x) for x in vs)
            ys = [gs.inner.pc_apply(x, gs.inner_pc) for x in (va, vb, va)]
            rb = read_back(gs.inner)
            rb["apps"] = [compare(y, vref[k]) for y, k in zip(ys, (0, 1, 0))]
            rb["one_rank_form"] = int(g1.inner.info()["sweep_form"])
            out["velocity"][name] = rb
        return out
    _report(out_q, rank, work)
