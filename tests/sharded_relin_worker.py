"""One rank of a time-sharded device re-linearisation (spawned by tests/test_gpu_sharded_relin.py,
one process per rank, all on GPU 0 over a host-staged pipe transport).

Every rank builds the same Navier-Stokes control problem twice in its own process: sharded over
the ranks, and on one rank as the reference.  What the sharded plan leaves in HBM is compared with
the same levels, rows and blocks of the one-rank plan, bit for bit.
"""
import ctypes as C

import numpy as np

N, N_T = 4, 6          # 4 x 4 P2-P1; six unknown blocks: n_t = 6 (BE), 7 (CN)


def _transport(rank, world, conns):
    from control_amd.dist import CallbackComm, PipeTransport
    tr = PipeTransport(rank, world, conns)
    return tr, CallbackComm(rank, world, tr.allreduce, tr.sendrecv)


def _solver_kw():
    import common
    s = common.STOKES_SPECS
    return dict(mass=s["mass"], schur=s["schur"], kp=s["kp"], mp=s["mp"],
                solver_parameters=common.NS_SOLVER_PARAMETERS)


def _state(pb, rng):
    th, n_t = pb.disc, pb.n_t
    m = n_t - 1 if pb.CN else n_t
    return [0.1 * rng.standard_normal((n_t, th.n_v)), rng.standard_normal((n_t, th.n_v)),
            rng.standard_normal((m, th.n_p)), rng.standard_normal((m, th.n_p))]


class _Vec:
    """A device vector of a system (local length)."""

    def __init__(self, system, host=None):
        self.s, self.d = system, C.c_void_p()
        system._ck(system._lib.kkt_vec_alloc(system.handle, C.byref(self.d)))
        if host is not None:
            host = np.ascontiguousarray(host, dtype=np.float64)
            assert host.size == system.local_size
            system._ck(system._lib.kkt_vec_upload(system.handle, self.d,
                                                  host.ctypes.data_as(C.POINTER(C.c_double))))

    def get(self):
        out = np.empty(self.s.local_size)
        self.s._ck(self.s._lib.kkt_vec_download(self.s.handle, self.d,
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.s._lib.kkt_vec_free(self.s.handle, self.d)


def _residual(system, dev, rhs):
    with _Vec(system) as d:
        norm = dev.residual(d.d, rhs=rhs)
        return d.get(), norm


def run_rank_kernels(rank, world, conns, CN, out_q):
    """Windows, assembly, residual / right-hand side, composition and update of one rank."""
    try:
        import common
        from control_amd import _lib, picard
        from control_amd.blocks import instationary_relinearisation_recipes
        from control_amd.dist import shard_range
        pb = common.navier_stokes_problem(n=N, n_t=N_T + 1 if CN else N_T, CN=CN)
        pb.nu = 0.2
        th, n_t = pb.disc, pb.n_t
        m, nv, n1 = (n_t - 1 if CN else n_t), th.n_v, th.n_p
        lo, hi = shard_range(m, rank, world)
        nl = hi - lo
        tr, comm = _transport(rank, world, conns)
        rng = np.random.default_rng(common.SEED)       # the same stream on every rank
        v_a = _state(pb, rng)[0]
        state = _state(pb, rng)
        kw = _solver_kw()
        sharded = picard.GpuLinearSolver(pb, comm=comm, host_allreduce=tr.allreduce,
                                         relinearise="device", **kw)
        one = picard.GpuLinearSolver(pb, relinearise="device", **kw)
        D_a, Dp_a = [pb.D_v(x) for x in v_a], [pb.D_p(x) for x in v_a]
        for ls in (sharded, one):
            ls._build(ls._blocks(D_a, Dp_a))
        dev, ref = sharded.device_plan(), one.device_plan()
        out = dict(lo=lo, hi=hi, window=dev.window, window_one=ref.window)

        # -- assembly: the halo slots are NaN on this rank's host and must come from the neighbours
        (v0, v1), (z0, z1), (D0, D1) = dev.window["v"], dev.window["zeta"], dev.window["D"]
        poisoned = [a.copy() for a in state]
        own_v = range(lo + 1, hi + 1) if CN else range(lo, hi)
        for lev in range(n_t):
            if lev not in own_v and not (CN and lev == 0):
                poisoned[0][lev] = np.nan           # every level of v another rank owns
            if not lo <= lev < hi and not (CN and lev == n_t - 1):
                poisoned[1][lev] = np.nan           # ... and of zeta (CN: the last level is fixed)
        dev.set_state(*poisoned)
        ref.set_state(*state)
        out["halo_poisoned"] = bool((rank == 0 or np.isnan(dev.debug_array("v")[0]).all())
                                    and (rank == world - 1
                                         or np.isnan(dev.debug_array("zeta")[-1]).all()))
        dev.assemble()
        ref.assemble()
        out["halo_travelled"] = bool(np.array_equal(dev.debug_array("v"), state[0][v0:v1])
                                     and np.array_equal(dev.debug_array("zeta"), state[1][z0:z1]))
        for name in ("Ev", "Ep", "D2", "Dp"):
            got, want = dev.debug_array(name), ref.debug_array(name)[D0:D1]
            out["asm_" + name] = bool(got.shape == want.shape and np.array_equal(got, want))

        # -- residual and right-hand side: the rank's rows of the four families
        pick = list(range(lo, hi)) + list(range(m + lo, m + hi))

        def rows(x):
            return np.concatenate([x[:2 * m * nv].reshape(2 * m, nv)[pick].ravel(),
                                   x[2 * m * nv:].reshape(2 * m, n1)[pick].ravel()])
        for rhs in (0, 1):
            got, norm = _residual(sharded.outer, dev, rhs)
            want, norm_one = _residual(one.outer, ref, rhs)
            out[f"res{rhs}"] = bool(np.array_equal(got, rows(want)))
            out[f"res{rhs}_nonzero"] = bool(np.abs(got).max() > 0)
            out[f"norm{rhs}"], out[f"norm{rhs}_one"] = norm, norm_one
        out["n_entries"] = 2 * m * (nv + n1)

        # -- composition: every owned linearised block, and a recipe for a row of another rank
        sharded.device_relinearise()
        one.device_relinearise()
        rec = instationary_relinearisation_recipes(pb.tau, pb.beta, n_t, CN)
        blocks_equal, n_blocks = True, 0
        for name, attr in (("outer", "outer"), ("inner", "inner"), ("commutator", "comm")):
            for (q, i, j, *_) in rec[name]:
                if lo <= i % m < hi:
                    a, pad_a = getattr(sharded, attr).block_values(q, i, j)
                    b, pad_b = getattr(one, attr).block_values(q, i, j)
                    blocks_equal = blocks_equal and pad_a and pad_b and np.array_equal(a, b)
                    n_blocks += 1
        out["blocks_equal"], out["n_blocks"] = bool(blocks_equal), n_blocks
        foreign = [r for r in rec["inner"] if not lo <= r[1] < hi][:1]
        try:
            dev.relinearise(sharded.inner, "inner", recipes=foreign)
            out["foreign"] = "accepted"
        except _lib.KktError as e:
            out["foreign"] = (e.code, str(e))

        # -- update: dyadic blocks, the same global update on every rank
        U0 = rng.integers(-16, 17, size=(2 * m, nv)) / 8.0
        U1 = rng.integers(-16, 17, size=(2 * m, n1)) / 8.0
        v, zeta, p, mu = [a.copy() for a in state]
        if CN:
            v[1:] += U0[:m]
            zeta[:m] += U0[m:]
        else:
            v += U0[:m]
            zeta += U0[m:]
        zeta[:, th.boundary_v] = 0.0
        mu += U1[:m]
        p += U1[m:]
        with _Vec(sharded.outer, np.concatenate([U0[pick].ravel(), U1[pick].ravel()])) as d:
            dev.update(d.d)
            out["u_zeroed"] = bool(not d.get().any())
        with _Vec(one.outer, np.concatenate([U0.ravel(), U1.ravel()])) as d:
            ref.update(d.d)
        wv, wz = dev.debug_array("v"), dev.debug_array("zeta")
        ov = [lev - v0 for lev in own_v]
        out["update_owned"] = bool(np.array_equal(wv[ov], v[list(own_v)])
                                   and np.array_equal(wz[:nl], zeta[lo:hi]))
        out["update_changed"] = bool(not np.array_equal(wv[ov], state[0][list(own_v)]))
        out["zeta_bc_zero"] = bool(not wz[:, th.boundary_v].any())
        # the halo slots still hold the levels of before the update ...
        out["halo_stale"] = bool((rank == 0 or np.array_equal(wv[0], state[0][v0]))
                                 and (rank == world - 1 or not np.array_equal(wz[-1], zeta[z1 - 1])))
        dev.assemble()           # ... and the next exchange brings the neighbours' updated ones
        out["halo_updated"] = bool(np.array_equal(dev.debug_array("v"), v[v0:v1])
                                   and np.array_equal(dev.debug_array("zeta"), zeta[z0:z1]))
        got = dev.get_state()                     # collective: every rank gathers the whole
        want = ref.get_state()
        out["state_gathered"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want))
                                     and all(np.array_equal(a, b)
                                             for a, b in zip(got, (v, zeta, p, mu))))
        try:
            dev.set_state(None, *state[1:])
            out["null_state"] = "accepted"
        except (ValueError, TypeError, _lib.KktError) as e:
            out["null_state"] = type(e).__name__
        out_q.put((rank, "ok", out))
    except Exception as e:   # report instead of hanging the other ranks' pipes
        import traceback
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))


def run_rank_loop(rank, world, conns, CN, out_q):
    """The Picard loop with the iterate in HBM, time-sharded, against the same loop on one rank:
    the lid-driven cavity of tests/sharded_worker.py's host-sharded loop (4 x 4, nu = 0.2)."""
    try:
        import common
        from control_amd import picard
        pb, v_init, _ = common.navier_stokes_cavity_problem(n=N, n_t=N_T + 1 if CN else N_T, CN=CN)
        pb.nu = 0.2
        kw = _solver_kw()
        ref = picard.incompressible_non_linear_solve(
            pb, picard.GpuLinearSolver(pb, relinearise="device", **kw), v=v_init, device=True,
            print_error_non_linear=False)
        tr, comm = _transport(rank, world, conns)
        gls = picard.GpuLinearSolver(pb, comm=comm, host_allreduce=tr.allreduce,
                                     relinearise="device", **kw)
        out = picard.incompressible_non_linear_solve(pb, gls, v=v_init, device=True,
                                                     print_error_non_linear=False)
        out_q.put((rank, "ok", dict(
            converged=out["converged"], n=len(out["norms"]), n_ref=len(ref["norms"]),
            e_norms=float(max(abs(a - b) / ref["norms"][0]
                              for a, b in zip(out["norms"], ref["norms"]))),
            e_v=float(np.abs(out["v"] - ref["v"]).max()),
            e_p=float(np.abs(out["p"] - ref["p"]).max()),
            its=out["linear_iterations"], its_ref=ref["linear_iterations"],
            uploads=gls.uploads, window=gls.device_plan().window,
            hist=[float(x) for x in out["norms"]])))
    except Exception as e:
        import traceback
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))
