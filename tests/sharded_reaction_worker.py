"""One rank of a time-sharded scalar device loop (spawned by tests/test_gpu_sharded_reaction.py,
one process per rank, all on GPU 0 over a host-staged pipe transport).

Every rank builds the same reaction control problem twice in its own process: sharded over the
ranks, and on one rank as the reference.  What the sharded plan leaves in HBM is compared with the
same levels, rows and blocks of the one-rank plan, bit for bit; the sharded loop is compared with
the one-rank device loop.
"""
import ctypes as C

import numpy as np

SCHUR = (40, 0.02, 2.2)                                    # tests/test_gpu_reaction_picard.py
MASS = {"triangles": (0.5, 2.0), "tetrahedra": (0.5, 2.5)}  # ... and test_gpu_reaction3d_picard.py


def _transport(rank, world, conns):
    from control_amd.dist import CallbackComm, PipeTransport
    tr = PipeTransport(rank, world, conns)
    return tr, CallbackComm(rank, world, tr.allreduce, tr.sendrecv)


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


def _device(ctl, comm=None, host_allreduce=None):
    """The pattern-only block system with the plan on it; nothing composed."""
    from control_amd import reaction
    from control_amd.control import GpuBackend
    plan = reaction.ReactionPlan(ctl)
    system, _, full = reaction.build_system(ctl, GpuBackend(), plan, comm)
    return system, reaction.DeviceReaction(ctl, system, plan=plan,
                                           host_allreduce=host_allreduce), full


def _kernels(rank, world, tr, comm, CN, mesh, newton, assembly_only=False):
    import common
    import reaction_shard_ref as sref
    from control_amd import _lib
    m = sref.M_BLOCKS
    lo, hi = sref.shard_range(m, rank, world)
    nl = hi - lo

    def make():
        ctl = sref.control(mesh, CN)
        ctl.set_Gauss_Newton(newton)
        return ctl
    ctl = make()
    disc, n_t = ctl._disc, ctl._n_t
    n, nodes = disc.n_dofs, disc.boundary
    system, dev, full = _device(make(), comm, tr.allreduce)
    one, ref, full_one = _device(make())
    out = dict(lo=lo, hi=hi, window=dev.window, window_one=ref.window,
               window_want=sref.shard_windows(m, CN, rank, world), n_t=n_t)

    # -- assembly: the levels another rank owns are NaN on this rank's host
    rng = np.random.default_rng(common.SEED + 3)          # the same stream on every rank
    state = [rng.standard_normal((n_t, n)), rng.standard_normal((n_t, n))]
    (v0, v1), (z0, z1), (D0, D1) = dev.window["v"], dev.window["zeta"], dev.window["D"]
    own_v, own_z = sref.owned_levels(m, CN, rank, world)
    poisoned = [a.copy() for a in state]
    for lev in range(n_t):
        if lev not in own_v:
            poisoned[0][lev] = np.nan
        if lev not in own_z:
            poisoned[1][lev] = np.nan
    dev.set_state(*poisoned)
    ref.set_state(*state)
    out["halo_poisoned"] = bool((rank == 0 or np.isnan(dev.debug_array("v")[0]).all())
                                and (rank == world - 1
                                     or np.isnan(dev.debug_array("zeta")[-1]).all()))
    dev.assemble()
    ref.assemble()
    out["halo_travelled"] = bool(np.array_equal(dev.debug_array("v"), state[0][v0:v1])
                                 and np.array_equal(dev.debug_array("zeta"), state[1][z0:z1]))
    for name in ("E", "D"):
        got, want = dev.debug_array(name), ref.debug_array(name)[D0:D1]
        out["asm_" + name] = bool(got.shape == want.shape and got.shape[0] == D1 - D0
                                  and np.array_equal(got, want))
    out["asm_nonlinear"] = bool(not np.array_equal(ref.debug_array("E")[0], ref.debug_array("E")[1]))
    if assembly_only:
        system.close()
        one.close()
        return out

    # -- residual and right-hand side: the rank's rows of both families
    pick = list(range(lo, hi)) + list(range(m + lo, m + hi))
    for rhs in (0, 1):
        got, norm = _residual(system, dev, rhs)
        want, norm_one = _residual(one, ref, rhs)
        out[f"res{rhs}"] = bool(np.array_equal(got, want.reshape(2 * m, n)[pick].ravel()))
        out[f"res{rhs}_nonzero"] = bool(np.abs(got).max() > 0)
        out[f"norm{rhs}"], out[f"norm{rhs}_one"] = norm, norm_one
    out["n_entries"] = 2 * m * n

    # -- composition: a recipe for a row of another rank first (nothing may be written), then
    # every owned block of the full recipe list
    unset = system.info()["blocks_unset"]
    foreign = [r for r in full_one if not lo <= r[1] < hi][:1]
    try:
        dev.relinearise(recipes=full[:1] + foreign)
        out["foreign"] = "accepted"
    except _lib.KktError as e:
        out["foreign"] = (e.code, str(e))
    out["foreign_wrote_nothing"] = bool(unset > 0 and system.info()["blocks_unset"] == unset)
    dev.relinearise(recipes=full)
    ref.relinearise(recipes=full_one)
    blocks_equal, n_blocks = system.info()["blocks_unset"] == 0, 0
    for (q, i, j, *_) in full_one:
        if lo <= i < hi:
            a, pad_a = system.block_values(q, i, j)
            b, pad_b = one.block_values(q, i, j)
            blocks_equal = blocks_equal and pad_a and pad_b and np.array_equal(a, b)
            n_blocks += 1
    out["blocks_equal"], out["n_blocks"] = bool(blocks_equal), n_blocks
    out["n_recipes"], out["n_full"] = len(full), len(full_one)
    out["default_recipes_owned"] = bool(dev.recipes[1] > 0 and dev.recipes[1] < ref.recipes[1])

    # -- update: dyadic blocks, the same global update on every rank
    U = rng.integers(-16, 17, size=(2 * m, n)) / 8.0
    cn = int(CN)
    v, zeta = [a.copy() for a in state]
    v[cn:cn + m] += U[:m]                     # unknown block i: v at level i (CN: i + 1)
    v[:, nodes] = state[0][:, nodes]          # the boundary values stay
    zeta[:m] += U[m:]
    zeta[:m, nodes] = 0.0                     # (CN: the last level is not an unknown)
    with _Vec(system, U[pick].ravel()) as d:
        dev.update(d.d)
        out["u_zeroed"] = bool(not d.get().any())
    with _Vec(one, U.ravel()) as d:
        ref.update(d.d)
    wv, wz = dev.debug_array("v"), dev.debug_array("zeta")
    blocks_v = [lev - v0 for lev in range(lo + cn, hi + cn)]
    out["update_owned"] = bool(np.array_equal(wv[blocks_v], v[lo + cn:hi + cn])
                               and np.array_equal(wz[:nl], zeta[lo:hi]))
    out["update_changed"] = bool(not np.array_equal(wv[blocks_v], state[0][lo + cn:hi + cn]))
    out["v_bc_kept"] = bool(np.array_equal(wv[:, nodes], state[0][v0:v1][:, nodes])
                            and np.abs(wv[:, nodes]).min() > 0)
    # zeta is zero on the Dirichlet dofs of the whole window: the owned levels and the halo (CN's
    # fixed last level on the last rank is nobody's unknown and is left as it was)
    unknowns = wz[:-1] if CN and rank == world - 1 else wz
    out["zeta_bc_zero"] = bool(not unknowns[:, nodes].any())
    # the halo slots still hold the levels of before the update ...
    stale_z = state[1][z1 - 1].copy()
    stale_z[nodes] = 0.0
    out["halo_stale"] = bool((rank == 0 or np.array_equal(wv[0], state[0][v0]))
                             and (rank == world - 1 or (np.array_equal(wz[-1], stale_z)
                                                        and not np.array_equal(wz[-1], zeta[z1 - 1]))))
    dev.assemble()           # ... and the next exchange brings the neighbours' updated ones
    out["halo_updated"] = bool(np.array_equal(dev.debug_array("v"), v[v0:v1])
                               and np.array_equal(dev.debug_array("zeta"), zeta[z0:z1]))
    got = dev.get_state()                     # collective: every rank gathers the whole
    want = ref.get_state()
    out["state_gathered"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want))
                                 and all(np.array_equal(a, b) for a, b in zip(got, (v, zeta))))
    system.close()
    one.close()
    return out


def run_rank_kernels(rank, world, conns, CN, out_q):
    """Windows, assembly, residual / right-hand side, composition and update of one rank, on
    triangles and on tetrahedra (Picard), and the assembly with Gauss-Newton coefficients."""
    try:
        tr, comm = _transport(rank, world, conns)
        out = {mesh: _kernels(rank, world, tr, comm, CN, mesh, False)
               for mesh in ("triangles", "tetrahedra")}
        out["newton"] = _kernels(rank, world, tr, comm, CN, "tetrahedra" if CN else "triangles",
                                 True, assembly_only=True)
        out_q.put((rank, "ok", out))
    except Exception as e:   # report instead of hanging the other ranks' pipes
        import traceback
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))


def _loop(ctl, mesh, **kw):
    import reaction_ref
    from control_amd.control import GpuBackend
    norms = ctl.non_linear_solve(solver_parameters=reaction_ref.KAT_SP, lambda_v_bounds=MASS[mesh],
                                 relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                 max_non_linear_iter=30, backend=GpuBackend(schur=SCHUR),
                                 device=True, **kw)
    return norms, ctl._v.copy(), ctl._zeta.copy(), list(ctl.non_linear_info["linear_iterations"])


def run_rank_loop(rank, world, conns, CN, out_q):
    """``Instationary.non_linear_solve(device=True, comm=...)`` against the one-rank device loop:
    triangles, and (BE) tetrahedra."""
    try:
        import reaction_ref
        import reaction_shard_ref as sref
        tr, comm = _transport(rank, world, conns)
        res = {}
        for mesh in ("triangles",) if CN else ("triangles", "tetrahedra"):
            ref = _loop(sref.control(mesh, CN), mesh)
            ctl = sref.control(mesh, CN)
            out = _loop(ctl, mesh, comm=comm, host_allreduce=tr.allreduce)
            nodes = ctl._disc.boundary
            res[mesh] = dict(
                n=len(out[0]), n_ref=len(ref[0]),
                converged=bool(out[0][-1] <= 1.0e-9 * out[0][0]),
                e_norms=float(max(abs(a - b) / b for a, b in zip(out[0], ref[0]))),
                e_norms_bar=float(max(abs(a - b) / (1e-8 * b + 2e-13 * max(1.0, ref[0][0]))
                                      for a, b in zip(out[0], ref[0]))),
                e_norms_abs=float(max(abs(a - b) for a, b in zip(out[0], ref[0]))
                                  / max(1.0, ref[0][0])),
                max_its=reaction_ref.KAT_SP["maximum_iterations"],
                e_v=float(np.abs(out[1] - ref[1]).max() / max(1.0, np.abs(ref[1]).max())),
                e_zeta=float(np.abs(out[2] - ref[2]).max() / max(1.0, np.abs(ref[2]).max())),
                bc_exact=bool(all(np.array_equal(out[1][i, nodes], ctl._bc_values(i)[nodes])
                                  for i in range(ctl._n_t))
                              and np.abs(out[1][:, nodes]).max() > 0),
                zeta_bc_zero=bool(np.all(out[2][:, nodes] == 0.0)),
                its=out[3], its_ref=ref[3], window=ctl.non_linear_info["window"],
                hist=[float(x) for x in out[0]])
        out_q.put((rank, "ok", res))
    except Exception as e:
        import traceback
        out_q.put((rank, "error", traceback.format_exc() + repr(e)))
