"""Host side of the device Picard re-linearisation (``control_amd.relinearise``, no GPU):
the contribution lists reproduce the host convection assembly in its summation order, and the
recipes of ``blocks.instationary_relinearisation_recipes`` rebuild every linearised block."""
import numpy as np
import pytest

import common
from control_amd import blocks, fem, picard
from control_amd.relinearise import (RelinearisationPlan, contribution_lists, gather,
                                     transpose_permutation)


def _element_matrices(th, w):
    """The element matrices of ``convection_v_data`` / ``convection_p`` (fem.py), as they are
    summed there."""
    e = th.elem
    n2 = th.n_v // 2
    V = e["V"]
    wq = np.stack([w[:n2][V] @ e["phi"].T, w[n2:][V] @ e["phi"].T], axis=2)
    adv = np.matmul(e["gphi"], wq[..., None])[..., 0]
    Nv = np.einsum("eq,qa,eqb->eab", e["W"], e["phi"], adv)
    wq = np.stack([e["phi"] @ w[:n2][V].T, e["phi"] @ w[n2:][V].T], axis=2)
    advp = np.einsum("qed,ecd->eqc", wq, e["glam"])
    Np = np.einsum("eq,qa,eqc->eac", e["W"], e["lam"], advp)
    return Nv, Np


@pytest.mark.parametrize("n", [4, 16])
def test_lists_reproduce_the_host_assembly(n):
    th = fem.rectangle_p2p1(n, n, 2.0, 2.0)
    n2 = th.n_v // 2
    K2 = th.K_v[:n2, :n2].tocsr()
    cptr, clist = contribution_lists(th.elem["V"], K2)
    pptr, plist = contribution_lists(th.elem["P"], th.K_p)
    assert cptr[-1] == 36 * len(th.elem["V"]) and pptr[-1] == 9 * len(th.elem["P"])
    assert np.array_equal(np.sort(clist), np.arange(cptr[-1]))
    rng = np.random.default_rng(common.SEED + n)
    for _ in range(3):
        w = rng.standard_normal(th.n_v)
        Nv, Np = _element_matrices(th, w)
        host_v = th.convection_v_data(w)
        dev_v = gather(Nv, cptr, clist)
        # bit for bit: the lists sum in np.bincount's order
        nnz2 = K2.nnz
        assert np.array_equal(dev_v, host_v[:nnz2]) and np.array_equal(dev_v, host_v[nnz2:])
        host_p = th.convection_p(w)
        assert np.array_equal(host_p.indptr, th.K_p.indptr)
        dev_p = gather(Np, pptr, plist)
        assert np.abs(dev_p - host_p.data).max() <= 1e-15 * np.abs(host_p.data).max()


def test_transpose_permutation():
    th = fem.rectangle_p2p1(4, 4)
    rng = np.random.default_rng(common.SEED)
    A = th.K_p.copy()
    A.data = rng.standard_normal(A.nnz)
    t = transpose_permutation(A)
    AT = A.T.tocsr()
    AT.sort_indices()
    assert np.array_equal(A.data[t], AT.data)
    assert np.array_equal(t[t], np.arange(A.nnz))


@pytest.mark.parametrize("CN", [False, True])
def test_recipes_rebuild_every_linearised_block(CN):
    pb = common.navier_stokes_problem(n=2, n_t=5, CN=CN)
    th, n_t = pb.disc, pb.n_t
    rng = np.random.default_rng(common.SEED)
    v = rng.standard_normal((n_t, th.n_v))
    D = [pb.D_v(v[i]) for i in range(n_t)]
    Dp = [pb.D_p(v[i]) for i in range(n_t)]
    bl = blocks.instationary_incompressible_blocks(th.M_v, D, th.B, th.M_p, Dp, pb.tau, pb.beta,
                                                   n_t, CN)
    # the same blocks at another linearisation point: only the recipes' blocks may change
    v2 = rng.standard_normal((n_t, th.n_v))
    bl2 = blocks.instationary_incompressible_blocks(
        th.M_v, [pb.D_v(x) for x in v2], th.B, th.M_p, [pb.D_p(x) for x in v2], pb.tau,
        pb.beta, n_t, CN)
    rec = blocks.instationary_relinearisation_recipes(pb.tau, pb.beta, n_t, CN)
    assert rec["m"] == bl["m"]
    for name, mats, M in (("inner", D, th.M_v), ("commutator", Dp, th.M_p),
                          ("outer", D, th.M_v)):
        systems = bl[name]
        seen = set()
        for (q, i, j, level, alpha, transpose, gamma) in rec[name]:
            A = systems[q][(i, j)]
            Dl = mats[level]
            d = Dl.data[transpose_permutation(Dl)] if transpose else Dl.data
            assert np.array_equal(A.indptr, M.indptr) and np.array_equal(A.indices, M.indices)
            assert np.array_equal(A.data, alpha * d + gamma * M.data), (name, q, i, j)
            seen.add((q, i, j))
        for q, blk in enumerate(systems):
            for key, A in blk.items():
                if A is None or (q, *key) in seen:
                    continue
                B2 = bl2[name][q][key]
                assert (A - B2).count_nonzero() == 0, (name, q, key)
        # every block that changed with the linearisation point has a recipe
        changed = {(q, *key) for q, blk in enumerate(systems) for key, A in blk.items()
                   if A is not None and (A - bl2[name][q][key]).count_nonzero()}
        assert changed <= seen and len(seen) == len(rec[name])


@pytest.mark.parametrize("CN", [False, True])
def test_plan_data_rows(CN):
    """The data rows are the residual at the zero iterate; with them the residual is
    ``data - A x`` row by row (what the device kernel evaluates)."""
    pb = common.navier_stokes_problem(n=2, n_t=4, CN=CN)
    plan = RelinearisationPlan(pb)
    th, m = pb.disc, plan.m
    assert plan.data.shape == (2 * m, th.n_v)
    assert np.all(plan.data[:, th.boundary_v] == 0.0)
    assert np.abs(plan.data).max() > 0.0
    d, keep = plan.descriptor()
    assert d.ne == len(th.elem["V"]) and d.nnz2 == plan.K2.nnz and d.nq == 7


def test_device_path_rejects_what_it_cannot_do():
    pb = common.navier_stokes_problem(n=2, n_t=3)
    q2 = fem.unit_square_q2q1(2)
    pb_q2 = picard.NavierStokesControl(disc=q2, nu=0.1, beta=1e-2, n_t=3, T=1.0,
                                       v_d=np.zeros((3, q2.n_v)), f=np.zeros((3, q2.n_v)))
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb_q2, relinearise="device")
    with pytest.raises(ValueError):
        picard.incompressible_non_linear_solve(pb_q2, None, device=True)
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb, relinearise="sometimes")

    class World2:
        world, rank = 2, 0
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb, relinearise="device", comm=World2(),
                               host_allreduce=lambda a, op: None)
    with pytest.raises(ValueError):    # a host-path solver cannot run the device loop
        picard.incompressible_non_linear_solve(pb, picard.GpuLinearSolver(pb), device=True)
