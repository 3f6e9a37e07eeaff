"""Host side of the device build (``GpuLinearSolver(build="device")``, no GPU): the recipes of
``blocks.instationary_build_recipes`` reproduce every block of
``instationary_incompressible_blocks`` but the ``tau B`` couplings, and the keyword's
rejections."""
import numpy as np
import pytest

import common
from control_amd import _lib, blocks, picard
from control_amd.relinearise import RelinearisationPlan, contribution_lists, gather


def _element_matrices(th, w):
    """The element matrices of ``convection_v_data`` / ``convection_p`` (fem.py), as
    tests/test_relinearise_plan.py forms them."""
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


def _device_D(pb, plan, w):
    """``D_v`` (one component) / ``D_p`` data as the device assembles them: the element matrices
    gathered in list order, then ``nu K + C`` with separate roundings."""
    th = pb.disc
    Nv, Np = _element_matrices(th, w)
    cv = gather(Nv, *contribution_lists(th.elem["V"], plan.K2))
    cp = gather(Np, *contribution_lists(th.elem["P"], plan.Kp))
    return pb.nu * plan.K2.data + cv, pb.nu * plan.Kp.data + cp


@pytest.mark.parametrize("CN", [False, True])
def test_build_recipes_reproduce_every_block(CN):
    pb = common.navier_stokes_problem(n=2, n_t=5, CN=CN)
    th, n_t = pb.disc, pb.n_t
    rng = np.random.default_rng(common.SEED)
    v = rng.standard_normal((n_t, th.n_v))
    D = [pb.D_v(v[i]) for i in range(n_t)]
    Dp = [pb.D_p(v[i]) for i in range(n_t)]
    bl = blocks.instationary_incompressible_blocks(th.M_v, D, th.B, th.M_p, Dp, pb.tau, pb.beta,
                                                   n_t, CN)
    plan = RelinearisationPlan(pb)
    rec = blocks.instationary_build_recipes(pb.tau, pb.beta, n_t, CN)
    old = blocks.instationary_relinearisation_recipes(pb.tau, pb.beta, n_t, CN)
    assert rec["m"] == bl["m"]
    ipv, ixv = plan.velocity_pattern()
    ipp, ixp = plan.pressure_pattern()
    # D from fem; the device's gather reproduces it (velocity: bit for bit, pressure: the bar of
    # test_lists_reproduce_the_host_assembly -- np.bincount's order against einsum's there)
    nnz2 = plan.K2.nnz
    for i in range(n_t):
        dv, dp = _device_D(pb, plan, v[i])
        assert np.array_equal(dv, D[i].data[:nnz2]) and np.array_equal(dv, D[i].data[nnz2:])
        assert np.abs(dp - Dp[i].data).max() <= 1e-15 * np.abs(Dp[i].data).max()
    tv = np.concatenate([plan.v_tperm, nnz2 + plan.v_tperm])
    tp = plan.p_tperm
    for name in ("inner", "commutator", "outer"):
        systems = bl[name]
        # the linearised ones among them are the existing recipes
        assert sorted(r for r in rec[name] if r[4] != 0.0) == sorted(old[name])
        pressure = name == "commutator"
        M = (plan.Mp if pressure else th.M_v).data
        seen = set()
        for (q, i, j, level, alpha, transpose, gamma) in rec[name]:
            A = systems[q][(i, j)]
            assert A is not None, (name, q, i, j)
            assert np.array_equal(A.indptr, ipp if pressure else ipv)
            assert np.array_equal(A.indices, ixp if pressure else ixv)
            if alpha == 0.0:
                assert not transpose
                want = gamma * M                        # one product, as the kernel forms it
            else:
                d = (Dp if pressure else D)[level].data
                d = d[tp if pressure else tv] if transpose else d
                want = alpha * d + gamma * M            # two products, one sum
            assert np.array_equal(want, A.data), (name, q, i, j)      # bit for bit
            assert (q, i, j) not in seen
            seen.add((q, i, j))
        # every block of the system has a recipe; the outer system's quadrants 1..3 (tau B^T,
        # tau B, nothing) stay with the host
        for q, blk in enumerate(systems):
            for key, A in blk.items():
                if name == "outer" and q > 0:
                    continue
                assert (A is not None) == ((q, *key) in seen), (name, q, key)
    # what is left: one value set per rectangular coupling
    _, o01, o10, o11 = bl["outer"]
    assert len({id(A) for A in o01.values() if A is not None}) == 1
    assert len({id(A) for A in o10.values() if A is not None}) == 1
    assert all(A is None for A in o11.values())


@pytest.mark.parametrize("CN", [False, True])
def test_recipes_come_in_dict_order(CN):
    """Row-major per quadrant: the order in which ``MultiBlockSystem`` adds blocks, which is the
    order the operator sums them in."""
    rec = blocks.instationary_build_recipes(0.25, 1e-2, 6, CN)
    for name in ("inner", "commutator", "outer"):
        keys = [r[:3] for r in rec[name]]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_build_keyword_rejections():
    pb = common.navier_stokes_problem(n=2, n_t=3)
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb, relinearise="host", build="device")
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb, build="device")            # relinearise defaults to "host"
    with pytest.raises(ValueError):
        picard.GpuLinearSolver(pb, relinearise="device", build="gpu")
    ls = picard.GpuLinearSolver(pb, relinearise="device", build="device")
    assert (ls.relinearise, ls.build) == ("device", "device")
    assert picard.GpuLinearSolver(pb).build == "host"
    with pytest.raises(RuntimeError):      # no host blocks on this path
        ls.linear_solve([], [], np.zeros((6, 1)), np.zeros((6, 1)))


def test_add_block_structure_is_exported():
    lib = _lib.load()
    assert hasattr(lib, "kkt_add_block_structure")
    assert "kkt_add_block_structure" in _lib.SIGNATURES
    assert _lib.Info._fields_[-1][0] == "blocks_unset"       # appended: earlier fields keep place
