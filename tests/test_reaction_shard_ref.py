"""Time shards of the scalar device loop, on the host: the level windows
of every rank, that a rank's residual rows need nothing of the iterate outside them, Crank-
Nicolson's right-hand side across a shard boundary, and the refusals of
``Instationary.non_linear_solve(comm=...)`` -- none of it touches a GPU."""
import numpy as np
import pytest

import common
import reaction_shard_ref as ref
from control_amd.control import _apply_T_1, _apply_T_2

M = ref.M_BLOCKS


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 6])
def test_windows(world, CN):
    """BE holds v [lo-1, hi), zeta [lo, hi], D [lo, hi) -- without level lo-1 on rank 0 and level
    hi on the last rank; CN holds [lo, hi] of all three, v_0 on rank 0 and the zero level
    zeta_{n_t-1} on the last rank inside them.  The block ranges tile [0, m)."""
    n_t = M + 1 if CN else M
    end = 0
    for rank in range(world):
        w = ref.shard_windows(M, CN, rank, world)
        lo, hi = w["blocks"]
        assert (lo, hi) == ref.shard_range(M, rank, world)
        assert lo == end and hi > lo
        end = hi
        if CN:
            assert w["v"] == w["zeta"] == w["D"] == (lo, hi + 1)
        else:
            assert w["v"] == ((lo - 1, hi) if rank > 0 else (0, hi))
            assert w["zeta"] == ((lo, hi + 1) if rank < world - 1 else (lo, hi))
            assert w["D"] == (lo, hi)
        for k in ("v", "zeta", "D"):
            assert 0 <= w[k][0] < w[k][1] <= n_t
        if world == 1:
            assert w == {"v": (0, n_t), "zeta": (0, n_t), "D": (0, n_t), "blocks": (0, M)}
        if hi - lo == 1 and 0 < rank < world - 1:      # a one-block shard has both halos
            assert w["v"][0] == lo - (0 if CN else 1) and w["zeta"][1] == hi + 1
            assert w["v"][1] - w["v"][0] == 2 and w["zeta"][1] - w["zeta"][0] == 2
        own_v, own_z = ref.owned_levels(M, CN, rank, world)
        assert set(own_v) <= set(range(*w["v"])) and set(own_z) <= set(range(*w["zeta"]))
    assert end == M
    if world == 6:
        assert all(np.diff(ref.shard_windows(M, CN, r, world)["blocks"]) == 1 for r in range(6))
    # every level of both fields is written by exactly one rank
    for k in (0, 1):
        levels = sorted(l for r in range(world) for l in ref.owned_levels(M, CN, r, world)[k])
        assert levels == list(range(n_t))


_STATE = {}


def _global_rows(mesh, CN):
    """The problem, a random iterate and the global rows, computed once per (mesh, scheme)."""
    key = (mesh, CN)
    if key not in _STATE:
        ctl = ref.control(mesh, CN)
        disc, n_t = ctl._disc, ctl._n_t
        rng = np.random.default_rng(common.SEED + 11)
        v, zeta = rng.standard_normal((2, n_t, disc.n_dofs))
        v_0 = np.asarray(ctl._initial_condition(disc.coords), dtype=np.float64)
        v_d, f = ctl.construct_v_d(), ctl.construct_f()
        r0, r1 = ctl.non_linear_res_eval(v, zeta, v_0, v_d, f)
        for a in (v, zeta, r0, r1):
            a.setflags(write=False)
        _STATE[key] = (ctl, v, zeta, v_0, v_d, f, r0, r1)
    return _STATE[key]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_windows_suffice(mesh, world, CN):
    """A rank's rows from arrays that are NaN outside its windows equal the global rows bit for
    bit, and CN's right-hand side from the rank's raw rows plus the two neighbour rows equals
    T_1 / T_2 of the global rows."""
    ctl, v, zeta, v_0, v_d, f, r0, r1 = _global_rows(mesh, CN)
    assert np.abs(r0).max() > 0 and np.abs(r1).max() > 0
    b0, b1 = (_apply_T_1(r0), _apply_T_2(r1)) if CN else (r0, r1)
    for rank in range(world):
        w = ref.shard_windows(M, CN, rank, world)
        lo, hi = w["blocks"]
        vp, zp = ref.poisoned(v, w["v"]), ref.poisoned(zeta, w["zeta"])
        assert np.isnan(vp).any() and np.isnan(zp).any()
        g0, g1 = ref.shard_rows(ctl, w, vp, zp, v_0, v_d, f)
        assert np.array_equal(g0, r0[lo:hi]) and np.array_equal(g1, r1[lo:hi]), (rank, w)
        if CN:
            up = r0[hi] if hi < M else np.full_like(v_0, np.nan)
            dn = r1[lo - 1] if lo > 0 else np.full_like(v_0, np.nan)
            c0, c1 = ref.shard_rhs(g0, g1, up, dn, lo, hi, M)
            assert np.array_equal(c0, b0[lo:hi]) and np.array_equal(c1, b1[lo:hi]), rank


def test_a_window_one_level_short_does_not_suffice():
    """The check above can fail: without the halo level the rows that read it are NaN."""
    ctl, v, zeta, v_0, v_d, f, r0, r1 = _global_rows("triangles", False)
    w = ref.shard_windows(M, False, 1, 3)
    lo, hi = w["blocks"]
    g0, g1 = ref.shard_rows(ctl, w, ref.poisoned(v, (lo, hi)), ref.poisoned(zeta, (lo, hi)),
                            v_0, v_d, f)
    assert np.isnan(g0[-1]).any() and np.isnan(g1[0]).any()
    assert np.array_equal(g0[:-1], r0[lo:hi - 1]) and np.array_equal(g1[1:], r1[lo + 1:hi])


def test_refusals():
    """``comm`` without ``device=True``, more than one rank without ``host_allreduce``, and a
    ``comm`` that is no transport of ``control_amd.dist``: ``ValueError`` before the GPU is
    touched."""
    from control_amd.dist import CallbackComm
    comm = CallbackComm(0, 2, None, None)
    ctl = ref.control("triangles", False)
    with pytest.raises(ValueError, match="not offered on time shards"):
        ctl.non_linear_solve(comm=comm, host_allreduce=lambda a, op: None)
    with pytest.raises(ValueError, match="needs host_allreduce"):
        ctl.non_linear_solve(device=True, comm=comm)

    class NoTransport:
        rank, world = 0, 2
    with pytest.raises(ValueError, match="must be a transport of control_amd.dist"):
        ctl.non_linear_solve(device=True, comm=NoTransport(), host_allreduce=lambda a, op: None)
