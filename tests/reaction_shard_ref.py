"""What a time shard of the scalar device loop holds and reads, restated in NumPy (DESIGN.md
section 6.6a): the level windows of a rank, the rank's rows of ``Instationary.non_linear_res_eval``
computed from those windows alone, Crank-Nicolson's right-hand side across a shard boundary, and
the small problems the sharded tests run (``tests/test_reaction_shard_ref.py`` on the host,
``tests/sharded_reaction_worker.py`` on the GPU)."""
import numpy as np
import scipy.sparse as sp

M_BLOCKS = 6                # unknown blocks: n_t = 6 (BE), n_t = 7 (CN)
G = (2.0, 0.0, 0.5)         # the reference's reaction coefficient 2 + 0.5 v^2
MESHES = ("triangles", "tetrahedra")


def shard_range(m, rank, world):
    """``kkt_shard_range``: the first ``m % world`` ranks hold one block more."""
    base, extra = divmod(m, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_windows(m, CN, rank, world):
    """Half-open ranges of global levels a rank holds: ``v``, ``zeta``, ``D`` (and the element
    matrices), and its block rows -- the dict of ``DeviceReaction.window``.

    BE (block ``i``: ``v_i``, ``zeta_i``): state row ``i`` reads ``v_{i-1}``, adjoint row ``i``
    reads ``zeta_{i+1}``; level ``-1`` and level ``n_t`` do not exist.  CN (block ``i``:
    ``v_{i+1}``, ``zeta_i``): every row ``i`` reads the levels ``i`` and ``i + 1`` of both."""
    lo, hi = shard_range(m, rank, world)
    if CN:
        w = (lo, hi + 1)
        return {"v": w, "zeta": w, "D": w, "blocks": (lo, hi)}
    return {"v": (max(lo - 1, 0), hi), "zeta": (lo, min(hi + 1, m)), "D": (lo, hi),
            "blocks": (lo, hi)}


def owned_levels(m, CN, rank, world):
    """The levels of ``v`` and of ``zeta`` a rank writes (and downloads): its blocks' levels, CN's
    fixed ``v_0`` on rank 0 and the zero level ``zeta_{n_t-1}`` on the last rank."""
    lo, hi = shard_range(m, rank, world)
    if not CN:
        return range(lo, hi), range(lo, hi)
    return (range(0 if lo == 0 else lo + 1, hi + 1), range(lo, hi + 1 if hi == m else hi))


def poisoned(a, window):
    """``a`` with every level outside the half-open ``window`` replaced by NaN."""
    out = np.full_like(a, np.nan)
    out[window[0]:window[1]] = a[window[0]:window[1]]
    return out


def shard_rows(ctl, w, v, zeta, v_0, v_d, f):
    """The rows ``lo .. hi-1`` of both families of ``Instationary.non_linear_res_eval`` with its
    expressions, from the levels of ``v``, ``zeta`` and ``D`` inside the windows ``w`` only: ``D``
    is built for the levels of ``w["D"]`` and nothing else of the iterate is touched, so NaN
    outside the windows must not reach a row.  ``v_d`` and ``f`` are data, global."""
    disc, n_t, beta, CN = ctl._disc, ctl._n_t, ctl._beta, ctl._CN
    M, nodes = disc.M, disc.boundary
    t_0, _, tau = ctl._times()
    lo, hi = w["blocks"]
    D = {i: sp.csr_matrix(ctl.construct_D_v(v[i], t_0 + i * tau)) for i in range(*w["D"])}
    r0 = np.zeros((hi - lo, disc.n_dofs))
    r1 = np.zeros((hi - lo, disc.n_dofs))
    if CN:
        h = 0.5 * tau
        for i in range(lo, hi):
            r0[i - lo] = (h * (v_d[i] + v_d[i + 1]) - h * (M @ (v[i] + v[i + 1]))
                          - (h * (D[i].T @ zeta[i]) + M @ zeta[i])
                          - (h * (D[i + 1].T @ zeta[i + 1]) - M @ zeta[i + 1]))
            r1[i - lo] = (h * (f[i] + f[i + 1])
                          - (h * (D[i] @ v[i]) - M @ v[i])
                          - (h * (D[i + 1] @ v[i + 1]) + M @ v[i + 1])
                          + (h / beta) * (M @ (zeta[i] + zeta[i + 1])))
    else:
        D_0 = sp.csr_matrix(ctl.construct_D_v(v_0, t_0))
        for i in range(lo, hi):
            Dz = tau * (D[i].T @ zeta[i]) + M @ zeta[i]
            r0[i - lo] = (tau * v_d[i] - tau * (M @ v[i]) - Dz + M @ zeta[i + 1]
                          if i < n_t - 1 else -Dz)
            Dv = tau * (D[i] @ v[i]) + M @ v[i]
            r1[i - lo] = (tau * (D_0 @ v_0) + M @ v_0 - Dv if i == 0 else
                          tau * f[i] + M @ v[i - 1] - Dv + (tau / beta) * (M @ zeta[i]))
    r0[:, nodes] = 0.0
    r1[:, nodes] = 0.0
    return r0, r1


def shard_rhs(r0, r1, up, dn, lo, hi, m):
    """Crank-Nicolson's right-hand side rows ``lo .. hi-1`` from the rank's raw rows and two
    neighbour rows: ``up`` = the raw adjoint row ``hi`` (``T_1`` adds row ``i + 1`` into ``i``),
    ``dn`` = the raw state row ``lo - 1`` (``T_2`` adds row ``i - 1``); either is ignored where
    the global system ends."""
    b0, b1 = r0.copy(), r1.copy()
    b0[:-1] += r0[1:]
    b1[1:] += r1[:-1]
    if hi < m:
        b0[-1] += up
    if lo > 0:
        b1[0] += dn
    return b0, b1


def control(mesh, CN, amplitude=None, lifted=True):
    """The reference's non-linear reaction problem on ``unit_square_p1(4)`` (25 nodes, 32 cells) or
    ``box_p1(3, 3, 3)`` (64 nodes, 162 cells) with six unknown blocks, desired states as in
    ``tests/reaction_ref.py`` (amplitude 1) and ``tests/test_gpu_reaction3d_picard.py`` (8), and
    -- ``lifted`` -- those files' boundary values and initial condition: ``v`` is non-zero on the
    Dirichlet dofs."""
    from control_amd import fem
    from control_amd.control import Instationary
    n_t = M_BLOCKS + 1 if CN else M_BLOCKS
    if mesh == "triangles":
        disc, a = fem.unit_square_p1(4), 1.0 if amplitude is None else amplitude

        def v_d(X, t):
            return a * (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.exp(X[:, 0])
        kw = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0]),
                  initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]))
    else:
        disc, a = fem.box_p1(3, 3, 3), 8.0 if amplitude is None else amplitude

        def v_d(X, t):
            return (a * (1.0 + t) * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1])
                    * np.sin(np.pi * X[:, 2]) * np.exp(X[:, 0]))
        kw = dict(bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * (1.0 + Xb[:, 0] + Xb[:, 2]),
                  initial_condition=lambda X: 0.5 * np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1])
                  * np.sin(np.pi * X[:, 2]))
    return Instationary(disc, fem.ReactionTerm(disc, G), desired_state=v_d, CN=CN, n_t=n_t,
                        time_interval=(0.0, 1.0), beta=1.0e-2, **(kw if lifted else {}))
