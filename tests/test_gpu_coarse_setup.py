"""Coarse set-up of the two-grid solves on the device: the Galerkin matrices P^T A P of all level
matrices of a build in one launch and their inverses by a blocked Gauss-Jordan over the batch
(kkt_coarse_setup_stats), against the previous column-by-column path (option "coarse_setup" =
"columns").  The Galerkin products of the two paths are equal bit for bit (same summation
orders); the inverses differ by round-off of two elimination orders."""
import numpy as np
import pytest
import scipy.sparse as sp

import coarse_ref
import common
import spectrum_ref
from control_amd._lib import KktError
from control_amd.coarse import multilinear_coarse_space

pytestmark = pytest.mark.gpu

MASS = (20, 0.5, 2.0)
SCHUR = (8, 0.07, 2.1)


def _apply(p, P, cycles, columns, x):
    g = common.gpu_system(p, options={"coarse_setup": "columns"} if columns else None)
    y = g.pc_apply(x, common.gpu_pc(p, MASS, SCHUR, coarse=(P, cycles)))
    return y, g.coarse_setup_stats()


def _batched_against_columns(p):
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=8)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    ref, st_ref = _apply(p, P, 2, True, x)
    got, st = _apply(p, P, 2, False, x)
    # one inverse per distinct value set among the matrices that are solved with
    assert st["matrices"] == st_ref["matrices"] == spectrum_ref.distinct_solved_matrices(p)
    assert st["n_coarse"] == P.shape[1]
    assert st["launches"] < st_ref["launches"]
    assert common.rel_err(got, ref) < 1e-11
    return st


# (time-invariant CN: test_batched_setup_of_cn_inverts_only_the_solved_matrix)
@pytest.mark.parametrize("time_dependent,CN", [(False, False), (True, False), (True, True)])
def test_batched_setup_matches_the_column_path(CN, time_dependent):
    """P1, shared interior levels (three distinct matrices for BE) and a forward operator that
    differs per level (one matrix per level)."""
    p = common.heat_problem(n=48, n_t=6, CN=CN, beta=1e-4, time_dependent=time_dependent)
    st = _batched_against_columns(p)
    assert st["matrices"] >= 3


def test_batched_setup_of_cn_inverts_only_the_solved_matrix():
    """Time-invariant CN solves with one value set (every level's forward and backward matrices
    are equal): exactly one inverse.  c M~ and the upper blocks h K^T + (c - 1) M are only
    multiplied with and get none."""
    p = common.heat_problem(n=48, n_t=6, CN=True, beta=1e-4)
    st = _batched_against_columns(p)
    assert st["matrices"] == 1


def test_stokes_setup_matches_the_column_path():
    """P2 two-component velocity sub-solves (block-diagonal E) and the K_p solve with its
    constants deflated."""
    p = common.stokes_problem(n=8, n_t=4)
    th = p["th"]
    Pv = multilinear_coarse_space(np.vstack([th.coords_v, th.coords_v]), th.boundary_v, cells=4)
    Pp = multilinear_coarse_space(th.coords_p, (), cells=3)
    specs = dict(common.STOKES_SPECS, kp=(6, 0.15, 2.1))
    x = common.rng_vector(2 * p["m"] * (th.n_v + th.n_p))
    out = {}
    for columns in (True, False):
        opts = {"coarse_setup": "columns"} if columns else None
        outer, gpc = common.stokes_gpu(p, specs, options=opts, coarse=(Pv, 1), kp_coarse=(Pp, 2))
        out[columns] = (outer.pc_apply(x, gpc), outer.coarse_setup_stats())
    assert out[False][1]["matrices"] == 1 and out[False][1]["n_coarse"] == Pp.shape[1]
    # (the deflated K_p inverse amplifies round-off: the oracle parity bar of this solve is 1e-4)
    assert common.rel_err(out[False][0], out[True][0]) < 1e-8


def test_two_grid_solve_with_the_batched_setup():
    """FGMRES with the batched set-up converges like the column path's (stopping test on the true
    residual, well below the comparison bar: two Krylov trajectories separate by round-off)."""
    p = common.heat_problem(n=64, n_t=8, beta=1e-2)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=8)
    m, nx = p["m"], p["sd"].n_dofs
    b = common.rng_vector(2 * m * nx).reshape(2 * m, nx)
    b[:, p["nodes"]] = 0.0
    sp_ = {"linear_solver": "fgmres", "fgmres_restart": 10, "maximum_iterations": 300,
           "relative_tolerance": 1e-10, "absolute_tolerance": 0.0, "monitor_convergence": False,
           "preconditioner": True}
    res = {}
    for columns in (True, False):
        g = common.gpu_system(p, options={"coarse_setup": "columns"} if columns else None)
        u = [np.zeros((m, nx)), np.zeros((m, nx))]
        r = g.solve(*u, b[:m].copy(), b[m:].copy(), solver_parameters=sp_,
                    pc_fn=common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2)))
        assert r.reason > 0
        res[columns] = (r.its, np.vstack(u))
    # (iteration counts are not compared: close to the attainable residual two trajectories
    # stagnate at different steps)
    assert common.rel_err(res[False][1], res[True][1]) < 1e-6


def test_launch_count_on_256_squared():
    """Three 1 089^2 Galerkin matrices (first, interior and last level of BE): the batched
    set-up issues at most 200 launches for all of them.  The benchmark's own coarse size, where
    every row loop of the panel kernel takes a second trip: each kept inverse against the
    extended-precision inverse of its kept matrix on sampled columns, and its residual over all
    entries, within 8 times what float64 attains (tests/coarse_ref.py)."""
    p = common.heat_problem(n=256, n_t=6, beta=1e-4)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=32)    # cells of 8 mesh widths
    assert P.shape[1] == 1089
    g = common.gpu_system(p, options={"coarse_keep": "1"})
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    g.pc_apply(x, common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2)))
    st = g.coarse_setup_stats()
    print("coarse set-up 256^2:", st)
    assert st["matrices"] == 3 and st["n_coarse"] == 1089
    assert st["launches"] <= 200
    E, inv = g.coarse_matrices(), g.coarse_inverses()
    assert E.shape == inv.shape == (3, 1089, 1089)
    for b in range(3):
        r_d, r_rho, change = coarse_ref.inverse_ratios(E[b], inv[b])
        print(f"1 089^2 inverse {b}: distance ratio {r_d:.3g}, residual ratio {r_rho:.3g}")
        assert change <= 2.0 ** -60
        assert r_d <= 8 and r_rho <= 8, (b, r_d, r_rho)


@pytest.mark.parametrize("eps", [0.0, 1e-15])
def test_singular_coarse_matrix_names_the_column(eps):
    """A coarse function supported on Dirichlet rows only (eps = 0: a zero row and column of
    P^T A P) or almost only (weight eps on one free node: row and column of E of size ~eps of
    max|diag E|, not zero -- an exact-zero pivot test misses it)."""
    p = common.heat_problem(n=24, n_t=4, beta=1e-4)
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=6))
    nodes = np.asarray(p["nodes"])
    free = np.setdiff1d(np.arange(P.shape[0]), nodes)[0]
    rows = np.append(nodes, free)
    vals = np.append(np.ones(len(nodes)), eps)
    extra = sp.csr_matrix((vals, (rows, np.zeros(len(rows), dtype=int))), shape=(P.shape[0], 1))
    P2 = sp.hstack([P[:, :5], extra, P[:, 5:]]).tocsr()
    g = common.gpu_system(p)
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    with pytest.raises(KktError, match="column 5"):
        g.pc_apply(x, common.gpu_pc(p, MASS, SCHUR, coarse=(P2, 1)))


def _convection_problem(n=40, n_t=6, beta=1e-4, scale=1.0):
    """Heat-control blocks with a forward operator K_i = K + 0.1 i M + w_i C per level, C
    skew-symmetric on K's structure: distinct, non-symmetric level matrices."""
    from control_amd.blocks import instationary_blocks
    from control_amd.fem import unit_square_p1
    sd = unit_square_p1(n)
    K = sp.csr_matrix(sd.K)
    C = sp.triu(K, 1) - sp.tril(K, -1)
    T = 2.0
    tau = T / (n_t - 1.0)
    Ks = [(K + (0.1 * i) * sd.M + (0.3 * scale * (1 + i)) * C).tocsr() for i in range(n_t)]
    b00, b01, b10, b11, m = instationary_blocks(sd.M, Ks, tau, beta, n_t, False, share=True)
    return dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=False, m=m,
                blocks=(b00, b01, b10, b11), nodes=sd.boundary)


def test_galerkin_matrices_equal_the_column_path_and_scipy():
    """Per-level convection (distinct, non-symmetric matrices): the batched Galerkin matrices equal
    the column path's entry by entry, and pair off one to one with P^T D A D P of SciPy (D: the
    free rows) over every matrix A = blk + c M the sub-solves solve with, within 1e-12 of max|E|."""
    p = _convection_problem()
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=5))
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    E = {}
    for columns in (True, False):
        opts = {"coarse_keep": "1"}
        if columns:
            opts["coarse_setup"] = "columns"
        g = common.gpu_system(p, options=opts)
        g.pc_apply(x, common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2)))
        E[columns] = g.coarse_matrices()
    # (one matrix per level for the forward sweep, one for the adjoint sweep)
    assert E[False].shape[0] >= p["n_t"] and E[False].shape[1] == P.shape[1]
    assert np.array_equal(E[False], E[True])               # bit for bit
    free = np.ones(P.shape[0])
    free[np.asarray(p["nodes"])] = 0.0
    D = sp.diags(free)
    # every matrix the sub-solves solve with, each distinct value set once
    refs, seen = [], set()
    for _, i, blk, c in spectrum_ref.schur_solve_map("BE", p["blocks"], p["m"], p["tau"], p["beta"]):
        key = spectrum_ref.value_key(blk, c)
        if key in seen:
            continue
        seen.add(key)
        A = sp.csr_matrix(blk) + c * sp.csr_matrix(p["sd"].M)
        refs.append((P.T @ (D @ A @ D) @ P).toarray())
        if 1 <= i < p["n_t"] - 1:                                         # non-symmetric
            assert np.abs(refs[-1] - refs[-1].T).max() > 1e-6 * np.abs(refs[-1]).max()
    assert len(refs) == len(E[False])
    # one-to-one: every kept matrix has exactly one reference, every reference one kept matrix
    match = np.array([[np.abs(e - r).max() < 1e-12 * np.abs(r).max() for r in refs]
                      for e in E[False]])
    assert (match.sum(axis=1) == 1).all() and (match.sum(axis=0) == 1).all(), match


def test_dense_inverse_matches_numpy():
    """The batched blocked Gauss-Jordan against numpy.linalg.inv: a batch of distinct matrices
    that need row swaps (random, permuted, anti-diagonal), sizes below, at and across the panel
    width of 32."""
    p = common.heat_problem(n=8, n_t=4)
    g = common.gpu_system(p)
    rng = np.random.default_rng(common.SEED)
    for n in (2, 31, 32, 33, 100, 300):
        perm = np.eye(n)[rng.permutation(n)]
        batch = np.stack([rng.standard_normal((n, n)),
                          3.0 * perm + 0.01 * rng.standard_normal((n, n)),
                          np.fliplr(np.eye(n)) + 1e-3 * rng.standard_normal((n, n)),
                          n * np.eye(n) + rng.standard_normal((n, n))])
        inv, bad = g.debug_dense_inverse(batch)
        assert (bad == n).all(), bad
        for b in range(len(batch)):
            ref = np.linalg.inv(batch[b])
            err = np.linalg.norm(inv[b] - ref) / np.linalg.norm(ref)
            assert err < 1e-10, (n, b, err)


def test_dense_inverse_flags_a_nearly_dependent_column():
    p = common.heat_problem(n=8, n_t=4)
    g = common.gpu_system(p)
    rng = np.random.default_rng(common.SEED)
    n = 70
    A = n * np.eye(n) + rng.standard_normal((n, n))
    B = A.copy()
    B[:, 40] = B[:, 12] + 1e-15 * rng.standard_normal(n)
    _, bad = g.debug_dense_inverse(np.stack([A, B]))
    assert bad[0] == n and bad[1] == 40


def test_rebuild_after_update_block_values_equals_a_fresh_build():
    """New values of the diagonal level blocks (a Picard re-linearisation): the rebuilt
    preconditioner -- batched Galerkin matrices and inverses included -- applies exactly as one
    built from scratch on the new values."""
    p = _convection_problem(n=32)
    q = _convection_problem(n=32, scale=2.0)
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=4))
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)
    g = common.gpu_system(p)
    pc = common.gpu_pc(p, MASS, SCHUR, coarse=(P, 2))
    before = g.pc_apply(x, pc)
    b10 = dict(p["blocks"][2])
    for i in range(p["n_t"]):
        g.update_block_values(2, i, i, q["blocks"][2][(i, i)])
        b10[(i, i)] = q["blocks"][2][(i, i)]
    rebuilt = g.pc_apply(x, pc)
    st = g.coarse_setup_stats()
    fresh_p = dict(p, blocks=(p["blocks"][0], p["blocks"][1], b10, p["blocks"][3]))
    fresh = common.gpu_system(fresh_p).pc_apply(x, common.gpu_pc(fresh_p, MASS, SCHUR, coarse=(P, 2)))
    assert st["matrices"] >= p["n_t"]          # every level matrix was re-formed
    assert common.rel_err(rebuilt, before) > 1e-6
    assert np.array_equal(rebuilt, fresh)
