"""The (sweep, level) -> (block, shift) map of tests/spectrum_ref.py against the matrices the
oracle's preconditioners actually solve with in one application: every Jacobi-Chebyshev call of
``pc_stationary`` / ``pc_instationary_BE`` / ``pc_instationary_CN`` is recorded, the mass solves
dropped, and each remaining matrix must equal ``assemble_with_bcs(blk + c M)`` of the map entry at
the same position.  The GPU spectrum tests build their dense references from this map."""
import numpy as np
import pytest
import scipy.sparse as sp

import common
import spectrum_ref
from control_amd.blocks import instationary_blocks, stationary_blocks
from control_amd.fem import unit_square_p1


def _record_application(monkeypatch, make_pc, n_mass, nx, n_blocks):
    from oracle import kkt_oracle as ko
    solved, assembled = [], []
    cheb, asm = ko.chebyshev_jacobi, ko.assemble_with_bcs

    def cheb_rec(A, *a, **kw):
        solved.append(A)
        return cheb(A, *a, **kw)

    def asm_rec(A, nodes):
        out = asm(A, nodes)
        assembled.append(out)
        return out
    monkeypatch.setattr(ko, "chebyshev_jacobi", cheb_rec)
    monkeypatch.setattr(ko, "assemble_with_bcs", asm_rec)
    pc = make_pc(ko)
    rng = np.random.default_rng(common.SEED)
    b0, b1 = rng.standard_normal((n_blocks, nx)), rng.standard_normal((n_blocks, nx))
    u0, u1 = np.zeros_like(b0), np.zeros_like(b1)
    pc(u0, u1, b0, b1)
    assert all(A is solved[0] for A in solved[:n_mass])          # the mass solves come first
    return solved[n_mass:], list(assembled)    # (the references below assemble too)


def _check(solved, assembled, expect, M, nodes):
    assert len(solved) == len(expect)
    for A, (sweep, level, blk, c) in zip(solved, expect):
        R = spectrum_ref.assembled(blk, c, M, nodes)
        assert A.shape == R.shape
        assert np.array_equal(A.toarray(), R.toarray()), (sweep, level)
    # one assembly per distinct (block, shift) of the map, besides the mass matrix
    distinct = {(id(blk), c) for _, _, blk, c in expect}
    assert len(assembled) == 1 + len(distinct)


def _convection(n, n_t):
    sd = unit_square_p1(n)
    C = sd.convection(lambda Xq: np.stack([Xq[:, 1] - 0.5, 0.5 - Xq[:, 0]], 1))
    return sd, [(sd.K + (1.0 + 0.2 * i) * C).tocsr() for i in range(n_t)]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("operator", ["shared", "time_dependent", "convection"])
def test_instationary_map_matches_the_oracle(monkeypatch, CN, operator):
    n_t, beta = 5, 1e-2
    if operator == "convection":
        sd, K = _convection(6, n_t)
        tau = 2.0 / (n_t - 1.0)
        b00, b01, b10, b11, m = instationary_blocks(sd.M, K, tau, beta, n_t, CN, share=True)
        p = dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                 nodes=sd.boundary)
    else:
        p = common.heat_problem(n=6, n_t=n_t, CN=CN, beta=beta,
                                time_dependent=operator == "time_dependent")
    sd, m = p["sd"], p["m"]
    mass, schur = (3, 0.5, 2.0), (3, 0.1, 2.0)
    _, b01, b10, _ = p["blocks"]

    def make_pc(ko):
        f = ko.pc_instationary_CN if CN else ko.pc_instationary_BE
        return f(sd.M, b01, b10, p["n_t"], p["tau"], p["beta"], p["nodes"],
                 ko.ChebSpec(*mass), ko.ChebSpec(*schur))
    solved, assembled = _record_application(monkeypatch, make_pc, m, sd.n_dofs, m)
    expect = spectrum_ref.schur_solve_map("CN" if CN else "BE", p["blocks"], m, p["tau"],
                                          p["beta"])
    _check(solved, assembled, expect, sd.M, p["nodes"])
    # the first level of BE solves with the block alone (shift 0), the last with sqrt(eps) shift
    if not CN:
        assert expect[0][3] == 0.0 and expect[m - 1][3] < expect[1][3]


def test_stationary_map_matches_the_oracle(monkeypatch):
    sd = unit_square_p1(6)
    beta = 1e-2
    blocks = stationary_blocks(sd.M, sd.K, beta)

    def make_pc(ko):
        return ko.pc_stationary(sd.M, blocks[2][(0, 0)], blocks[1][(0, 0)], beta, sd.boundary,
                                ko.ChebSpec(3, 0.5, 2.0), ko.ChebSpec(3, 0.1, 2.0))
    solved, assembled = _record_application(monkeypatch, make_pc, 1, sd.n_dofs, 1)
    expect = spectrum_ref.schur_solve_map("stationary", blocks, 1, 1.0, beta)
    _check(solved, assembled, expect, sd.M, sd.boundary)


def test_jacobi_spectra_of_a_known_matrix():
    """The dense reference itself: tridiag(-1, 2, -1) has Jacobi-scaled eigenvalues
    1 - cos(k pi / (n + 1)); adding a skew part leaves the symmetric part's interval alone and
    bounds every |Im lambda| by rho of the scaled skew part (Bendixson)."""
    n = 12
    T = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A = sp.block_diag([sp.identity(1), T, sp.identity(1)]).tocsr()      # bc rows 0 and n + 1
    nodes = [0, n + 1]
    r = spectrum_ref.jacobi_spectra(A, nodes)
    k = np.arange(1, n + 1)
    lam = 1.0 - np.cos(k * np.pi / (n + 1))
    assert r["symmetric"] and r["rho_skew"] == 0.0 and r["n"] == n
    assert np.isclose(r["lmin"], lam.min(), rtol=1e-12) and np.isclose(r["lmax"], lam.max(), rtol=1e-12)
    W = sp.diags([-0.3 * np.ones(n - 1), 0.3 * np.ones(n - 1)], [-1, 1])
    A2 = sp.block_diag([sp.identity(1), T + W, sp.identity(1)]).tocsr()
    r2 = spectrum_ref.jacobi_spectra(A2, nodes)
    assert not r2["symmetric"]
    assert np.isclose(r2["lmin"], lam.min(), rtol=1e-12) and np.isclose(r2["lmax"], lam.max(), rtol=1e-12)
    assert np.isclose(r2["rho_skew"], 0.3 * np.cos(np.pi / (n + 1)), rtol=1e-12)
    assert np.max(np.abs(r2["ev"].imag)) <= r2["rho_skew"] * (1 + 1e-12)
    assert np.all(r2["ev"].real >= r2["lmin"] * (1 - 1e-12))
    assert np.all(r2["ev"].real <= r2["lmax"] * (1 + 1e-12))
