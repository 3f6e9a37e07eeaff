"""Host side of the stationary Navier-Stokes Picard loop on the device (no GPU):
``fem.ConvectionTerm``, the recipes of the three systems against the host's block constructors
bit for bit, the ``ValueError``s of ``incompressible_non_linear_solve(device=True)`` (raised
before the library is loaded) and the data rows of the one-level plan."""
import numpy as np
import pytest
import scipy.sparse as sp

import common
from control_amd import _lib, blocks, fem, relinearise, stationary_picard
from control_amd.control import GpuBackend, Stationary

MESH = (3, 2, 3.0, 1.0)
NU = 0.1


def _v_d(X):
    return np.concatenate([np.sin(X[:, 0]) * X[:, 1], -np.cos(X[:, 1]) * X[:, 0]])


def _f(X):
    return np.concatenate([X[:, 0] + 2.0 * X[:, 1], X[:, 0] * X[:, 1]])


def _same_structure(A, like):
    return (A.shape == like.shape and np.array_equal(A.indptr, like.indptr)
            and np.array_equal(A.indices, like.indices))


@pytest.mark.parametrize("wind", ["random", "zero"])
def test_convection_term_entry_by_entry(wind):
    th = fem.rectangle_p2p1(*MESH)
    term = fem.ConvectionTerm(th, NU)
    w = (np.random.default_rng(common.SEED).standard_normal(th.n_v) if wind == "random"
         else np.zeros(th.n_v))
    A, Ap = term(w), term.pressure(w)
    assert _same_structure(A, th.K_v) and _same_structure(Ap, th.K_p)      # explicit zeros kept
    Cv, Cp = th.convection_v(w), th.convection_p(w)
    assert _same_structure(Cv, th.K_v) and _same_structure(Cp, th.K_p)
    assert np.array_equal(A.data, NU * th.K_v.data + Cv.data)
    assert np.array_equal(Ap.data, NU * th.K_p.data + Cp.data)
    if wind == "zero":
        assert np.array_equal(A.data, NU * th.K_v.data)
    else:
        assert np.any(A.data != NU * th.K_v.data) and np.any(Ap.data != NU * th.K_p.data)
    # Stationary.construct_D_v calls the one-argument operator: the host path runs unchanged
    ctl = Stationary(th, term, desired_state=_v_d, beta=1.0e-2)
    assert np.array_equal(ctl.construct_D_v(w).data, A.data)


def test_convection_term_needs_element_data():
    with pytest.raises(ValueError, match="element data"):
        fem.ConvectionTerm(fem.unit_square_q2q1(2), NU)


def _evaluate(recipe, M, D):
    """``fl(fl(alpha D(^T)) + fl(gamma M))`` (``fl(gamma M)`` for ``alpha = 0``) on the structure
    of ``M``."""
    *_, level, alpha, transpose, gamma = recipe
    assert level == 0
    if alpha == 0.0:
        return gamma * M.data
    d = blocks._transpose(D).data if transpose else D.data
    return alpha * d + gamma * M.data


@pytest.mark.parametrize("beta", [2.0 ** -6, 1.0e-2])
def test_recipes_reproduce_the_host_blocks(beta):
    th = fem.rectangle_p2p1(*MESH)
    term = fem.ConvectionTerm(th, NU)
    w = np.random.default_rng(common.SEED + 1).standard_normal(th.n_v)
    M_v, M_p = blocks._csr(th.M_v), blocks._csr(th.M_p)
    D_v, D_p = blocks.conform_to(term(w), M_v), blocks.conform_to(term.pressure(w), M_p)
    full = blocks.stationary_incompressible_build_recipes(beta)
    assert list(full) == ["outer", "inner", "commutator"]
    outer = blocks.stationary_incompressible_blocks(M_v, D_v, th.B, beta)
    # row-major dict order of block_00; B / B^T stay host values
    assert [r[:3] for r in full["outer"]] == [(0, i, j) for (i, j) in outer[0]]
    for r in full["outer"]:
        assert np.array_equal(_evaluate(r, M_v, D_v), outer[0][(r[1], r[2])].data), r
    for name, M, D in (("inner", M_v, D_v), ("commutator", M_p, D_p)):
        host = blocks.stationary_blocks(M, D, beta)
        assert full[name] == blocks.stationary_build_recipes(beta)
        assert [r[0] for r in full[name]] == [0, 1, 2, 3]
        for r in full[name]:
            assert r[1:3] == (0, 0)
            want = host[r[0]][(0, 0)]
            assert _same_structure(want, M)
            assert np.array_equal(_evaluate(r, M, D), want.data), (name, r)
    relin = blocks.stationary_incompressible_relinearisation_recipes(beta)
    for name in full:
        assert relin[name] == [r for r in full[name] if r[4] != 0.0]
        assert len(relin[name]) == 2 and {r[5] for r in relin[name]} == {True, False}


def _control(th=None, term=None, **kw):
    th = fem.rectangle_p2p1(*MESH) if th is None else th
    term = fem.ConvectionTerm(th, NU) if term is None else term
    return Stationary(th, term, desired_state=_v_d, force_f=_f, beta=1.0e-2, **kw), th


def test_value_errors_come_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)

    def refused(ctl, match, **kw):
        with pytest.raises(ValueError, match=match):
            ctl.incompressible_non_linear_solve(device=True, **kw)
    th = fem.rectangle_p2p1(*MESH)
    opaque = Stationary(th, lambda w: NU * th.K_v + th.convection_v(w), desired_state=_v_d)
    refused(opaque, "ConvectionTerm")
    ctl, th = _control()
    refused(ctl, "does not take P", P=lambda *a: None)
    refused(ctl, "forward_operator_p", forward_operator_p=lambda w: th.K_p)
    other = fem.ConvectionTerm(fem.rectangle_p2p1(*MESH), NU)
    refused(ctl, "forward_operator_p", forward_operator_p=other.pressure)
    q2 = fem.unit_square_q2q1(2)
    refused(_control(q2, fem.ConvectionTerm(th, NU))[0], "element data")
    refused(ctl, "GpuBackend", backend=common.OracleBackend(schur=(40, 0.01, 2.25)))
    # the term's own pressure passes the checks: the next thing is the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        ctl.incompressible_non_linear_solve(device=True, backend=GpuBackend(),
                                            forward_operator_p=ctl._forward.pressure)
    # a scalar Stationary has no pressure space on either path
    with pytest.raises(ValueError, match="space_p"):
        Stationary(fem.unit_square_p1(2), desired_state=lambda X: X[:, 0]) \
            .incompressible_non_linear_solve(device=True)


def test_plan_of_the_stationary_problem():
    ctl, th = _control()
    pb = stationary_picard.StationaryNavierStokes(ctl)
    plan = relinearise.RelinearisationPlan(pb)
    X = th.coords_v
    assert np.array_equal(plan.data, np.stack([th.M_v @ _v_d(X), th.M_v @ _f(X)]))
    assert plan.data.shape == (2, th.n_v) and np.all(plan.data[:, th.boundary_v].any(axis=1))
    assert (pb.n_t, plan.m, pb.CN, plan.stationary) == (1, 1, False, True)
    d, keep = plan.descriptor()
    assert (d.n_t, d.cn, d.nu, d.beta) == (1, 0, NU, 1.0e-2)
    # the instationary plan's tables are the same code path: the same arrays
    from control_amd import picard
    z = np.zeros((2, th.n_v))
    inst = relinearise.RelinearisationPlan(picard.NavierStokesControl(
        disc=th, nu=NU, beta=1.0e-2, n_t=2, T=1.0, v_d=z, f=z))
    assert not inst.stationary
    for a, b in zip(plan.v_lists + plan.p_lists, inst.v_lists + inst.p_lists):
        assert np.array_equal(a, b)
    assert np.array_equal(plan.K2.data, inst.K2.data) and np.array_equal(plan.B.data, inst.B.data)


def test_the_host_path_takes_the_terms_pressure_by_default(monkeypatch):
    """``forward_operator_p=None`` with a ``ConvectionTerm`` means ``term.pressure`` on the host
    path: the linear solve is handed that operator."""
    ctl, th = _control()
    seen = []

    def linear_solve(nullspace_p=None, *, forward_operator_p=None, **kw):
        seen.append(forward_operator_p)
        ctl._v, ctl._zeta = np.zeros(th.n_v), np.zeros(th.n_v)
        ctl._p, ctl._mu = np.zeros(th.n_p), np.zeros(th.n_p)
    monkeypatch.setattr(ctl, "incompressible_linear_solve", linear_solve)
    ctl.incompressible_non_linear_solve(max_non_linear_iter=1)
    assert seen == [ctl._forward.pressure]
    Ap = seen[0](np.ones(th.n_v))
    assert sp.issparse(Ap) and Ap.shape == (th.n_p, th.n_p)
