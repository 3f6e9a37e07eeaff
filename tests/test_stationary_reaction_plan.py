"""The host side of the stationary scalar device loop (no GPU): the recipes of
``blocks.stationary_build_recipes`` / ``stationary_relinearisation_recipes`` reproduce
``stationary_blocks`` bit for bit, the one-level ``ReactionPlan`` holds ``Stationary._data()``,
``Stationary`` takes a ``fem.ReactionTerm``, and everything ``non_linear_solve(device=True)``
refuses is refused before the GPU is touched.

The term against the callable form of ``tests/test_control_driver.py``: that file's callables go
through ``weighted_mass`` (one ``einsum`` over the points), the term through its operation-by-
operation statement -- two roundings of one quadrature sum (``tests/test_reaction_ref.py``
records the same for the instationary driver).  Measured on ``unit_square_p1(8)``: bit for bit
at the zero iterate both tests of the reference start from; at the standard-normal iterate of
the test 10 of 497 stored entries differ for Picard and 18 for Gauss-Newton, each by a rounding of
an entry of size 1e-2 (0.47 and 0.05 of the bound below).  So the test holds the driver bit for bit to a callable that wraps the same
statement at every iterate, to ``weighted_mass``'s callables bit for bit at the zero iterate, and
to them elsewhere within ``32 u S`` (``reaction_ref.ELEMENT_BAR``) on the reaction part plus the
one rounding with which each side adds its linear part."""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import blocks, fem, relinearise
from control_amd.control import Stationary
from control_amd.reaction import ReactionPlan
from test_control_driver import _gauss_newton_reference_problem

U = reaction_ref.U


def _numpy_block(recipe, M, D, tperm):
    """``fl(fl(alpha D(^T)) + fl(gamma M))``; ``alpha = 0``: ``fl(gamma M)`` -- the statement
    the composition kernel is held to (``tests/test_gpu_reaction_kernels.py::_composed``)."""
    _, _, _, level, alpha, transpose, gamma = recipe
    assert level == 0
    if alpha == 0.0:
        return gamma * M.data
    return alpha * (D.data[tperm] if transpose else D.data) + gamma * M.data


@pytest.mark.parametrize("beta", [2.0 ** -6, 0.3])
@pytest.mark.parametrize("mesh", [(2, 2, 2.0, 2.0), (3, 2, 3.0, 1.0)])
def test_recipes_reproduce_stationary_blocks(mesh, beta):
    disc = fem.rectangle_p1(*mesh)
    wind = lambda X: np.stack([1.0 + X[:, 1], -0.5 - X[:, 0]], axis=1)   # noqa: E731
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5), linear=disc.K + disc.convection(wind))
    v = np.random.default_rng(common.SEED).standard_normal(disc.n_dofs)
    M, D = term.M, term(v, None)
    tperm = relinearise.transpose_permutation(M)
    assert np.any(D.data[tperm] != D.data)                  # D is not symmetric
    want = blocks.stationary_blocks(M, D, beta)
    full = blocks.stationary_build_recipes(beta)
    assert [r[:3] for r in full] == [(q, 0, 0) for q in range(4)]
    for r in full:
        A = want[r[0]][(0, 0)]
        assert np.array_equal(A.indices, M.indices) and np.array_equal(A.indptr, M.indptr)
        assert np.array_equal(_numpy_block(r, M, D, tperm), A.data), r
    relin = blocks.stationary_relinearisation_recipes(beta)
    assert relin == [(1, 0, 0, 0, 1.0, True, 0.0), (2, 0, 0, 0, 1.0, False, 0.0)]
    assert full[0] == (0, 0, 0, 0, 0.0, False, 1.0)
    assert full[3] == (3, 0, 0, 0, 0.0, False, -1.0 / beta)


def _lifted(disc, term, seed=0, **kw):
    rng = np.random.default_rng(common.SEED + seed)
    tables = rng.standard_normal((2, disc.n_dofs))
    return Stationary(disc, term, desired_state=lambda X: tables[0], force_f=lambda X: tables[1],
                      beta=2.0 ** -6, bcs_v=lambda Xb: 0.25 + Xb[:, 0], **kw)


@pytest.mark.parametrize("newton", [False, True])
def test_data_rows_are_the_drivers_data(newton):
    disc = fem.rectangle_p1(3, 2, 3.0, 1.0)
    ctl = _lifted(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)))
    if newton:
        ctl.set_Gauss_Newton()               # needs no forward_jacobian
    plan = ReactionPlan(ctl)
    assert plan.stationary and (plan.n_t, plan.m, plan.CN) == (1, 1, False)
    assert plan.coefficients == ((2.0, 0.0, 1.5) if newton else (2.0, 0.0, 0.5))
    v_d, f = ctl._data()
    assert np.any(v_d[disc.boundary] != 0.0) and np.any(f[disc.boundary] != 0.0)
    v_d[disc.boundary] = 0.0
    f[disc.boundary] = 0.0
    assert plan.data.shape == (2, disc.n_dofs)
    assert np.array_equal(plan.data, np.stack([v_d, f]))
    # what the rows are for: the residual at the zero iterate
    z = np.zeros(disc.n_dofs)
    r0, r1 = ctl.non_linear_res_eval(*ctl._data(), z, z, ctl.construct_D_v(z))
    assert np.array_equal(plan.data, np.stack([r0, r1]))
    d, keep = plan.descriptor()
    assert (d.n_t, d.cn, d.nq) == (1, 0, 7)
    del keep


@pytest.mark.parametrize("newton", [False, True])
def test_the_term_against_the_callable_form(newton):
    ref, disc, v_d, forward, jacobian = _gauss_newton_reference_problem()
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    ctl = Stationary(disc, term, desired_state=v_d, beta=1.0)
    wrapped = Stationary(disc, lambda v: term(v, None), desired_state=v_d, beta=1.0,
                         forward_jacobian=lambda v: term.jacobian(v, None))
    if newton:
        for c in (ctl, ref, wrapped):
            c.set_Gauss_Newton()
    zero = np.zeros(disc.n_dofs)
    assert np.array_equal(ctl.construct_D_v(zero).data, ref.construct_D_v(zero).data)
    assert np.array_equal(ctl.construct_D_v(zero).indices, ref.construct_D_v(zero).indices)
    v = np.random.default_rng(common.SEED + 1).standard_normal(disc.n_dofs)
    got, want = ctl.construct_D_v(v), ref.construct_D_v(v)
    assert np.array_equal(got.data, wrapped.construct_D_v(v).data)
    assert np.array_equal(got.indices, want.indices) and np.array_equal(got.indptr, want.indptr)
    c = term.jacobian_coefficients if newton else term.coefficients
    S = np.bincount(term.scatter, weights=reaction_ref.scales(term, v, c).ravel(),
                    minlength=term.M.nnz)
    # the reaction parts are two roundings of one sum (32 u S between them at the most), and each
    # side adds its linear part with one rounding of a sum no larger than |L| + S (1 + 32 u)
    bound = (reaction_ref.ELEMENT_BAR * U * S
             + 2.0 * U * (np.abs(term.L.data) + S) * (1 + 2.0 ** -40))
    ratio = float((np.abs(got.data - want.data) / bound).max())
    print(f"newton={newton}: {(got.data != want.data).sum()} of {got.nnz} entries differ, worst "
          f"difference / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_the_host_loop_takes_the_term():
    """Picard and Gauss-Newton on the host with the declared term, against the callable form."""
    out = []
    for declared in (False, True):
        ref, disc, v_d, _, _ = _gauss_newton_reference_problem()
        ctl = Stationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d,
                         beta=1.0) if declared else ref
        ctl.set_Gauss_Newton()
        norms = ctl.non_linear_solve(solver_parameters=reaction_ref.KAT_SP,
                                     lambda_v_bounds=(0.5, 2.0), max_non_linear_iter=30,
                                     relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                     backend=common.OracleBackend(schur=(40, 0.02, 2.2)))
        out.append((norms, ctl._v.copy(), ctl._zeta.copy()))
    assert len(out[0][0]) == len(out[1][0])
    assert np.abs(out[0][1] - out[1][1]).max() < 1e-9
    assert np.abs(out[0][2] - out[1][2]).max() < 1e-9


def test_what_is_refused_is_refused_without_a_gpu():
    disc = fem.unit_square_p1(4)
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    v_d = lambda X: X[:, 0]   # noqa: E731
    ctl = Stationary(disc, lambda v: disc.K + 2.0 * disc.M, desired_state=v_d)
    with pytest.raises(ValueError, match="ReactionTerm"):
        ctl.non_linear_solve(device=True)
    ctl = Stationary(disc, term, desired_state=v_d)
    with pytest.raises(ValueError, match="P="):
        ctl.non_linear_solve(device=True, P=lambda *a: None)
    with pytest.raises(ValueError, match="GpuBackend"):
        ctl.non_linear_solve(device=True, backend=common.OracleBackend(schur=(40, 0.02, 2.2)))
    other = fem.unit_square_p1(4)
    ctl = Stationary(other, term, desired_state=v_d)
    with pytest.raises(ValueError, match="another discretisation"):
        ctl.non_linear_solve(device=True)
    with pytest.raises(ValueError, match="another discretisation"):
        ReactionPlan(ctl)
    th = fem.rectangle_p2p1(2, 2)
    ctl = Stationary(th, None, desired_state=lambda X: np.zeros(th.n_v))
    with pytest.raises(ValueError):
        ctl.non_linear_solve(device=True)
    ctl._forward = term            # a term on a Taylor-Hood discretisation: still not offered
    with pytest.raises(ValueError, match="Taylor-Hood"):
        ctl.non_linear_solve(device=True)
    # the host path is as it was: a callable without a derivative has no Gauss-Newton
    ctl = Stationary(disc, lambda v: disc.K, desired_state=v_d)
    with pytest.raises(ValueError, match="forward_jacobian"):
        ctl.set_Gauss_Newton()
