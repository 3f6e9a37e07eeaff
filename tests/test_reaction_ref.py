"""``fem.ReactionTerm`` on the host (no GPU): its element matrices against the exact rational
quadrature sums of ``tests/reaction_ref.py`` (``reaction_ref.ELEMENT_BAR`` derives the bar of
``32 u S``), the assembled matrices against the mass matrix and against the callable form of
``tests/test_control_driver.py``, and the host Picard loop with the declared term."""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import fem
from control_amd.blocks import conform_to
from control_amd.control import Instationary

U = reaction_ref.U
BAR = reaction_ref.ELEMENT_BAR
MESHES = [(2, 2, 2.0, 2.0), (4, 4, 2.0, 2.0), (3, 2, 3.0, 1.0)]
COEFFICIENTS = [(2.0, 0.0, 0.5), (2.0, 0.0, 1.5), (1.25, -0.75, 0.5, -2.0, 0.375)]


def _assembled_scale(term, S):
    return np.bincount(term.scatter, weights=S.ravel(), minlength=term.M.nnz)


@pytest.mark.parametrize("nx,ny,lx,ly", MESHES)
def test_host_element_matrices_are_exact_to_the_bar(nx, ny, lx, ly):
    disc = fem.rectangle_p1(nx, ny, lx, ly)
    rng = np.random.default_rng(common.SEED + nx)
    worst = asym = 0.0
    for c in COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        for size in (1.0, 0.1):
            v = size * rng.standard_normal(disc.n_dofs)
            E = term.element_matrices(v)
            S = reaction_ref.scales(term, v)
            r = reaction_ref.worst_ratio(E, reaction_ref.exact_element_matrices(term, v), S)
            print(f"{nx}x{ny} c={c} v x {size}: worst err / (u S) = {r:.2f}")
            worst = max(worst, r)
            # the exact matrix is symmetric: two entries within the bar of one value
            asym = max(asym, float((np.abs(E - E.transpose(0, 2, 1)) / (U * S)).max()))
    print(f"{nx}x{ny}: worst ratio {worst:.2f}, worst asymmetry {asym:.2f} u S")
    assert worst <= BAR
    assert asym <= 2 * BAR


def test_a_constant_coefficient_gives_the_mass_matrix():
    for mesh in MESHES:
        disc = fem.rectangle_p1(*mesh)
        term = fem.ReactionTerm(disc, (1.75,))
        v = np.random.default_rng(common.SEED).standard_normal(disc.n_dofs)
        C = term(v, 0.0).data - term.L.data
        S = _assembled_scale(term, reaction_ref.scales(term, v))
        assert np.all(np.abs(C - 1.75 * term.M.data) <= BAR * U * S)
        assert np.array_equal(term(v, 0.0).indices, disc.M.indices)


@pytest.mark.parametrize("nx,ny,lx,ly", MESHES)
def test_term_agrees_with_the_callable_form(nx, ny, lx, ly):
    """The reaction part against ``weighted_mass`` of the callable form (both are roundings of
    one quadrature sum), and ``D = L + C`` with one rounding per entry."""
    disc = fem.rectangle_p1(nx, ny, lx, ly)
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    v = np.random.default_rng(common.SEED + 1).standard_normal(disc.n_dofs)
    want = conform_to(disc.weighted_mass(
        lambda lam, cells: 2.0 + 0.5 * (v[cells] @ lam.T) ** 2), term.M)
    C = term.reaction_values(v)
    S = _assembled_scale(term, reaction_ref.scales(term, v))
    ratio = float((np.abs(C - want.data) / (U * S)).max())
    print(f"{nx}x{ny}: declared against callable, worst difference {ratio:.2f} u S")
    assert ratio <= BAR
    got = term(v, 0.25)
    assert np.array_equal(got.data, term.L.data + C)
    assert np.array_equal(got.indices, term.M.indices)
    full = disc.K + want
    assert abs(got - full).max() <= 1e-14 * abs(full).max()


def test_jacobian_coefficients_and_linear_part():
    disc = fem.rectangle_p1(3, 2, 3.0, 1.0)
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5), nu=0.5)
    assert term.jacobian_coefficients == (2.0, 0.0, 1.5)
    v = np.random.default_rng(common.SEED + 2).standard_normal(disc.n_dofs)
    newton = fem.ReactionTerm(disc, (2.0, 0.0, 1.5), nu=0.5)
    assert np.array_equal(term.jacobian(v, 0.0).data, newton(v, 0.0).data)
    assert np.array_equal(term.L.data, 0.5 * disc.K.data)
    # a non-symmetric linear part, conformed to the structure of M
    wind = lambda X: np.stack([1.0 + X[:, 1], -X[:, 0]], axis=1)   # noqa: E731
    L = disc.K + disc.convection(wind)
    skew = fem.ReactionTerm(disc, (2.0, 0.0, 0.5), linear=L)
    assert np.array_equal(skew.L.indices, disc.M.indices)
    assert abs(skew.L - L).max() == 0.0 and abs(skew.L - skew.L.T).max() > 0.1
    # Instationary takes the term's derivative when none is given
    ctl = Instationary(disc, term, desired_state=lambda X, t: X[:, 0], n_t=3)
    ctl.set_Gauss_Newton()
    assert np.array_equal(ctl.construct_D_v(v, 0.0).data, newton(v, 0.0).data)


# ------------------------------------------------------------------ the host loop with the term
@pytest.mark.parametrize("CN", [False, True])
def test_host_loop_with_the_declared_term(CN):
    out = []
    for declared in (False, True):
        ctl = reaction_ref.reaction_heat_control(CN, declared)
        norms = ctl.non_linear_solve(solver_parameters=reaction_ref.KAT_SP,
                                     lambda_v_bounds=(0.5, 2.0), max_non_linear_iter=30,
                                     relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                     backend=common.OracleBackend(schur=(40, 0.02, 2.2)))
        out.append((norms, ctl._v.copy(), ctl._zeta.copy()))
    assert len(out[0][0]) == len(out[1][0])
    assert np.abs(out[0][1] - out[1][1]).max() < 1e-9
    assert np.abs(out[0][2] - out[1][2]).max() < 1e-9
