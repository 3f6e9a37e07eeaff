"""``fem.rectangle_p2`` and ``fem.ReactionTerm`` on P2 triangles, on the host (no GPU): the 5 x 5
conical rule against the exact integrals of the barycentric monomials, the scalar P2 space against
one velocity component of ``rectangle_p2p1`` bit for bit, the term's statement written out here,
known answers from exact polynomial integrals, the element matrices against the exact rational
sums of ``tests/reaction_p2_ref.py`` (which derives the bar of ``64 u S``), and the plan."""
import numpy as np
import pytest

import common
import reaction_p2_ref as ref
from control_amd import fem, relinearise
from control_amd.control import Instationary, Stationary
from control_amd.reaction import ReactionPlan

U = ref.U
BAR = ref.ELEMENT_BAR_P2


def _monomials(degree):
    return [(a, b, degree - a - b) for a in range(degree + 1) for b in range(degree + 1 - a)]


# ------------------------------------------------------------------------------- the rule
def test_conical_rule_weights_and_points():
    lam, wq = fem._conical_rule()
    assert lam.shape == (25, 3) and wq.shape == (25,)
    assert np.all(wq > 0.0) and abs(wq.sum() - 1.0) <= 25 * U
    assert np.all(lam > 0.0) and np.all(lam < 1.0)              # strictly inside the triangle
    assert np.all(np.abs(lam.sum(axis=1) - 1.0) <= 4 * U)
    # point 5 i + j: lam_1 = u_i, lam_2 = (1 - u_i) t_j with both node sets ascending
    l1 = lam[:, 1].reshape(5, 5)
    assert np.all(l1 == l1[:, :1]) and np.all(np.diff(l1[:, 0]) > 0.0)
    t = lam[:, 2].reshape(5, 5) / (1.0 - l1)
    assert np.all(np.diff(t, axis=1) > 0.0) and np.all(np.abs(t - t[0]) <= 4 * U)
    print(f"smallest weight {wq.min():.3g}, smallest barycentric coordinate {lam.min():.3g}")


def test_conical_rule_is_exact_to_degree_nine_and_not_ten():
    """Against ``2 a! b! c! / (a + b + c + 2)!`` in ``Fraction``s from the float tables; the bound
    is ``reaction_p2_ref.monomial_defect_bound``: what tables within 16 units of the exact Gauss
    nodes and weights allow, a 25-term sum per monomial."""
    lam, wq = fem._conical_rule()
    worst, worst_rel = 0.0, 0.0
    for degree in range(10):
        for alpha in _monomials(degree):
            exact = ref.monomial_integral(alpha)
            err = float(abs(ref.monomial_sum(lam, wq, alpha) - exact))
            worst = max(worst, err / ref.monomial_defect_bound(lam, wq, alpha))
            worst_rel = max(worst_rel, err / float(exact))
    print(f"degree <= 9: worst error / bound {worst:.3f}, worst relative error {worst_rel:.2e}")
    assert worst <= 1.0
    off = [float(abs(ref.monomial_sum(lam, wq, alpha) - ref.monomial_integral(alpha)))
           / ref.monomial_defect_bound(lam, wq, alpha) for alpha in _monomials(10)]
    print(f"degree 10: worst error / bound {max(off):.3g}")
    assert max(off) > 1.0e3            # a stronger rule left in by accident would pass degree 10


# -------------------------------------------------------------------------- the space
@pytest.mark.parametrize("mesh", [(2, 2, 1.0, 1.0), (3, 2, 3.0, 0.5)])
def test_rectangle_p2_is_one_velocity_component_of_rectangle_p2p1(mesh):
    disc, th = fem.rectangle_p2(*mesh), fem.rectangle_p2p1(*mesh)
    nx, ny = mesh[:2]
    n2 = (2 * nx + 1) * (2 * ny + 1)
    assert disc.n_dofs == n2 == th.n_v // 2
    for mine, theirs in ((disc.M, th.M_v), (disc.K, th.K_v)):
        want = fem._canonical_csr(theirs[:n2, :n2])
        assert np.array_equal(mine.indptr, want.indptr) and mine.indptr.dtype == np.int32
        assert np.array_equal(mine.indices, want.indices) and mine.indices.dtype == np.int32
        assert np.array_equal(mine.data, want.data)
        other = fem._canonical_csr(theirs[n2:, n2:])           # the second component alike
        assert np.array_equal(mine.data, other.data)
    assert np.array_equal(disc.coords, th.coords_v)
    assert np.array_equal(disc.boundary, th.boundary_v[:len(th.boundary_v) // 2])
    assert disc.boundary.dtype == th.boundary_v.dtype
    cells = disc.cells
    assert cells.shape == (2 * nx * ny, 6) and cells.dtype == np.int32
    assert np.array_equal(cells, th.elem["V"])
    i, j = cells % (2 * nx + 1), cells // (2 * nx + 1)
    assert np.all(i[:, :3] % 2 == 0) and np.all(j[:, :3] % 2 == 0)     # vertices: even indices
    # the midpoints of edges (0,1), (1,2), (0,2), in that order
    X = disc.coords[cells]
    for k, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):
        assert np.array_equal(X[:, 3 + k], 0.5 * (X[:, a] + X[:, b]))
    assert np.diff(disc.M.indptr).max() == 19
    if mesh[0] == mesh[1]:
        unit = fem.unit_square_p2(mesh[0])
        assert np.array_equal(unit.M.data, disc.M.data) and np.array_equal(unit.cells, cells)
    with pytest.raises(NotImplementedError):
        disc.weighted_mass(lambda lam, cells: np.ones((len(cells), len(lam))))
    with pytest.raises(NotImplementedError):
        disc.convection(lambda X: X)


# -------------------------------------------------------------------------- the statement
def test_the_p2_statement_written_out_bit_for_bit():
    disc = fem.rectangle_p2(3, 2, 3.0, 0.5)
    lam, wq = fem._conical_rule()
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    phi = np.stack([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), l2 * (2 * l2 - 1), 4 * l0 * l1,
                    4 * l1 * l2, 4 * l0 * l2], axis=1)
    X = disc.coords[disc.cells[:, :3]]
    d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    W = wq[None, :] * area[:, None]
    ne = len(disc.cells)
    rows = np.repeat(disc.cells, 6, axis=1).ravel()
    cols = np.tile(disc.cells, (1, 6)).ravel()
    M = disc.M
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        assert term.nv == 6 and term.basis.shape == (25, 6) and term.W.shape == (ne, 25)
        assert np.array_equal(term.lam, lam) and np.array_equal(term.wq, wq)
        assert np.array_equal(term.basis, phi)
        assert np.array_equal(term.area, area) and np.array_equal(term.W, W)
        # flat entry e 36 + 6 a + b sits at (cells[e, a], cells[e, b]) of M
        assert term.scatter.shape == (36 * ne,)
        assert np.array_equal(M.indices[term.scatter], cols)
        assert np.all((M.indptr[rows] <= term.scatter) & (term.scatter < M.indptr[rows + 1]))
        for kind in ref.ITERATES:
            v = ref.iterate(kind, disc, seed=common.SEED)[0]
            vc = v[disc.cells]
            E = np.zeros((ne, 6, 6))
            for q in range(25):
                s = ((((phi[q, 0] * vc[:, 0] + phi[q, 1] * vc[:, 1]) + phi[q, 2] * vc[:, 2])
                      + phi[q, 3] * vc[:, 3]) + phi[q, 4] * vc[:, 4]) + phi[q, 5] * vc[:, 5]
                g = np.full(ne, c[-1])
                for k in range(len(c) - 2, -1, -1):
                    g = g * s + c[k]
                wg = W[:, q] * g
                for a in range(6):
                    wa = wg * phi[q, a]
                    for b in range(6):
                        E[:, a, b] = E[:, a, b] + wa * phi[q, b]
            assert np.array_equal(term.element_matrices(v), E)
            C = np.bincount(term.scatter, weights=E.ravel(), minlength=M.nnz)
            assert np.array_equal(term.reaction_values(v), C)
            assert np.array_equal(term(v, 0.0).data, term.L.data + C)
    newton = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    assert np.array_equal(newton.jacobian(v, 0.0).data,
                          fem.ReactionTerm(disc, (2.0, 0.0, 1.5))(v, 0.0).data)


def test_p1_terms_keep_their_tables():
    for disc, rule in ((fem.rectangle_p1(3, 2, 3.0, 1.0), fem._radon_rule),
                       (fem.box_p1(2, 1, 1), fem._stroud_rule)):
        term = fem.ReactionTerm(disc, (1.0,))
        assert term.basis is term.lam and np.array_equal(term.lam, rule()[0])


def test_other_cells_are_still_refused():
    disc = fem.rectangle_p2(1, 1)
    for cells in (np.zeros((2, 5), dtype=np.int32), np.zeros((2, 2), dtype=np.int32),
                  np.zeros((2, 7), dtype=np.int32), None):
        bad = fem.SpatialDiscretisation(disc.M, disc.K, disc.coords, disc.boundary, "bad", cells)
        with pytest.raises(ValueError, match="triangles.*tetrahedra"):
            fem.ReactionTerm(bad, (1.0,))


# -------------------------------------------------------------------------- known answers
# M of rectangle_p2 is a sum of up to six element entries from Radon's tables, relative to the
# same sum of absolute values: W 1; a shape function from a table entry (its rounding carried
# twice, a product, a difference, a product) 4, two of them 8; two products 2; the seven-term
# sum 6; the assembly of at most six entries 5; Radon's tables off by a unit in a weight and in a
# coordinate of a degree-4 integrand 5: 27 -- rounded up to a power of two.
MASS_BAR = 32


@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_a_constant_coefficient_gives_the_mass_matrix(mesh):
    """The rule is exact for degree 4: ``reaction_values`` with ``c = (c0,)`` is ``c0 M``.  Bar:
    the statement's ``64 u S`` and the gather's five additions on the term's side, the rule's
    defect for ``phi_a phi_b`` (``polynomial_defect_bound``), and ``MASS_BAR`` on ``M``'s."""
    disc = fem.rectangle_p2(*ref.MESHES[mesh])
    c0 = 1.75
    term = fem.ReactionTerm(disc, (c0,))
    v = np.random.default_rng(common.SEED).standard_normal(disc.n_dofs)
    C = term.reaction_values(v)
    nnz = disc.M.nnz

    def gathered(Ee):
        return np.bincount(term.scatter, weights=Ee.ravel(), minlength=nnz)
    S = gathered(ref.scales(term, v))
    pair_defect = np.array([[ref.polynomial_defect_bound(term, ref._mul(ref._PHI[a], ref._PHI[b]))
                             for b in range(6)] for a in range(6)])
    defect = gathered(c0 * term.area[:, None, None] * pair_defect[None])
    lam7, wq7 = fem._radon_rule()
    phi7 = np.abs(fem._p2_shape_functions(lam7))
    S_M = gathered(np.einsum("e,q,qa,qb->eab", term.area, wq7, phi7, phi7))
    bound = (BAR + 5) * U * S + defect + c0 * MASS_BAR * U * S_M
    err = np.abs(C - c0 * disc.M.data)
    print(f"{mesh}: worst error / bound {np.max(err / bound):.3f}; worst relative to "
          f"max |M| {err.max() / np.abs(disc.M.data).max():.2e}")
    assert np.all(err <= bound)
    assert np.all(bound <= 1e-12 * c0 * np.abs(disc.M.data).max())   # the bar is no loophole


@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_the_reference_coefficient_against_exact_polynomial_integrals(mesh):
    """``c = (2, 0, 0.5)`` and a P2 iterate: the integrand has degree 8, the rule is exact, and the
    element matrices are the polynomial integrals by the monomial formula -- computed without the
    rule, so the 36 shape-function pairs and the local node order are checked."""
    disc = fem.rectangle_p2(*ref.MESHES[mesh])
    c = (2.0, 0.0, 0.5)
    term = fem.ReactionTerm(disc, c)
    v = np.random.default_rng(common.SEED + 1).standard_normal(disc.n_dofs)
    E = term.element_matrices(v)
    X, defect = ref.true_element_matrices(term, v, c)
    S = ref.scales(term, v)
    err = np.abs(np.vectorize(float)(np.vectorize(ref.Fraction)(E) - X))
    bound = BAR * U * S + defect
    print(f"{mesh}: worst error / bound {np.max(err / bound):.3f}; the rule's share of the bound "
          f"{np.max(defect / bound):.2f}; bound / S at most {np.max(bound / S):.2e}")
    assert np.all(err <= bound)
    # the bar is no loophole: a wrong pair or node order is an error of the order of S (the
    # monomials of the integrand enter the defect with absolute coefficients, hence not 1e-13)
    assert np.all(bound <= 1e-10 * S)
    # a swapped pair of local nodes would be far outside: the vertex and midpoint entries differ
    assert np.abs(E[:, 0, 0] - E[:, 3, 3]).min() > 1e-3 * np.abs(E[:, 0, 0]).max()


# ----------------------------------------------------------------------- element matrices
@pytest.mark.parametrize("kind", ref.ITERATES)
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_host_element_matrices_are_exact_to_the_bar(mesh, kind):
    disc = fem.rectangle_p2(*ref.MESHES[mesh])
    v = ref.iterate(kind, disc, seed=common.SEED)
    worst = 0.0
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        for l, (X, S) in enumerate(ref.exact_elements(mesh, kind, c, common.SEED)):
            E = term.element_matrices(v[l])
            assert E.shape == (len(term.cells), 6, 6)
            worst = max(worst, ref.worst_ratio(E, X, S))
        print(f"{mesh} {kind} c={c}: worst err / (u S) so far = {worst:.2f}")
    assert worst <= BAR


# ----------------------------------------------------------------------------------- plan
def _instationary(disc, term, **kw):
    return Instationary(disc, term, desired_state=lambda X, t: X[:, 0], n_t=3, **kw)


def test_the_plan_on_p2():
    disc = fem.rectangle_p2(3, 2, 3.0, 0.5)
    term = fem.ReactionTerm(disc, ref.COEFFICIENTS[2])
    plan = ReactionPlan(_instationary(disc, term))
    d, keep = plan.descriptor()
    assert d.nq == 25 and d.ne == len(term.cells) and d.n1 == disc.n_dofs
    assert np.array_equal(np.ctypeslib.as_array(d.lam, shape=(25, 6)), term.basis)
    cptr, clist = plan.lists
    assert cptr[-1] == len(clist) == 36 * len(term.cells) and len(cptr) == term.M.nnz + 1
    for kind in ref.ITERATES:
        v = ref.iterate(kind, disc, seed=common.SEED)[0]
        E = term.element_matrices(v)
        assert np.array_equal(relinearise.gather(E, cptr, clist), term.reaction_values(v))
    M = term.M
    assert np.diff(M.indptr).max() == 19
    assert np.array_equal(plan.tperm, relinearise.transpose_permutation(M))
    assert np.array_equal(M.data[plan.tperm], M.T.tocsr().sorted_indices().data)
    assert np.array_equal(plan.tperm[plan.tperm], np.arange(M.nnz))
    del keep
    stationary = ReactionPlan(Stationary(disc, term, desired_state=lambda X: X[:, 0], beta=1.0))
    assert stationary.n_t == 1 and stationary.descriptor()[0].nq == 25


def test_what_is_refused_is_refused_as_before():
    disc = fem.rectangle_p2(2, 2)
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    ctl = _instationary(disc, lambda v, t: disc.K)
    with pytest.raises(ValueError, match="ReactionTerm"):
        ctl.non_linear_solve(device=True)
    ctl = _instationary(disc, term)
    with pytest.raises(ValueError, match="P="):
        ctl.non_linear_solve(device=True, P=lambda *a: None)
    with pytest.raises(ValueError, match="another discretisation"):
        _instationary(fem.rectangle_p2(2, 2), term).non_linear_solve(device=True)
    with pytest.raises(ValueError, match="host_allreduce"):
        class Comm:
            world = 2

            def attach(self, system):
                pass
        ctl.non_linear_solve(device=True, comm=Comm())
