"""``fem.ReactionTerm`` on P1 tetrahedra, on the host (no GPU): Stroud's 15-point rule against the
exact integrals of the barycentric monomials, the element matrices against the exact rational sums
of ``tests/reaction3d_ref.py`` (which derives the bar of ``64 u S``), the assembled matrices against
the mass matrix, the ordered gather on tetrahedra, ``box_p1(n, n, n)`` against ``unit_cube_p1(n)`` -- and the
triangle branch against its statement written out here, bit for bit."""
import itertools
import math

import numpy as np
import pytest

import common
import reaction3d_ref as ref
from control_amd import fem, relinearise

U = ref.U
BAR = ref.ELEMENT_BAR_TET


# ------------------------------------------------------------------------------- the rule
def _monomial_sum(lam, wq, alpha):
    return float((wq * np.prod(lam ** np.array(alpha), axis=1)).sum())


def _monomial_integral(alpha):
    """``int lam^alpha`` over a tetrahedron of volume 1: ``6 alpha! / (|alpha| + 3)!``."""
    return 6.0 * math.prod(math.factorial(a) for a in alpha) / math.factorial(sum(alpha) + 3)


def test_stroud_rule_weights_and_points():
    lam, wq = fem._stroud_rule()
    assert lam.shape == (15, 4) and wq.shape == (15,)
    assert np.all(wq > 0.0) and abs(wq.sum() - 1.0) <= 4 * U
    assert np.all(np.abs(lam.sum(axis=1) - 1.0) <= 4 * U) and np.all(lam > 0.0)
    # the order of the points: centroid, two orbits of four, the six edge points
    assert np.array_equal(lam[0], np.full(4, 0.25))
    for first in (1, 5):
        for k in range(4):
            row = lam[first + k]
            assert np.all(np.delete(row, k) == row[(k + 1) % 4]) and row[k] != row[(k + 1) % 4]
    pairs = list(itertools.combinations(range(4), 2))
    for r, (i, j) in enumerate(pairs):
        row = lam[9 + r]
        assert row[i] == row[j] < 0.25 and np.all(np.delete(row, [i, j]) > 0.25)


def test_stroud_rule_is_exact_to_degree_five_and_not_six():
    lam, wq = fem._stroud_rule()
    worst = 0.0
    for degree in range(6):
        for alpha in itertools.product(range(degree + 1), repeat=4):
            if sum(alpha) == degree:
                exact = _monomial_integral(alpha)
                worst = max(worst, abs(_monomial_sum(lam, wq, alpha) - exact) / exact)
    print(f"degree <= 5: worst relative error {worst / U:.2f} u")
    assert worst <= 16 * U
    off = [abs(_monomial_sum(lam, wq, alpha) - _monomial_integral(alpha))
           / _monomial_integral(alpha)
           for alpha in itertools.product(range(7), repeat=4) if sum(alpha) == 6]
    print(f"degree 6: worst relative error {max(off):.3g}")
    assert max(off) > 1e-3


# ----------------------------------------------------------------------- element matrices
@pytest.mark.parametrize("kind", ref.ITERATES)
@pytest.mark.parametrize("box", list(ref.BOXES))
def test_host_element_matrices_are_exact_to_the_bar(box, kind):
    disc = fem.box_p1(*ref.BOXES[box])
    v = ref.iterate(kind, disc, seed=common.SEED)
    worst = 0.0
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        for l, (X, S) in enumerate(ref.exact_elements(box, kind, c, common.SEED)):
            E = term.element_matrices(v[l])
            assert E.shape == (len(term.cells), 4, 4)
            r = ref.worst_ratio(E, X, S)
            worst = max(worst, r)
        print(f"{box} {kind} c={c}: worst err / (u S) so far = {worst:.2f}")
    print(f"{box} {kind}: worst ratio {worst:.2f}")
    assert worst <= BAR


def test_volumes_and_tables():
    for box, (nx, ny, nz, lx, ly, lz) in ref.BOXES.items():
        disc = fem.box_p1(*ref.BOXES[box])
        term = fem.ReactionTerm(disc, (1.0,))
        assert term.cells.shape == (6 * nx * ny * nz, 4) and term.W.shape == (len(term.cells), 15)
        assert abs(term.volume.sum() - lx * ly * lz) <= 1e-14 * lx * ly * lz
        assert np.array_equal(term.W, term.wq[None, :] * term.volume[:, None])
        assert disc.coords.shape == ((nx + 1) * (ny + 1) * (nz + 1), 3)
        i, j, k = nx, 1, nz - 1                       # node (i, j, k) at (k (ny+1) + j)(nx+1) + i
        at = (k * (ny + 1) + j) * (nx + 1) + i
        assert np.allclose(disc.coords[at], [lx, ly / ny, lz * (nz - 1) / nz], rtol=1e-15)


def test_a_unit_coefficient_gives_the_mass_matrix():
    """Connectivity, scatter and volume in one line: the rule integrates ``lam_a lam_b`` exactly."""
    for box in ref.BOXES.values():
        disc = fem.box_p1(*box)
        term = fem.ReactionTerm(disc, (1.0,))
        v = np.random.default_rng(common.SEED).standard_normal(disc.n_dofs)
        C = term.reaction_values(v)
        assert np.all(np.abs(C - disc.M.data) <= 1e-14 * np.abs(disc.M.data))
        got = term(v, 0.0)
        assert np.array_equal(got.data, term.L.data + C)
        assert np.array_equal(got.indices, disc.M.indices)
        newton = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
        assert np.array_equal(newton.jacobian(v, 0.0).data,
                              fem.ReactionTerm(disc, (2.0, 0.0, 1.5))(v, 0.0).data)


def test_gather_on_tetrahedra_is_bincount_bit_for_bit():
    disc = fem.box_p1(*ref.BOXES["flat"])
    term = fem.ReactionTerm(disc, ref.COEFFICIENTS[2])
    cptr, clist = relinearise.contribution_lists(term.cells, term.M)
    assert cptr[-1] == len(clist) == 16 * len(term.cells)
    for kind in ref.ITERATES:
        E = term.element_matrices(ref.iterate(kind, disc, seed=common.SEED)[0])
        want = np.bincount(term.scatter, weights=E.ravel(), minlength=term.M.nnz)
        assert np.array_equal(relinearise.gather(E, cptr, clist), want)


def test_the_unit_box_is_the_unit_cube_with_its_cells():
    """``box_p1(n, n, n)`` is ``unit_cube_p1(n)`` array for array, and its cells are the Kuhn
    tetrahedra those matrices were assembled from.  ``unit_cube_p1`` itself is as it was: no
    cells, and a ``ReactionTerm`` on it is refused (``tests/test_reaction_plan.py``)."""
    disc, box = fem.unit_cube_p1(3), fem.box_p1(3, 3, 3)
    assert box.cells.shape == (162, 4)
    M, K = fem._p1_simplex_assemble(box.coords, box.cells)
    for got, mine, want in ((M, box.M, disc.M), (K, box.K, disc.K)):
        for A in (got, mine):
            assert np.array_equal(A.indptr, want.indptr) and np.array_equal(A.indices, want.indices)
            assert np.array_equal(A.data, want.data)
    assert np.array_equal(box.coords, disc.coords) and np.array_equal(box.boundary, disc.boundary)
    assert disc.cells is None
    with pytest.raises(ValueError, match="triangles.*tetrahedra"):
        fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    with pytest.raises(NotImplementedError):          # no 3-D weighted mass on the host
        box.weighted_mass(lambda lam, cells: np.ones((len(cells), len(lam))))


# ------------------------------------------------------------------- the triangle branch
def test_the_triangle_branch_is_unchanged_bit_for_bit():
    """Tables and element matrices from ``_radon_rule()`` by the triangle statement written out."""
    disc = fem.rectangle_p1(3, 2, 3.0, 1.0)
    lam, wq = fem._radon_rule()
    X = disc.coords[disc.cells]
    d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    W = wq[None, :] * area[:, None]
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        assert np.array_equal(term.lam, lam) and np.array_equal(term.wq, wq)
        assert np.array_equal(term.area, area) and np.array_equal(term.W, W)
        for kind in ref.ITERATES:
            v = ref.iterate(kind, disc, seed=common.SEED)[0]
            vc = v[disc.cells]
            v0, v1, v2 = vc[:, 0], vc[:, 1], vc[:, 2]
            E = np.zeros((len(disc.cells), 3, 3))
            for q in range(7):
                s = (lam[q, 0] * v0 + lam[q, 1] * v1) + lam[q, 2] * v2
                g = np.full(len(s), c[-1])
                for k in range(len(c) - 2, -1, -1):
                    g = g * s + c[k]
                wg = W[:, q] * g
                for a in range(3):
                    wa = wg * lam[q, a]
                    for b in range(3):
                        E[:, a, b] += wa * lam[q, b]
            assert np.array_equal(term.element_matrices(v), E)
            assert np.array_equal(
                term.reaction_values(v),
                np.bincount(term.scatter, weights=E.ravel(), minlength=term.M.nnz))


def test_other_cells_are_refused():
    disc = fem.box_p1(1, 1, 1)
    for cells in (np.zeros((2, 5), dtype=np.int32), np.zeros((2, 2), dtype=np.int32), None):
        bad = fem.SpatialDiscretisation(disc.M, disc.K, disc.coords, disc.boundary, "bad", cells)
        with pytest.raises(ValueError, match="triangles.*tetrahedra"):
            fem.ReactionTerm(bad, (1.0,))
