"""``fem.rectangle_q2`` and ``fem.ReactionTerm`` on Q2 quadrilaterals, on the host (no GPU): the
element-assembled space against the tensor-product ``unit_square_q2``, the 5 x 5 Gauss-Legendre
product rule against the exact integrals of the tensor monomials, the term's statement written out
here, known answers from exact polynomial integrals, the element matrices against the exact
rational sums (``tests/reaction_q2_ref.py`` derives the bars ``128 u S`` and ``32 u S``), and the
plan with its descriptor.

``unit_square_q2(n)`` stores explicit zeros at ``n = 2, 3``: ``scipy.sparse.kron`` goes through
dense blocks when its second factor is more than half full, which the 1-D matrices on 5 and 7
nodes are.  So its ``indptr`` / ``indices`` are compared with ``rectangle_q2``'s after
``eliminate_zeros`` on a copy -- the entries that are not identically zero sit at the same places
-- and the values of both ``M`` and ``K`` through ``conform_to`` on such copies.
"""
import ctypes as C

import numpy as np
import pytest

import common
import reaction_q2_ref as ref
from control_amd import _lib, fem, relinearise
from control_amd.blocks import conform_to
from control_amd.control import Instationary, Stationary
from control_amd.reaction import ReactionPlan

U = ref.U
BAR = ref.ELEMENT_BAR_Q2


def _absolute_contributions(disc, nx, ny, lx, ly):
    """``M`` and ``K`` of ``rectangle_q2`` with every element entry -- for ``K`` each of its two
    tensor products -- replaced by its absolute value: what ``MESH_BAR`` is relative to."""
    hx, hy = lx / nx, ly / ny
    m = np.abs(np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]]))
    k = np.abs(np.array([[7.0, -8.0, 1.0], [-8.0, 16.0, -8.0], [1.0, -8.0, 7.0]]))
    Mx, My, Kx, Ky = hx / 30.0 * m, hy / 30.0 * m, 1.0 / (3.0 * hx) * k, 1.0 / (3.0 * hy) * k
    ne, n, cells = nx * ny, disc.n_dofs, disc.cells
    SM = fem._assemble_like(np.broadcast_to(np.kron(My, Mx), (ne, 9, 9)), cells, cells, (n, n))
    SK = fem._assemble_like(np.broadcast_to(np.kron(My, Kx) + np.kron(Ky, Mx), (ne, 9, 9)),
                            cells, cells, (n, n))
    return SM, SK


# -------------------------------------------------------------------------- the space
@pytest.mark.parametrize("L", [1.0, 2.0])
@pytest.mark.parametrize("n", [2, 3])
def test_rectangle_q2_is_unit_square_q2_assembled_from_elements(n, L):
    disc, tensor = fem.rectangle_q2(n, n, L, L), fem.unit_square_q2(n, L)
    assert tensor.cells is None                                   # left alone
    assert np.array_equal(disc.coords, tensor.coords) and disc.coords.dtype == tensor.coords.dtype
    assert np.array_equal(disc.boundary, tensor.boundary)
    assert disc.boundary.dtype == tensor.boundary.dtype == np.int32
    nn = 2 * n + 1
    cells = disc.cells
    assert cells.shape == (n * n, 9) and cells.dtype == np.int32
    for ey in range(n):
        for ex in range(n):
            want = [(2 * ey + j) * nn + 2 * ex + i for j in range(3) for i in range(3)]
            assert cells[ey * n + ex].tolist() == want
    assert disc.M.indptr.dtype == disc.M.indices.dtype == np.int32
    assert np.array_equal(disc.M.indptr, disc.K.indptr)
    assert np.array_equal(disc.M.indices, disc.K.indices)
    assert sorted(set(np.diff(disc.M.indptr))) == [9, 15, 25]
    assert np.all(disc.M.data != 0.0)
    stored = tensor.M.copy()
    stored.eliminate_zeros()
    assert np.array_equal(stored.indptr, disc.M.indptr)
    assert np.array_equal(stored.indices, disc.M.indices)
    SM, SK = _absolute_contributions(disc, n, n, L, L)
    worst = {}
    for name, mine, theirs, S in (("M", disc.M, tensor.M, SM), ("K", disc.K, tensor.K, SK)):
        theirs = theirs.copy()
        theirs.eliminate_zeros()
        theirs = conform_to(theirs, disc.M)
        assert np.array_equal(theirs.indices, mine.indices)
        worst[name] = float((np.abs(mine.data - theirs.data) / (U * S.data)).max())
        assert np.all(S.data >= np.abs(mine.data))
    print(f"n={n} L={L}: worst |rectangle_q2 - unit_square_q2| / (u S): M {worst['M']:.2f}, "
          f"K {worst['K']:.2f} (bar {ref.MESH_BAR})")
    assert worst["M"] <= ref.MESH_BAR and worst["K"] <= ref.MESH_BAR
    with pytest.raises(NotImplementedError):
        disc.weighted_mass(lambda lam, cells: np.ones((len(cells), len(lam))))
    with pytest.raises(NotImplementedError):
        disc.convection(lambda X: X)


def test_a_stretched_mesh():
    """``K 1 = 0`` and ``1^T M 1 = lx ly``: every entry is within ``MESH_BAR`` (12 and 10 of it on
    this path) of the exact one, a row sum adds at most 24 additions, the sum of the row sums
    ``n - 1`` more."""
    nx, ny, lx, ly = ref.MESHES["stretched"]
    disc = fem.rectangle_q2(nx, ny, lx, ly)
    assert disc.n_dofs == 35 and len(disc.cells) == 6
    X = disc.coords[disc.cells]
    assert np.array_equal(X[:, 2, 0] - X[:, 0, 0], np.full(6, lx / nx))
    assert np.array_equal(X[:, 6, 1] - X[:, 0, 1], np.full(6, ly / ny))
    assert np.array_equal(X[:, 4], 0.5 * (X[:, 0] + X[:, 8]))             # the centre node
    SM, SK = _absolute_contributions(disc, nx, ny, lx, ly)
    one = np.ones(disc.n_dofs)
    rows = np.abs(disc.K @ one)
    bound = (ref.MESH_BAR + 24) * U * (SK @ one)
    print(f"worst |K 1| / bound {np.max(rows / bound):.3f}")
    assert np.all(rows <= bound)
    total = one @ (disc.M @ one)
    bound = (ref.MESH_BAR + 24 + disc.n_dofs) * U * (one @ (SM @ one))
    print(f"|1^T M 1 - lx ly| / bound {abs(total - lx * ly) / bound:.3f}")
    assert abs(total - lx * ly) <= bound
    assert abs(disc.K - disc.K.T).max() <= 2 * ref.MESH_BAR * U * SK.data.max()


# ------------------------------------------------------------------------------- the rule
def test_gauss_square_rule_weights_points_and_basis():
    pts, wq, basis = fem._gauss_square_rule()
    assert pts.shape == (25, 2) and wq.shape == (25,) and basis.shape == (25, 9)
    assert np.all(wq > 0.0) and abs(wq.sum() - 1.0) <= 25 * U
    assert np.all(pts > 0.0) and np.all(pts < 1.0)                # strictly inside the square
    t, wt = fem._gauss(5)
    assert np.all(np.diff(t) > 0.0)
    l = [2 * (t - 0.5) * (t - 1.0), 4 * t * (1.0 - t), 2 * t * (t - 0.5)]     # as _p1p2_1d
    for r in range(5):
        for s in range(5):
            q = 5 * r + s
            assert pts[q, 0] == t[s] and pts[q, 1] == t[r] and wq[q] == wt[r] * wt[s]
            for j in range(3):
                for i in range(3):
                    assert basis[q, 3 * j + i] == l[i][s] * l[j][r]
    # a partition of unity, and each function 1 at its own node: the 1-D functions at 0, 1/2, 1
    assert np.all(np.abs(basis.sum(axis=1) - 1.0) <= 16 * U)
    nodes = np.array([0.0, 0.5, 1.0])
    assert np.array_equal(fem._q2_shape_functions_1d(nodes), np.eye(3))
    print(f"smallest weight {wq.min():.3g}, smallest coordinate {pts.min():.3g}")


def test_gauss_square_rule_is_exact_to_degree_nine_per_variable_and_not_ten():
    """Against ``1 / ((a + 1) (b + 1))`` in ``Fraction``s from the float tables; the bound is
    ``reaction_q2_ref.monomial_defect_bound``: what tables within 16 units of the exact Gauss
    nodes and weights allow."""
    pts, wq, _ = fem._gauss_square_rule()
    worst, worst_rel = 0.0, 0.0
    for a in range(10):
        for b in range(10):
            exact = ref.monomial_integral((a, b))
            err = float(abs(ref.monomial_sum(pts, wq, (a, b)) - exact))
            worst = max(worst, err / ref.monomial_defect_bound(pts, wq, (a, b)))
            worst_rel = max(worst_rel, err / float(exact))
    print(f"a, b <= 9: worst error / bound {worst:.3f}, worst relative error {worst_rel:.2e}")
    assert worst <= 1.0
    off = [float(abs(ref.monomial_sum(pts, wq, alpha) - ref.monomial_integral(alpha)))
           / ref.monomial_defect_bound(pts, wq, alpha)
           for b in range(10) for alpha in ((10, b), (b, 10))]
    print(f"a = 10 or b = 10: smallest error / bound {min(off):.3g}")
    assert min(off) > 1.0e3            # a stronger rule left in by accident would pass degree 10


# -------------------------------------------------------------------------- the statement
def test_the_q2_statement_written_out_bit_for_bit():
    disc = fem.rectangle_q2(3, 2, 3.0, 0.5)
    pts, wq, phi = fem._gauss_square_rule()
    X = disc.coords[disc.cells]
    area = np.abs((X[:, 2, 0] - X[:, 0, 0]) * (X[:, 6, 1] - X[:, 0, 1]))
    W = wq[None, :] * area[:, None]
    ne = len(disc.cells)
    rows = np.repeat(disc.cells, 9, axis=1).ravel()
    cols = np.tile(disc.cells, (1, 9)).ravel()
    M = disc.M
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        assert term.nv == 9 and term.basis.shape == (25, 9) and term.W.shape == (ne, 25)
        assert np.array_equal(term.lam, pts) and np.array_equal(term.wq, wq)
        assert np.array_equal(term.basis, phi)
        assert np.array_equal(term.area, area) and np.array_equal(term.W, W)
        # flat entry e 81 + 9 a + b sits at (cells[e, a], cells[e, b]) of M
        assert term.scatter.shape == (81 * ne,)
        assert np.array_equal(M.indices[term.scatter], cols)
        assert np.all((M.indptr[rows] <= term.scatter) & (term.scatter < M.indptr[rows + 1]))
        for kind in ref.ITERATES:
            v = ref.iterate(kind, disc, seed=common.SEED)[0]
            vc = v[disc.cells]
            E = np.zeros((ne, 9, 9))
            for q in range(25):
                s = phi[q, 0] * vc[:, 0]
                for k in range(1, 9):
                    s = s + phi[q, k] * vc[:, k]
                g = np.full(ne, c[-1])
                for k in range(len(c) - 2, -1, -1):
                    g = g * s + c[k]
                wg = W[:, q] * g
                for a in range(9):
                    wa = wg * phi[q, a]
                    for b in range(9):
                        E[:, a, b] = E[:, a, b] + wa * phi[q, b]
            assert np.array_equal(term.element_matrices(v), E)
            C_ = np.bincount(term.scatter, weights=E.ravel(), minlength=M.nnz)
            assert np.array_equal(term.reaction_values(v), C_)
            assert np.array_equal(term(v, 0.0).data, term.L.data + C_)
    newton = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    assert np.array_equal(newton.jacobian(v, 0.0).data,
                          fem.ReactionTerm(disc, (2.0, 0.0, 1.5))(v, 0.0).data)


def test_unit_square_q2_and_other_cells_are_still_refused():
    with pytest.raises(ValueError, match="triangles.*tetrahedra"):
        fem.ReactionTerm(fem.unit_square_q2(2), (2.0, 0.0, 0.5))
    disc = fem.rectangle_q2(1, 1)
    for cells in (np.zeros((2, 5), dtype=np.int32), np.zeros((2, 8), dtype=np.int32),
                  np.zeros((2, 10), dtype=np.int32), None):
        bad = fem.SpatialDiscretisation(disc.M, disc.K, disc.coords, disc.boundary, "bad", cells)
        with pytest.raises(ValueError, match="quadrilaterals"):
            fem.ReactionTerm(bad, (1.0,))


# -------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_a_unit_coefficient_gives_the_mass_matrix(mesh):
    """The rule is exact for ``phi_a phi_b``: ``reaction_values`` with ``c = (1.0,)`` is ``M``.
    Bar: the statement's ``128 u S`` and the gather's three additions on the term's side, the
    rule's defect for ``phi_a phi_b``, and ``MESH_BAR`` on ``M``'s."""
    dims = ref.MESHES[mesh]
    disc = fem.rectangle_q2(*dims)
    term = fem.ReactionTerm(disc, (1.0,))
    v = np.random.default_rng(common.SEED).standard_normal(disc.n_dofs)
    C_ = term.reaction_values(v)
    nnz = disc.M.nnz

    def gathered(Ee):
        return np.bincount(term.scatter, weights=Ee.ravel(), minlength=nnz)
    S = gathered(ref.scales(term, v))
    pair_defect = np.array([[ref.polynomial_defect_bound(term, ref._mul(ref.PHI[a], ref.PHI[b]))
                             for b in range(9)] for a in range(9)])
    defect = gathered(term.area[:, None, None] * pair_defect[None])
    S_M = _absolute_contributions(disc, *dims)[0].data
    bound = (BAR + 3) * U * S + defect + ref.MESH_BAR * U * S_M
    err = np.abs(C_ - disc.M.data)
    print(f"{mesh}: worst error / bound {np.max(err / bound):.3f}; worst relative to "
          f"max |M| {err.max() / np.abs(disc.M.data).max():.2e}")
    assert np.all(err <= bound)
    # the bar is no loophole (the monomials of phi_a phi_b, of degree 4 per variable, enter the
    # defect with absolute coefficients: hence not 1e-13)
    print(f"{mesh}: bound / max |M| at most {bound.max() / np.abs(disc.M.data).max():.2e}")
    assert np.all(bound <= 1e-10 * np.abs(disc.M.data).max())


@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_the_reference_coefficient_against_exact_polynomial_integrals(mesh):
    """``c = (2, 0, 0.5)`` and a Q2 iterate: the integrand has degree 8 per variable, the rule is
    exact, and the element matrices are the tensor-monomial integrals -- computed without the
    rule, so the 81 shape-function pairs and the local node order are checked."""
    disc = fem.rectangle_q2(*ref.MESHES[mesh])
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
    # monomials of the integrand, of degree 8 per variable and expanded about a corner, enter the
    # defect with absolute coefficients, hence not 1e-13)
    assert np.all(bound <= 1e-5 * S)
    # a swapped pair of local nodes would be far outside: corner, edge and centre entries differ
    top = np.abs(E[:, 0, 0]).max()
    assert np.abs(E[:, 0, 0] - E[:, 1, 1]).min() > 1e-3 * top
    assert np.abs(E[:, 1, 1] - E[:, 4, 4]).min() > 1e-3 * top


# ----------------------------------------------------------------------- element matrices
@pytest.mark.parametrize("kind", ref.ITERATES)
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_host_element_matrices_are_exact_to_the_bar(mesh, kind):
    disc = fem.rectangle_q2(*ref.MESHES[mesh])
    v = ref.iterate(kind, disc, seed=common.SEED)
    worst = 0.0
    for c in ref.COEFFICIENTS:
        term = fem.ReactionTerm(disc, c)
        for l, (X, S) in enumerate(ref.exact_elements(mesh, kind, c, common.SEED)):
            E = term.element_matrices(v[l])
            assert E.shape == (len(term.cells), 9, 9)
            worst = max(worst, ref.worst_ratio(E, X, S))
        print(f"{mesh} {kind} c={c}: worst err / (u S) so far = {worst:.2f}")
    assert worst <= BAR


# ----------------------------------------------------------------------------------- plan
def _instationary(disc, term, **kw):
    return Instationary(disc, term, desired_state=lambda X, t: X[:, 0], n_t=3, **kw)


def test_the_plan_on_q2():
    disc = fem.rectangle_q2(3, 2, 3.0, 0.5)
    term = fem.ReactionTerm(disc, ref.COEFFICIENTS[2])
    plan = ReactionPlan(_instationary(disc, term))
    d, keep = plan.descriptor()
    assert d.nv == 9 and d.nq == 25 and d.ne == len(term.cells) and d.n1 == disc.n_dofs
    assert np.array_equal(np.ctypeslib.as_array(d.lam, shape=(25, 9)), term.basis)
    cptr, clist = plan.lists
    assert cptr[-1] == len(clist) == 81 * len(term.cells) and len(cptr) == term.M.nnz + 1
    assert np.diff(cptr).max() == 4                   # the vertex shared by four cells
    for kind in ref.ITERATES:
        v = ref.iterate(kind, disc, seed=common.SEED)[0]
        E = term.element_matrices(v)
        assert np.array_equal(relinearise.gather(E, cptr, clist), term.reaction_values(v))
    M = term.M
    assert np.diff(M.indptr).max() == 25
    assert np.array_equal(plan.tperm, relinearise.transpose_permutation(M))
    assert np.array_equal(plan.tperm[plan.tperm], np.arange(M.nnz))
    del keep
    stationary = ReactionPlan(Stationary(disc, term, desired_state=lambda X: X[:, 0], beta=1.0))
    d = stationary.descriptor()[0]
    assert stationary.n_t == 1 and d.nq == 25 and d.nv == 9


def test_the_descriptor_names_the_element_inside_the_old_layout():
    """``nv`` fills the four bytes of padding between ``nq`` and the 8-byte ``ne``: neither the
    size of the structure nor the offset of any earlier field moves, and a descriptor of the
    earlier layout (padding zero) reads as ``nv = 0``."""
    D = _lib.ReactionDesc
    assert (D.n_t.offset, D.cn.offset, D.nq.offset, D.nv.offset, D.ne.offset) == (0, 4, 8, 12, 16)
    assert D.n1.offset == 24 and D.tau.offset == 32

    class Before(C.Structure):
        _fields_ = [f for f in D._fields_ if f[0] != "nv"]
    assert C.sizeof(D) == C.sizeof(Before) and Before.ne.offset == D.ne.offset
    assert all(getattr(Before, f[0]).offset == getattr(D, f[0]).offset for f in Before._fields_)
    p2 = fem.rectangle_p2(2, 2)
    d, keep = ReactionPlan(_instationary(p2, fem.ReactionTerm(p2, (2.0, 0.0, 0.5)))).descriptor()
    assert d.nv == 6 and d.nq == 25
    p1 = fem.rectangle_p1(2, 2)
    d, keep = ReactionPlan(_instationary(p1, fem.ReactionTerm(p1, (2.0, 0.0, 0.5)))).descriptor()
    assert d.nv == 3 and d.nq == 7


def test_what_is_refused_is_refused_as_before():
    disc = fem.rectangle_q2(2, 2)
    term = fem.ReactionTerm(disc, (2.0, 0.0, 0.5))
    ctl = _instationary(disc, lambda v, t: disc.K)
    with pytest.raises(ValueError, match="ReactionTerm"):
        ctl.non_linear_solve(device=True)
    ctl = _instationary(disc, term)
    with pytest.raises(ValueError, match="P="):
        ctl.non_linear_solve(device=True, P=lambda *a: None)
    with pytest.raises(ValueError, match="another discretisation"):
        _instationary(fem.rectangle_q2(2, 2), term).non_linear_solve(device=True)
