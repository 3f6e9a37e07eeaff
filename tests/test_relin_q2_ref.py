"""``fem.rectangle_q2q1`` and its convection element matrices on the host (no GPU): the
element-assembled Taylor-Hood space against the tensor-product ``unit_square_q2q1`` and against
``rectangle_q2``, the 4 x 4 Gauss-Legendre product rule against the exact integrals of the tensor
monomials, the host element matrices against the exact rational ones of ``tests/relin_q2_ref.py``
(``ELEMENT_BAR_Q2 u S``), the contribution lists, the descriptor and the ``ValueError``s.

``B`` of the two constructions is compared on the union of the stored entries: where a pressure
vertex and a velocity node at the same place are shared by two or four cells, the contributions to
``int psi d phi / d x`` cancel, and each path is left with either 0.0 or a residue of a few
``1e-17`` there -- not at the same places.  Such an entry is held to the value bound like any
other (against 0.0 on the side that does not store it); the patterns of the other four matrices
are equal after ``eliminate_zeros``.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import common
import reaction_q2_ref
import relin_q2_ref as ref
import test_gpu_relin_kernels as p2p1
from control_amd import _lib, fem, picard
from control_amd.control import Stationary
from control_amd.relinearise import RelinearisationPlan, contribution_lists, gather

U = ref.U
BAR = ref.ELEMENT_BAR_Q2
MESHES = [(2, 2, 2.0, 2.0), (3, 2, 3.0, 1.0)]
WINDS = p2p1.WINDS

# M_v and K_v are kron(I_2, .) of rectangle_q2's M and K on one side and of unit_square_q2's on
# the other: reaction_q2_ref.MESH_BAR (M 19, K 23 roundings on the two paths together, relative
# to the sum of the absolute element contributions) holds for them as it stands.
#
# B, M_p, K_p: the roundings on both construction paths, to first order and relative to the sum
# of the absolute element contributions (on the tensor path the product of the 1-D sums of
# absolute values: the same number).  A 1-D table value at a Gauss point: the point (1) and the
# operations on it -- l_i 3, l_i' 2 (counted with the point: 3), psi 1; a weight 2 (numpy's value
# and the halving is exact: 1; counted 2).
#   tensor path (_p1p2_1d, 4 points): MX = h sum psi phi w: psi 2, phi 4, w 2, two products, three
#   additions, h = L / n and the scaling 2: 15; DX = sum psi phi' w: 2 + 3 + 2 + 2 + 3 = 12;
#   M1 = h sum psi psi w: 2 + 2 + 2 + 2 + 3 + 2 = 13; K1 = (1 / h) (+-1): 2; the 1-D assembly one
#   addition each; the Kronecker product one product, the sum of K_p's two one more:
#   B 16 + 13 + 1 = 30, M_p 14 + 14 + 1 = 29, K_p 14 + 3 + 1 + 1 = 19;
#   element path (16 points): W = (wt wt) (hx hy): 2 + 2 + 1 + 2 + 1 + 1 = 9; lam = psi psi:
#   2 + 2 + 1 = 5; grad phi = (l' l) (1 / h): 3 + 4 + 1 + 1 + 1 = 10; grad lam = (+-psi) (1 / h):
#   2 + 1 + 1 = 4; two products and the 16-term sum 15 (K_p: the two-term sum over x, y one
#   more); the assembly of at most four cells 3:
#   B 9 + 5 + 10 + 2 + 15 + 3 = 44, M_p 9 + 5 + 5 + 2 + 15 + 3 = 39, K_p 9 + 4 + 4 + 2 + 1 + 15
#   + 3 = 38.
# B 74, M_p 68, K_p 57 -- one bar, rounded up to a power of two.
TAYLOR_HOOD_BAR = 128


def _absolute_contributions(th):
    """``B`` (both components), ``M_p`` and ``K_p`` of ``rectangle_q2q1`` with every term of every
    element entry replaced by its absolute value, dense."""
    e = th.elem
    V, Pn, W = e["V"], e["P"], e["W"]
    lam, gphi, glam = np.abs(e["lam"]), np.abs(e["gphi"]), np.abs(e["glam"])
    n2, n1 = th.n_v // 2, th.n_p
    asm = fem._assemble_like
    SB = [asm(np.einsum("eq,qc,eqa->eca", W, lam, gphi[..., d]), Pn, V, (n1, n2)).toarray()
          for d in range(2)]
    SM = asm(np.einsum("eq,qc,qd->ecd", W, lam, lam), Pn, Pn, (n1, n1)).toarray()
    SK = asm(np.einsum("eq,eqcx,eqdx->ecd", W, glam, glam), Pn, Pn, (n1, n1)).toarray()
    return np.hstack(SB), SM, SK


# ------------------------------------------------------------------------------ the space
@pytest.mark.parametrize("dims", [(2, 2, 2.0, 2.0), (3, 3, 3.0, 3.0)])
def test_rectangle_q2q1_is_unit_square_q2q1_assembled_from_elements(dims):
    n, L = dims[0], dims[2]
    th, tensor = fem.rectangle_q2q1(*dims), fem.unit_square_q2q1(n, L)
    assert tensor.elem is None                                    # left alone
    for name in ("coords_v", "coords_p", "boundary_v"):
        a, b = getattr(th, name), getattr(tensor, name)
        assert np.array_equal(a, b) and a.dtype == b.dtype, name
    # connectivity: Q2 as rectangle_q2; Q1 the cell's vertices, local node 2 j + i
    V, Pn = th.elem["V"], th.elem["P"]
    assert V.dtype == Pn.dtype == np.int32 and V.shape == (n * n, 9) and Pn.shape == (n * n, 4)
    nn = 2 * n + 1
    for ey in range(n):
        for ex in range(n):
            assert V[ey * n + ex].tolist() == [(2 * ey + j) * nn + 2 * ex + i
                                               for j in range(3) for i in range(3)]
            assert Pn[ey * n + ex].tolist() == [(ey + j) * (n + 1) + ex + i
                                                for j in range(2) for i in range(2)]
    # a pressure vertex sits on the velocity node at the same place
    assert np.array_equal(th.coords_p[Pn], th.coords_v[V][:, [0, 2, 6, 8]])
    sd = fem.rectangle_q2(*dims)
    SM2, SK2 = (np.kron(np.eye(2), S.toarray())
                for S in (fem._assemble_like(np.abs(np.broadcast_to(E, (n * n, 9, 9))), V, V,
                                             (sd.n_dofs,) * 2) for E in _q2_element_terms(dims)))
    SB, SMp, SKp = _absolute_contributions(th)
    bars = {"M_v": (SM2, reaction_q2_ref.MESH_BAR), "K_v": (SK2, reaction_q2_ref.MESH_BAR),
            "B": (SB, TAYLOR_HOOD_BAR), "M_p": (SMp, TAYLOR_HOOD_BAR),
            "K_p": (SKp, TAYLOR_HOOD_BAR)}
    for name, (S, bar) in bars.items():
        mine, theirs = getattr(th, name).toarray(), getattr(tensor, name).toarray()
        assert mine.shape == theirs.shape == S.shape, name
        stored = (mine != 0.0) | (theirs != 0.0)
        if name != "B":           # the patterns after eliminate_zeros
            assert np.array_equal(mine != 0.0, theirs != 0.0), name
        assert np.all(S[stored] > 0.0) and np.all(S >= np.abs(mine) * (1 - 8 * U)), name
        worst = float((np.abs(mine - theirs)[stored] / (U * S[stored])).max())
        print(f"n={n} L={L}: worst |rectangle_q2q1 - unit_square_q2q1| / (u S) of {name}: "
              f"{worst:.2f} (bar {bar})")
        assert worst <= bar, name
        assert np.all(mine[~stored] == 0.0) and np.all(theirs[~stored] == 0.0)
    # the assembled matrices keep one structure per space, sorted, int32
    assert np.array_equal(th.M_v.indptr, th.K_v.indptr)
    assert np.array_equal(th.M_v.indices, th.K_v.indices)
    assert np.array_equal(th.M_p.indptr, th.K_p.indptr)
    assert np.array_equal(th.M_p.indices, th.K_p.indices)
    assert sorted(set(np.diff(th.M_p.indptr))) == [4, 6, 9]
    # div of a constant field and of (x, y): B 1 = 0 row by row, 1^T B (x, y) = -2 lx ly
    x, y = th.coords_v[:, 0], th.coords_v[:, 1]
    one, zero = np.ones(len(x)), np.zeros(len(x))
    assert np.abs(th.B @ np.concatenate([one, zero])).max() <= 64 * U * SB.sum(axis=1).max()
    total = np.ones(th.n_p) @ (th.B @ np.concatenate([x, y]))
    assert abs(total + 2 * L * L) <= 1e-13 * L * L


def _q2_element_terms(dims):
    """The absolute element contributions of ``rectangle_q2``'s ``M`` and ``K`` (for ``K`` each of
    its two tensor products), as ``tests/test_reaction_q2_ref.py`` forms them."""
    nx, ny, lx, ly = dims
    hx, hy = lx / nx, ly / ny
    m = np.abs(np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]]))
    k = np.abs(np.array([[7.0, -8.0, 1.0], [-8.0, 16.0, -8.0], [1.0, -8.0, 7.0]]))
    Mx, My, Kx, Ky = hx / 30.0 * m, hy / 30.0 * m, 1.0 / (3.0 * hx) * k, 1.0 / (3.0 * hy) * k
    return np.kron(My, Mx), np.kron(My, Kx) + np.kron(Ky, Mx)


def test_one_velocity_component_is_rectangle_q2_bit_for_bit():
    dims = (3, 2, 3.0, 1.0)
    th, sd = fem.rectangle_q2q1(*dims), fem.rectangle_q2(*dims)
    n2 = sd.n_dofs
    assert th.n_v == 2 * n2 and np.array_equal(th.elem["V"], sd.cells)
    assert np.array_equal(th.coords_v, sd.coords)
    assert np.array_equal(th.boundary_v, np.concatenate([sd.boundary, sd.boundary + n2]))
    for name, A in (("M", th.M_v), ("K", th.K_v)):
        want = getattr(sd, name)
        for c in range(2):
            blk = A[c * n2:(c + 1) * n2, c * n2:(c + 1) * n2].tocsr()
            blk.sort_indices()
            assert np.array_equal(blk.indptr, want.indptr), name
            assert np.array_equal(blk.indices, want.indices), name
            assert np.array_equal(blk.data, want.data), name
        assert A[:n2, n2:].nnz == 0 and A[n2:, :n2].nnz == 0


def test_the_element_tables():
    dims = (3, 2, 3.0, 1.0)
    th = fem.rectangle_q2q1(*dims)
    e, ne = th.elem, 6
    hx, hy = 3.0 / 3, 1.0 / 2
    assert e["kind"] == "q2q1"
    shapes = {"V": (ne, 9), "P": (ne, 4), "W": (ne, 16), "phi": (16, 9), "gref": (16, 9, 2),
              "lam": (16, 4), "lref": (16, 4, 2), "jinv": (ne, 2), "gphi": (ne, 16, 9, 2),
              "glam": (ne, 16, 4, 2)}
    for name, shape in shapes.items():
        assert e[name].shape == shape, name
    t, wt = fem._gauss(4)
    l = fem._q2_shape_functions_1d(t)
    dl = [4 * t - 3.0, 4.0 - 8 * t, 4 * t - 1.0]
    psi, dpsi = [1.0 - t, t], [-1.0, 1.0]
    assert np.array_equal(e["jinv"], np.broadcast_to([1.0 / hx, 1.0 / hy], (ne, 2)))
    for r in range(4):
        for s in range(4):
            q = 4 * r + s
            assert np.all(e["W"][:, q] == (wt[r] * wt[s]) * (hx * hy))
            for j in range(3):
                for i in range(3):
                    a = 3 * j + i
                    assert e["phi"][q, a] == l[i][s] * l[j][r]
                    assert e["gref"][q, a, 0] == dl[i][s] * l[j][r]
                    assert e["gref"][q, a, 1] == l[i][s] * dl[j][r]
            for j in range(2):
                for i in range(2):
                    c = 2 * j + i
                    assert e["lam"][q, c] == psi[i][s] * psi[j][r]
                    assert e["lref"][q, c, 0] == dpsi[i] * psi[j][r]
                    assert e["lref"][q, c, 1] == psi[i][s] * dpsi[j]
    # one rounded product ref * jinv per entry
    assert np.array_equal(e["gphi"], e["gref"][None] * e["jinv"][:, None, None, :])
    assert np.array_equal(e["glam"], e["lref"][None] * e["jinv"][:, None, None, :])
    # partitions of unity; gradients sum to zero
    assert np.all(np.abs(e["phi"].sum(axis=1) - 1.0) <= 16 * U)
    assert np.all(np.abs(e["lam"].sum(axis=1) - 1.0) <= 4 * U)
    assert np.all(np.abs(e["gref"].sum(axis=1)) <= 64 * U)
    assert np.all(np.abs(e["lref"].sum(axis=1)) <= 4 * U)


# ------------------------------------------------------------------------------- the rule
def _rule():
    t, wt = fem._gauss(4)
    pts = np.stack([np.tile(t, 4), np.repeat(t, 4)], axis=1)      # q = 4 r + s: (t_s, t_r)
    return pts, np.repeat(wt, 4) * np.tile(wt, 4)


def test_the_rule_is_exact_to_degree_seven_per_variable_and_not_eight():
    """Against ``1 / ((a + 1) (b + 1))`` in ``Fraction``s from the float tables.  The bound is
    ``reaction_q2_ref.monomial_defect_bound``: what tables within ``TABLE_ULPS`` units of the
    exact Gauss nodes and weights allow -- a few ``u`` of the integral."""
    pts, wq = _rule()
    th = fem.rectangle_q2q1(1, 1)
    assert np.array_equal(th.elem["W"][0], wq)                    # hx hy = 1: the rule itself
    assert np.all(wq > 0.0) and abs(wq.sum() - 1.0) <= 16 * U
    assert np.all(pts > 0.0) and np.all(pts < 1.0)
    worst = worst_rel = 0.0
    for a in range(8):
        for b in range(8):
            exact = reaction_q2_ref.monomial_integral((a, b))
            err = float(abs(reaction_q2_ref.monomial_sum(pts, wq, (a, b)) - exact))
            worst = max(worst, err / reaction_q2_ref.monomial_defect_bound(pts, wq, (a, b)))
            worst_rel = max(worst_rel, err / float(exact))
    err77 = float(abs(reaction_q2_ref.monomial_sum(pts, wq, (7, 7)) - Fraction(1, 64))) * 64
    print(f"a, b <= 7: worst error / bound {worst:.3f}, worst relative error {worst_rel / U:.2f} u; "
          f"x^7 y^7: {err77 / U:.2f} u")
    assert worst <= 1.0
    assert err77 <= 8 * reaction_q2_ref.TABLE_ULPS * U   # 1 + 7 + 7 at points below 1: a few u
    off = [float(abs(reaction_q2_ref.monomial_sum(pts, wq, alpha)
                     - reaction_q2_ref.monomial_integral(alpha)))
           / reaction_q2_ref.monomial_defect_bound(pts, wq, alpha)
           for b in range(8) for alpha in ((8, b), (b, 8))]
    print(f"a = 8 or b = 8: smallest error / bound {min(off):.3g}")
    assert min(off) > 1.0e3            # a stronger rule left in by accident would pass degree 8


# ----------------------------------------------------------------------- element matrices
def _element_matrices(th, w):
    """The element matrices of ``convection_v_data`` / ``convection_p`` (fem.py) on Q2-Q1, as they
    are summed there."""
    e = th.elem
    n2 = th.n_v // 2
    V = e["V"]
    wq = np.stack([w[:n2][V] @ e["phi"].T, w[n2:][V] @ e["phi"].T], axis=2)
    adv = np.matmul(e["gphi"], wq[..., None])[..., 0]
    Nv = np.einsum("eq,qa,eqb->eab", e["W"], e["phi"], adv)
    wq = np.stack([e["phi"] @ w[:n2][V].T, e["phi"] @ w[n2:][V].T], axis=2)
    advp = np.einsum("qed,eqcd->eqc", wq, e["glam"])
    Np = np.einsum("eq,qa,eqc->eac", e["W"], e["lam"], advp)
    return Nv, Np


@pytest.mark.parametrize("kind", WINDS)
@pytest.mark.parametrize("mesh", MESHES)
def test_host_element_matrices_are_exact_to_the_bar(mesh, kind):
    """fem.py's element matrices lie within ``ELEMENT_BAR_Q2 u S`` of the exact ones; a zero wind
    gives exact zeros."""
    th = fem.rectangle_q2q1(*mesh)
    v = p2p1._winds(kind, th)
    worst_v = worst_p = 0.0
    for w, (Xv, Xp, Sv, Sp) in zip(v, ref.exact_elements(mesh, kind, p2p1._winds)):
        Nv, Np = _element_matrices(th, w)
        assert Nv.shape == (len(th.elem["V"]), 9, 9) and Np.shape == (len(th.elem["V"]), 4, 4)
        worst_v = max(worst_v, ref.worst_ratio(Nv, Xv, Sv))
        worst_p = max(worst_p, ref.worst_ratio(Np, Xp, Sp))
        if not w.any():
            assert not Nv.any() and not Np.any()
    print(f"{mesh} {kind}: host worst err / (u S) = {worst_v:.2f} (velocity), {worst_p:.2f} "
          f"(pressure), bar {BAR}")
    assert worst_v <= BAR and worst_p <= BAR


def test_the_reference_itself():
    """Zero for a zero wind, the form annihilates constants (rows sum to zero over the trial
    index), it is linear in the wind, and a uniform wind along x on the unit cell gives the known
    ``int phi_a d phi_b / d x``: entry (0, 2) of the 1-D ``int l_0 l_2' = -1 / 6`` times
    ``int l_0 l_0 = 2 / 15``."""
    xy = np.zeros((9, 2))
    xy[8] = [0.75, 2.5]
    rng = np.random.default_rng(common.SEED)
    z = np.zeros(9)
    Nv0, Np0 = ref.element_matrices(xy, z, z)
    assert all(x == 0 for row in Nv0 for x in row) and all(x == 0 for row in Np0 for x in row)
    w1, w2 = rng.standard_normal((2, 9)), rng.standard_normal((2, 9))
    Cm, Cp = ref.element_matrices(xy, *w1)
    assert any(x != 0 for row in Cm for x in row)
    assert all(sum(Cm[a]) == 0 for a in range(9)) and all(sum(Cp[a]) == 0 for a in range(4))
    w3, w4 = np.round(w1 * 64) / 64, np.round(w2 * 64) / 64       # dyadic: the sum is exact
    A, Ap = ref.element_matrices(xy, *w3)
    B, Bp = ref.element_matrices(xy, *w4)
    Cm, Cp = ref.element_matrices(xy, *(w3 + w4))
    assert all(A[a][b] + B[a][b] == Cm[a][b] for a in range(9) for b in range(9))
    assert all(Ap[a][b] + Bp[a][b] == Cp[a][b] for a in range(4) for b in range(4))
    unit = np.zeros((9, 2))
    unit[8] = [1.0, 1.0]
    Nx, Npx = ref.element_matrices(unit, np.ones(9), z)
    assert Nx[0][2] == Fraction(-1, 6) * Fraction(2, 15)
    assert Nx[0][0] == Fraction(-1, 2) * Fraction(2, 15)          # int l_0 l_0' = -1 / 2
    assert Npx[0][1] == Fraction(1, 2) * Fraction(1, 3)           # int psi_0 psi_1' int psi_0^2


# ----------------------------------------------------------------------- binding and errors
@pytest.mark.parametrize("mesh", MESHES)
def test_lists_reproduce_the_host_assembly(mesh):
    th = fem.rectangle_q2q1(*mesh)
    ne, n2 = len(th.elem["V"]), th.n_v // 2
    K2 = th.K_v[:n2, :n2].tocsr()
    K2.sort_indices()
    cptr, clist = contribution_lists(th.elem["V"], K2)
    pptr, plist = contribution_lists(th.elem["P"], th.K_p)
    assert cptr[-1] == len(clist) == 81 * ne and pptr[-1] == len(plist) == 16 * ne
    assert np.array_equal(np.sort(clist), np.arange(81 * ne))
    assert np.array_equal(np.sort(plist), np.arange(16 * ne))
    assert np.diff(cptr).max() == 4 and np.diff(pptr).max() == 4  # a vertex shared by four cells
    Pn = th.elem["P"]
    rows, cols = np.repeat(Pn, 4, axis=1).ravel(), np.tile(Pn, (1, 4)).ravel()
    scatter_p = th.K_p.indptr[rows] + fem._row_positions(th.K_p, rows, cols)
    rng = np.random.default_rng(common.SEED)
    for _ in range(3):
        w = rng.standard_normal(th.n_v)
        Nv, Np = _element_matrices(th, w)
        host_v = th.convection_v_data(w)
        dev_v = gather(Nv, cptr, clist)
        # bit for bit: the lists sum in np.bincount's order
        assert np.array_equal(dev_v, host_v[:K2.nnz]) and np.array_equal(dev_v, host_v[K2.nnz:])
        dev_p = gather(Np, pptr, plist)
        assert np.array_equal(dev_p, np.bincount(scatter_p, weights=Np.ravel(),
                                                 minlength=th.K_p.nnz))
        host_p = th.convection_p(w)
        assert np.array_equal(host_p.indptr, th.K_p.indptr)
        assert np.array_equal(host_p.indices, th.K_p.indices)
        # the same four terms per entry, summed by scipy in another order
        Sp = np.bincount(scatter_p, weights=np.abs(Np).ravel(), minlength=th.K_p.nnz)
        assert np.all(np.abs(dev_p - host_p.data) <= 3 * U * Sp)
    # the term: nu K + C on the structures of K_v and K_p
    term = fem.ConvectionTerm(th, 0.1)
    assert np.array_equal(term(w).data, 0.1 * th.K_v.data + th.convection_v(w).data)
    assert np.array_equal(term.pressure(w).data, 0.1 * th.K_p.data + th.convection_p(w).data)


def _problem(th, n_t=3, CN=False):
    return p2p1._problem(th, n_t, CN)


def test_the_descriptor_names_the_element_inside_the_old_layout():
    """``nv`` fills the four bytes of padding between ``nq`` and the 8-byte ``ne``, ``jinv``
    follows the last field: no offset of an earlier field moves, and a descriptor of the earlier
    layout (padding zero) reads as ``nv = 0``."""
    D = _lib.RelinDesc
    assert (D.n_t.offset, D.cn.offset, D.nq.offset, D.nv.offset, D.ne.offset) == (0, 4, 8, 12, 16)

    class Before(C.Structure):
        _fields_ = [f for f in D._fields_ if f[0] not in ("nv", "jinv")]
    assert all(getattr(Before, f[0]).offset == getattr(D, f[0]).offset for f in Before._fields_)
    assert D.jinv.offset == C.sizeof(Before) and C.sizeof(D) == C.sizeof(Before) + 8
    assert D._fields_[-1][0] == "jinv"

    th = fem.rectangle_q2q1(3, 2, 3.0, 1.0)
    plan = RelinearisationPlan(_problem(th))
    d, keep = plan.descriptor()
    e, ne = th.elem, 6
    assert plan.kind == "q2q1" and (d.nv, d.nq, d.ne, d.n2, d.n1) == (9, 16, ne, 35, 12)
    as_array = np.ctypeslib.as_array
    assert np.array_equal(as_array(d.V, shape=(ne, 9)), e["V"])
    assert np.array_equal(as_array(d.W, shape=(ne, 16)), e["W"])
    assert np.array_equal(as_array(d.phi, shape=(16, 9)), e["phi"])
    assert np.array_equal(as_array(d.gphi, shape=(16, 9, 2)), e["gref"])   # reference gradients
    assert np.array_equal(as_array(d.lam, shape=(16, 4)), e["lam"])
    assert np.array_equal(as_array(d.glam, shape=(16, 4, 2)), e["lref"])
    assert np.array_equal(as_array(d.jinv, shape=(ne, 2)), e["jinv"])
    assert plan.v_lists[0][-1] == 81 * ne and plan.p_lists[0][-1] == 16 * ne
    assert len(as_array(d.v_clist, shape=(81 * ne,))) == len(plan.v_lists[1])
    del keep
    # the triangles' descriptor: nv = 0, no jinv
    tri = fem.rectangle_p2p1(2, 2)
    plan = RelinearisationPlan(_problem(tri))
    d, keep = plan.descriptor()
    assert plan.kind == "p2p1" and (d.nv, d.nq) == (0, 7) and not d.jinv


def test_the_plan_and_the_term_on_q2q1_against_the_host_residual():
    """The plan's data rows are the host residual at the zero iterate, for both time schemes and
    the stationary problem's one level."""
    th = fem.rectangle_q2q1(2, 2, 2.0, 2.0)
    for CN in (False, True):
        pb = _problem(th, 3, CN)
        plan = RelinearisationPlan(pb)
        m = 2 if CN else 3
        assert plan.m == m and plan.data.shape == (2 * m, th.n_v)
        z = np.zeros((3, th.n_v))
        r00, r01, _, _ = picard.non_linear_res_eval(pb, [th.K_v] * 3, z, z.copy(),
                                                    np.zeros((m, th.n_p)), np.zeros((m, th.n_p)))
        assert np.array_equal(plan.data, np.concatenate([r00, r01]))
        ip, ix = plan.velocity_pattern()
        assert np.array_equal(ip, th.K_v.indptr) and np.array_equal(ix, th.K_v.indices)


def test_unit_square_q2q1_is_still_refused_and_the_messages_name_both_constructors(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    both = r"fem\.rectangle_p2p1 or fem\.rectangle_q2q1"
    q2 = fem.unit_square_q2q1(2)
    assert q2.elem is None
    w = np.zeros(q2.n_v)
    with pytest.raises(NotImplementedError, match="rectangle_p2p1 or rectangle_q2q1"):
        q2.convection_v(w)
    with pytest.raises(NotImplementedError, match="rectangle_p2p1 or rectangle_q2q1"):
        q2.convection_p(w)
    with pytest.raises(ValueError, match=both):
        fem.ConvectionTerm(q2, 0.1)
    pb = _problem(q2)
    with pytest.raises(ValueError, match=both):
        RelinearisationPlan(pb)
    with pytest.raises(ValueError, match=both):
        picard.GpuLinearSolver(pb, relinearise="device")
    with pytest.raises(ValueError, match=both):
        picard.incompressible_non_linear_solve(pb, device=True)
    th = fem.rectangle_q2q1(2, 2)
    ctl = Stationary(q2, fem.ConvectionTerm(th, 0.1),
                     desired_state=lambda X: np.concatenate([X[:, 0], X[:, 1]]), beta=1.0e-2)
    with pytest.raises(ValueError, match=both):
        ctl.incompressible_non_linear_solve(device=True)
    # with element data the checks pass: the next thing is the library
    ctl = Stationary(th, fem.ConvectionTerm(th, 0.1),
                     desired_state=lambda X: np.concatenate([X[:, 0], X[:, 1]]), beta=1.0e-2)
    with pytest.raises(AssertionError, match="the library was loaded"):
        ctl.incompressible_non_linear_solve(device=True)
