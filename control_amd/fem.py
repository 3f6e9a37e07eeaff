"""Host-side finite-element input generation (NumPy/SciPy, no Firedrake).

The reference gets its spatial blocks from Firedrake ``assemble`` of UFL forms
(``preconditioner/preconditioner.py:305-328``).  Firedrake is not available in
this pipeline, so synthetic systems of the BASELINE.json shapes are produced
here: the mass matrix ``M = int u w`` and the stiffness matrix
``K = int grad u . grad w`` (the README's ``forw_diff_operator``,
``README.md:31-32``) on structured meshes, as SciPy CSR with sorted int32
column indices -- exactly what ``petscmat.getValuesCSR()`` would hand over.

This module is input generation only.  It is shared by the product host layer
(bench / smoke build their synthetic systems with it) and by the tests; it holds
no solver arithmetic.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

__all__ = [
    "SpatialDiscretisation",
    "unit_square_p1",
    "unit_cube_p1",
    "unit_square_q2",
    "rectangle_p1",
    "box_p1",
    "rectangle_p2",
    "unit_square_p2",
    "rectangle_q2",
    "rectangle_q2q1",
    "ReactionTerm",
    "ConvectionTerm",
]


@dataclass
class SpatialDiscretisation:
    """One spatial function space: matrices, boundary dofs and dof coordinates."""

    M: sp.csr_matrix          # mass matrix
    K: sp.csr_matrix          # stiffness matrix (grad-grad)
    coords: np.ndarray        # (N_x, dim) dof coordinates
    boundary: np.ndarray      # int32 sorted dof indices on the whole boundary
    name: str = ""
    cells: np.ndarray = None  # (n_cells, 3 | 4 | 6 | 9) node indices (P1 triangles / tetrahedra,
    #                           P2 triangles: ``rectangle_p2``, Q2 quadrilaterals: ``rectangle_q2``)

    @property
    def n_dofs(self) -> int:
        return self.M.shape[0]

    def weighted_mass(self, w) -> sp.csr_matrix:
        """``w(X) * inner(trial, test) * dx`` for a coefficient given by its values at
        quadrature points: ``w(lam)`` receives the barycentric coordinates ``(nq, 3)`` of
        Radon's 7-point rule and the cell connectivity and returns ``(n_cells, nq)`` values.
        P1 triangles; same structure as ``M``."""
        if self.cells is None or np.shape(self.cells)[1] != 3:
            raise NotImplementedError("weighted_mass needs a P1 triangle discretisation")
        s15 = np.sqrt(15.0)
        a1, a2 = (6.0 - s15) / 21.0, (6.0 + s15) / 21.0
        w1, w2 = (155.0 - s15) / 1200.0, (155.0 + s15) / 1200.0
        lam = np.array([[1 / 3, 1 / 3, 1 / 3],
                        [a1, a1, 1 - 2 * a1], [a1, 1 - 2 * a1, a1], [1 - 2 * a1, a1, a1],
                        [a2, a2, 1 - 2 * a2], [a2, 1 - 2 * a2, a2], [1 - 2 * a2, a2, a2]])
        wq = np.array([9.0 / 40.0, w1, w1, w1, w2, w2, w2])
        X = self.coords[self.cells]
        d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
        W = np.asarray(w(lam, self.cells)) * wq[None, :] * area[:, None]
        Me = np.einsum("cq,qa,qb->cab", W, lam, lam)
        return _assemble_like(Me, self.cells, self.cells, self.M.shape)


def _p1_convection(self, wind) -> sp.csr_matrix:
    """``inner(dot(grad(trial), wind), test) * dx`` for P1 triangles: ``wind(X) -> (n, 2)`` is
    evaluated at the points of Radon's 7-point rule (degree 5); same structure as ``M``."""
    if self.cells is None or np.shape(self.cells)[1] != 3:
        raise NotImplementedError("convection needs a P1 triangle discretisation")
    s15 = np.sqrt(15.0)
    a1, a2 = (6.0 - s15) / 21.0, (6.0 + s15) / 21.0
    w1, w2 = (155.0 - s15) / 1200.0, (155.0 + s15) / 1200.0
    lam = np.array([[1 / 3, 1 / 3, 1 / 3],
                    [a1, a1, 1 - 2 * a1], [a1, 1 - 2 * a1, a1], [1 - 2 * a1, a1, a1],
                    [a2, a2, 1 - 2 * a2], [a2, 1 - 2 * a2, a2], [1 - 2 * a2, a2, a2]])
    wq = np.array([9.0 / 40.0, w1, w1, w1, w2, w2, w2])
    X = self.coords[self.cells]                                   # (nc, 3, 2)
    A = np.concatenate([np.ones((len(X), 3, 1)), X], axis=2)
    grads = np.transpose(np.linalg.inv(A)[:, 1:, :], (0, 2, 1))   # (nc, 3, 2): grad of phi_b
    d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    Xq = np.einsum("qa,cad->cqd", lam, X)                         # quadrature points
    W = np.asarray(wind(Xq.reshape(-1, 2))).reshape(len(X), len(wq), 2)
    wg = np.einsum("cqd,cbd->cqb", W, grads)                      # wind . grad(phi_b)
    Ce = np.einsum("cq,qa,cqb->cab", wq[None, :] * area[:, None], lam, wg)
    return _assemble_like(Ce, self.cells, self.cells, self.M.shape)


SpatialDiscretisation.convection = _p1_convection


def _radon_rule():
    """``(lam, wq)`` of Radon's 7-point rule, the tables of ``weighted_mass``."""
    s15 = np.sqrt(15.0)
    a1, a2 = (6.0 - s15) / 21.0, (6.0 + s15) / 21.0
    w1, w2 = (155.0 - s15) / 1200.0, (155.0 + s15) / 1200.0
    lam = np.array([[1 / 3, 1 / 3, 1 / 3],
                    [a1, a1, 1 - 2 * a1], [a1, 1 - 2 * a1, a1], [1 - 2 * a1, a1, a1],
                    [a2, a2, 1 - 2 * a2], [a2, 1 - 2 * a2, a2], [1 - 2 * a2, a2, a2]])
    wq = np.array([9.0 / 40.0, w1, w1, w1, w2, w2, w2])
    return lam, wq


def _stroud_rule():
    """``(lam, wq)`` of Stroud's T3:5-1: 15 points, degree 5 on the tetrahedron, all weights
    positive (the sibling of Radon's rule, with the same root of 15).  Barycentric points,
    weights as fractions of the volume: the centroid; two orbits of four points ``(1 - 3a, a, a,
    a)`` with the odd coordinate at position 0, 1, 2, 3; the six points with ``b`` at the positions
    ``(i, j)``, ``i < j`` in lexicographic order, and ``c`` at the other two."""
    s15 = np.sqrt(15.0)
    lam = [[0.25, 0.25, 0.25, 0.25]]
    wq = [16.0 / 135.0]
    for a, w in (((7.0 - s15) / 34.0, (2665.0 + 14.0 * s15) / 37800.0),
                 ((7.0 + s15) / 34.0, (2665.0 - 14.0 * s15) / 37800.0)):
        for k in range(4):
            lam.append([1.0 - 3.0 * a if c == k else a for c in range(4)])
            wq.append(w)
    b, c = (10.0 - 2.0 * s15) / 40.0, (10.0 + 2.0 * s15) / 40.0
    for i in range(4):
        for j in range(i + 1, 4):
            lam.append([b if k in (i, j) else c for k in range(4)])
            wq.append(10.0 / 189.0)
    return np.array(lam), np.array(wq)


def _conical_rule():
    """``(lam, wq)`` of the 5 x 5 conical product rule on the triangle: 25 interior points,
    positive weights, degree 9 (and not 10), built from ``numpy`` / ``scipy`` Gauss rules alone.
    With ``u_i`` the Gauss-Jacobi nodes of weight ``(1 - u)`` on [0, 1] (``roots_jacobi(5, 1, 0)``
    mapped from [-1, 1]: the weights take a factor 1/4) and ``t_j`` the Gauss-Legendre nodes on
    [0, 1], point ``5 i + j`` has ``lam_1 = u_i``, ``lam_2 = (1 - u_i) t_j``, ``lam_0 = 1 - lam_1 -
    lam_2``; the weights are fractions of the area.

    Degree 9 is what the reference's coefficient ``2 + 0.5 v^2`` needs on P2 to be integrated
    exactly: ``v^2`` has degree 4 and ``phi_a phi_b`` degree 4, together 8.  (The degree-4
    coefficients ``ReactionTerm`` also takes are inexact here, as they are under Radon's and
    Stroud's degree-5 rules on P1.)"""
    from scipy.special import roots_jacobi
    x, w = np.polynomial.legendre.leggauss(5)
    t, wt = 0.5 * (x + 1.0), 0.5 * w
    xj, wj = roots_jacobi(5, 1, 0)
    u, wu = 0.5 * (xj + 1.0), 0.25 * wj
    l1 = np.repeat(u, 5)
    l2 = np.repeat(1.0 - u, 5) * np.tile(t, 5)
    lam = np.stack([(1.0 - l1) - l2, l1, l2], axis=1)
    wq = 2.0 * (np.repeat(wu, 5) * np.tile(wt, 5))
    return lam, wq


def _q2_shape_functions_1d(x: np.ndarray) -> np.ndarray:
    """The three 1-D quadratic Lagrange functions on [0, 1] (nodes 0, 1/2, 1) at ``x``: (3, n),
    the expressions of ``_p1p2_1d``."""
    return np.stack([2 * (x - 0.5) * (x - 1.0), 4 * x * (1.0 - x), 2 * x * (x - 0.5)])


def _gauss_square_rule():
    """``(points, wq, basis)`` of the 5 x 5 Gauss-Legendre product rule on the unit square: 25
    interior points, positive weights, degree 9 in each variable (and not 10).  With ``t`` / ``wt``
    the Gauss-Legendre nodes and weights on [0, 1], point ``q = 5 r + s`` is ``(t_s, t_r)`` and
    its weight ``wt_r wt_s``, a fraction of the area.  ``basis[q, 3 j + i] = l_i(t_s) l_j(t_r)``
    are the nine Q2 shape functions at the points (``i`` along x, ``j`` along y), each entry one
    rounded product of the 1-D values.

    Degree 9 per variable is what the reference's coefficient ``2 + 0.5 v^2`` needs on Q2 to be
    integrated exactly: ``v^2`` has degree 4 per variable and so has ``phi_a phi_b``, together 8."""
    t, wt = _gauss(5)
    pts = np.stack([np.tile(t, 5), np.repeat(t, 5)], axis=1)
    wq = np.repeat(wt, 5) * np.tile(wt, 5)
    l = _q2_shape_functions_1d(t)                               # (3, 5): l[i, s]
    basis = (l.T[None, :, None, :] * l.T[:, None, :, None]).reshape(25, 9)   # [r, s, j, i]
    return pts, wq, basis


class ReactionTerm:
    """The forward form ``(L u, w) + (g(v_old) u, w)`` with a polynomial reaction coefficient
    ``g(s) = sum_k c_k s^k`` (``coefficients = (c_0, ..., c_p)``, ``p <= 4``) on P1 triangles,
    P1 tetrahedra, P2 triangles or Q2 quadrilaterals (``disc.cells`` with 3, 4, 6 or 9 columns)
    -- the reference's non-linear scalar problem is ``grad v . grad w + (2 + 0.5 v^2) v w``
    (``test/test_control.py:715-719``): ``ReactionTerm(disc, (2, 0, 0.5))``.

    ``L`` is ``nu * disc.K``, or any CSR matrix ``linear`` inside the structure of ``disc.M``
    (``disc.K + disc.convection(wind)``: a non-symmetric linear part).  ``term(v, t)`` is the
    Picard matrix, ``term.jacobian(v, t)`` the Gateaux derivative of ``g(v) v`` in ``v``: the same
    form with the coefficients ``(k + 1) c_k``.  Declaring the term instead of passing a callable
    is what lets ``Instationary.non_linear_solve(device=True)`` re-linearise on the GPU.

    The element matrix is stated operation by operation, and the device kernel evaluates the same
    statement (``csrc/reaction_kernels.hip``): over Radon's 7 points ``q``, ascending,

        s_q = (lam_q0 v_0 + lam_q1 v_1) + lam_q2 v_2
        g   = c_p;  g = g s_q + c_k  for k = p - 1, ..., 0            (Horner)
        E[a][b] = sum_q ((W_eq g) lam_qa) lam_qb   from 0.0,  W_eq = wq_q area_e

    every product and sum rounded separately.  On tetrahedra the points are the 15 of Stroud's
    T3:5-1 (``_stroud_rule``), ``s_q = ((lam_q0 v_0 + lam_q1 v_1) + lam_q2 v_2) + lam_q3 v_3``,
    ``W_eq = wq_q volume_e`` with ``volume = |det [1 x]| / 6``, and all 16 entries are computed
    separately (``(wg la) lb`` and ``(wg lb) la`` round differently).

    On P2 triangles (``rectangle_p2``: vertices 0, 1, 2, then the midpoints of edges (0,1), (1,2),
    (0,2)) the points are the 25 of ``_conical_rule`` (degree 9) and the shape functions are no
    longer the barycentric coordinates: ``basis`` (25, 6) holds ``phi_qa``, computed once from the
    barycentric table ``lam`` (25, 3).  ``area`` comes from the three vertices, ``W_eq = wq_q
    area_e``,

        s_q = ((((phi_q0 v_0 + phi_q1 v_1) + phi_q2 v_2) + phi_q3 v_3) + phi_q4 v_4) + phi_q5 v_5
        g   by Horner from c_p down, as above
        E[a][b] = sum_q ((W_eq g) phi_qa) phi_qb   from 0.0, q ascending

    and all 36 entries are computed on their own.  On P1 elements ``basis`` is ``lam``.

    On Q2 quadrilaterals (``rectangle_q2``: axis-parallel cells, local node ``3 j + i`` with ``i``
    along x and ``j`` along y) the points are the 25 of ``_gauss_square_rule`` (degree 9 per
    variable): ``lam`` (25, 2) holds their coordinates in the unit square, ``basis`` (25, 9) the
    tensor-product shape functions ``l_i(x_q) l_j(y_q)``.  ``area = hx hy`` comes from the corner
    nodes 0, 2 and 6, ``W_eq = wq_q area_e``; ``s_q`` is summed left to right over the nine nodes,
    ``g`` and ``E[a][b]`` are as on P2 triangles, and all 81 entries are computed on their own.

    The flat element entry is ``e nv^2 + nv a + b`` for ``nv`` nodes per cell.  The entries are
    summed into the structure of ``M`` by ``np.bincount`` (ascending element-entry order), and
    ``D = L + C`` with one rounding."""

    MAX_DEGREE = 4

    def __init__(self, disc, coefficients, *, nu=1.0, linear=None):
        from .blocks import conform_to
        cells = getattr(disc, "cells", None)
        if cells is None or np.ndim(cells) != 2 or np.shape(cells)[1] not in (3, 4, 6, 9):
            raise ValueError("ReactionTerm needs a discretisation by P1 or P2 triangles, P1 "
                             "tetrahedra or Q2 quadrilaterals (disc.cells with 3, 6, 4 or 9 "
                             "columns: rectangle_q2, not unit_square_q2)")
        self.coefficients = tuple(float(c) for c in coefficients)
        if not 1 <= len(self.coefficients) <= self.MAX_DEGREE + 1:
            raise ValueError(f"ReactionTerm: the degree must be 0 .. {self.MAX_DEGREE}")
        self.disc = disc
        self.M = _canonical_csr(disc.M)
        self.L = conform_to(nu * disc.K if linear is None else linear, self.M)
        self.cells = np.ascontiguousarray(cells, dtype=np.int32)
        nv = self.nv = self.cells.shape[1]
        X = disc.coords[self.cells]
        if nv == 3:
            self.lam, self.wq = _radon_rule()
            d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
            self.area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
            self.W = self.wq[None, :] * self.area[:, None]
        elif nv == 6:
            self.lam, self.wq = _conical_rule()
            d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
            self.area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
            self.W = self.wq[None, :] * self.area[:, None]
        elif nv == 9:
            self.lam, self.wq, basis = _gauss_square_rule()
            hx, hy = X[:, 2, 0] - X[:, 0, 0], X[:, 6, 1] - X[:, 0, 1]
            self.area = np.abs(hx * hy)
            self.W = self.wq[None, :] * self.area[:, None]
        else:
            self.lam, self.wq = _stroud_rule()
            A = np.concatenate([np.ones((len(X), 4, 1)), X], axis=2)
            self.volume = np.abs(np.linalg.det(A)) / 6.0
            self.W = self.wq[None, :] * self.volume[:, None]
        #: (nq, nv) values of the shape functions at the points (P1: the barycentric coordinates)
        self.basis = (_p2_shape_functions(self.lam) if nv == 6 else basis if nv == 9
                      else self.lam)
        rows = np.repeat(self.cells, nv, axis=1).ravel()
        cols = np.tile(self.cells, (1, nv)).ravel()
        #: position in the structure of ``M`` of every flat element entry ``e nv^2 + nv a + b``
        self.scatter = self.M.indptr[rows].astype(np.int64) + _row_positions(self.M, rows, cols)

    @property
    def degree(self):
        return len(self.coefficients) - 1

    @property
    def jacobian_coefficients(self):
        return tuple((k + 1) * c for k, c in enumerate(self.coefficients))

    def element_matrices(self, v, coefficients=None):
        """``E`` (n_cells, nv, nv) at the nodal values ``v``: the statement above, an explicit
        loop over the points, vectorised over the cells."""
        c = self.coefficients if coefficients is None else tuple(coefficients)
        lam, W, nv = self.basis, self.W, self.nv
        vc = np.asarray(v, dtype=np.float64)[self.cells]
        E = np.zeros((len(self.cells), nv, nv))
        for q in range(len(self.wq)):
            s = lam[q, 0] * vc[:, 0]
            for k in range(1, nv):                       # left to right, each product rounded
                s = s + lam[q, k] * vc[:, k]
            g = np.full(len(s), c[-1])
            for k in range(len(c) - 2, -1, -1):
                g = g * s + c[k]
            wg = W[:, q] * g
            for a in range(nv):
                wa = wg * lam[q, a]
                for b in range(nv):
                    E[:, a, b] += wa * lam[q, b]
        return E

    def reaction_values(self, v, coefficients=None):
        """``C``: the element matrices summed into the structure of ``M`` (its ``data``)."""
        return np.bincount(self.scatter, weights=self.element_matrices(v, coefficients).ravel(),
                           minlength=self.M.nnz)

    def _matrix(self, v, coefficients):
        return sp.csr_matrix((self.L.data + self.reaction_values(v, coefficients),
                              self.M.indices, self.M.indptr), shape=self.M.shape)

    def __call__(self, v, t):
        return self._matrix(v, self.coefficients)

    def jacobian(self, v, t):
        return self._matrix(v, self.jacobian_coefficients)


def _canonical_csr(A: sp.spmatrix) -> sp.csr_matrix:
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indptr = A.indptr.astype(np.int32)
    A.indices = A.indices.astype(np.int32)
    A.data = np.ascontiguousarray(A.data, dtype=np.float64)
    return A


def _p1_simplex_assemble(coords: np.ndarray, cells: np.ndarray):
    """Mass and stiffness for P1 on simplices (dim 2 or 3), fully vectorised."""
    n_nodes, dim = coords.shape
    nv = dim + 1
    X = coords[cells]                                   # (nc, nv, dim)
    # barycentric gradients: rows of inv([1 x]) without the constant row
    A = np.concatenate([np.ones((len(cells), nv, 1)), X], axis=2)  # (nc,nv,nv)
    Ainv = np.linalg.inv(A)                             # columns = coefficients
    grads = np.transpose(Ainv[:, 1:, :], (0, 2, 1))     # (nc, nv, dim)
    fact = {2: 2.0, 3: 6.0}[dim]
    vol = np.abs(np.linalg.det(A)) / fact               # (nc,)
    Ke = np.einsum("cid,cjd->cij", grads, grads) * vol[:, None, None]
    Mref = (np.ones((nv, nv)) + np.eye(nv)) / ((dim + 1.0) * (dim + 2.0))
    Me = vol[:, None, None] * Mref[None, :, :]
    rows = np.repeat(cells, nv, axis=1).ravel()
    cols = np.tile(cells, (1, nv)).ravel()
    M = sp.coo_matrix((Me.ravel(), (rows, cols)), shape=(n_nodes, n_nodes))
    K = sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(n_nodes, n_nodes))
    return _canonical_csr(M), _canonical_csr(K)


def rectangle_p1(nx: int, ny: int, lx: float = 1.0, ly: float = 1.0,
                 diagonal: str = "right") -> SpatialDiscretisation:
    """P1 on a structured triangulation of ``[0,lx] x [0,ly]``.

    Node ``(i, j)`` has index ``j * (nx + 1) + i``.  ``diagonal="right"`` cuts every
    cell from its lower-left to its upper-right corner.
    """
    xs = np.linspace(0.0, lx, nx + 1)
    ys = np.linspace(0.0, ly, ny + 1)
    XX, YY = np.meshgrid(xs, ys, indexing="xy")
    coords = np.stack([XX.ravel(), YY.ravel()], axis=1)
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    n00 = (jj * (nx + 1) + ii).ravel()
    n10 = n00 + 1
    n01 = n00 + (nx + 1)
    n11 = n01 + 1
    if diagonal == "right":
        cells = np.concatenate([np.stack([n00, n10, n11], 1),
                                np.stack([n00, n11, n01], 1)], 0)
    elif diagonal == "left":
        cells = np.concatenate([np.stack([n00, n10, n01], 1),
                                np.stack([n10, n11, n01], 1)], 0)
    else:
        raise ValueError("diagonal must be 'right' or 'left'")
    M, K = _p1_simplex_assemble(coords, cells)
    onb = ((coords[:, 0] == xs[0]) | (coords[:, 0] == xs[-1])
           | (coords[:, 1] == ys[0]) | (coords[:, 1] == ys[-1]))
    return SpatialDiscretisation(M, K, coords,
                                 np.flatnonzero(onb).astype(np.int32),
                                 f"P1 {nx}x{ny}", cells)


def unit_square_p1(n: int, diagonal: str = "right") -> SpatialDiscretisation:
    """``UnitSquareMesh(n, n)`` with ``FunctionSpace(mesh, "Lagrange", 1)``."""
    return rectangle_p1(n, n, 1.0, 1.0, diagonal)


def unit_cube_p1(n: int) -> SpatialDiscretisation:
    """P1 on the 6-tetrahedra-per-cube (Kuhn) subdivision of the unit cube."""
    xs = np.linspace(0.0, 1.0, n + 1)
    ZZ, YY, XX = np.meshgrid(xs, xs, xs, indexing="ij")
    coords = np.stack([XX.ravel(), YY.ravel(), ZZ.ravel()], axis=1)
    np1 = n + 1

    def nid(i, j, k):
        return (k * np1 + j) * np1 + i

    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n),
                             indexing="ij")
    ii, jj, kk = ii.ravel(), jj.ravel(), kk.ravel()
    cells = []
    # Kuhn: one tetrahedron per permutation of the axes, all sharing the main diagonal
    import itertools
    for perm in itertools.permutations(range(3)):
        off = np.zeros(3, dtype=np.int64)
        verts = [nid(ii, jj, kk)]
        for ax in perm:
            off = off.copy()
            off[ax] = 1
            verts.append(nid(ii + off[0], jj + off[1], kk + off[2]))
        cells.append(np.stack(verts, 1))
    cells = np.concatenate(cells, 0)
    M, K = _p1_simplex_assemble(coords, cells)
    onb = np.zeros(len(coords), dtype=bool)
    for d in range(3):
        onb |= (coords[:, d] == 0.0) | (coords[:, d] == 1.0)
    return SpatialDiscretisation(M, K, coords,
                                 np.flatnonzero(onb).astype(np.int32),
                                 f"P1 {n}^3")


def box_p1(nx: int, ny: int, nz: int, lx: float = 1.0, ly: float = 1.0,
           lz: float = 1.0) -> SpatialDiscretisation:
    """P1 on the Kuhn subdivision (six tetrahedra per cell, as ``unit_cube_p1``) of
    ``[0,lx] x [0,ly] x [0,lz]``.  Node ``(i, j, k)`` has index ``(k (ny+1) + j)(nx+1) + i``.
    It carries its ``cells`` (``(6 nx ny nz, 4)``), which ``ReactionTerm`` needs:
    ``box_p1(n, n, n)`` is ``unit_cube_p1(n)``, array for array, with them -- ``unit_cube_p1``
    itself carries none, and a ``ReactionTerm`` on it is refused as before."""
    import itertools
    xs = np.linspace(0.0, lx, nx + 1)
    ys = np.linspace(0.0, ly, ny + 1)
    zs = np.linspace(0.0, lz, nz + 1)
    ZZ, YY, XX = np.meshgrid(zs, ys, xs, indexing="ij")
    coords = np.stack([XX.ravel(), YY.ravel(), ZZ.ravel()], axis=1)

    def nid(i, j, k):
        return (k * (ny + 1) + j) * (nx + 1) + i

    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ii, jj, kk = ii.ravel(), jj.ravel(), kk.ravel()
    cells = []
    for perm in itertools.permutations(range(3)):
        off = [0, 0, 0]
        verts = [nid(ii, jj, kk)]
        for ax in perm:
            off[ax] = 1
            verts.append(nid(ii + off[0], jj + off[1], kk + off[2]))
        cells.append(np.stack(verts, 1))
    cells = np.concatenate(cells, 0)
    M, K = _p1_simplex_assemble(coords, cells)
    onb = np.zeros(len(coords), dtype=bool)
    for d, ax in enumerate((xs, ys, zs)):
        onb |= (coords[:, d] == ax[0]) | (coords[:, d] == ax[-1])
    return SpatialDiscretisation(M, K, coords,
                                 np.flatnonzero(onb).astype(np.int32),
                                 f"P1 {nx}x{ny}x{nz}", cells)


def _p2_1d(n: int, length: float):
    """1-D quadratic Lagrange mass and stiffness on ``n`` elements (2n+1 nodes)."""
    h = length / n
    Me = h / 30.0 * np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]])
    Ke = 1.0 / (3.0 * h) * np.array([[7.0, -8.0, 1.0], [-8.0, 16.0, -8.0],
                                     [1.0, -8.0, 7.0]])
    nn = 2 * n + 1
    M = sp.lil_matrix((nn, nn))
    K = sp.lil_matrix((nn, nn))
    for e in range(n):
        idx = np.array([2 * e, 2 * e + 1, 2 * e + 2])
        M[np.ix_(idx, idx)] += Me
        K[np.ix_(idx, idx)] += Ke
    return sp.csr_matrix(M), sp.csr_matrix(K), np.linspace(0.0, length, nn)


def unit_square_q2(n: int, length: float = 1.0) -> SpatialDiscretisation:
    """Q2 on ``UnitSquareMesh(n, n, quadrilateral=True)`` (tensor-product form); ``length``
    scales the square (``RectangleMesh(n, n, length, length, quadrilateral=True)``).

    This is the space of the reference's known-answer tests
    (``test/test_control.py:1244-1247``).  Dof ``(i, j)`` of the ``(2n+1)^2`` grid
    has index ``j * (2n + 1) + i``.
    """
    M1, K1, xs = _p2_1d(n, length)
    M = sp.kron(M1, M1)
    K = sp.kron(M1, K1) + sp.kron(K1, M1)
    XX, YY = np.meshgrid(xs, xs, indexing="xy")
    coords = np.stack([XX.ravel(), YY.ravel()], axis=1)
    onb = ((coords[:, 0] == 0.0) | (coords[:, 0] == xs[-1])
           | (coords[:, 1] == 0.0) | (coords[:, 1] == xs[-1]))
    return SpatialDiscretisation(_canonical_csr(M), _canonical_csr(K), coords,
                                 np.flatnonzero(onb).astype(np.int32),
                                 f"Q2 {n}x{n}")


def _gauss(npts=4):
    x, w = np.polynomial.legendre.leggauss(npts)
    return 0.5 * (x + 1.0), 0.5 * w          # on [0, 1]


def rectangle_q2(nx: int, ny: int, lx: float = 1.0, ly: float = 1.0) -> SpatialDiscretisation:
    """Q2 on the ``nx x ny`` quadrilateral mesh of ``[0,lx] x [0,ly]``, assembled from elements:
    the space of ``unit_square_q2`` (for ``nx = ny``, ``lx = ly``: its ``coords`` and ``boundary``
    array for array, its matrices to rounding) with the element data ``ReactionTerm`` needs.  Dofs
    are the points of the ``(2nx+1) x (2ny+1)`` grid in y-major order; ``cells`` is ``(nx ny, 9)``
    int32 with local node ``3 j + i`` (``i`` along x, ``j`` along y, each 0..2), cell ``(ex, ey)``
    at index ``ey nx + ex``.  The element matrices are the tensor products of the 1-D ones of
    ``_p2_1d``.  The Jacobi-scaled mass matrix has its spectrum in ``(0.25, 1.5625)`` (the
    reference's interval for Q2)."""
    nvx, nvy = 2 * nx + 1, 2 * ny + 1
    hx, hy = lx / nx, ly / ny
    m = np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]])
    k = np.array([[7.0, -8.0, 1.0], [-8.0, 16.0, -8.0], [1.0, -8.0, 7.0]])
    Mx, My = hx / 30.0 * m, hy / 30.0 * m
    Kx, Ky = 1.0 / (3.0 * hx) * k, 1.0 / (3.0 * hy) * k
    Me = np.kron(My, Mx)                                        # [3 j + i, 3 j' + i']
    Ke = np.kron(My, Kx) + np.kron(Ky, Mx)
    ex, ey = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    first = (2 * ey.ravel() * nvx + 2 * ex.ravel())[:, None]
    i, j = np.tile(np.arange(3), 3), np.repeat(np.arange(3), 3)
    cells = np.ascontiguousarray(first + (j * nvx + i)[None, :], dtype=np.int32)
    ne, n = nx * ny, nvx * nvy
    xs, ys = np.linspace(0.0, lx, nvx), np.linspace(0.0, ly, nvy)
    XX, YY = np.meshgrid(xs, ys, indexing="xy")
    coords = np.stack([XX.ravel(), YY.ravel()], axis=1)
    onb = ((coords[:, 0] == 0.0) | (coords[:, 0] == xs[-1])
           | (coords[:, 1] == 0.0) | (coords[:, 1] == ys[-1]))
    return SpatialDiscretisation(
        _assemble_like(np.broadcast_to(Me, (ne, 9, 9)), cells, cells, (n, n)),
        _assemble_like(np.broadcast_to(Ke, (ne, 9, 9)), cells, cells, (n, n)), coords,
        np.flatnonzero(onb).astype(np.int32), f"rectangle_q2({nx},{ny})", cells)


# --------------------------------------------------------------- Taylor-Hood (Q2-Q1)


def _p1p2_1d(n: int, length: float):
    """1-D mixed matrices between P1 (n+1 nodes) test and P2 (2n+1 nodes) trial functions:
    ``MX[i, j] = int psi_i phi_j`` and ``DX[i, j] = int psi_i phi_j'``; plus P1 mass/stiffness."""
    h = length / n
    xq, wq = _gauss(4)
    psi = np.stack([1.0 - xq, xq])                                    # P1 on [0,1]
    phi = np.stack([2 * (xq - 0.5) * (xq - 1.0), 4 * xq * (1.0 - xq), 2 * xq * (xq - 0.5)])
    dphi = np.stack([4 * xq - 3.0, 4.0 - 8 * xq, 4 * xq - 1.0])       # d/d(xi)
    MXe = h * np.einsum("iq,jq,q->ij", psi, phi, wq)
    DXe = np.einsum("iq,jq,q->ij", psi, dphi, wq)                     # h * (1/h)
    M1e = h * np.einsum("iq,jq,q->ij", psi, psi, wq)
    K1e = (1.0 / h) * np.array([[1.0, -1.0], [-1.0, 1.0]])
    MX = sp.lil_matrix((n + 1, 2 * n + 1))
    DX = sp.lil_matrix((n + 1, 2 * n + 1))
    M1 = sp.lil_matrix((n + 1, n + 1))
    K1 = sp.lil_matrix((n + 1, n + 1))
    for e in range(n):
        ip = np.array([e, e + 1])
        iv = np.array([2 * e, 2 * e + 1, 2 * e + 2])
        MX[np.ix_(ip, iv)] += MXe
        DX[np.ix_(ip, iv)] += DXe
        M1[np.ix_(ip, ip)] += M1e
        K1[np.ix_(ip, ip)] += K1e
    return sp.csr_matrix(MX), sp.csr_matrix(DX), sp.csr_matrix(M1), sp.csr_matrix(K1)


@dataclass
class TaylorHoodDiscretisation:
    """Q2 velocity (two components, component-major dof order) and Q1 pressure on
    ``UnitSquareMesh(n, n, quadrilateral=True)`` -- the spaces of the reference's
    incompressible known-answer test (``test/test_control.py:232-237``)."""
    M_v: sp.csr_matrix        # vector mass
    K_v: sp.csr_matrix        # vector grad-grad
    B: sp.csr_matrix          # -(div v, q): shape (n_p, n_v)
    M_p: sp.csr_matrix
    K_p: sp.csr_matrix
    coords_v: np.ndarray      # (n_v / 2, 2) node coordinates of one component
    coords_p: np.ndarray
    boundary_v: np.ndarray    # Dirichlet dofs of the vector space (both components)
    elem: dict = None         # element data for re-assembly (rectangle_p2p1, rectangle_q2q1)

    @property
    def n_v(self):
        return self.M_v.shape[0]

    def convection_v(self, w: np.ndarray) -> sp.csr_matrix:
        """``inner(dot(grad(trial), w), test) * dx`` on the velocity space for a P2 vector
        field ``w`` (component-major), the Picard linearisation of the Navier-Stokes
        convection term (``test/test_control.py:4194-4199``).  Same sparsity structure as
        ``M_v`` / ``K_v`` entry by entry, so it can be re-uploaded with
        ``kkt_update_block_values``."""
        data = self.convection_v_data(w)
        return sp.csr_matrix((data, self.K_v.indices.copy(), self.K_v.indptr.copy()),
                             shape=self.K_v.shape)

    def convection_v_data(self, w: np.ndarray) -> np.ndarray:
        """The values of ``convection_v(w)`` on the structure of ``K_v`` (no sparse-matrix
        construction: element entries are summed through a cached scatter map)."""
        e = self._need_elem()
        n2 = self.n_v // 2
        V = e["V"]
        wq = np.stack([w[:n2][V] @ e["phi"].T, w[n2:][V] @ e["phi"].T], axis=2)  # (ne, nq, 2)
        adv = np.matmul(e["gphi"], wq[..., None])[..., 0]              # (w . grad phi_b)
        Ne = np.einsum("eq,qa,eqb->eab", e["W"], e["phi"], adv)
        if "scatter_v" not in e:
            # CSR position of every element entry in the scalar P2 structure (one component)
            K2 = self.K_v[:n2, :n2].tocsr()
            K2.sort_indices()
            rows = np.repeat(V, V.shape[1], axis=1).ravel()
            cols = np.tile(V, (1, V.shape[1])).ravel()
            key = K2.indptr[rows].astype(np.int64)
            # position of `cols` inside each row's sorted index list
            pos = np.empty(len(rows), dtype=np.int64)
            for r0 in range(0, len(rows), 1 << 20):
                sl = slice(r0, r0 + (1 << 20))
                pos[sl] = [0] * 0 or _row_positions(K2, rows[sl], cols[sl])
            e["scatter_v"] = key + pos
            e["nnz2"] = K2.nnz
        d2 = np.bincount(e["scatter_v"], weights=Ne.ravel(), minlength=e["nnz2"])
        return np.concatenate([d2, d2])

    def convection_p(self, w: np.ndarray) -> sp.csr_matrix:
        """The same form on the pressure space (``construct_D_v(p_trial, p_test, ...)``,
        ``control/control.py:3783-3785``): structure of ``M_p`` / ``K_p``."""
        e = self._need_elem()
        n2 = self.n_v // 2
        V, Pn = e["V"], e["P"]
        wq = np.stack([e["phi"] @ w[:n2][V].T, e["phi"] @ w[n2:][V].T], axis=2)
        if e["glam"].ndim == 4:          # gradients that depend on the point (Q1)
            adv = np.einsum("qed,eqcd->eqc", wq, e["glam"])
        else:
            adv = np.einsum("qed,ecd->eqc", wq, e["glam"])             # (w . grad lambda_c)
        Ne = np.einsum("eq,qa,eqc->eac", e["W"], e["lam"], adv)
        return _assemble_like(Ne, Pn, Pn, (self.n_p, self.n_p))

    def _need_elem(self):
        if self.elem is None:
            raise NotImplementedError("re-assembly needs element data (rectangle_p2p1 or "
                                      "rectangle_q2q1)")
        return self.elem

    @property
    def n_p(self):
        return self.M_p.shape[0]


class ConvectionTerm:
    """The declared forward form ``nu (grad u, grad v) + ((w . grad) u, v)`` of Navier-Stokes
    control on a Taylor-Hood discretisation with element data (``rectangle_p2p1``,
    ``rectangle_q2q1``) -- a forward
    operator the library can read: ``Stationary.incompressible_non_linear_solve(device=True)``
    assembles it on the GPU from ``nu`` and the element tables.

    ``term(w)``: ``nu K_v + C_v(w)`` on the structure of ``K_v`` (explicit zeros kept), built as
    ``picard.NavierStokesControl.D_v`` builds it; ``term.pressure(w)``: ``nu K_p + C_p(w)`` on
    the structure of ``K_p``, the ``forward_operator_p`` of the incompressible drivers."""

    def __init__(self, disc, nu):
        if getattr(disc, "elem", None) is None:
            raise ValueError("ConvectionTerm needs a Taylor-Hood discretisation with element data "
                             "(fem.rectangle_p2p1 or fem.rectangle_q2q1)")
        self.disc, self.nu = disc, float(nu)

    def __call__(self, w):
        from .picard import _same_structure_sum
        th = self.disc
        return _same_structure_sum(th.K_v, [(self.nu, th.K_v), (1.0, th.convection_v(w))])

    def pressure(self, w):
        from .picard import _same_structure_sum
        th = self.disc
        return _same_structure_sum(th.K_p, [(self.nu, th.K_p), (1.0, th.convection_p(w))])


def _row_positions(A, rows, cols):
    """Index of ``cols[k]`` inside row ``rows[k]`` of the CSR matrix ``A`` (sorted indices)."""
    out = np.empty(len(rows), dtype=np.int64)
    # vectorised binary search per entry inside its row segment
    lo = A.indptr[rows].astype(np.int64)
    hi = A.indptr[rows + 1].astype(np.int64)
    idx = A.indices
    base = lo.copy()
    n = (hi - lo).max()
    step = 1
    while step < n:
        step <<= 1
    pos = np.zeros(len(rows), dtype=np.int64)
    while step:
        cand = pos + step
        ok = (cand < hi - base) & (idx[np.minimum(base + cand, len(idx) - 1)] <= cols)
        pos = np.where(ok, cand, pos)
        step >>= 1
    out[:] = pos
    assert np.array_equal(idx[base + pos], cols)
    return out


def _assemble_like(Ee, rows, cols, shape):
    """Sum element matrices ``Ee[e, a, b]`` into CSR; entries are ordered by (row, column)
    whatever their values, so every matrix assembled over the same connectivity has the
    same ``indptr`` / ``indices``."""
    r = np.repeat(rows, cols.shape[1], axis=1).ravel()
    c = np.tile(cols, (1, rows.shape[1])).ravel()
    return _canonical_csr(sp.coo_matrix((Ee.ravel(), (r, c)), shape=shape))


def unit_square_q2q1(n: int, length: float = 1.0) -> TaylorHoodDiscretisation:
    sd = unit_square_q2(n, length)
    M2, K2 = sd.M, sd.K
    I2 = sp.identity(2, format="csr")
    M_v = _canonical_csr(sp.kron(I2, M2))
    K_v = _canonical_csr(sp.kron(I2, K2))
    MX, DX, M1, K1 = _p1p2_1d(n, length)
    # dof (i, j) -> j * n_nodes_x + i  (y index major), as in unit_square_q2
    Bx = sp.kron(MX, DX)          # int q  d(v_x)/dx : (y: psi*phi) x (x: psi*phi')
    By = sp.kron(DX, MX)          # int q  d(v_y)/dy
    B = _canonical_csr(-sp.hstack([Bx, By]))
    M_p = _canonical_csr(sp.kron(M1, M1))
    K_p = _canonical_csr(sp.kron(M1, K1) + sp.kron(K1, M1))
    xs = np.linspace(0.0, length, n + 1)
    XX, YY = np.meshgrid(xs, xs, indexing="xy")
    coords_p = np.stack([XX.ravel(), YY.ravel()], axis=1)
    nb = sd.boundary
    boundary_v = np.concatenate([nb, nb + sd.n_dofs]).astype(np.int32)
    return TaylorHoodDiscretisation(M_v, K_v, B, M_p, K_p, sd.coords, coords_p, boundary_v)


def rectangle_q2q1(nx: int, ny: int, lx: float = 1.0, ly: float = 1.0) -> TaylorHoodDiscretisation:
    """Q2 velocity / Q1 pressure on the ``nx x ny`` quadrilateral mesh of ``[0,lx] x [0,ly]``,
    assembled from elements, with the element data the convection re-assembly needs: the spaces of
    ``unit_square_q2q1`` (for ``nx = ny``, ``lx = ly``: its ``coords_*`` and ``boundary_v`` array
    for array, its matrices to rounding).

    Velocity nodes and cells are those of ``rectangle_q2`` (y-major ``(2nx+1) x (2ny+1)`` grid,
    ``V`` (ne, 9) with local node ``3 j + i``, cell ``(ex, ey)`` at index ``ey nx + ex``), and
    ``M_v`` / ``K_v`` are its ``M`` / ``K`` once per component (component-major).  Pressure nodes
    are the ``(nx+1) x (ny+1)`` vertices, y-major; ``P`` is (ne, 4) with local node ``2 j + i``.

    The rule is the 4 x 4 Gauss-Legendre product rule on the unit square: point ``q = 4 r + s`` is
    ``(t_s, t_r)`` with weight ``wt_r wt_s``, exact to degree 7 in each variable.  On axis-parallel
    cells the velocity integrand ``phi_a (w . grad phi_b)`` with a Q2 wind has degree at most 6 per
    variable (2 + 2 + 2; the derivative lowers one of them), the pressure integrand
    ``lam_c (w . grad lam_d)`` at most 4 (1 + 2 + 1), and those of ``B``, ``M_p``, ``K_p`` at most
    3: all are integrated exactly.

    ``elem``: ``V``, ``P``, ``W`` (ne, 16) weight times ``hx hy``, ``phi`` (16, 9) the rounded
    products of the 1-D values as ``_gauss_square_rule`` forms them, ``gref`` (16, 9, 2) the
    gradients on the unit square, ``lam`` (16, 4), ``lref`` (16, 4, 2), ``jinv`` (ne, 2) =
    ``1 / hx, 1 / hy``, and the physical gradients ``gphi`` (ne, 16, 9, 2), ``glam``
    (ne, 16, 4, 2), each entry the one rounded product ``ref jinv`` (views of one cell's tables:
    all cells are congruent); ``kind = "q2q1"``."""
    sd = rectangle_q2(nx, ny, lx, ly)
    V, n2 = sd.cells, sd.n_dofs
    ne, npx = nx * ny, nx + 1
    n1 = npx * (ny + 1)
    hx, hy = lx / nx, ly / ny
    ex, ey = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    first = (ey.ravel() * npx + ex.ravel())[:, None]
    i, j = np.tile(np.arange(2), 2), np.repeat(np.arange(2), 2)
    Pn = np.ascontiguousarray(first + (j * npx + i)[None, :], dtype=np.int32)

    t, wt = _gauss(4)
    wq = np.repeat(wt, 4) * np.tile(wt, 4)

    def tensor(fx, fy):           # [q = 4 r + s, k j + i] = fx[i, s] fy[j, r]
        k = len(fx)
        return (fx.T[None, :, None, :] * fy.T[:, None, :, None]).reshape(16, k * k)
    l = _q2_shape_functions_1d(t)                                     # (3, 4): l[i, s]
    dl = np.stack([4 * t - 3.0, 4.0 - 8 * t, 4 * t - 1.0])
    psi = np.stack([1.0 - t, t])
    dpsi = np.stack([-np.ones(4), np.ones(4)])
    phi, lam = tensor(l, l), tensor(psi, psi)
    gref = np.stack([tensor(dl, l), tensor(l, dl)], axis=2)           # (16, 9, 2)
    lref = np.stack([tensor(dpsi, psi), tensor(psi, dpsi)], axis=2)   # (16, 4, 2)
    j1 = np.array([1.0 / hx, 1.0 / hy])
    gphi1, glam1 = gref * j1, lref * j1
    W1 = wq * (hx * hy)
    Bxe = -np.einsum("q,qc,qa->ca", W1, lam, gphi1[..., 0])           # (4, 9)
    Bye = -np.einsum("q,qc,qa->ca", W1, lam, gphi1[..., 1])
    Mpe = np.einsum("q,qc,qd->cd", W1, lam, lam)
    Kpe = np.einsum("q,qcx,qdx->cd", W1, glam1, glam1)

    def asm(Ee, rows, cols, shape):
        return _assemble_like(np.broadcast_to(Ee, (ne,) + Ee.shape), rows, cols, shape)
    Bx, By = asm(Bxe, Pn, V, (n1, n2)), asm(Bye, Pn, V, (n1, n2))
    I2 = sp.identity(2, format="csr")
    xp, yp = np.linspace(0.0, lx, npx), np.linspace(0.0, ly, ny + 1)
    XP, YP = np.meshgrid(xp, yp, indexing="xy")
    coords_p = np.stack([XP.ravel(), YP.ravel()], axis=1)
    nb = sd.boundary
    elem = dict(V=V, P=Pn, W=np.broadcast_to(W1, (ne, 16)), phi=phi, gref=gref, lam=lam,
                lref=lref, jinv=np.broadcast_to(j1, (ne, 2)),
                gphi=np.broadcast_to(gphi1, (ne, 16, 9, 2)),
                glam=np.broadcast_to(glam1, (ne, 16, 4, 2)), kind="q2q1")
    return TaylorHoodDiscretisation(
        _canonical_csr(sp.kron(I2, sd.M)), _canonical_csr(sp.kron(I2, sd.K)),
        _canonical_csr(sp.hstack([Bx, By])), asm(Mpe, Pn, Pn, (n1, n1)),
        asm(Kpe, Pn, Pn, (n1, n1)), sd.coords, coords_p,
        np.concatenate([nb, nb + n2]).astype(np.int32), elem=elem)


# ------------------------------------------------------- Taylor-Hood (P2-P1, triangles)

def _p2_triangle_elements(nx: int, ny: int, lx: float, ly: float) -> dict:
    """The P2 element data of the right-diagonal triangulation of ``[0,lx] x [0,ly]``, shared by
    ``rectangle_p2p1`` (one velocity component) and ``rectangle_p2`` (the scalar space): the
    connectivity ``V`` (ne, 6) and ``P`` (ne, 3), Radon's tables, the shape functions and their
    gradients at the points, the element matrices ``Me`` / ``Ke``, dof coordinates and boundary
    dofs.  P2 dofs are the points of the ``(2nx+1) x (2ny+1)`` grid in y-major order; local P2
    order: vertices 0, 1, 2, then the midpoints of edges (0,1), (1,2), (0,2)."""
    nvx, nvy = 2 * nx + 1, 2 * ny + 1
    npx = nx + 1

    def vid(i, j):          # P2 grid index
        return j * nvx + i

    def pid(i, j):
        return j * npx + i
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    ii, jj = ii.ravel(), jj.ravel()
    hx, hy = lx / nx, ly / ny
    # two triangles per cell: (00, 10, 11) and (00, 11, 01)
    tri_v, tri_p, tri_x = [], [], []
    for (a, b, c) in (((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1))):
        verts = [a, b, c]
        mids = [((a[0] + b[0]), (a[1] + b[1])), ((b[0] + c[0]), (b[1] + c[1])),
                ((a[0] + c[0]), (a[1] + c[1]))]
        v_idx = [vid(2 * ii + 2 * v[0], 2 * jj + 2 * v[1]) for v in verts] + \
                [vid(2 * ii + m[0], 2 * jj + m[1]) for m in mids]
        p_idx = [pid(ii + v[0], jj + v[1]) for v in verts]
        xy = [np.stack([(ii + v[0]) * hx, (jj + v[1]) * hy], 1) for v in verts]
        tri_v.append(np.stack(v_idx, 1))
        tri_p.append(np.stack(p_idx, 1))
        tri_x.append(np.stack(xy, 1))
    V = np.concatenate(tri_v, 0)            # (ne, 6)
    Pn = np.concatenate(tri_p, 0)           # (ne, 3)
    X = np.concatenate(tri_x, 0)            # (ne, 3, 2)
    ne = len(V)
    # degree-5 quadrature on the reference triangle (Radon's 7 points), barycentric: exact
    # for the mass matrix (degree 4) and for the convection form with a P2 field (degree 5)
    s15 = np.sqrt(15.0)
    a1, a2 = (6.0 - s15) / 21.0, (6.0 + s15) / 21.0
    w1, w2 = (155.0 - s15) / 1200.0, (155.0 + s15) / 1200.0
    lam = np.array([[1 / 3, 1 / 3, 1 / 3],
                    [a1, a1, 1 - 2 * a1], [a1, 1 - 2 * a1, a1], [1 - 2 * a1, a1, a1],
                    [a2, a2, 1 - 2 * a2], [a2, 1 - 2 * a2, a2], [1 - 2 * a2, a2, a2]])
    wq = 0.5 * np.array([9.0 / 40.0, w1, w1, w1, w2, w2, w2])
    # gradients of barycentric coordinates per element
    A = np.concatenate([np.ones((ne, 3, 1)), X], axis=2)
    Ainv = np.linalg.inv(A)
    glam = np.transpose(Ainv[:, 1:, :], (0, 2, 1))          # (ne, 3, 2)
    detJ = np.abs(np.linalg.det(A))                         # 2 * area
    l = lam                                                 # (nq, 3)
    phi = _p2_shape_functions(l)                            # (nq, 6)
    # d phi / d lambda_k, (nq, 6, 3)
    dphi = np.zeros((len(l), 6, 3))
    for k in range(3):
        dphi[:, k, k] = 4 * l[:, k] - 1
    dphi[:, 3, 0], dphi[:, 3, 1] = 4 * l[:, 1], 4 * l[:, 0]
    dphi[:, 4, 1], dphi[:, 4, 2] = 4 * l[:, 2], 4 * l[:, 1]
    dphi[:, 5, 0], dphi[:, 5, 2] = 4 * l[:, 2], 4 * l[:, 0]
    gphi = np.einsum("qak,ekd->eqad", dphi, glam)           # (ne, nq, 6, 2)
    W = wq[None, :] * detJ[:, None]                         # (ne, nq)
    Me = np.einsum("eq,qa,qb->eab", W, phi, phi)
    Ke = np.einsum("eq,eqad,eqbd->eab", W, gphi, gphi)
    xs, ys = np.linspace(0, lx, nvx), np.linspace(0, ly, nvy)
    XX, YY = np.meshgrid(xs, ys, indexing="xy")
    coords_v = np.stack([XX.ravel(), YY.ravel()], 1)
    onb = ((coords_v[:, 0] == 0) | (coords_v[:, 0] == xs[-1]) | (coords_v[:, 1] == 0)
           | (coords_v[:, 1] == ys[-1]))
    return dict(V=V, P=Pn, X=X, lam=l, glam=glam, detJ=detJ, phi=phi, gphi=gphi, W=W, Me=Me,
                Ke=Ke, n2=nvx * nvy, coords=coords_v, boundary=np.flatnonzero(onb))


def _p2_shape_functions(l: np.ndarray) -> np.ndarray:
    """The six P2 shape functions at the barycentric points ``l`` (nq, 3), in the local order
    of ``_p2_triangle_elements``: ``(nq, 6)``."""
    return np.stack([l[:, 0] * (2 * l[:, 0] - 1), l[:, 1] * (2 * l[:, 1] - 1),
                     l[:, 2] * (2 * l[:, 2] - 1), 4 * l[:, 0] * l[:, 1],
                     4 * l[:, 1] * l[:, 2], 4 * l[:, 0] * l[:, 2]], 1)


def rectangle_p2(nx: int, ny: int, lx: float = 1.0, ly: float = 1.0) -> SpatialDiscretisation:
    """Scalar P2 on the right-diagonal triangulation of ``[0,lx] x [0,ly]``: one velocity
    component of ``rectangle_p2p1(nx, ny, lx, ly)``, array for array (``M``, ``K``, ``coords``,
    ``boundary``).  Dofs are the points of the ``(2nx+1) x (2ny+1)`` grid in y-major order;
    ``cells`` is ``(ne, 6)`` int32 in the local order vertices 0, 1, 2, then the midpoints of
    edges (0,1), (1,2), (0,2) -- what ``ReactionTerm`` needs.  The Jacobi-scaled mass matrix has
    its spectrum in ``(0.3924, 2.0598)`` (the reference's interval for P2 triangles)."""
    e = _p2_triangle_elements(nx, ny, lx, ly)
    V, n2 = e["V"], e["n2"]
    return SpatialDiscretisation(_assemble_like(e["Me"], V, V, (n2, n2)),
                                 _assemble_like(e["Ke"], V, V, (n2, n2)), e["coords"],
                                 e["boundary"].astype(np.int32), name=f"rectangle_p2({nx},{ny})",
                                 cells=np.ascontiguousarray(V, dtype=np.int32))


def unit_square_p2(n: int) -> SpatialDiscretisation:
    return rectangle_p2(n, n)


def rectangle_p2p1(nx: int, ny: int, lx: float = 1.0, ly: float = 1.0) -> TaylorHoodDiscretisation:
    """P2 velocity / P1 pressure on the right-diagonal triangulation of ``[0,lx] x [0,ly]``
    (``RectangleMesh(nx, ny, lx, ly)``, the spaces of the reference's Stokes-control tests,
    ``test/test_control.py:3546-3560``).  P2 dofs are the points of the ``(2nx+1) x (2ny+1)``
    grid, P1 dofs the mesh vertices, both in lexicographic (y-major) order; the velocity
    vector is component-major."""
    e = _p2_triangle_elements(nx, ny, lx, ly)
    V, Pn, W, l, phi, gphi, glam, detJ = (e[k] for k in ("V", "P", "W", "lam", "phi", "gphi",
                                                         "glam", "detJ"))
    npx = nx + 1
    Bxe = -np.einsum("eq,qc,eqa->eca", W, l, gphi[..., 0])  # (ne, 3, 6)
    Bye = -np.einsum("eq,qc,eqa->eca", W, l, gphi[..., 1])
    Mpe = np.einsum("eq,qc,qd->ecd", W, l, l)
    Kpe = np.einsum("e,ecx,edx->ecd", 0.5 * detJ, glam, glam)
    n2, n1 = e["n2"], npx * (ny + 1)

    asm = _assemble_like
    M2 = asm(e["Me"], V, V, (n2, n2))
    K2 = asm(e["Ke"], V, V, (n2, n2))
    Bx = asm(Bxe, Pn, V, (n1, n2))
    By = asm(Bye, Pn, V, (n1, n2))
    M_p = asm(Mpe, Pn, Pn, (n1, n1))
    K_p = asm(Kpe, Pn, Pn, (n1, n1))
    I2 = sp.identity(2, format="csr")
    xp, yp = np.linspace(0, lx, npx), np.linspace(0, ly, ny + 1)
    XP, YP = np.meshgrid(xp, yp, indexing="xy")
    coords_p = np.stack([XP.ravel(), YP.ravel()], 1)
    nb = e["boundary"]
    return TaylorHoodDiscretisation(
        _canonical_csr(sp.kron(I2, M2)), _canonical_csr(sp.kron(I2, K2)),
        _canonical_csr(sp.hstack([Bx, By])), M_p, K_p, e["coords"], coords_p,
        np.concatenate([nb, nb + n2]).astype(np.int32),
        elem=dict(V=V, P=Pn, W=W, phi=phi, gphi=gphi, lam=l, glam=glam))
