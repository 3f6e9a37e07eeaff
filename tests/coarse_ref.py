"""Host references for the coarse set-up and correction kernels of the two-grid sub-solves
(``galerkin_kernel``, the blocked Gauss-Jordan ``gj_init_kernel`` / ``gj_panel_kernel`` /
``gj_update_kernel``, ``coarse_block_scatter_kernel``, ``coarse_restrict_kernel`` /
``coarse_dense_kernel`` / ``coarse_prolong_kernel`` and their batched forms), for
``tests/test_gpu_coarse_kernels.py``.  Nothing here reads the project's sources: the constants below
restate the launch shapes of ``kernels.hip``.

* ``galerkin_exact``: ``P^T At P`` entry by entry in ``numpy.longdouble`` with
  ``G = |P|^T |At| |P|``, and ``galerkin_depth``, the roundings on the longest path of the kernel.
* ``inverse_columns``: chosen columns of ``A^-1`` far beyond float64 -- a LAPACK solve, then
  iterative refinement on an unevaluated pair of float64 with the residual in double-double.  (A
  residual in ``numpy.longdouble`` alone leaves the iterate moving by ``cond(A) 2^-64`` per step:
  above 2^-60 for every matrix here that is not nearly orthogonal.)
* ``gauss_jordan_f64`` / ``gauss_jordan_unblocked``: the device's algorithm -- partial pivoting, ties
  to the smallest row, the 1e-13 max|diag| threshold -- restated in NumPy, blocked with one matrix
  product per panel and unblocked.  They put a number on what this algorithm loses in float64; run
  on ``fractions.Fraction`` entries they show which intermediates a matrix family produces.
* ``permuted_scaling`` / ``unit_bidiagonal`` / ``tie_blocks``: the exact families, with closed-form
  inverses; the third is exact only under the tie rule.
* ``real_family``, ``sample_columns``, ``distance`` / ``residual``: inputs and measures of the
  inverse tests.
* ``reduce_depth`` and ``stage_ok``: the bound of one stage of the correction from
  ``structures.matvec_exact`` and ``structures.componentwise_ok``.
"""
from fractions import Fraction

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import structures as st

GJ_PANEL = 32             # columns per panel of the blocked Gauss-Jordan
GJ_PANEL_THREADS = 1024   # threads of the panel kernel: its row loops take a second trip above this
GJ_UPDATE_COLS = 64       # columns per workgroup of the update kernel
GJ_TOL = 1e-13            # pivots below GJ_TOL max|diag A| are flagged
REDUCE_THREADS = 256      # threads of the restriction, the dense product and the Galerkin kernel
PROLONG_ROWS = 256 * 2048         # rows one pass of coarse_prolong_kernel covers
PROLONG_BATCHED_ROWS = 256 * 256  # ... of coarse_prolong_batched_kernel
U = st.U
SEED = 20250317


# --------------------------------------------------------------------------- Galerkin matrices
def galerkin_exact(At, P):
    """``(E, G)``: ``E = P^T At P`` accumulated in ``numpy.longdouble`` (products of float64 are
    exact in its 64-bit significand up to one rounding, sums carry 11 more bits than float64) and
    ``G = |P|^T |At| |P|`` in float64, both dense ``n_c x n_c``."""
    At, P = sp.csr_matrix(At), sp.csr_matrix(P)
    n, nc = P.shape
    ld = np.longdouble

    def triple(A, Q):
        Qd = Q.toarray().astype(ld)
        AQ = np.zeros((n, nc), dtype=ld)
        w = np.diff(A.indptr)
        for k in range(int(w.max(initial=0))):          # slot k of every row that has one
            rows = np.flatnonzero(w > k)
            at = A.indptr[rows] + k
            AQ[rows] += A.data[at].astype(ld)[:, None] * Qd[A.indices[at]]
        Qt = Q.T.tocsr()
        E = np.zeros((nc, nc), dtype=ld)
        for i in range(nc):
            s = slice(Qt.indptr[i], Qt.indptr[i + 1])
            E[i] = (Qt.data[s].astype(ld)[:, None] * AQ[Qt.indices[s]]).sum(axis=0)
        return E
    return triple(At, P), triple(abs(At), abs(P)).astype(np.float64)


def galerkin_depth(width, pt_row_lengths):
    """Roundings between one product and entry (i, k), per row i: the fma chain over the ``width``
    slots of a row of A, the thread's fma chain over its ``ceil(L_i / 256)`` entries of row i of
    P^T, and -- tree, final rounding, the rounding of ``blk + c M`` -- 10."""
    L = np.asarray(pt_row_lengths, dtype=np.int64)
    return width + -(-L // REDUCE_THREADS) + 10


# ------------------------------------------------------------------------ extended inverse
def _split(v):
    t = 134217729.0 * v
    hi = t - (t - v)
    return hi, v - hi


def _dd_residual(A, Xh, Xl, B):
    """``B - A (Xh + Xl)`` in double-double (error-free products and sums, the low parts summed
    in float64), rounded to float64."""
    Ah, Al = _split(A)
    Yh, Yl = _split(-Xh)
    sh = B.astype(np.float64).copy()
    sl = np.zeros_like(sh)
    for j in range(A.shape[0]):
        a, ah, al = A[:, j, None], Ah[:, j, None], Al[:, j, None]
        y, yh, yl = -Xh[None, j], Yh[None, j], Yl[None, j]
        p = a * y
        e = ((ah * yh - p) + ah * yl + al * yh) + al * yl        # p + e == a y
        s = sh + p
        bb = s - sh
        sl += ((sh - (s - bb)) + (p - bb)) + e - a * Xl[None, j]
        sh = s
    return sh + sl


def inverse_columns(A, cols, steps=3):
    """``(X, changes)``: columns ``cols`` of ``A^-1`` as ``numpy.longdouble`` (n x len(cols)), and
    per refinement step the largest change of a column relative to its largest entry."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    cols = np.asarray(cols, dtype=np.int64)
    B = np.zeros((n, len(cols)))
    B[cols, np.arange(len(cols))] = 1.0
    lu = scipy.linalg.lu_factor(A)
    Xh = scipy.linalg.lu_solve(lu, B)
    Xl = np.zeros_like(Xh)
    changes = []
    for _ in range(steps):
        d = scipy.linalg.lu_solve(lu, _dd_residual(A, Xh, Xl, B))
        t = Xl + d
        s = Xh + t
        bb = s - Xh
        Xl = (Xh - (s - bb)) + (t - bb)
        Xh = s
        changes.append(float(np.max(np.abs(d).max(axis=0) / np.abs(Xh).max(axis=0))))
    return Xh.astype(np.longdouble) + Xl.astype(np.longdouble), changes


def sample_columns(n, seed=0, random=24):
    """Columns 0, 1, 31 to 33, 1 023 to 1 025 where present, n - 1, and 24 random ones."""
    fixed = [c for c in (0, 1, 31, 32, 33, 1023, 1024, 1025, n - 1) if 0 <= c < n]
    rng = np.random.default_rng([SEED, n, seed])
    extra = rng.choice(n, size=min(random, n), replace=False)
    return np.unique(np.concatenate([fixed, extra]).astype(np.int64))


def distance(X, cols, ref):
    """Largest entrywise distance of the columns ``cols`` of ``X`` from ``ref``."""
    return float(np.max(np.abs(np.asarray(X)[:, cols].astype(np.longdouble) - ref)))


def residual(A, X):
    """``max |A X - I|`` over all entries, in float64."""
    R = np.asarray(A, dtype=np.float64) @ np.asarray(X, dtype=np.float64)
    R[np.diag_indices_from(R)] -= 1.0
    return float(np.max(np.abs(R)))


# ------------------------------------------------------------- the algorithm, restated
def _zero_like(v):
    return v - v


def _pivot(col, c, tie_smallest=True):
    """Row of the largest magnitude among ``col[c:]``; equal magnitudes take the smallest row."""
    v = np.abs(col[c:])
    if tie_smallest:
        return c + int(np.argmax(v))
    return c + len(v) - 1 - int(np.argmax(v[::-1]))


def _is_singular(best, tol):
    return not (best >= tol and best > 0)


def _start(A):
    """Working copy, the identity in A's arithmetic, and the pivot threshold."""
    a = np.array(A, copy=True)
    n = a.shape[0]
    inv = np.empty_like(a)
    inv[...] = a[0, 0] * 0
    inv[np.diag_indices(n)] = a[0, 0] * 0 + 1
    dmax = max(abs(a[r, r]) for r in range(n))
    return a, inv, (Fraction(GJ_TOL) if a.dtype == object else GJ_TOL) * dmax


def _nonzero_rows(f):
    return np.flatnonzero(np.asarray(f != 0, dtype=bool))


def gauss_jordan_unblocked(A, check=None, tie_smallest=True):
    """``(A^-1, bad)`` by Gauss-Jordan on ``[A | I]``, column by column.  ``A``: float64, or an
    object array of ``Fraction``.  ``check``: called with every array of newly computed values."""
    a, inv, tol = _start(A)
    n = a.shape[0]
    M = np.concatenate([a, inv], axis=1)
    bad = n
    for c in range(n):
        p = _pivot(M[:, c], c, tie_smallest)
        d = M[p, c]
        sing = _is_singular(abs(d), tol)
        if p != c:
            M[[c, p]] = M[[p, c]]
        if sing:
            bad = min(bad, c)
            M[c] = _zero_like(M[c])
        else:
            M[c] = M[c] / d
        if check is not None:
            check(M[c])
        f = M[:, c].copy()
        f[c] = f[c] * 0
        rows = _nonzero_rows(f)
        if len(rows):
            M[rows] = M[rows] - f[rows, None] * M[None, c]
            if check is not None:
                check(M[rows])
    return M[:, n:], bad


def gauss_jordan_f64(A, panel=GJ_PANEL, check=None, tie_smallest=True):
    """``(A^-1, bad)`` by the blocked form: the ``panel`` Gauss-Jordan steps of a panel act on
    its columns Y and on the panel's identity columns Z alone; the panel's effect on the rest,
    ``M <- T' Pi M`` (Pi its row swaps; Z holds the columns of T' that differ from I), is one
    matrix product.  With ``check`` the product is the device's chain of multiply-adds, every
    partial sum checked; without, a GEMM."""
    a, inv, tol = _start(A)
    n = a.shape[0]
    zero = a[0, 0] * 0
    one = zero + 1
    bad = n
    for c0 in range(0, n, panel):
        nb = min(panel, n - c0)
        Y = a[:, c0:c0 + nb].copy()
        Z = np.empty_like(Y)
        Z[...] = zero
        Z[c0 + np.arange(nb), np.arange(nb)] = one
        piv = []
        for cc in range(nb):
            c = c0 + cc
            p = _pivot(Y[:, cc], c, tie_smallest)
            d = Y[p, cc]
            sing = _is_singular(abs(d), tol)
            piv.append(p)
            if p != c:                      # ... of Y, and of the processed columns of Z
                Y[[c, p]] = Y[[p, c]]
                Z[[c, p], :cc] = Z[[p, c], :cc]
            if sing:
                bad = min(bad, c)
                Y[c] = _zero_like(Y[c])
                Z[c] = _zero_like(Z[c])
            else:
                Y[c] = Y[c] / d
                Z[c] = Z[c] / d
            f = Y[:, cc].copy()
            f[c] = zero
            rows = _nonzero_rows(f)
            if len(rows):
                Y[rows, cc:] = Y[rows, cc:] - f[rows, None] * Y[None, c, cc:]
                Z[rows, :cc + 1] = Z[rows, :cc + 1] - f[rows, None] * Z[None, c, :cc + 1]
            if check is not None:
                check(Y[c])
                check(Z[c])
                check(Y[rows])
                check(Z[rows])
        for m in (a[:, c0 + nb:], inv):              # the live columns (views)
            for l, p in enumerate(piv):
                if p != c0 + l:
                    m[[c0 + l, p]] = m[[p, c0 + l]]
            Uu = m[c0:c0 + nb].copy()
            m[c0:c0 + nb] = zero
            if check is None:
                m += Z @ Uu
            else:
                for l in range(nb):
                    m += Z[:, l, None] * Uu[None, l]
                    check(m)
    return inv, bad


def to_fractions(A):
    out = np.empty(np.shape(A), dtype=object)
    for idx, v in np.ndenumerate(np.asarray(A, dtype=np.float64)):
        out[idx] = Fraction(float(v))
    return out


def fraction_inverse(A):
    """The exact inverse of a small matrix by Gaussian elimination on ``Fraction`` entries (first
    non-zero pivot: no rounding, so no pivoting strategy)."""
    n = len(A)
    M = [[Fraction(float(v)) for v in row] + [Fraction(int(i == j)) for j in range(n)]
         for i, row in enumerate(np.asarray(A, dtype=np.float64))]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        d = M[c][c]
        M[c] = [v / d for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [v - f * w for v, w in zip(M[r], M[c])]
    return np.array([[float(v) for v in row[n:]] for row in M])


def short_dyadic(values, bits=53):
    """Every value is ``m 2^e`` with ``|m| < 2^bits`` and ``|e| < 200``: float64 holds it exactly,
    far from the ends of its exponent range."""
    for v in np.ravel(values):
        v = Fraction(v)
        num, den = abs(v.numerator), v.denominator
        if den & (den - 1) or den.bit_length() > 200 or num.bit_length() > 200:
            return False
        if num and (num // (num & -num)).bit_length() > bits:
            return False
    return True


# ------------------------------------------------------------------------------ families
def permuted_scaling(n, seed=0):
    """``(A, A^-1)`` with ``A = Pi D``: row i holds ``d_i = +-2^k``, |k| <= 18, in column pi(i)."""
    rng = np.random.default_rng([SEED, n, seed, 1])
    perm = rng.permutation(n)
    d = np.ldexp(rng.choice([-1.0, 1.0], size=n), rng.integers(-18, 19, size=n))
    A = np.zeros((n, n))
    A[np.arange(n), perm] = d
    X = np.zeros((n, n))
    X[perm, np.arange(n)] = 1.0 / d
    return A, X


def unit_bidiagonal(n, seed=0):
    """``(A, A^-1)``, A unit lower bidiagonal with the sub-diagonal drawn from {0, +-1/2, +-1} and
    zero at least every 40 rows: the entries of the inverse are single products of at most 39
    sub-diagonal entries, none below 2^-39.  The +-1 entries tie with the diagonal pivot."""
    rng = np.random.default_rng([SEED, n, seed, 2])
    s = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], size=max(n - 1, 0), p=[0.1, 0.25, 0.25, 0.2, 0.2])
    s[39::40] = 0.0
    A = np.eye(n)
    A[np.arange(1, n), np.arange(n - 1)] = s
    X = np.eye(n)
    for i in range(1, n):
        X[i, :i] = -s[i - 1] * X[i - 1, :i]
    return A, X


def tie_blocks(n, seed=0):
    """``(A, A^-1)``: the identity with 3 x 3 blocks ``[[1, 0, 0], [s, 1, 0], [g, h, 1]]`` on
    scattered index triples, ``s = +-1`` and ``g``, ``h`` odd multiples of 1/64 with |g|, |h| < 1
    < |h - g s|.  The first column of a block ties between its first two rows.  Taking the smaller
    row keeps every pivot on the diagonal and every intermediate a multiple of 2^-12; taking the
    larger one makes ``h - g s`` the next pivot and divides by it, which rounds -- the result then
    misses the closed form in some entries."""
    rng = np.random.default_rng([SEED, n, seed, 3])
    triples = rng.permutation(n)[:3 * (n // 3)].reshape(-1, 3)
    triples.sort(axis=1)
    A, X = np.eye(n), np.eye(n)
    for tr in triples:
        s = rng.choice([-1.0, 1.0])
        h = (2 * rng.integers(16, 32) + 1) / 64.0
        g = -s * (2 * rng.integers(16, 32) + 1) / 64.0
        A[np.ix_(tr, tr)] = [[1, 0, 0], [s, 1, 0], [g, h, 1]]
        X[np.ix_(tr, tr)] = [[1, 0, 0], [-s, 1, 0], [s * h - g, -h, 1]]
    return A, X


EXACT_FAMILIES = {"permuted_scaling": permuted_scaling, "unit_bidiagonal": unit_bidiagonal,
                  "tie_blocks": tie_blocks}
REAL_FAMILIES = ("normal", "permuted", "antidiagonal", "dominant")


def real_family(name, n, seed=0):
    """The four matrices of ``test_gpu_coarse_setup.py::test_dense_inverse_matches_numpy``."""
    rng = np.random.default_rng([SEED, n, seed, REAL_FAMILIES.index(name)])
    noise = rng.standard_normal((n, n))
    if name == "normal":
        return noise
    if name == "permuted":
        return 3.0 * np.eye(n)[rng.permutation(n)] + 0.01 * noise
    if name == "antidiagonal":
        return np.fliplr(np.eye(n)) + 1e-3 * noise
    return n * np.eye(n) + noise


def cpu_measures(A, cols, ref):
    """``(d, rho)``: the larger of the distances and of the residuals that ``gauss_jordan_f64`` and
    ``numpy.linalg.inv`` reach on ``A`` -- what float64 attains on this matrix."""
    gj, bad = gauss_jordan_f64(A)
    assert bad == len(A)
    la = np.linalg.inv(A)
    return (max(distance(gj, cols, ref), distance(la, cols, ref)),
            max(residual(A, gj), residual(A, la)))


def inverse_ratios(A, X):
    """How far the inverse ``X`` of ``A`` is from what float64 attains on ``A``: its distance from
    ``inverse_columns`` on the sampled columns and its residual over all entries, each divided by
    the figure of ``cpu_measures``; and the last change of the refinement.  The bar of the GPU
    tests is 8 on both ratios, the margin of the pressure-stage tests."""
    n = len(A)
    cols = sample_columns(n)
    Xref, changes = inverse_columns(A, cols, steps=2 if n > 1000 else 3)
    d, rho = cpu_measures(A, cols, Xref)
    got_d, got_rho = distance(X, cols, Xref), residual(A, X)

    def over(a, b):
        return a / b if b > 0 else (0.0 if a == 0 else np.inf)
    return over(got_d, d), over(got_rho, rho), changes[-1]


# ------------------------------------------------------------------- correction stages
def reduce_depth(lengths):
    """Roundings on the longest path of a 256-thread strided fma chain with its LDS tree."""
    L = np.asarray(lengths, dtype=np.int64)
    return -(-L // REDUCE_THREADS) + 8


def stage_ok(y, A, x, terms=None, plus=None):
    """``(ratio, equal)``: the worst ratio of ``|y - (A x + plus)|`` to the componentwise bound of
    ``structures.componentwise_ok`` with ``terms`` roundings per row (default: the row's stored
    entries), one more where ``plus`` is added; and whether ``y`` equals the correctly rounded
    result bit for bit."""
    A = sp.csr_matrix(A)
    if plus is None:
        ref, absum, k = st.matvec_exact(A, x)
    else:
        one = sp.identity(A.shape[0], format="csr")
        ref, absum, k = st.rows_exact([(A, x), (one, plus)], A.shape[0])
        k = (k - 1 if terms is None else np.asarray(terms)) + 1
    if plus is None and terms is not None:
        k = np.asarray(terms)
    return st.componentwise_ok(y, ref, absum, k), bool(np.array_equal(y, ref))
