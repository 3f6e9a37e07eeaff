"""Sparse structures chosen for the kernel dispatch, and exact references for the products.

The operator apply and the sweep steps pick their kernel from the widths of the SELL-64R slices
(128 rows at R = 2, ``system.cpp`` ``find_or_add_pattern``): a fixed-width kernel per width
1..16, a width-switched kernel for ragged structures whose slots lie in the unrolled widths, and
the slot loop for the rest.  The generators here give each of those a structure of its own.  Plain
host code (NumPy / SciPy); imported like ``common``.
"""
import math

import numpy as np
import scipy.sparse as sp

from control_amd.fem import SpatialDiscretisation

SLICE = 128                                   # rows per slice at R = 2
ROW_COUNTS = (1, 63, 64, 65, 127, 128, 129, 4133)   # around the slices; 4133 = 32 * 128 + 37
SWITCH_WIDTHS = (4, 5, 7, 9, 12, 15, 19, 24, 38)     # unrolled by the width-switched kernel
GENERIC_WIDTHS = (25, 40)                            # ... not unrolled: the slot loop inside it
PAD_LIMIT = 0.03                              # near-uniform structures padded up to 3 % more slots


# ---------------------------------------------------------------------------- generators
def _values(nnz, rng, integer):
    if integer:
        # small integers, zeros among them: stored explicit zeros
        return rng.integers(-4, 5, size=nnz).astype(np.float64)
    return rng.standard_normal(nnz)


def banded(nrows, widths, seed, integer=False, ncols=None):
    """CSR, ``nrows`` x ``ncols`` (default square), row r holding ``widths[r]`` entries (an int:
    every row).  Columns are distinct, sorted, drawn around the diagonal so that gathers stay
    mostly local, as in a mesh; a width of 0 is an empty row.  ``integer``: values in -4..4."""
    ncols = nrows if ncols is None else ncols
    w = np.full(nrows, widths, dtype=np.int64) if np.isscalar(widths) else np.asarray(widths,
                                                                                      np.int64)
    if w.shape != (nrows,) or w.min(initial=0) < 0 or w.max(initial=0) > ncols:
        raise ValueError("row widths must be 0..ncols, one per row")
    rng = np.random.default_rng(seed)
    indptr = np.zeros(nrows + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(w)
    indices = np.empty(indptr[-1], dtype=np.int32)
    for r in range(nrows):
        k = int(w[r])
        if k == 0:
            continue
        span = min(ncols, max(2 * k, 8))
        c0 = min(max(0, (r * ncols) // max(nrows, 1) - span // 2), ncols - span)
        indices[indptr[r]:indptr[r + 1]] = np.sort(c0 + rng.choice(span, size=k, replace=False))
    A = sp.csr_matrix((_values(indptr[-1], rng, integer), indices, indptr), shape=(nrows, ncols))
    A.has_sorted_indices = True
    return A


def with_values(A, seed, integer=False):
    """The structure of ``A`` (index arrays shared) with new values."""
    rng = np.random.default_rng(seed)
    B = sp.csr_matrix((_values(A.nnz, rng, integer), A.indices, A.indptr), shape=A.shape)
    B.has_sorted_indices = True
    return B


def slice_row_widths(slice_widths, nrows=None, seed=0, ragged=False):
    """Row widths whose slice s (rows 128 s .. 128 s + 127) is ``slice_widths[s]`` wide.
    ``ragged``: rows of a slice vary in 1..w (one row at w); else every row is w wide."""
    rng = np.random.default_rng(seed)
    sw = np.asarray(slice_widths, dtype=np.int64)
    nrows = len(sw) * SLICE if nrows is None else nrows
    w = np.repeat(sw, SLICE)[:nrows].copy()
    if ragged:
        for s, ws in enumerate(sw):
            lo, hi = s * SLICE, min(nrows, (s + 1) * SLICE)
            if ws > 1 and hi > lo:
                w[lo:hi] = rng.integers(1, ws + 1, size=hi - lo)
                w[lo + rng.integers(0, hi - lo)] = ws
    return w


def mixture(shares, nslices, seed=0):
    """Slice widths of a ragged structure: ``shares`` maps width -> share of the SLOTS (not of
    the slices) in slices of that width; slices shuffled."""
    ws = np.array(sorted(shares), dtype=np.int64)
    frac = np.array([shares[w] for w in ws], dtype=np.float64)
    per_slice = frac / ws            # slices needed per slot
    counts = np.maximum(1, np.round(nslices * per_slice / per_slice.sum())).astype(np.int64)
    out = np.repeat(ws, counts)
    np.random.default_rng(seed).shuffle(out)
    return out


def near_uniform(width, over, nslices=40):
    """Slice widths: ``width`` everywhere except slices one narrower, as many as keep the padding
    cost of the uniform layout just under 3 % (``over`` False) or just over it."""
    k = 0
    while padding_fraction_of(np.r_[np.full(nslices - k - 1, width),
                                    np.full(k + 1, width - 1)]) <= PAD_LIMIT:
        k += 1
    # k narrow slices: at most 3 %; k + 1: more
    k = k + 1 if over else k
    return np.r_[np.full(nslices - k, width), np.full(k, width - 1)]


# ----------------------------------------------------------------------- storage accounting
def row_widths(A):
    return np.diff(sp.csr_matrix(A).indptr)


def slice_widths(A, R=2):
    """Slice widths of the unsorted SELL-64R storage."""
    w = row_widths(A)
    C = 64 * R
    n = (len(w) + C - 1) // C
    return np.array([w[s * C:(s + 1) * C].max(initial=0) for s in range(n)], dtype=np.int64)


def padding_fraction_of(sw):
    """Extra slots of padding every slice to the widest, relative to the stored slots."""
    sw = np.asarray(sw, dtype=np.int64)
    return (sw.max() * len(sw) - sw.sum()) / sw.sum()


def padding_fraction(A, R=2):
    return padding_fraction_of(slice_widths(A, R))


def width_histogram(A):
    w, c = np.unique(row_widths(A), return_counts=True)
    return dict(zip(w.tolist(), c.tolist()))


# --------------------------------------------------------------------------- model meshes
def _p1_1d(n):
    h = 1.0 / n
    e = np.ones(n + 1)
    m = sp.diags([e[:-1] * h / 6, np.r_[h / 3, np.full(n - 1, 2 * h / 3), h / 3], e[:-1] * h / 6],
                 [-1, 0, 1])
    k = sp.diags([-e[:-1] / h, np.r_[1 / h, np.full(n - 1, 2 / h), 1 / h], -e[:-1] / h],
                 [-1, 0, 1])
    return sp.csr_matrix(m), sp.csr_matrix(k)


def _grid(n):
    x = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(x, x)                 # node iy * (n + 1) + ix
    coords = np.column_stack([X.ravel(), Y.ravel()])
    b = np.flatnonzero((X.ravel() == 0) | (X.ravel() == 1) | (Y.ravel() == 0) | (Y.ravel() == 1))
    return coords, b.astype(np.int32)


def _canonical(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def q1_square(n):
    """Q1 on the unit square, n x n cells: mass and stiffness as Kronecker products of the 1-D P1
    matrices (what a Firedrake quadrilateral mesh assembles).  Interior rows are 9 wide."""
    m, k = _p1_1d(n)
    coords, b = _grid(n)
    return SpatialDiscretisation(M=_canonical(sp.kron(m, m, format="coo")),
                                 K=_canonical(sp.kron(k, m, format="coo") + sp.kron(m, k, format="coo")),
                                 coords=coords, boundary=b, name=f"q1_{n}")


def fd5_square(n):
    """5-point Laplacian on the (n + 1)^2 grid points of the unit square with the lumped mass
    h^2 I: level rows 5 wide (4 / 3 on the boundary), mass rows 1 wide."""
    e = np.ones(n + 1)
    t = sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
    i = sp.identity(n + 1)
    coords, b = _grid(n)
    return SpatialDiscretisation(M=_canonical(sp.identity((n + 1) ** 2) / n**2),
                                 K=_canonical(sp.kron(i, t, format="coo") + sp.kron(t, i, format="coo")),
                                 coords=coords, boundary=b, name=f"fd5_{n}")


# ------------------------------------------------------------------------ exact references
_SPLIT = 134217729.0          # 2^27 + 1 (Veltkamp)
U = 2.0 ** -53                # unit round-off of fp64


def two_prod(a, b):
    """p, e with p + e == a * b exactly (Dekker; no fma).  |a|, |b| far from overflow."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b

    def split(v):
        t = _SPLIT * v
        hi = t - (t - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def matvec_exact(A, x):
    """A x correctly rounded per row (error-free products summed with ``math.fsum``), with
    (|A| |x|)_i and the stored entries per row: what a componentwise bound needs."""
    A = sp.csr_matrix(A)
    x = np.asarray(x, dtype=np.float64)
    p, e = two_prod(A.data, x[A.indices])
    y = np.empty(A.shape[0])
    for r in range(A.shape[0]):
        s = slice(A.indptr[r], A.indptr[r + 1])
        y[r] = math.fsum(np.concatenate([p[s], e[s]]))
    absum = abs(A) @ np.abs(x)
    return y, absum, row_widths(A)


def rows_exact(terms, n):
    """Correctly rounded sum over several products per row: ``terms`` is a list of (A, x); all A
    have ``n`` rows.  Returns (y*, sum |A||x|, stored entries per row)."""
    parts = [[] for _ in range(n)]
    absum = np.zeros(n)
    k = np.zeros(n, dtype=np.int64)
    for A, x in terms:
        A = sp.csr_matrix(A)
        p, e = two_prod(A.data, np.asarray(x, np.float64)[A.indices])
        for r in range(n):
            s = slice(A.indptr[r], A.indptr[r + 1])
            parts[r].append(p[s])
            parts[r].append(e[s])
        absum += abs(A) @ np.abs(x)
        k += row_widths(A)
    return np.array([math.fsum(np.concatenate(q)) if q else 0.0 for q in parts]), absum, k


def componentwise_ok(y, y_ref, absum, k):
    """|y_i - y*_i| <= (k_i + 2) u (|A||x|)_i + u |y*_i| for every row; returns the worst
    ratio of error to bound (<= 1 passes)."""
    bound = (k + 2) * U * absum + U * np.abs(y_ref)
    err = np.abs(np.asarray(y) - y_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.inf))
    return float(ratio.max(initial=0.0))
