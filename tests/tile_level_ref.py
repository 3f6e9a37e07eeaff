"""Host reference for ONE launch of the tile program's two-grid levels (``kkt_debug_tile_levels``,
``pc_tile_sweep<..., COARSE = true>``), for ``tests/test_gpu_tile_levels.py``; checked without a GPU
by ``tests/test_tile_level_ref.py``.  NumPy and SciPy only; nothing here reads the project's sources
or the lists ``build_tile_coarse_lists`` makes -- the only plan data that enters is which rows a
tile owns, in its local order.

A launch runs levels one after the other; a level is ``cycles`` x [coarse correction of the
iterate, ``its`` sweeps] from ``x = 0``, on the rows outside the mask (masked rows stay ``+0.0``):

* right-hand side: ``b = bin`` (solo level) or the LIN epilogue of ``rowstep_ref`` (candidate
  ``ff``) on the update's chain, ``b = fma(cy, bin, fl(ca acc(U, x_prev)))`` with ``x_prev`` the
  previous level's result (chained level); masked rows ``+0.0``.
* residual: ``r = b`` in cycle 0, later ``r = fl(b - acc(A, x))`` -- the chain ``acc`` of
  ``rowstep_ref`` (one fma per stored entry from ``+0.0``, CSR order = slot order), one rounding
  after it.
* restriction, per tile ``t`` and per coarse function ``j`` its own rows touch: the entries ``(P[g,
  j], r[g])`` in ascending local own row; lane ``l`` of 64 accumulates entries ``l, l + 64, ...`` by
  fma from ``+0.0``; the lanes are reduced by the butterfly ``a[l] += a[l ^ o]``, ``o = 32 .. 1``,
  and lane 0 is the tile's partial sum.
* coarse residual: ``rc[j] = 0.0``, then the partial sums of the tiles that touch ``j`` are added
  in ascending tile number, plain additions.
* products: ``ec[j]`` accumulates the columns ``q`` with ``q % 64 == l`` in ascending ``q`` by fma
  in lane ``l`` from ``+0.0``, then the same butterfly; over ``[e_lo[j], e_hi[j])`` for block rows,
  over all ``n_c`` columns for full rows.  ``e_lo`` / ``e_hi`` come from the connected components
  of the pattern of ``P^T A P`` (SciPy): the smallest member rounded down to a multiple of 64, the
  largest member plus one.
* prolongation: ``a[g]`` = the fma chain over the entries of row ``g`` of ``P`` in stored order from
  ``+0.0``; ``x = a`` in cycle 0 and ``x = fl(x + a)`` later.
* sweeps ``s = 1 .. its``: the CHEB epilogue of ``rowstep_ref`` (candidate ``ff``) on ``acc(A, x)``
  with the triple ``coef[s - 1]``; the ``p_{k-1}`` term is absent in the first sweep after a
  correction; ``post1`` / ``post2`` apply to the last sweep of the last cycle only.

Where the kernel states a detail differently from a plain reading of the scheme above, the kernel's
order is what is restated:

* the kernel computes a first step ``p_1 = p1_scale dinv b`` before the first cycle and the
  correction of cycle 0 overwrites it on every row (``x = a``): it leaves no trace and is not
  formed here;
* a lane of a product takes ``q = e_lo + l, e_lo + l + 64, ...``; that is ``q % 64 == l`` because
  ``e_lo`` is a multiple of 64, which is why the components' first members are rounded down;
* the chain of a row includes the columns that point at masked rows (they read an exact zero) and
  the padded slots of a short row (value ``0.0``): neither changes ``acc``, which is never
  ``-0.0`` (it starts at ``+0.0`` and a sum with ``+0.0`` or an exact cancellation is ``+0.0``),
  so the chain over the stored entries with ``x = +0.0`` on masked rows is the same;
* the in-memory product loop holds eight loads in flight but multiplies them in ascending ``q``: the
  same order as the loop over the rows kept in LDS.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import rowstep_ref as rr

LD = np.longdouble
U = 2.0 ** -53
LANES = 64


# ------------------------------------------------------------------------------ chains
def fma(a, b, c):
    """``rowstep_ref.fma_np`` on equal-shaped arrays.  Where a factor is zero the product is an exact
    signed zero and IEEE addition gives the fused result itself; those elements (the columns of
    masked rows, mostly) then stay clear of ``fma_np``'s rational arithmetic for zero results."""
    z = (a == 0.0) | (b == 0.0)
    out = np.empty_like(c)
    out[z] = c[z] + a[z] * b[z]
    nz = ~z
    out[nz] = rr.fma_np(a[nz], b[nz], c[nz])
    return out


class Chain:
    """The fma chain of every row of a CSR matrix, in stored order, from ``+0.0``."""

    def __init__(self, A):
        A = sp.csr_matrix(A)
        self.n = A.shape[0]
        self.data = np.asarray(A.data, np.float64)
        self.indices = np.asarray(A.indices)
        self.indptr = np.asarray(A.indptr)
        w = np.diff(self.indptr)
        self.width = int(w.max(initial=0))
        self.rows = [np.flatnonzero(w > k) for k in range(self.width)]

    def __call__(self, x):
        acc = np.zeros(self.n)
        for k, rows in enumerate(self.rows):
            p = self.indptr[rows] + k
            acc[rows] = fma(self.data[p], x[self.indices[p]], acc[rows])
        return acc


def wave_sums(w, v, start, end):
    """Per segment ``[start[i], end[i])`` of the entry arrays ``w``, ``v``: lane ``l`` accumulates
    the entries ``l, l + 64, ...`` by fma from ``+0.0``, then the xor butterfly; lane 0."""
    start = np.asarray(start, np.int64)
    end = np.asarray(end, np.int64)
    a = np.zeros((len(start), LANES))
    lane = np.arange(LANES)
    rounds = int(-(-(end - start).max(initial=0) // LANES))
    for t in range(rounds):
        idx = start[:, None] + LANES * t + lane[None, :]
        ok = idx < end[:, None]
        a[ok] = fma(w[idx[ok]], v[idx[ok]], a[ok])
    o = LANES // 2
    while o:
        a = a + a[:, lane ^ o]
        o //= 2
    return a[:, 0]


# ------------------------------------------------------------------------- coarse tables
def inverse_ranges(A, P, rows="block"):
    """``(e_lo, e_hi)`` of every row of the coarse inverse: the columns of its diagonal block of
    ``P^T A P`` (connected components of the pattern), from a multiple of 64; ``rows`` = "full":
    all columns."""
    P = sp.csr_matrix(P)
    nc = P.shape[1]
    if rows == "full":
        return np.zeros(nc, np.int64), np.full(nc, nc, np.int64)
    pat = lambda M: sp.csr_matrix((np.ones(len(M.data)), M.indices, M.indptr), shape=M.shape)
    E = (pat(P).T @ pat(sp.csr_matrix(A)) @ pat(P)).tocsr()
    _, comp = connected_components(E, directed=False)
    lo = np.zeros(nc, np.int64)
    hi = np.zeros(nc, np.int64)
    for c in np.unique(comp):
        members = np.flatnonzero(comp == c)
        lo[members] = members.min() & ~63
        hi[members] = members.max() + 1
    return lo, hi


class Restriction:
    """The tiles' restriction lists, from ``P`` and the rows each tile owns (local order)."""

    def __init__(self, P, own):
        P = sp.csr_matrix(P)
        self.nc = P.shape[1]
        seg_w, seg_g, self.start, self.end, self.tile_ptr, self.seg_j = [], [], [], [], [0], []
        at = 0
        for rows in own:
            lists = {}
            for g in rows:
                for q in range(P.indptr[g], P.indptr[g + 1]):
                    lists.setdefault(int(P.indices[q]), []).append((P.data[q], g))
            for j in sorted(lists):
                self.start.append(at)
                at += len(lists[j])
                self.end.append(at)
                self.seg_j.append(j)
                seg_w += [e[0] for e in lists[j]]
                seg_g += [e[1] for e in lists[j]]
            self.tile_ptr.append(len(self.seg_j))
        self.w = np.array(seg_w, np.float64)
        self.g = np.array(seg_g, np.int64)
        self.seg_j = np.array(self.seg_j, np.int64)
        self.longest = max((e - s for s, e in zip(self.start, self.end)), default=0)
        self.most_tiles = int(np.bincount(self.seg_j, minlength=self.nc).max(initial=0))

    def shared(self):
        """Coarse functions that more than one tile touches."""
        return np.flatnonzero(np.bincount(self.seg_j, minlength=self.nc) > 1)

    def __call__(self, r):
        part = wave_sums(self.w, r[self.g], self.start, self.end)
        rc = np.zeros(self.nc)
        for t in range(len(self.tile_ptr) - 1):
            s = slice(self.tile_ptr[t], self.tile_ptr[t + 1])
            rc[self.seg_j[s]] = rc[self.seg_j[s]] + part[s]       # a tile names a function once
        return rc


def products(einv, rc, lo, hi):
    nc = len(rc)
    einv = np.asarray(einv, np.float64).reshape(nc, nc)
    w = np.concatenate([einv[j, lo[j]:hi[j]] for j in range(nc)])
    v = np.concatenate([rc[lo[j]:hi[j]] for j in range(nc)])
    end = np.cumsum(hi - lo)
    return wave_sums(w, v, end - (hi - lo), end)


# -------------------------------------------------------------------------------- a launch
def run(levels, mask, P, own, its, cycles, rows="block", trace=None):
    """The launch.  ``levels``: dicts with ``A`` (CSR), ``dinv``, ``b``, ``coef`` (its x 3), ``einv``,
    ``post1``, ``post2`` (default 1) and, chained, ``U`` (CSR), ``ca``, ``cy``.  ``own``: per tile the
    global rows it owns, local order.  Returns per level ``(out, b)``.  ``trace`` (a list): receives
    ``(level, cycle, rc, ec)`` of every correction."""
    P = sp.csr_matrix(P)
    n = P.shape[0]
    masked = np.zeros(n, bool) if mask is None else np.asarray(mask, bool)
    restrict = Restriction(P, own)
    prolong = Chain(P)
    chains, ranges = {}, {}
    res, x_prev = [], None
    for li, L in enumerate(levels):
        A = L["A"]
        if id(A) not in chains:
            chains[id(A)] = Chain(A)
            ranges[id(A)] = inverse_ranges(A, P, rows)
        spmv = chains[id(A)]
        lo, hi = ranges[id(A)]
        dinv = np.asarray(L["dinv"], np.float64)
        coef = np.asarray(L["coef"], np.float64).reshape(its, 3)
        if "U" in L:
            op = rr.Op("lin", terms=[(L["U"], x_prev)], mask=masked, ca=L["ca"], cy=L["cy"],
                       yin=np.asarray(L["b"], np.float64))
            b = rr.run(op, "ff")[0]
        else:
            b = np.where(masked, 0.0, np.asarray(L["b"], np.float64))
        x = np.zeros(n)
        xo = None
        for cyc in range(cycles):
            r = b if cyc == 0 else np.where(masked, 0.0, b - spmv(x))
            rc = restrict(r)
            ec = products(L["einv"], rc, lo, hi)
            if trace is not None:
                trace.append((li, cyc, rc, ec))
            a = prolong(ec)
            x = a if cyc == 0 else x + a
            for s in range(1, its + 1):
                last = cyc + 1 == cycles and s == its
                op = rr.Op("cheb", mask=masked, dinv=dinv, c1=coef[s - 1, 0], c2=coef[s - 1, 1],
                           c3=coef[s - 1, 2], post1=L.get("post1", 1.0) if last else 1.0,
                           post2=L.get("post2", 1.0) if last else 1.0, b=b,
                           pkm1=xo if s >= 2 else None, pk=x)
                xn = rr.run(op, "ff", acc=spmv(x))[0]
                xo, x = x, xn
        res.append((x, b))
        x_prev = x
    return res


# ------------------------------------------------------- the recurrence in extended precision
def run_exact(levels, mask, P, own, its, cycles, majorant=False):
    """The same recurrence in ``numpy.longdouble`` with sums in any order (no tiles, no lanes), or
    its majorant: every matrix, coefficient and vector replaced by its absolute value and every
    subtraction by an addition -- what bounds the error of any evaluation order.  Returns per level
    the result (or majorant) and the number of roundings on the longest path to it in ``run``."""
    P = sp.csr_matrix(P)
    n = P.shape[0]
    ab = (lambda v: np.abs(v)) if majorant else (lambda v: v)
    sgn = 1 if majorant else -1
    masked = np.zeros(n, bool) if mask is None else np.asarray(mask, bool)
    keep = np.where(masked, LD(0), LD(1))
    ld = lambda v: ab(np.asarray(v, np.float64).astype(LD))
    Pm = sp.csr_matrix(P)
    rows_p = np.repeat(np.arange(n), np.diff(Pm.indptr))

    def mat(A):
        A = sp.csr_matrix(A)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        data = ld(A.data)

        def mv(x):
            y = np.zeros(A.shape[0], LD)
            np.add.at(y, rows, data * x[A.indices])
            return y
        return mv, int(np.diff(A.indptr).max(initial=0))
    pd = ld(Pm.data)
    wp = int(np.diff(Pm.indptr).max(initial=0))
    restr = Restriction(P, own)
    out, x_prev, k_prev = [], None, 0
    for L in levels:
        mv, wa = mat(L["A"])
        E = ld(np.asarray(L["einv"]).reshape(P.shape[1], P.shape[1]))
        dinv = ld(L["dinv"])
        coef = np.asarray(L["coef"], np.float64).reshape(its, 3)
        if "U" in L:
            mu, wu = mat(L["U"])
            b = keep * (ab(LD(L["ca"])) * mu(x_prev) + ab(LD(L["cy"])) * ld(L["b"]))
            kb = k_prev + wu + 2
        else:
            b, kb = keep * ld(L["b"]), 0
        x = np.zeros(n, LD)
        xo, kx, kxo = None, 0, 0
        for cyc in range(cycles):
            r = b if cyc == 0 else keep * (b + sgn * mv(x))
            kr = kb if cyc == 0 else max(kb, kx + wa) + 1
            rc = np.zeros(P.shape[1], LD)
            np.add.at(rc, Pm.indices, pd * r[rows_p])
            ec = E @ rc
            a = np.zeros(n, LD)
            np.add.at(a, rows_p, pd * ec[Pm.indices])
            ka = (kr + -(-restr.longest // LANES) + 6 + restr.most_tiles
                  + -(-P.shape[1] // LANES) + 6 + wp)
            x = a if cyc == 0 else x + a
            kx = ka if cyc == 0 else max(kx, ka) + 1
            for s in range(1, its + 1):
                last = cyc + 1 == cycles and s == its
                c1, c2, c3 = (ab(LD(c)) for c in coef[s - 1])
                v = c2 * x + c3 * dinv * (b + sgn * mv(x))
                if s >= 2:
                    v = v + c1 * xo
                if last:
                    v = v * ab(LD(L.get("post1", 1.0))) * ab(LD(L.get("post2", 1.0)))
                kn = max(kx + wa, kb, kxo if s >= 2 else 0) + 6
                xo, kxo, x, kx = x, kx, keep * v, kn
        out.append((x, kx))
        x_prev, k_prev = x, kx
    return out
