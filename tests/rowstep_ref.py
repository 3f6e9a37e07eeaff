"""Host reference for ONE row step of the preconditioner (``RowOp`` / ``IlOp``, ``csrc/kernels.hpp``),
for ``tests/test_gpu_row_steps.py``; checked without a GPU by ``tests/test_rowstep_ref.py``.  Nothing
here reads the project's sources.

The step, per row ``r``:

* ``acc`` -- one fused multiply-add per stored entry from ``+0.0``, term-major and in CSR order
  inside a term, every fma exact (``fma``).  Padded slots add an exact zero, which leaves ``acc`` as
  it is, so they do not appear here.
* the epilogue under a named *contraction candidate*: a way the sums of the expression can be fused
  without reassociating them.  The library writes candidate ``ff`` (``csrc/epilogue.hpp``, explicit
  fmas under ``contract(off)``); the others are the chains a different epilogue would produce.

  ``EPI_CHEB``  ``v = c1 pkm1; v += c2 pk; v += c3 (dinv (b - acc)); y = post2 (post1 v)``.  First
  letter, the sum ``c1 pkm1 + c2 pk``: ``u`` both products rounded, ``f`` = ``fma(c2, pk, fl(c1
  pkm1))``, ``g`` = ``fma(c1, pkm1, fl(c2 pk))``.  Second letter, ``+ c3 t`` with ``t = fl(dinv fl(b -
  acc))``: ``u`` product rounded then added, ``f`` one fma.  ``post2 (post1 v)`` and ``t`` have no
  choice.  Without ``pkm1`` the first letter has no choice (``0 + c2 pk``), without ``pk`` neither
  has (``0 + c3 t``).
  ``EPI_LIN``   ``v = ca acc; v += cy yin; v += cz z``.  First letter, the first addend present:
  ``u``, ``f`` = ``fma(c, w, fl(ca acc))``, ``g`` = ``fma(ca, acc, fl(c w))``.  Second letter, the
  second addend: ``u`` | ``f``.  ``y2 = c3 (dinv y)`` has no choice.
  Masked rows: ``+0.0`` (CHEB); ``malpha mx`` or ``+0.0`` (LIN), and ``y2`` follows from them.

* ``exact``: the unrounded expression in ``numpy.longdouble`` (64-bit significand: its own error is
  2^-11 of the bound below) with the sum of absolute values of the same expression and the number
  of roundings on the longest path of the unfused chain -- entries of the row (one per fma), then
  CHEB: ``b - acc``, ``dinv *``, ``c3 *``, the add, ``post1 *``, ``post2 *`` = entries + 6; LIN: ``ca
  *`` and one per addend present = entries + 1 + addends; ``y2``: two more.  The bound is
  ``roundings * u * sum``.
"""
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
SEED = 20250310
LD = np.longdouble


# ------------------------------------------------------------------------ exact arithmetic
def fma(a, b, c):
    """``a b + c`` rounded once (``float`` of a ``Fraction`` rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _two_product(a, b):
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_np(a, b, c):
    """Elementwise ``fma`` on arrays, correctly rounded.  With ``p + e = a b``, ``s + t = p + c``, ``r +
    d = t + e`` and ``h + l = s + r`` exactly, the value is ``h + l + d`` with ``h = fl(s + r)``; ``l2 =
    fl(l + d)`` is ``l + d`` to a relative 2^-53.  ``h`` is the answer when ``d == 0``, or when ``fl(h +
    (1 + 2^-20) l2) == h``: ``l + d`` then lies strictly inside the rounding interval of ``h``.  The
    remaining elements (``l + d`` within 2^-20 of a rounding boundary, or past it) and results that
    are zero go through ``Fraction``."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64),
                                  np.asarray(c, np.float64))
    p, e = _two_product(a, b)
    s, t = _two_sum(p, c)
    r, d = _two_sum(t, e)
    h, l = _two_sum(s, r)
    out = np.array(h, dtype=np.float64)
    redo = (d != 0.0) & (h + (1.0 + 2.0 ** -20) * (l + d) != h)
    # signed zeros: decided below by the rules of IEEE 754
    redo |= (out == 0.0)
    for k in np.flatnonzero(redo.ravel()):
        ak, bk, ck = float(a.ravel()[k]), float(b.ravel()[k]), float(c.ravel()[k])
        v = Fraction(ak) * Fraction(bk) + Fraction(ck)
        if v == 0:
            # IEEE: the sum of two zeros of opposite sign, or an exact cancellation, is +0.0;
            # (-0) + (-0) is -0.0
            prod_neg = np.signbit(ak) != np.signbit(bk)
            both_zero = (ak == 0.0 or bk == 0.0) and ck == 0.0
            out.ravel()[k] = -0.0 if (both_zero and prod_neg and np.signbit(ck)) else 0.0
        else:
            out.ravel()[k] = float(v)
    return out


# ---------------------------------------------------------------------------------- one op
@dataclass
class Op:
    """One block-row operation on host data.  ``terms``: list of ``(A, x)`` (CSR, vector); absent
    operands are ``None``; ``mask``: boolean rows or ``None``."""
    mode: str                       # "lin" | "cheb"
    terms: list = field(default_factory=list)
    mask: object = None
    dinv: object = None
    # lin
    ca: float = 1.0
    cy: float = 0.0
    cz: float = 0.0
    malpha: float = 0.0
    yin: object = None
    z: object = None
    mx: object = None
    y2: bool = False
    # cheb (c3 also scales y2)
    c1: float = 0.0
    c2: float = 0.0
    c3: float = 0.0
    post1: float = 1.0
    post2: float = 1.0
    b: object = None
    pkm1: object = None
    pk: object = None

    @property
    def n(self):
        for v in (self.b, self.yin, self.z, self.dinv, self.mx):
            if v is not None:
                return len(v)
        return self.terms[0][0].shape[0]

    def operands(self):
        """The operand set that decides which candidates are distinct."""
        if self.mode == "cheb":
            return ("cheb", self.pkm1 is not None, self.pk is not None)
        return ("lin", self.yin is not None, self.z is not None, bool(self.terms))


def candidates(op):
    """The distinct candidates of the op's operand set."""
    a, b = op.operands()[1:3]
    if op.mode == "cheb":
        first = "ufg" if (a and b) else "u"
        second = "uf" if b else "u"          # 0 + c3 t: both ways give fl(c3 t)
    else:
        # (without terms ``ca acc`` is a zero and the first sum has nothing to round twice)
        first = "ufg" if ((a or b) and op.terms) else "u"
        second = "uf" if (a and b) else "u"
    return tuple(x + y for x in first for y in second)


def accumulate(op, drop_last=False):
    """``acc`` of every row: the fma chain, term-major, CSR order.  ``drop_last``: without the last
    stored entry of every row of the last term (a perturbation for the host tests)."""
    acc = np.zeros(op.n)
    for ti, (A, x) in enumerate(op.terms):
        A = sp.csr_matrix(A)
        x = np.asarray(x, np.float64)
        w = np.diff(A.indptr)
        if drop_last and ti == len(op.terms) - 1:
            w = np.maximum(w - 1, 0)
        for k in range(int(w.max(initial=0))):
            rows = np.flatnonzero(w > k)
            p = A.indptr[rows] + k
            acc[rows] = fma_np(A.data[p], x[A.indices[p]], acc[rows])
    return acc


def _sum2(kind, cp, wp, cq, wq):
    """``cp wp + cq wq``, ``cp wp`` first in the source."""
    if kind == "u":
        return cp * wp + cq * wq
    if kind == "f":
        return fma_np(cq, wq, cp * wp)
    return fma_np(cp, wp, cq * wq)


def _add(kind, v, c, w):
    return v + c * w if kind == "u" else fma_np(c, w, v)


def run(op, cand, acc=None):
    """``(y, y2)`` of the op under candidate ``cand`` (``y2`` None unless asked for)."""
    acc = accumulate(op) if acc is None else acc
    n = op.n
    masked = np.zeros(n, bool) if op.mask is None else np.asarray(op.mask, bool)
    if op.mode == "cheb":
        t = op.dinv * (op.b - acc)
        if op.pkm1 is not None and op.pk is not None:
            v = _sum2(cand[0], op.c1, op.pkm1, op.c2, op.pk)
        elif op.pk is not None:
            v = 0.0 + op.c2 * op.pk
        elif op.pkm1 is not None:
            v = op.c1 * op.pkm1
        else:
            v = np.zeros(n)
        v = _add(cand[1], v, op.c3, t)
        y = op.post2 * (op.post1 * v)
        return np.where(masked, 0.0, y), None
    adds = [(c, w) for c, w in ((op.cy, op.yin), (op.cz, op.z)) if w is not None]
    if adds:
        v = _sum2(cand[0], op.ca, acc, adds[0][0], adds[0][1])
        if len(adds) == 2:
            v = _add(cand[1], v, adds[1][0], adds[1][1])
    else:
        v = op.ca * acc
    my = op.malpha * op.mx if op.mx is not None else np.zeros(n)
    y = np.where(masked, my, v)
    y2 = op.c3 * (op.dinv * y) if op.y2 else None
    return y, y2


def exact(op):
    """``(value, abs_sum, roundings)`` of ``y`` on the unmasked rows, in ``numpy.longdouble``; and the
    same triple for ``y2`` (None without it)."""
    n = op.n
    s = np.zeros(n, LD)
    a = np.zeros(n, LD)
    k = np.zeros(n, np.int64)
    for A, x in op.terms:
        A = sp.csr_matrix(A)
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        prod = A.data.astype(LD) * np.asarray(x, np.float64)[A.indices].astype(LD)
        np.add.at(s, rows, prod)
        np.add.at(a, rows, np.abs(prod))
        k += np.diff(A.indptr)

    def ld(v):
        return np.asarray(v, np.float64).astype(LD)
    if op.mode == "cheb":
        d, c3 = ld(op.dinv), LD(op.c3)
        val, ab = c3 * d * (ld(op.b) - s), abs(c3) * np.abs(d) * (np.abs(ld(op.b)) + a)
        for c, w in ((op.c1, op.pkm1), (op.c2, op.pk)):
            if w is not None:
                val = val + LD(c) * ld(w)
                ab = ab + abs(LD(c)) * np.abs(ld(w))
        pp = LD(op.post1) * LD(op.post2)
        return (val * pp, ab * abs(pp), k + 6), None
    val, ab, kk = LD(op.ca) * s, abs(LD(op.ca)) * a, k + 1
    for c, w in ((op.cy, op.yin), (op.cz, op.z)):
        if w is not None:
            val = val + LD(c) * ld(w)
            ab = ab + abs(LD(c)) * np.abs(ld(w))
            kk = kk + 1
    second = None
    if op.y2:
        f = LD(op.c3) * ld(op.dinv)
        second = (f * val, np.abs(f) * ab, kk + 2)
    return (val, ab, kk), second


def matching(op, y, y2=None, acc=None):
    """The candidates of the op's operand set that give ``y`` (and ``y2``) bit for bit on every
    element, masked rows included."""
    acc = accumulate(op) if acc is None else acc
    found = []
    for cand in candidates(op):
        w, w2 = run(op, cand, acc)
        if same_bits(y, w) and (w2 is None or same_bits(y2, w2)):
            found.append(cand)
    return found


def bound_ratio(y, triple, rows):
    """Largest ``|y - value| / (roundings u abs_sum)`` over ``rows`` (0 where both vanish)."""
    val, ab, k = triple
    err = np.abs(np.asarray(y, np.float64).astype(LD) - val)[rows]
    bnd = (k.astype(LD) * LD(U) * ab)[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / np.where(bnd > 0, bnd, LD(1e-4000)))
    return float(ratio.max(initial=0.0))


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def differ(a, b):
    """Elements whose bits differ."""
    return np.ascontiguousarray(a, np.float64).view(np.int64) != \
        np.ascontiguousarray(b, np.float64).view(np.int64)


# ------------------------------------------------------------------- interleaved levels
def interleave(levels, n):
    """Per-level vectors (``None``: zeros) in the layout of ``IlOp``: groups of four levels, element
    (group g, row r, level l) at ``4 (g n + r) + l``; levels past the last are zero."""
    ng = (len(levels) + 3) // 4
    out = np.zeros((ng, n, 4))
    for q, v in enumerate(levels):
        if v is not None:
            out[q // 4, :, q % 4] = v
    return out.ravel()


def deinterleave(buf, nlev, n):
    """``(levels [nlev, n], rest)``: the levels of an interleaved buffer and the elements of the
    unused levels of its last group."""
    a = np.asarray(buf).reshape(-1, n, 4)
    lev = np.stack([a[q // 4, :, q % 4] for q in range(nlev)])
    rest = np.concatenate([a[nlev // 4, :, l] for l in range(nlev % 4, 4)]) if nlev % 4 else \
        np.zeros(0)
    return lev, rest


# --------------------------------------------------------------------------- SELL layout
def sell_index(r, k, off, R=2, pos=None):
    """Index into a SELL-64R value array of entry ``k`` of row ``r``: position ``p`` (``pos[r]`` in
    row-sorted storage) lies in slice ``p // (64 R)`` at lane ``(p % (64 R)) % 64`` and sub-row ``(p %
    (64 R)) // 64``; ``off``: the slices' first slots."""
    C = 64 * R
    p = r if pos is None else pos[r]
    s, rin = divmod(p, C)
    return (off[s] + k) * C + (rin % 64) * R + rin // 64


def sell_index_swapped(r, k, off, R=2, pos=None):
    """The same with ``R`` and 64 exchanged inside the slice (a wrong layout, for the host tests)."""
    C = 64 * R
    p = r if pos is None else pos[r]
    s, rin = divmod(p, C)
    return (off[s] + k) * C + (rin % R) * 64 + rin // R


# ---------------------------------------------------------------------------------- inputs
def real_vec(n, *key):
    return np.random.default_rng([SEED, n, *key]).standard_normal(n)


def int_vec(n, *key, amp=64):
    rng = np.random.default_rng([SEED, n, *key, amp])
    return (rng.integers(1, amp + 1, size=n) * rng.choice([-1, 1], size=n)).astype(np.float64)


def pow2_vec(n, *key):
    """Powers of two 2^-3 .. 2^2 (a Jacobi diagonal whose products are exact on integer data)."""
    return np.exp2(np.random.default_rng([SEED, n, *key, 7]).integers(-3, 3, size=n).astype(np.float64))


def row_mask(n, R=2, *key):
    """About a quarter of the rows, with the first and last position of every slice of 64 R rows
    (and row n - 1) among them."""
    rng = np.random.default_rng([SEED, n, *key, 11])
    m = rng.random(n) < 0.25
    C = 64 * R
    m[0::C] = True
    m[C - 1::C] = True
    m[n - 1] = True
    return m
