"""Host references for the time-transform, nullspace and value set-up kernels
(``time_transform``, ``time_transform_mask``, ``mask_blocks``, ``const_sums`` / ``const_shift``,
``csr_to_sell``, ``mask_columns``, ``vals_axpy``, ``vals_differ``, ``vals_sym_skew``,
``extract_dinv``), for ``tests/test_gpu_block_kernels.py``.  Plain NumPy, ``int64``, ``Fraction``
and ``math.fsum``, written from the mathematics and from the orders the kernel comments document.
Nothing here calls the library or reads its sources; the constants below restate the launch shapes.

Every float64 operation of NumPy is one IEEE rounding, so a result that is one addition,
subtraction or product -- or a chain of them in a stated order -- is reproduced bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

THREADS = 256             # threads of a workgroup: chains and tree of the const_sums reduction
LANES = 64                # rows of a SELL slice per row slot: slice width C = 64 R
U = 2.0 ** -53            # unit roundoff of float64
SEED = 20241019


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """The comparison every bit-for-bit assertion goes through (``-0.0`` differs from ``+0.0``,
    a NaN equals a NaN of the same bits)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------- Crank-Nicolson transforms
def time_transform(kind, x, lo=None, hi=None):
    """``T_1`` (kind 1: ``new_i = old_i + old_{i+1}``), ``T_2`` (2: ``new_i = old_i + old_{i-1}``),
    ``T_1^-1`` (3: ``for i = n-2 .. 0: x_i -= x_{i+1}``, the updated one) and ``T_2^-1`` (4:
    ``for i = 1 .. n-1: x_i -= x_{i-1}``) of ``x`` (n levels by nx).  ``hi`` stands for a level
    after the last one (kinds 1, 3), ``lo`` for one before the first (kinds 2, 4); for the inverses
    it is the neighbour's already updated value.  A level without a neighbour keeps its bits."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y = x.copy()
    if kind == 1:
        y[:-1] = x[:-1] + x[1:]
        if hi is not None:
            y[-1] = x[-1] + hi
    elif kind == 2:
        y[1:] = x[1:] + x[:-1]
        if lo is not None:
            y[0] = x[0] + lo
    elif kind == 3:
        nxt = hi
        for i in range(n - 1, -1, -1):
            if nxt is not None:
                y[i] = x[i] - nxt
            nxt = y[i]
    elif kind == 4:
        prev = lo
        for i in range(n):
            if prev is not None:
                y[i] = x[i] - prev
            prev = y[i]
    else:
        raise ValueError(kind)
    return y


def split_halos(kind, x, y, cut, lo=None, hi=None):
    """``((lo_a, hi_a), (lo_b, hi_b))`` for the pieces ``x[:cut]`` and ``x[cut:]`` of a transform
    whose unsplit result is ``y``: the outer halos stay where they are, and at the cut a piece reads
    its neighbour's first or last level -- of ``x`` for ``T_1`` / ``T_2``, of ``y`` (the updated
    one) for the inverses."""
    if kind == 1:
        return (None, x[cut]), (None, hi)
    if kind == 2:
        return (lo, None), (x[cut - 1], None)
    if kind == 3:
        return (None, y[cut]), (None, hi)
    return (lo, None), (y[cut - 1], None)


def time_transform_mask(kind, t, xin, masks, alpha, lo=None, hi=None):
    """The fused form: ``y_i[r] = mask_i[r] ? alpha_i * xin_i[r] : T(t)_i[r]`` for kind 1 | 2.
    ``masks``: per level a boolean array or ``None``."""
    assert kind in (1, 2)
    y = time_transform(kind, t, lo, hi)
    for i, m in enumerate(masks):
        if m is not None:
            m = np.asarray(m, dtype=bool)
            y[i][m] = alpha[i] * np.asarray(xin[i], dtype=np.float64)[m]
    return y


def mask_blocks(x, mx, masks, alpha):
    """``y = mask ? (mx ? alpha * mx : +0.0) : x`` per block."""
    y = np.array(x, dtype=np.float64, copy=True)
    for i, m in enumerate(masks):
        if m is not None:
            m = np.asarray(m, dtype=bool)
            y[i][m] = alpha[i] * np.asarray(mx[i], dtype=np.float64)[m] if mx is not None else 0.0
    return y


# ------------------------------------------------------------------------------ the sums
def ordered_sum(x):
    """The sum in the documented order: thread ``t`` of 256 adds the elements ``t, t + 256, ...``
    from ``+0.0``, then a tree over the threads with strides 128, 64, ..., 1.  (A chain that starts
    at ``+0.0`` never holds ``-0.0``, so the absent elements of the last row may be ``+0.0``.)"""
    x = np.asarray(x, dtype=np.float64)
    rows = -(-len(x) // THREADS)
    pad = np.zeros(rows * THREADS)
    pad[:len(x)] = x
    pad = pad.reshape(rows, THREADS)
    acc = np.zeros(THREADS)
    for k in range(rows):
        acc = acc + pad[k]
    st = THREADS // 2
    while st:
        acc = acc[:st] + acc[st:2 * st]
        st >>= 1
    return float(acc[0])


def exact_sum(x):
    """The exact sum rounded once."""
    return math.fsum(np.asarray(x, dtype=np.float64))


def sum_depth(nx):
    """Roundings between an element and the result: its thread's chain, the eight tree levels."""
    return -(-nx // THREADS) + 8


# -------------------------------------------------------------------- fused multiply-add
def fma(a, b, c):
    """``a b + c`` rounded once (``float`` of a ``Fraction`` rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_product(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(a, b):
    """``a + b`` rounded to odd: the exact sum when it is a float64, else the neighbour with an odd
    last mantissa bit."""
    s, t = two_sum(a, b)
    s = np.array(s, dtype=np.float64, copy=True)
    fix = (t != 0.0) & ((bits(s) & 1) == 0)
    toward = np.where(t > 0.0, np.inf, -np.inf)
    s[fix] = np.nextafter(s[fix], toward[fix])
    return s


def fma_np(a, b, c):
    """``fma`` on arrays, still one rounding: ``a b = p + e`` exactly (Dekker), then the correctly
    rounded sum of the three numbers ``p, e, c`` through rounding to odd (Boldo and Melquiond,
    "Emulation of a FMA and correctly rounded sums", IEEE Trans. Computers 57, 2008):
    ``(uh, ul) = e + c``, ``(th, tl) = p + uh``, ``v = odd(tl + ul)``, result ``th + v``.  No
    overflow or underflow in the ranges used here; ``tests/test_blockops_ref.py`` holds it against
    ``fma`` above, ties and near-ties included."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p, e = two_product(a, b)
    uh, ul = two_sum(e, c)
    th, tl = two_sum(p, uh)
    return th + _round_to_odd_sum(tl, ul)


# ------------------------------------------------------- ConstantNullspace corrections
def const_jobs_sums(vec, jobs, summer=ordered_sum):
    """One sum per job ``(off, nx, c1, c2_one, c2_alpha)`` over its range of ``vec``."""
    return np.array([summer(vec[off:off + nx]) for off, nx, *_ in jobs])


def shift_candidates(src, out, jobs, sums_a, second=0, sums_b=None):
    """The two candidate results of ``out_j = (src_j + c1_j s_a) [+ c2_j s_b]`` on the jobs' ranges
    (everything else of ``out`` as it is): the products rounded and then added, and every
    product-and-add fused into one rounding.  ``second``: 0 none, 1 ``c2_one``, 2 ``c2_alpha``."""
    rounded = np.array(out, dtype=np.float64, copy=True)
    fused = rounded.copy()
    for j, (off, nx, c1, c2_one, c2_alpha) in enumerate(jobs):
        s = np.asarray(src[off:off + nx], dtype=np.float64)
        r = s + c1 * sums_a[j]
        f = fma_np(c1, sums_a[j], s)
        if second:
            c2 = c2_alpha if second == 2 else c2_one
            r = r + c2 * sums_b[j]
            f = fma_np(c2, sums_b[j], f)
        rounded[off:off + nx] = r
        fused[off:off + nx] = f
    return rounded, fused


# ----------------------------------------------------------------------- value arrays
def vals_axpy(a, c, b):
    """``round(a + round(c b))``: two roundings; ``a`` absent counts as ``+0.0``."""
    b = np.asarray(b, dtype=np.float64)
    return (0.0 if a is None else np.asarray(a, dtype=np.float64)) + c * b


def vals_axpy_fused(a, c, b):
    """What a contracted build would give instead (one rounding): the perturbation the test of
    ``vals_axpy`` must tell apart."""
    b = np.asarray(b, dtype=np.float64)
    return fma_np(c, b, np.zeros_like(b) if a is None else a)


def csr_to_sell(csr, sell2csr):
    m = np.asarray(sell2csr)
    return np.where(m >= 0, np.asarray(csr, dtype=np.float64)[np.maximum(m, 0)], 0.0)


def mask_columns(vals, col, colmask):
    out = np.array(vals, dtype=np.float64, copy=True)
    out[np.asarray(colmask)[np.asarray(col)] != 0] = 0.0
    return out


def vals_differ(a, b, flag=0):
    return flag | int(not np.array_equal(bits(a), bits(b)))


def vals_sym_skew(a, tpos, flag=0):
    """``(h, sk, flag)``: symmetric and skew parts on a transpose map (``-1``: padding, which keeps
    ``a`` and gets ``+0.0``); the flag is set when a pair of entries that are both non-zero differs
    by more than ``1e-12`` of ``|x| + |y|``."""
    a, t = np.asarray(a, dtype=np.float64), np.asarray(tpos)
    y = a[np.maximum(t, 0)]
    pad = t < 0
    h = np.where(pad, a, 0.5 * (a + y))
    sk = np.where(pad, 0.0, 0.5 * (a - y))
    differs = ~pad & (a != 0.0) & (y != 0.0) & (np.abs(a - y) > 1e-12 * (np.abs(a) + np.abs(y)))
    return h, sk, flag | int(np.any(differs))


def apart(x, rel):
    """``y`` with ``|x - y| = rel (|x| + |y|)`` (up to rounding), the measure of the flag."""
    return x * (1.0 + 2.0 * rel / (1.0 - rel))


def transpose_map(indptr, indices):
    """Position of the transposed entry of every entry of a structurally symmetric CSR pattern."""
    where = {}
    for r in range(len(indptr) - 1):
        for p in range(indptr[r], indptr[r + 1]):
            where[(r, int(indices[p]))] = p
    out = np.empty(len(indices), dtype=np.int32)
    for (r, c), p in where.items():
        out[p] = where[(c, r)]
    return out


# --------------------------------------------------------------------------- SELL-64R
def sell_position(off0, k, rin, R):
    """Index of entry ``k`` of the row at position ``rin`` of a slice whose first slot is ``off0``:
    slice width ``C = 64 R``, ``(off0 + k) C + (rin % 64) R + rin / 64``."""
    return (off0 + k) * (LANES * R) + (rin % LANES) * R + rin // LANES


def sell_position_swapped(off0, k, rin, R):
    """The same with ``R`` and 64 exchanged -- a perturbation for the tests, wrong for ``R`` = 2."""
    return (off0 + k) * (LANES * R) + (rin % R) * LANES + rin // R


def build_sell(indptr, indices, data, R, perm=None, extra_width=None, pad_self=True,
               position=sell_position):
    """A CSR matrix laid out as the kernels read it.  ``perm``: ``None`` (row ``r`` at position
    ``r``) or an array over the ``nslices * C`` positions with the row stored there (``-1``: a
    padding row).  A slice is as wide as its longest row plus ``extra_width[s]``; the padding
    entries hold value ``+0.0`` and, as the library's patterns do, the row's own index as column
    (``pad_self=False``: ``-1``).  Returns ``dict(col, slice_off, vals, perm, nslices, R, nrows)``."""
    nrows = len(indptr) - 1
    C = LANES * R
    if perm is None:
        nslices = -(-nrows // C)
        row_of = np.where(np.arange(nslices * C) < nrows, np.arange(nslices * C), -1)
    else:
        row_of = np.asarray(perm, dtype=np.int64)
        nslices = len(row_of) // C
        assert len(row_of) == nslices * C
        assert sorted(row_of[row_of >= 0].tolist()) == list(range(nrows))
    lens = np.diff(indptr)
    off = np.zeros(nslices + 1, dtype=np.int32)
    for s in range(nslices):
        rows = row_of[s * C:(s + 1) * C]
        w = max([int(lens[r]) for r in rows if r >= 0], default=0)
        off[s + 1] = off[s] + w + (0 if extra_width is None else int(extra_width[s]))
    col = np.empty(int(off[-1]) * C, dtype=np.int32)
    vals = np.zeros(int(off[-1]) * C)
    for s in range(nslices):
        for rin in range(C):
            r = int(row_of[s * C + rin])
            pad = (r if r >= 0 else nrows - 1) if pad_self else -1
            for k in range(int(off[s + 1] - off[s])):
                p = position(int(off[s]), k, rin, R)
                if r >= 0 and k < lens[r]:
                    col[p] = indices[indptr[r] + k]
                    vals[p] = data[indptr[r] + k]
                else:
                    col[p] = pad
    return dict(col=col, slice_off=off, vals=vals, R=R, nslices=nslices, nrows=nrows,
                perm=None if perm is None else np.asarray(perm, dtype=np.int32))


def sell_to_csr(S, position=sell_position):
    """``(indptr, indices, data)`` back from the layout: per row the entries whose value is not a
    padding zero (the builder's matrices store no zeros), in slot order."""
    R, C, nrows = S["R"], LANES * S["R"], S["nrows"]
    rows = [[] for _ in range(nrows)]
    for s in range(S["nslices"]):
        for rin in range(C):
            pos = s * C + rin
            r = int(S["perm"][pos]) if S["perm"] is not None else (pos if pos < nrows else -1)
            if r < 0:
                continue
            for k in range(int(S["slice_off"][s + 1] - S["slice_off"][s])):
                p = position(int(S["slice_off"][s]), k, rin, R)
                if S["vals"][p] != 0.0:
                    rows[r].append((int(S["col"][p]), float(S["vals"][p])))
    indptr = np.cumsum([0] + [len(r) for r in rows])
    indices = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r])
    return indptr, indices, data


def extract_dinv(S, rowmask=None, init=None, position=sell_position):
    """``dinv[r] = rowmask[r] ? 1 : 1 / d`` with ``d`` the first entry of the row's slots whose
    column is ``r`` (none: 1.0); rows without a position keep ``init``."""
    R, C, nrows = S["R"], LANES * S["R"], S["nrows"]
    out = np.full(nrows, np.nan) if init is None else np.array(init, dtype=np.float64, copy=True)
    for s in range(S["nslices"]):
        for rin in range(C):
            pos = s * C + rin
            r = int(S["perm"][pos]) if S["perm"] is not None else (pos if pos < nrows else -1)
            if r < 0:
                continue
            d = 1.0
            for k in range(int(S["slice_off"][s + 1] - S["slice_off"][s])):
                p = position(int(S["slice_off"][s]), k, rin, R)
                if S["col"][p] == r:
                    d = float(S["vals"][p])
                    break
            masked = rowmask is not None and rowmask[r] != 0
            with np.errstate(divide="ignore"):
                out[r] = 1.0 if masked else float(np.float64(1.0) / np.float64(d))
    return out


def random_csr(nrows, seed, max_len=7, no_diag=(), diag_last=()):
    """A square matrix with sorted, unique columns, rows of 1 .. max_len non-zero entries of
    differing lengths and a stored diagonal -- except the rows ``no_diag``; the rows ``diag_last``
    hold only columns up to their own, so that the diagonal is the last entry of the row."""
    rng = np.random.default_rng([SEED, nrows, seed])
    indptr, indices, data = [0], [], []
    for r in range(nrows):
        want = int(rng.integers(1, max_len + 1))
        hi = r + 1 if r in diag_last else nrows
        cols = set(rng.integers(0, hi, size=want).tolist())
        cols.add(r)
        if r in no_diag:
            cols.discard(r)
            if not cols:
                cols.add((r + 1) % nrows if nrows > 1 else 0)
                if nrows == 1:
                    cols = set()
        cols = sorted(cols)
        indices += cols
        data += (rng.uniform(0.5, 2.0, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))).tolist()
        indptr.append(len(indices))
    return (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data))


# ---------------------------------------------------------------------------------- inputs
def int_data(shape, seed, amp=512):
    """Non-zero integers in ``[-amp, amp]`` as float64 (a dropped or doubled element shows).  With
    ``amp = 512`` a sum of a million of them stays below ``2^30``: exact in any order."""
    rng = np.random.default_rng([SEED, seed, amp] + list(np.atleast_1d(shape)))
    x = rng.integers(1, amp + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return x.astype(np.float64)


def real_data(shape, seed, binades=8):
    """Gaussians scaled by ``2^e``, ``e`` uniform in ``[-binades, binades]``: sums round at every
    step and neighbours differ in size."""
    rng = np.random.default_rng([SEED, seed, binades] + list(np.atleast_1d(shape)))
    return rng.standard_normal(shape) * np.exp2(rng.uniform(-binades, binades, size=shape))
