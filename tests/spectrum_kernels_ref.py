"""Host references for the kernels of the batched spectrum estimates and the twin search
(``spec_dot_stage1`` / ``spec_dot_stage2``, ``spec_update_kernel``, ``spec_sym_skew_kernel``,
``spec_fingerprint_kernel``, ``spec_pairs_differ_kernel``), for
``tests/test_gpu_spectrum_kernels.py``.  Nothing here calls the library or reads its sources; the
constants restate the launch shapes.

* The dots are ``krylov_ref``'s (``tree_dots``, ``dot_depth``, ``gamma``), the split and the
  comparison ``blockops_ref``'s (``vals_sym_skew``, ``vals_differ``): the batched kernels claim the
  one-matrix kernels' arithmetic, so they are held against the one-matrix references.
* ``stage2``: the scalars of a step on ``numpy.float64`` -- each one IEEE quotient, square root,
  product or comparison -- with the step-major store ``alpha[s B + b]`` and its ``s < max_steps``
  guard.
* ``update``: the three fused multiply-adds the kernel's header states and the copy; ``fma_array``
  has one rounding per element (``Fraction``; Dekker / Boldo-Melquiond where the operands are in
  the safe range, which ``tests/test_spectrum_kernels_ref.py`` holds against ``Fraction``).
* ``fingerprint``: ``spec_mix``, the per-thread strided fold, the LDS tree and the host's fold in
  64-bit wrap-around arithmetic, over all threads at once; ``fingerprint_scalar`` is the same in
  plain Python integers, one thread at a time.

IEEE 754 leaves the sign and payload of a NaN an operation generates open, so ``same`` -- the
comparison of everything that may hold a generated NaN -- takes any two NaNs for equal; all other
values compare by their bits.
"""
import math
from fractions import Fraction

import numpy as np

import blockops_ref
import krylov_ref

THREADS = 256                       # threads per workgroup, every kernel
REDUCE_BLOCKS = krylov_ref.REDUCE_BLOCKS
UPDATE_BLOCKS = 256                 # most workgroups per matrix: update, pair comparison
SPLIT_BLOCKS = 512                  # ... of the symmetric / skew split
UPDATE_TRIP = UPDATE_BLOCKS * THREADS      # elements one grid-stride trip covers
SPLIT_TRIP = SPLIT_BLOCKS * THREADS
FP_SHARE = 2048                     # elements per fingerprint workgroup before the cap
FP_BLOCKS = 64                      # most fingerprint words per array
POWER_MIN_STEPS = 8                 # the 0.5 % rule of the power iteration from this step on
MASK = (1 << 64) - 1

START, PAP, RZ, NORM0, NORM = range(5)
UPD_R, UPD_P, UPD_SCALE, UPD_COPY = range(4)


def batch_stride(n):
    """Spacing of a batch's vectors: n + 32 rounded up to even."""
    return (n + 32 + 1) & ~1


def same(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (a, b))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)
                and np.array_equal(blockops_ref.bits(a)[~na], blockops_ref.bits(b)[~nb]))


# ------------------------------------------------------------------------------ stage 2
def new_state(B, max_steps, fill=-7.25):
    """A scalar state with recognisable contents: every field of every matrix differs."""
    k = np.arange(B, dtype=np.float64)
    return dict(active=np.ones(B, dtype=np.uint32), na=np.zeros(B, dtype=np.int32),
                nb=np.zeros(B, dtype=np.int32), rz=3.0 + k, coef=fill - k, last=0.5 + k,
                mu2=fill * 2 - k, alpha=fill * 3 - np.arange(max_steps * B, dtype=np.float64),
                beta=fill * 5 - np.arange(max_steps * B, dtype=np.float64))


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def stage2(state, dots, mode, k, max_steps):
    """What the second stage makes of the sums ``dots`` (one per matrix): a new state.  A matrix
    whose ``active`` word is 0 keeps everything."""
    s = copy_state(state)
    B = len(s["active"])
    f = np.float64
    with np.errstate(all="ignore"):
        for b in range(B):
            if not s["active"][b]:
                continue
            dot = f(dots[b])
            if mode == START:
                if not (dot > 0.0 and np.isfinite(dot)):
                    s["active"][b] = 0
                s["rz"][b] = dot
            elif mode == PAP:
                if not (dot > 0.0) or not np.isfinite(dot):
                    s["active"][b] = 0
                    continue
                al = f(s["rz"][b]) / dot
                n = int(s["na"][b])
                if n < max_steps:
                    s["alpha"][n * B + b] = al
                s["na"][b] = n + 1
                s["coef"][b] = al
            elif mode == RZ:
                if not (dot > f(1e-28) * f(s["rz"][b])) or not np.isfinite(dot):
                    s["active"][b] = 0
                    continue
                be = dot / f(s["rz"][b])
                n = int(s["nb"][b])
                if n < max_steps:
                    s["beta"][n * B + b] = be
                s["nb"][b] = n + 1
                s["coef"][b] = be
                s["rz"][b] = dot
            elif mode == NORM0:
                nv = np.sqrt(dot)
                if nv > 0.0 and np.isfinite(nv):
                    s["coef"][b] = f(1.0) / nv
                else:
                    s["active"][b] = 0
            elif mode == NORM:
                nv = np.sqrt(dot)
                s["mu2"][b] = nv
                s["na"][b] = k + 1
                if power_settled(k, nv, f(s["last"][b])) or not (nv > 0.0 and np.isfinite(nv)):
                    s["active"][b] = 0
                    continue
                s["last"][b] = nv
                s["coef"][b] = f(1.0) / nv
            else:
                raise ValueError(mode)
    return s


def power_settled(k, mu2, last):
    with np.errstate(all="ignore"):
        diff = np.float64(mu2) - np.float64(last)
        return bool(k >= POWER_MIN_STEPS and abs(diff) <= np.float64(0.005) * np.float64(mu2))


# ------------------------------------------------------------------------------ updates
def fma_scalar(a, b, c):
    """``a b + c`` rounded once, with IEEE's rules for zeros, infinities and NaNs."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))     # the product is exact
    if not math.isfinite(c):
        return c                                 # a finite product, however large, changes nothing
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        if a == 0.0 or b == 0.0:                 # a zero product and c = +-0: the sum of two zeros
            neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
            return -0.0 if neg and math.copysign(1.0, c) < 0 else 0.0
        return 0.0                               # exact cancellation: +0 in round-to-nearest
    try:
        r = float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf
    return math.copysign(0.0, exact) if r == 0.0 else r


def fma_array(a, b, c):
    """``fma_scalar`` over arrays.  Where ``a`` is 0 or +-1 the product is exact and the result is
    the IEEE sum ``a b + c``; where all three operands are finite, non-zero and between ``2^-300``
    and ``2^300`` in size, ``blockops_ref.fma_np``; every other element through ``Fraction``."""
    a, b, c = (np.array(v, dtype=np.float64) for v in np.broadcast_arrays(
        *(np.asarray(v, dtype=np.float64) for v in (a, b, c))))
    out = np.empty_like(c)
    with np.errstate(all="ignore"):
        plain = (a == 0.0) | (np.abs(a) == 1.0)
        out[plain] = a[plain] * b[plain] + c[plain]
        lo, hi = 2.0 ** -300, 2.0 ** 300
        safe = ~plain
        for v in (a, b, c):
            safe &= np.isfinite(v) & (np.abs(v) >= lo) & (np.abs(v) <= hi)
        out[safe] = blockops_ref.fma_np(a[safe], b[safe], c[safe])
    for i in np.flatnonzero(~(plain | safe).ravel()):
        idx = np.unravel_index(i, out.shape)
        out[idx] = fma_scalar(a[idx], b[idx], c[idx])
    return out


def update(kind, v, x, coef, active, n):
    """``v``, ``x``: (B, stride).  R ``v = fma(-c, x, v)``; P ``v = fma(1, x, fl(c v))``; SCALE
    ``v = fma(0, x, fl(c v))``; COPY ``v = x`` -- on the first ``n`` elements of every active
    matrix; everything else keeps its bits."""
    out = np.array(v, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        for b in range(len(out)):
            if not active[b]:
                continue
            c, vb, xb = np.float64(coef[b]), out[b, :n].copy(), np.asarray(x[b, :n], dtype=np.float64)
            if kind == UPD_R:
                out[b, :n] = fma_array(-c, xb, vb)
            elif kind == UPD_P:
                out[b, :n] = fma_array(1.0, xb, c * vb)
            elif kind == UPD_SCALE:
                out[b, :n] = fma_array(0.0, xb, c * vb)
            elif kind == UPD_COPY:
                out[b, :n] = xb
            else:
                raise ValueError(kind)
    return out


def axpby_coefficients(kind, c):
    """``(a, b)`` of the one-matrix loop's ``y = a x + b y`` for the update (COPY: ``None``)."""
    return {UPD_R: (-c, 1.0), UPD_P: (1.0, c), UPD_SCALE: (0.0, c), UPD_COPY: None}[kind]


# -------------------------------------------------------------------------- fingerprint
def fingerprint_blocks(n):
    return max(1, min(FP_BLOCKS, -(-n // FP_SHARE)))


def _mix(h, v):
    h = h ^ (v + np.uint64(0x9e3779b97f4a7c15) + (h << np.uint64(6)) + (h >> np.uint64(2)))
    return h * np.uint64(0xff51afd7ed558ccd)


def fingerprint(a):
    """``(words, fold)`` of one array: workgroup ``g`` of ``fingerprint_blocks(n)`` folds the
    elements ``g 256 + t + j (blocks 256)`` per thread ``t`` in ascending ``j``, then a tree over
    its threads with strides 128 ... 1; the host folds the words."""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    n, nb = len(u), fingerprint_blocks(len(u))
    step = nb * THREADS
    with np.errstate(over="ignore"):
        h = np.full(step, 0x2545f4914f6cdd1d, dtype=np.uint64)
        for j in range(-(-n // step)):
            m = min(step, n - j * step)
            h[:m] = _mix(h[:m], u[j * step:j * step + m])
        sh = h.reshape(nb, THREADS)
        st = THREADS // 2
        while st:
            sh = _mix(sh[:, :st], sh[:, st:2 * st])
            st >>= 1
    words = sh[:, 0].copy()
    return words, fold(words)


def fold(words):
    h = 0x9e3779b97f4a7c15
    for w in words:
        h = (((h ^ int(w)) * 0xff51afd7ed558ccd) + (h >> 29)) & MASK
    return h


def _mix_int(h, v):
    h ^= (v + 0x9e3779b97f4a7c15 + (h << 6) + (h >> 2)) & MASK
    return (h * 0xff51afd7ed558ccd) & MASK


def fingerprint_scalar(a):
    """The same in Python integers, thread by thread."""
    u = [int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)]
    n, nb = len(u), fingerprint_blocks(len(u))
    words = []
    for g in range(nb):
        sh = []
        for t in range(THREADS):
            h = 0x2545f4914f6cdd1d
            for p in range(g * THREADS + t, n, nb * THREADS):
                h = _mix_int(h, u[p])
            sh.append(h)
        st = THREADS // 2
        while st:
            for t in range(st):
                sh[t] = _mix_int(sh[t], sh[t + st])
            st >>= 1
        words.append(sh[0])
    return np.array(words, dtype=np.uint64), fold(words)


def last_share_position(n):
    """The last position the last workgroup of the fingerprint reads."""
    nb = fingerprint_blocks(n)
    first = (nb - 1) * THREADS
    if first >= n:
        return n - 1
    step = nb * THREADS
    best = 0
    for t in range(THREADS):
        p = first + t
        if p < n:
            best = max(best, p + ((n - 1 - p) // step) * step)
    return best


# ------------------------------------------------------------------- one-bit differences
BIT_KINDS = ("mantissa", "zero sign", "nan payload")


def flip(a, pos, kind):
    """A copy of ``a`` and its one-bit neighbour at ``pos``: ``(base, flipped)``.  ``mantissa``:
    the lowest mantissa bit of the value there; ``zero sign``: ``+0.0`` against ``-0.0``;
    ``nan payload``: two NaNs one payload bit apart."""
    base = np.array(a, dtype=np.float64, copy=True)
    if kind == "zero sign":
        base[pos] = 0.0
    elif kind == "nan payload":
        base.view(np.uint64)[pos] = np.uint64(0x7ff8000000000100)
    elif kind != "mantissa":
        raise ValueError(kind)
    other = base.copy()
    bit = np.uint64(1 << 63) if kind == "zero sign" else np.uint64(1)
    other.view(np.uint64)[pos] ^= bit
    return base, other


def fingerprint_positions(n):
    """Where the fingerprint tests flip a bit: first, last, 255 and 256, the end of the last
    workgroup's share."""
    return sorted({0, n - 1, 255, 256, last_share_position(n)} & set(range(n)))


def pair_positions(n):
    """Where the pair comparison tests flip a bit: first, last, the last element of the first
    grid-stride trip and the first of the second, the middle."""
    return sorted({0, n - 1, UPDATE_TRIP - 1, UPDATE_TRIP, n // 2} & set(range(n)))


# ---------------------------------------------------------------------------------- inputs
# the sizes of the fingerprint cases: one word (a thread's share of one element at most, +-1 around
# the workgroup), two words, 64 words and a second trip, 37 trips with a ragged last one
FP_N = (1, THREADS - 1, THREADS, THREADS + 1, FP_SHARE, FP_SHARE + 1, FP_BLOCKS * FP_SHARE + 1, 600001)
FP_NMAT = (1, 4)


def fingerprint_arrays(n, nmat):
    """The candidates of the fingerprint case (n, nmat): (nmat, n), read only."""
    a = blockops_ref.real_data((nmat, n), 41)
    a.setflags(write=False)
    return a


def special_values(x, seed):
    """``x`` with signed zeros, subnormals and the smallest normal number sprinkled in (and always at
    the first and last place)."""
    x = np.array(x, dtype=np.float64, copy=True)
    flat = x.reshape(-1)
    rng = np.random.default_rng([blockops_ref.SEED, seed, flat.size])
    vals = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -3e-320, 2.2250738585072014e-308])
    where = rng.permutation(flat.size)[:max(2, flat.size // 50)]
    flat[where] = vals[rng.integers(0, len(vals), size=len(where))]
    flat[0] = -0.0
    flat[-1] = 5e-324
    return x
