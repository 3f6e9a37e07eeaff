"""Host references for the vector kernels of the Krylov loops (``mdot_stage1`` / ``mdot_stage2``,
``maxpy_kernel``, ``maxpy_norm_kernel``, ``norm2_finish``, ``scale_inv``, ``axpby``, ``copy``,
``fill``), for ``tests/test_gpu_krylov_kernels.py``.  Nothing here reads the project's sources: the
three constants below restate ``kernels.hpp`` and the launch shape of the reduction.

* ``exact_dots``: the correctly rounded exact inner products (error-free products, ``math.fsum``).
* ``fma`` / ``maxpy_exact``: the documented elementwise chain of the multi-axpy, every fused
  multiply-add exact through ``fractions.Fraction`` -- compared bit for bit.
* ``dot_depth`` / ``gamma``: the number of roundings on the longest path of the device reduction,
  counted from the constants, and the classical bound ``gamma(k) = k u / (1 - k u)`` it gives.
* ``tree_dots``: a plain NumPy walk through the same reduction tree (float64 adds in the device's
  order), which ``tests/test_krylov_ref.py`` holds against the bound before a GPU sees it.
* ``int_data`` / ``real_data``: the inputs.
"""
import functools
import math
from fractions import Fraction

import numpy as np

REDUCE_BLOCKS = 1024      # workgroups of stage 1 = partial sums per inner product
MDOT_MAX = 8              # vectors per fused pass
THREADS = 256             # threads per workgroup, each reading double2 pairs at stride 512
U = 2.0 ** -53            # unit roundoff of float64
SEED = 20240611


def chunk(n):
    """Elements per stage-1 workgroup: ``ceil(n / REDUCE_BLOCKS)`` rounded up to even."""
    return ((n + REDUCE_BLOCKS - 1) // REDUCE_BLOCKS + 1) & ~1


def stride(n):
    """Spacing of the vectors in the solver's allocation, in doubles."""
    return (n + 31) & ~31


def dot_depth(n):
    """Roundings between one product ``w_p v_p`` and the result, on the longest path: the
    thread's chain of fused multiply-adds (two per trip of the strided loop, ``ceil(chunk / 512)``
    trips), six steps of the wavefront shuffle tree, three adds of the four wave results, the
    chain of ``REDUCE_BLOCKS / 256`` adds of stage 2 and its eight-step tree."""
    trips = -(-chunk(n) // (2 * THREADS))
    return 2 * trips + 6 + 3 + REDUCE_BLOCKS // THREADS + 8


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------ exact arithmetic
def two_product(a, b):
    """``(p, e)`` with ``p = fl(a b)`` and ``p + e = a b`` exactly (Dekker's product on
    Veltkamp's split; no overflow or underflow in the ranges used here)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def two_sum(a, b):
    """``(s, t)`` with ``s = fl(a + b)`` and ``s + t = a + b`` exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def exact_dots(w, V):
    """The inner products ``<w, V_i>``, each the exact value rounded once."""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty(len(V))
    for i, v in enumerate(V):
        p, e = two_product(w, v)
        out[i] = math.fsum(np.concatenate([p, e]))
    return out


def abs_dots(w, V):
    """``sum_p |w_p V_ip|``, the scale of the rounding-error bound of an inner product."""
    return exact_dots(np.abs(w), np.abs(np.asarray(V)))


def fma(a, b, c):
    """``a b + c`` rounded once (``float`` of a ``Fraction`` rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def maxpy_exact(w, V, coef, sign, group=MDOT_MAX):
    """The multi-axpy as the kernels document it: groups of ``group`` vectors in ascending order;
    per group and element ``a = fma(c_i, v_i, a)`` for ascending ``i`` from ``a = 0``, then
    ``w = fma(sign, a, w)``."""
    w = np.asarray(w, dtype=np.float64)
    nv, s = len(V), Fraction(float(sign))
    cf = [Fraction(float(c)) for c in coef]
    out = np.empty_like(w)
    for p in range(len(w)):
        x = float(w[p])
        for g in range(0, nv, group):
            a = 0.0
            for i in range(g, min(g + group, nv)):
                a = float(cf[i] * Fraction(float(V[i][p])) + Fraction(a))
            x = float(s * Fraction(a) + Fraction(x))
        out[p] = x
    return out


# ------------------------------------------------------------- the device's reduction tree
def _fma_np(a, b, c):
    """``a b + c`` from the error-free product and sum: ``fl(s + fl(t + e))`` with
    ``p + e = a b`` and ``s + t = p + c``.  Within ``u (1 + 2 u)`` of the exact value relative to
    the result -- one rounding for the purpose of the bound, and the correctly rounded result
    whenever ``a b + c`` is a float64."""
    p, e = two_product(a, b)
    s, t = two_sum(p, c)
    return s + (t + e)


def tree_dots(w, V):
    """The inner products summed in the order of the two-stage device reduction."""
    w = np.asarray(w, dtype=np.float64)
    n, c = len(w), chunk(len(w))
    trips = -(-c // (2 * THREADS))
    # element (block b, trip k, thread t, half j) is p = b c + 512 k + 2 t + j, present while it
    # lies in the block's chunk and below n; an absent element adds an exact zero
    b = np.arange(REDUCE_BLOCKS)[:, None, None, None]
    k = np.arange(trips)[None, :, None, None]
    t = np.arange(THREADS)[None, None, :, None]
    j = np.arange(2)[None, None, None, :]
    inside = 2 * THREADS * k + 2 * t + j
    p = b * c + inside
    ok = (inside < c) & (p < n)
    idx = np.where(ok, p, 0)
    wq = np.where(ok, w[idx], 0.0)
    out = np.empty(len(V))
    for i, v in enumerate(V):
        vq = np.where(ok, np.asarray(v, dtype=np.float64)[idx], 0.0)
        acc = np.zeros((REDUCE_BLOCKS, THREADS))
        for kk in range(trips):
            acc = _fma_np(wq[:, kk, :, 0], vq[:, kk, :, 0], acc)
            acc = _fma_np(wq[:, kk, :, 1], vq[:, kk, :, 1], acc)
        x = acc.reshape(REDUCE_BLOCKS, THREADS // 64, 64)
        off = 32
        while off:                        # lane 0 of the shuffle tree
            x = x[..., :off] + x[..., off:2 * off]
            off >>= 1
        x = x[..., 0]
        part = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
        a = np.zeros(THREADS)
        for q in range(REDUCE_BLOCKS // THREADS):
            a = a + part[q * THREADS:(q + 1) * THREADS]
        st = THREADS // 2
        while st:
            a = a[:st] + a[st:2 * st]
            st >>= 1
        out[i] = a[0]
    return out


# ---------------------------------------------------------------------------------- inputs
def int_data(n, nv, seed, amp=512):
    """``(w, V)`` of non-zero integers in ``[-amp, amp]`` (a dropped or doubled element always
    shows).  With ``amp = 512`` every product is below ``2^18`` and every sum of up to two million
    of them below ``2^39``: exact in float64 in any order."""
    rng = np.random.default_rng([SEED, n, nv, seed, amp])
    x = rng.integers(1, amp + 1, size=(nv + 1, n)) * rng.choice([-1, 1], size=(nv + 1, n))
    x = x.astype(np.float64)
    return x[0].copy(), x[1:].copy()


@functools.lru_cache(maxsize=None)
def orth_amp(n, nv, seed):
    """The largest power of two ``amp <= 512`` for which the Gram-Schmidt step on
    ``int_data(n, nv, seed, amp)`` is exact in float64 whatever the order of its sums: every
    partial sum of the update is bounded by ``max_p sum_i |h_i v_ip| + |w_p| < 2^53``, and every
    partial sum of the squared norm by ``n max_p w_out_p^2 < 2^53``."""
    # (the search starts two binades above amp^6 nv n^2 = 2^53, the size of n w_out^2 for
    # independent entries)
    amp = min(512, 4 * 2 ** int(math.log2(2.0 ** 53 / (nv * n * n)) / 6))
    while amp >= 1:
        w, V = int_data(n, nv, seed, amp)
        h, w_out, _ = int_orthogonalise(w, V)
        spread = float(np.max(np.abs(h)[:, None] * np.abs(V))) * nv + amp
        if spread < 2.0 ** 53 and n * float(np.max(np.abs(w_out))) ** 2 < 2.0 ** 53:
            return amp
        amp //= 2
    raise AssertionError("no integer range keeps the Gram-Schmidt step exact")


def int_orthogonalise(w, V):
    """``(h, w_out, ||w_out||^2)`` in ``int64`` (the caller keeps the values inside its range)."""
    wi, Vi = w.astype(np.int64), V.astype(np.int64)
    h = Vi @ wi
    w_out = wi - h @ Vi
    wf = w_out.astype(np.float64)
    sq = int(w_out @ w_out) if len(wf) * float(np.max(np.abs(wf))) ** 2 < 2.0 ** 62 else None
    return h, w_out, sq


def real_data(n, nv, seed, orthonormal=True):
    """``(w, V)`` with entries over forty binades: the rows of a Gaussian matrix scaled by
    ``2^e_p``, ``e_p`` uniform in ``[-20, 20]``, then orthonormalised by columns (a Gram-Schmidt
    step needs an orthonormal basis to leave a small ``w``; ``n < nv``: left as it is).  ``w`` is
    ``8 V_0`` plus a perturbation of ``2^-24`` of its size and a little of the other vectors:
    nearly parallel to ``V_0`` and inside the span but for the perturbation, so the step cancels
    seven digits and ``tt`` is far below ``||w||``.  ``orthonormal=False`` leaves the scaled Gaussian
    columns as they are (cheap at any size, for checks that compare bits and not sizes)."""
    rng = np.random.default_rng([SEED, n, nv, seed])
    scale = np.exp2(rng.uniform(-20.0, 20.0, size=n))
    k = max(nv, 1)
    A = rng.standard_normal((n, k)) * scale[:, None]
    if n >= k and orthonormal:
        A = np.linalg.qr(A)[0]
    V = np.ascontiguousarray(A.T[:nv])
    r = rng.standard_normal(n) * scale
    w = A[:, 0] + 2.0 ** -24 * r / np.linalg.norm(r)
    for i in range(1, nv):
        w = w + 0.25 ** i * V[i]
    return np.ascontiguousarray(w * 8.0), V
