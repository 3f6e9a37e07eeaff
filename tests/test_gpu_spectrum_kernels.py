"""The kernels of the batched spectrum estimates and of the twin search against exact references,
one launch at a time through ``kkt_debug_spectrum_op``: ``spec_dot_stage1`` / ``spec_dot_stage2``
(``launch_spec_dot``, every mode), ``spec_update_kernel`` (R, P, SCALE, COPY),
``spec_sym_skew_kernel``, ``spec_fingerprint_kernel`` and ``spec_pairs_differ_kernel``.  The hook
calls the launchers the preconditioner build calls, so the grids are production's.  References:
``tests/spectrum_kernels_ref.py`` (checked on the host by ``tests/test_spectrum_kernels_ref.py``),
``krylov_ref`` for the dots, ``blockops_ref`` for the split and the comparison.

Sizes -- each the smallest that reaches its regime, from the launch constants (256 threads per
workgroup everywhere):

    dots          the sizes of ``test_gpu_krylov_kernels.py``: 1, 2, 3 (one workgroup with work,
                  with and without the scalar tail), 2047, 2048, 2049 (chunk 2 -> 4), 2421, 65537,
                  524289 (chunk 514: the second trip of the strided loop)
    updates,      at most 256 x 256 threads: 1, 255, 256, 257; 65535, 65536 (one trip exactly),
    pairs         65537 (the second trip's first element), 131073 (the third's); pairs also 200001
    split         at most 512 x 256 threads: 1, 2, 255, 257; 131071, 131072, 131073, 262145
    fingerprint   min(64, ceil(n / 2048)) workgroups: 1, 255, 256, 257, 2048 (one word), 2049 (two),
                  131073 (64 words, a second trip), 600001 (37 trips, a ragged last one)

What is asserted, bit for bit unless a bound is named (a NaN an operation generates equals any
NaN: IEEE leaves its sign and payload open): the guard elements around every written array, every
array a launch only reads (``inputs_changed == 0``) and the padding between the vectors of a batch
are as they were; every launch gives identical bits when repeated.

* Dots.  Integer data: the partial sums of every workgroup and the dot equal ``int64`` arithmetic.
  Real data: the dot equals ``krylov_ref.tree_dots``, equals the multi-dot of
  ``kkt_debug_krylov_op`` with one vector on the same data (the header's "operation for
  operation"), and lies within ``gamma(dot_depth(n) + 1) sum |x y|`` of the exact dot.  The state
  after the launch equals ``stage2`` of the reference in every field; an inactive matrix keeps
  the caller's fill in every scalar and partial sum.
* Stage 2 at n = 3, thirteen matrices in one launch whose dots are exactly: a positive number, +0,
  a negative number, +inf (an overflowing product), NaN (0 inf, and inf - inf), ``1e-28 rz`` and
  its upper neighbour, values that settle the power iteration and that do not (4 against
  ``last`` = 2; 4.2; ``(1 + m 2^-20)^2`` for m = 5269, 5270, the neighbours between which the 0.5 %
  rule flips), and an inactive one: START, PAP, RZ, NORM0, NORM at k = 7 and 8, with ``na`` /
  ``nb`` at 0, ``max_steps - 1`` and ``max_steps`` -- the last entry is stored, then nothing is and
  the count still advances.
* Updates: all kinds against the fused multiply-adds the header states, on data with signed zeros
  and subnormals, ``coef`` = 0 and -0, a NaN and an inf in the second vector (SCALE gives NaN), one
  inactive matrix; and against ``axpby`` / ``copy`` of ``kkt_debug_krylov_op`` with the one-matrix
  loop's coefficients.
* Split: ``h``, ``sk`` and the flag per matrix against ``blockops_ref.vals_sym_skew`` and against
  ``VALS_SYM_SKEW`` of ``kkt_debug_block_op``; flags per matrix (asymmetry of 2e-12 at the last
  pair of one matrix, 0.5e-12 and a zero on one side in its neighbours); a set flag stays.
* Fingerprint: words and fold against the reference; equal bits give equal words; one flipped bit
  (lowest mantissa bit, the sign of a zero, a NaN payload bit) at the first, the last, positions
  255 and 256 and the end of the last workgroup's share changes the fold.
* Pair comparison: 1, 3 and 5 pairs over four arrays, one paired with itself; one flipped bit at
  0, n - 1, 65535, 65536 or n / 2 raises exactly the pairs with that array on one side; every flag
  equals ``VALS_DIFFER`` of ``kkt_debug_block_op``; a set flag stays.
* Every ``KKT_ERR_ARG`` path of the hook.

Measured on an MI355X (gfx950): every case passes as the kernels stand; largest error / bound of a
real-data dot 0.079 (``n`` = 2049, B = 5; depth 23), 0.075 at ``n`` = 2, 0.067 at 524289 (depth 25),
and several dots are the correctly rounded value itself (ratio 0).  Seeded in scratch copies of the
library, the pair comparison without its second trip fails ``test_pair_comparison`` from 65537
on, the update ignoring ``active`` every ``test_updates[...-B3]``, the store guard removed
``test_stage2_branches[pap-*]`` and ``[rz-*]``.  95 cases in 5 s.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import blockops_ref as bref
import krylov_ref as kref
import spectrum_kernels_ref as ref
import test_gpu_block_kernels as blk
import test_gpu_krylov_kernels as kry
from control_amd import _lib

pytestmark = pytest.mark.gpu

G = _lib.BLOCK_GUARD
FILL = -1.2345e300          # what a written array, and the padding of a vector, holds before a launch
PAD64 = np.array([_lib.KRYLOV_PAD]).view(np.uint64)[0]
PADS = {np.dtype(np.float64): _lib.KRYLOV_PAD, np.dtype(np.uint32): _lib.BLOCK_FLAG_PAD,
        np.dtype(np.int32): np.array([_lib.BLOCK_FLAG_PAD], dtype=np.uint32).view(np.int32)[0],
        np.dtype(np.uint64): PAD64}
# the record's arrays: guarded ones (read and written by some operation) and plain inputs
GUARDED = {"v": np.float64, "active": np.uint32, "na": np.int32, "nb": np.int32, "rz": np.float64,
           "coef": np.float64, "last": np.float64, "mu2": np.float64, "alpha": np.float64,
           "beta": np.float64, "part": np.float64, "h": np.float64, "sk": np.float64,
           "flag": np.uint32, "words": np.uint64}
PLAIN = {"x": np.float64, "y": np.float64, "a": np.float64, "tpos": np.int32, "pair_a": np.int32,
         "pair_b": np.int32, "fold": np.uint64}
SCALARS = ("mode", "k", "nmat", "max_steps", "npairs", "n", "stride")
_FIELD_TYPES = dict(_lib.SpectrumOp._fields_)
STATE = ("active", "na", "nb", "rz", "coef", "last", "mu2", "alpha", "beta")

DOT_N = (1, 2, 3, 2047, 2048, 2049, 2421, 65537, 524289)
UPDATE_N = (1, ref.THREADS - 1, ref.THREADS, ref.THREADS + 1, ref.UPDATE_TRIP - 1, ref.UPDATE_TRIP,
            ref.UPDATE_TRIP + 1, 2 * ref.UPDATE_TRIP + 1)
SPLIT_N = (1, 2, ref.THREADS - 1, ref.THREADS + 1, ref.SPLIT_TRIP - 1, ref.SPLIT_TRIP,
           ref.SPLIT_TRIP + 1, 2 * ref.SPLIT_TRIP + 1)
PAIRS_N = UPDATE_N + (200001,)         # ... and a fourth, ragged trip
assert UPDATE_N == (1, 255, 256, 257, 65535, 65536, 65537, 131073)
assert SPLIT_N == (1, 2, 255, 257, 131071, 131072, 131073, 262145)
assert PAIRS_N == (1, 255, 256, 257, 65535, 65536, 65537, 131073, 200001)
# the dot sizes by what they reach: chunks of 2, 4 and 514 elements, the scalar tail, the second trip
assert [kref.chunk(n) for n in DOT_N] == [2, 2, 2, 2, 2, 4, 4, 66, 514] and 514 > 2 * ref.THREADS


@pytest.fixture(scope="module")
def handle():
    """A created handle and nothing else: the entry does not depend on a layout."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0, lib.kkt_last_error(None)
    yield lib, h
    assert lib.kkt_destroy(h) == 0


# ------------------------------------------------------------------------------ the call
def _record(op, fields):
    """``(SpectrumOp, {name: guarded allocation}, [arrays kept alive])``."""
    a = _lib.SpectrumOp()
    a.op = _lib.SPECTRUM_OPS[op] if isinstance(op, str) else op
    guarded, keep = {}, []
    for k, v in fields.items():
        if v is None:
            continue
        if k == "y" and v is fields.get("x"):
            continue                                  # one family on both sides: set below
        if k in SCALARS:
            setattr(a, k, v)
        elif k in GUARDED:
            init = np.asarray(v, dtype=GUARDED[k]).ravel()
            g = np.zeros(len(init) + 2 * G, dtype=GUARDED[k])
            g[G:G + len(init)] = init
            guarded[k] = g
            setattr(a, k, g.ctypes.data_as(_FIELD_TYPES[k]))
        else:
            v = np.ascontiguousarray(v, dtype=PLAIN[k])
            keep.append(v)
            setattr(a, k, v.ctypes.data_as(_FIELD_TYPES[k]))
            if k == "fold":
                guarded[k] = v
    if fields.get("y") is not None and fields["y"] is fields.get("x"):
        a.y = a.x
    return a, guarded, keep


def call(handle, op, **fields):
    """One launch: the guarded arrays without their guards (and ``fold``, ``batch_stride``), the
    guards and the hook's comparison of its inputs checked here."""
    lib, h = handle
    a, guarded, keep = _record(op, fields)
    a.inputs_changed = -1
    rc = lib.kkt_debug_spectrum_op(h, C.byref(a))
    if rc == -2:      # KKT_ERR_HIP: nothing more is started on a device that reported an error
        pytest.exit(f"HIP error in {op}: {lib.kkt_last_error(h)}", returncode=3)
    assert rc == 0, (op, rc, lib.kkt_last_error(h))
    assert a.inputs_changed == 0, (op, "an input array was written")
    out = {"batch_stride": a.batch_stride}
    for k, g in guarded.items():
        if k == "fold":
            out[k] = g.copy()
            continue
        pad = PADS[g.dtype]
        assert np.all(g[:G] == pad) and np.all(g[-G:] == pad), (op, k, "guard elements were written")
        out[k] = g[G:-G].copy()
    return out


def same_out(u, v):
    """Two results of ``call``: identical bits."""
    assert u.keys() == v.keys()
    for k in u:
        if isinstance(u[k], np.ndarray):
            assert u[k].dtype == v[k].dtype and u[k].tobytes() == v[k].tobytes(), (k, "not reproducible")
        else:
            assert u[k] == v[k], k
    return True


def run(handle, op, **fields):
    """``call`` twice: identical bits."""
    first = call(handle, op, **fields)
    assert same_out(first, call(handle, op, **fields)), op
    return first


def state_matches(got, want, B):
    """Every field of the scalar state equals the reference's (NaNs as NaNs)."""
    for k in STATE:
        if want[k].dtype == np.float64:
            assert ref.same(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
        else:
            assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())


def batch_vectors(vecs, n, stride):
    """(B, stride): the vectors with ``FILL`` in the padding."""
    out = np.full((len(vecs), stride), FILL)
    for b, v in enumerate(vecs):
        out[b, :n] = v
    return out


def actives(B):
    return np.array({1: [1], 3: [1, 0, 7], 5: [1, 1, 0, 0x80000000, 0]}[B], dtype=np.uint32)


# --------------------------------------------------------------------- dots, stage 1 + 2
def call_dot(handle, x, y, n, stride, mode, state, k=0, max_steps=3):
    """The launch with two families; ``y is x``: one family on both sides (the hook gets one
    pointer twice, as the power iteration's norm does)."""
    B = len(x)
    got = run(handle, "dot", mode=mode, k=k, nmat=B, max_steps=max_steps, n=n, stride=stride, x=x, y=y,
              part=np.full(B * ref.REDUCE_BLOCKS, FILL), **state)
    assert got["batch_stride"] == ref.batch_stride(n)
    return got


def int_parts(x, y, n):
    """The partial sum of every stage-1 workgroup in ``int64``."""
    c = kref.chunk(n)
    prod = np.zeros(ref.REDUCE_BLOCKS * c, dtype=np.int64)
    prod[:n] = x[:n].astype(np.int64) * y[:n].astype(np.int64)
    return prod.reshape(ref.REDUCE_BLOCKS, c).sum(axis=1)


@pytest.mark.parametrize("B", (1, 3, 5), ids=lambda v: f"B{v}")
@pytest.mark.parametrize("n", DOT_N, ids=lambda v: f"n{v}")
def test_dots(handle, n, B):
    stride = ref.batch_stride(n) + (6 if B == 3 else 0)      # the caller's: production's, or wider
    act = actives(B)
    live = [b for b in range(B) if act[b]]
    state = ref.new_state(B, 3)
    state["active"] = act

    # integer data: partial sums and dot in int64
    xs, ys = zip(*((w, V[0]) for w, V in (kref.int_data(n, 1, 10 + b) for b in range(B))))
    x, y = batch_vectors(xs, n, stride), batch_vectors(ys, n, stride)
    got = call_dot(handle, x, y, n, stride, ref.START, state)
    parts = got["part"].reshape(B, ref.REDUCE_BLOCKS)
    dots = np.zeros(B)
    for b in range(B):
        if act[b]:
            want = int_parts(xs[b], ys[b], n)
            assert np.array_equal(parts[b], want), (b, "partial sums")
            dots[b] = float(want.sum())
        else:
            assert bref.same_bits(parts[b], np.full(ref.REDUCE_BLOCKS, FILL)), (b, "inactive")
    state_matches(got, ref.stage2(state, dots, ref.START, 0, 3), B)

    # real data: the tree, the one-matrix kernels, the bound
    xs, ys = zip(*((w, V[0]) for w, V in (kref.real_data(n, 1, 20 + b, orthonormal=False)
                                          for b in range(B))))
    x, y = batch_vectors(xs, n, stride), batch_vectors(ys, n, stride)
    got = call_dot(handle, x, y, n, stride, ref.START, state)
    dots, worst = np.zeros(B), 0.0
    for b in live:
        dots[b] = kref.tree_dots(xs[b], [ys[b]])[0]
        one = kry._call(handle, "mdot", xs[b], np.asarray([ys[b]]), None, 0.0, 0.0)[1][0]
        assert bref.same_bits(got["rz"][b], one), (b, "differs from mdot_stage1<1> / mdot_stage2")
        exact, scale = kref.exact_dots(xs[b], [ys[b]])[0], kref.abs_dots(xs[b], [ys[b]])[0]
        bound = kref.gamma(kref.dot_depth(n) + 1) * scale
        assert abs(got["rz"][b] - exact) <= bound, (b, abs(got["rz"][b] - exact) / bound)
        worst = max(worst, abs(got["rz"][b] - exact) / bound)
    print(f"spectrum dots n{n} B{B}: depth {kref.dot_depth(n)} largest error / bound {worst:.4f}")
    state_matches(got, ref.stage2(state, dots, ref.START, 0, 3), B)
    for b in range(B):
        if not act[b]:
            assert bref.same_bits(got["part"].reshape(B, -1)[b], np.full(ref.REDUCE_BLOCKS, FILL))

    # one family on both sides (the power iteration's norm): <x, x>, coef = 1 / sqrt
    got = call_dot(handle, x, x, n, stride, ref.NORM0, state)
    for b in live:
        dots[b] = kref.tree_dots(xs[b], [xs[b]])[0]
    state_matches(got, ref.stage2(state, dots, ref.NORM0, 0, 3), B)
    assert all(got["coef"][b] == 1.0 / math.sqrt(dots[b]) for b in live)


# ------------------------------------------------------------------- stage 2, every branch
THR = np.float64(1e-28) * np.float64(3.0)          # 1e-28 rz with rz = 3
NV = [1.0 + m * 2.0 ** -20 for m in (5269, 5270)]   # the 0.5 % rule flips between them (last = 1)
INF, NAN = math.inf, math.nan
#          (x, y, the dot, last)
BRANCHES = [([2.5, 0, 0], [1, 0, 0], 2.5, 2.0),
            ([0.0, 0, 0], [1, 0, 0], 0.0, 2.0),
            ([-1.5, 0, 0], [1, 0, 0], -1.5, 2.0),
            ([1e200, 0, 0], [1e200, 0, 0], INF, 2.0),
            ([INF, 0, 0], [0.0, 0, 0], NAN, 2.0),
            ([1e200, 0, -1e200], [1e200, 0, 1e200], NAN, 2.0),     # +inf and -inf of two workgroups
            ([THR, 0, 0], [1, 0, 0], THR, 2.0),
            ([0, 0, np.nextafter(THR, 1.0)], [0, 0, 1], np.nextafter(THR, 1.0), 2.0),
            ([2.0, 0, 0], [2.0, 0, 0], 4.0, 2.0),
            ([0, 4.2, 0], [0, 1, 0], 4.2, 2.0),
            ([NV[0], 0, 0], [NV[0], 0, 0], NV[0] * NV[0], 1.0),
            ([0, 0, NV[1]], [0, 0, NV[1]], NV[1] * NV[1], 1.0),
            ([3.0, 0, 0], [3.0, 0, 0], 9.0, 2.0)]           # the inactive one
MODES = ("start", "pap", "rz", "norm0", "norm")


@pytest.mark.parametrize("k", (7, 8), ids=lambda v: f"k{v}")
@pytest.mark.parametrize("mode", MODES)
def test_stage2_branches(handle, mode, k):
    n, B, ms = 3, len(BRANCHES), 4
    stride = ref.batch_stride(n)
    x = batch_vectors([c[0] for c in BRANCHES], n, stride)
    y = batch_vectors([c[1] for c in BRANCHES], n, stride)
    dots = [c[2] for c in BRANCHES]
    m = _lib.SPECTRUM_DOT_MODES[mode]
    for count in (0, ms - 1, ms):
        state = ref.new_state(B, ms)
        state["active"][B - 1] = 0
        state["rz"][:] = 3.0
        state["last"][:] = [c[3] for c in BRANCHES]
        state["na"][:] = count
        state["nb"][:] = count
        want = ref.stage2(state, dots, m, k, ms)
        got = call_dot(handle, x, y, n, stride, m, state, k=k, max_steps=ms)
        state_matches(got, want, B)
        # the reference takes the branches the case is about
        act = want["active"].tolist()
        if mode in ("start", "pap"):
            assert act == [1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0]
        elif mode == "rz":
            assert act == [1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0]
        elif mode == "norm0":
            assert act == [1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0]
        else:
            settled = [0, 1, 0, 1] if k == 8 else [1, 1, 1, 1]
            assert act == [1, 0, 0, 0, 0, 0, 1, 1] + settled + [0]
            assert got["na"].tolist() == [k + 1] * (B - 1) + [count]
        # the store guard, on the device's own arrays
        for name, cnt, md in (("alpha", "na", "pap"), ("beta", "nb", "rz")):
            changed = np.flatnonzero(got[name] != state[name])
            if mode != md:
                assert len(changed) == 0, name
                continue
            alive = [b for b in range(B) if want["active"][b]]
            assert got[cnt][alive].tolist() == [count + 1] * len(alive)
            if count < ms:
                assert changed.tolist() == [count * B + b for b in alive], name
            else:
                assert len(changed) == 0, (name, "stored past max_steps")
        # the inactive matrix: nothing of it written, its partial sums included
        assert bref.same_bits(got["part"].reshape(B, -1)[B - 1], np.full(ref.REDUCE_BLOCKS, FILL))


# ------------------------------------------------------------------------------ updates
KINDS = ("r", "p", "scale", "copy")


@functools.lru_cache(maxsize=4)
def _update_data(n, B):
    stride = ref.batch_stride(n)
    v = ref.special_values(bref.real_data((B, stride), 31), 4)
    x = ref.special_values(bref.real_data((B, stride), 32), 5)
    if n >= 3:                     # the second vector's NaN and inf, in the last (active) matrix
        x[B - 1, n // 2], x[B - 1, n // 3] = NAN, INF
        v[B - 1, n // 2], v[B - 1, n // 3] = 1.5, -0.0
    v[:, n:] = FILL
    x[:, n:] = FILL
    v.setflags(write=False)
    x.setflags(write=False)
    return v, x, stride


@pytest.mark.parametrize("B", (1, 3), ids=lambda v: f"B{v}")
@pytest.mark.parametrize("n", UPDATE_N, ids=lambda v: f"n{v}")
def test_updates(handle, n, B):
    v, x, stride = _update_data(n, B)
    act = actives(B)
    for coefs in ([1.0 / 3.0, 9.0, -2.5][:B], [0.0, 9.0, -0.0][:B]):
        coef = np.array(coefs)
        for kind in KINDS:
            kd = _lib.SPECTRUM_UPDATES[kind]
            got = run(handle, "update", mode=kd, nmat=B, n=n, stride=stride, x=x, v=v, coef=coef,
                      active=act)
            assert got["batch_stride"] == stride
            out = got["v"].reshape(B, stride)
            assert ref.same(out, ref.update(kd, v, x, coef, act, n)), (kind, coefs)
            assert bref.same_bits(out[:, n:], v[:, n:]), (kind, "padding")
            for b in range(B):
                if not act[b]:
                    assert bref.same_bits(out[b], v[b]), (kind, "an inactive matrix was written")
                    continue
                ab = ref.axpby_coefficients(kd, coef[b])        # the one-matrix loop's call
                if ab is None:
                    one = kry._call(handle, "copy", v[b, :n], x[b:b + 1, :n], None, 0.0, 0.0)[0]
                else:
                    one = kry._call(handle, "axpby", v[b, :n], x[b:b + 1, :n], None, ab[0], ab[1])[0]
                assert ref.same(out[b, :n], one), (kind, b, "differs from the one-matrix kernel")
            if kind == "scale" and n >= 3:
                assert np.isnan(out[B - 1, n // 2]) and np.isnan(out[B - 1, n // 3])


# -------------------------------------------------------------------------------- split
def _split(handle, a, t, flags_in):
    nmat, n = a.shape
    got = run(handle, "sym_skew", nmat=nmat, n=n, a=a, tpos=t, h=np.full(nmat * n, FILL),
              sk=np.full(nmat * n, FILL), flag=flags_in)
    h, sk = got["h"].reshape(nmat, n), got["sk"].reshape(nmat, n)
    for m in range(nmat):
        wh, wsk, wf = bref.vals_sym_skew(a[m], t, int(flags_in[m]))
        assert bref.same_bits(h[m], wh) and bref.same_bits(sk[m], wsk), m
        assert got["flag"][m] == wf, (m, got["flag"].tolist())
    return h, sk, got["flag"].tolist()


@pytest.mark.parametrize("nmat", (1, 3), ids=lambda v: f"nmat{v}")
@pytest.mark.parametrize("n", SPLIT_N, ids=lambda v: f"n{v}")
def test_split(handle, n, nmat):
    t = blk._involution(n, 33)
    a = bref.real_data((nmat, n), 34)
    a[a == 0.0] = 1.0
    paired = np.flatnonzero((t >= 0) & (t != np.arange(n)))
    zeros = np.zeros(nmat, dtype=np.uint32)
    # general matrices; the one-matrix kernel on the same data
    h, sk, f = _split(handle, a, t, zeros)
    assert f == [1 if len(paired) else 0] * nmat
    for m in range(nmat):
        oh, osk, of = blk.call(handle, "vals_sym_skew", nx=n, x=a[m], idx=t, y=np.full(n, FILL),
                               y2=np.full(n, FILL), flag=0)
        assert bref.same_bits(h[m], oh) and bref.same_bits(sk[m], osk) and f[m] == of, m
    # symmetric ones; a flag that comes in set stays
    sym = a.copy()
    sym[:, t >= 0] = 0.5 * (a[:, t >= 0] + a[:, t[t >= 0]])
    assert _split(handle, sym, t, zeros)[2] == [0] * nmat
    ones = np.array([0, 1, 0][:nmat] if nmat > 1 else [1], dtype=np.uint32)
    assert _split(handle, sym, t, ones)[2] == ones.tolist()
    if not len(paired):
        return
    # flags are per matrix: the first asymmetric at the last pair alone, its neighbours below the
    # measure and with an exact zero on one side
    p = int(paired[-1])
    q = int(t[p])
    m3 = sym.copy()
    m3[0, q] = bref.apart(m3[0, p], 2e-12)
    if nmat > 1:
        m3[1, q] = bref.apart(m3[1, p], 0.5e-12)
        m3[2, q] = 0.0
    assert _split(handle, m3, t, zeros)[2] == [1, 0, 0][:nmat]
    for m in range(nmat):
        of = blk.call(handle, "vals_sym_skew", nx=n, x=m3[m], idx=t, y=np.full(n, FILL),
                      y2=np.full(n, FILL), flag=0)[2]
        assert of == [1, 0, 0][m]


# -------------------------------------------------------------------------- fingerprint
def _fingerprints(handle, a, launch=call, want=None):
    """Words and folds of the candidates, held against the reference's (``want``: per candidate,
    where the caller has them already)."""
    nmat, n = a.shape
    nw = ref.fingerprint_blocks(n)
    got = launch(handle, "fingerprint", nmat=nmat, n=n, a=a,
                 words=np.full(nmat * nw, 0x0123456789abcdef, dtype=np.uint64),
                 fold=np.zeros(nmat, dtype=np.uint64))
    words = got["words"].reshape(nmat, nw)
    for m in range(nmat):
        ww, wf = want[m] if want else ref.fingerprint(a[m])
        assert np.array_equal(words[m], ww), (m, "words")
        assert int(got["fold"][m]) == wf == ref.fold(words[m]), (m, "fold")
    return words, [int(f) for f in got["fold"]]


@pytest.mark.parametrize("nmat", ref.FP_NMAT, ids=lambda v: f"nmat{v}")
@pytest.mark.parametrize("n", ref.FP_N, ids=lambda v: f"n{v}")
def test_fingerprint(handle, n, nmat):
    a = ref.fingerprint_arrays(n, nmat)
    words, folds = _fingerprints(handle, a, run)
    assert len(set(folds)) == nmat
    m = nmat - 1
    for pos in ref.fingerprint_positions(n):
        for kind in ref.BIT_KINDS:
            base, other = ref.flip(a[m], pos, kind)
            wb, wo = ref.fingerprint(base), ref.fingerprint(other)
            w3, f3 = _fingerprints(handle, np.stack([base, other, base]), want=[wb, wo, wb])
            assert np.array_equal(w3[0], w3[2]) and f3[0] == f3[2], (pos, kind, "equal bits")
            assert f3[0] != f3[1], (pos, kind, "a flipped bit kept the fingerprint")
            if kind == "mantissa":
                assert np.array_equal(w3[0], words[m])


# --------------------------------------------------------------------- pair comparison
PAIR_SETS = ([(0, 2)], [(0, 1), (0, 2), (2, 2)], [(0, 1), (2, 0), (1, 2), (3, 3), (0, 3)])
FLIPPED = 2                  # of the arrays 0..3, this one carries the flipped bit


def _pairs(handle, arrays, pairs, flags_in):
    got = run(handle, "pairs_differ", nmat=len(arrays), n=arrays.shape[1], npairs=len(pairs), a=arrays,
              pair_a=[p[0] for p in pairs], pair_b=[p[1] for p in pairs], flag=flags_in)
    return got["flag"].tolist()


@pytest.mark.parametrize("n", PAIRS_N, ids=lambda v: f"n{v}")
def test_pair_comparison(handle, n):
    a = bref.real_data(n, 35)
    # equal arrays: nothing is raised, a set flag stays
    same4 = np.stack([a, a, a, a])
    for pairs in PAIR_SETS:
        assert _pairs(handle, same4, pairs, np.zeros(len(pairs), dtype=np.uint32)) == [0] * len(pairs)
    assert _pairs(handle, same4, PAIR_SETS[1], np.array([0, 1, 0], dtype=np.uint32)) == [0, 1, 0]
    for pos in ref.pair_positions(n):
        for kind in ref.BIT_KINDS:
            base, other = ref.flip(a, pos, kind)
            arrays = np.stack([base, base, base, base])
            arrays[FLIPPED] = other
            one = {}                      # the one-matrix kernel per distinct pair of arrays
            for pairs in PAIR_SETS:
                flags = _pairs(handle, arrays, pairs, np.zeros(len(pairs), dtype=np.uint32))
                want = [int((i == FLIPPED) != (j == FLIPPED)) for i, j in pairs]
                assert flags == want, (pos, kind, pairs)
                assert flags == [bref.vals_differ(arrays[i], arrays[j]) for i, j in pairs]
                for (i, j), f in zip(pairs, flags):
                    key = (i == FLIPPED, j == FLIPPED)
                    if key not in one:
                        one[key] = blk.call(handle, "vals_differ", nx=n, x=arrays[i], x2=arrays[j],
                                            flag=0)[2]
                    assert f == one[key], (pos, kind, i, j, "differs from vals_differ_kernel")
            # raised flags join the ones that came in
            flags = _pairs(handle, arrays, PAIR_SETS[2], np.array([1, 0, 0, 1, 0], dtype=np.uint32))
            assert flags == [1, 1, 1, 1, 0], (pos, kind)


# --------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_rejected(handle):
    lib, h = handle
    n, B, ms = 5, 2, 3
    stride = ref.batch_stride(n)
    vec = np.arange(1.0, B * stride + 1.0)

    def rc(op, **fields):
        a, guarded, keep = _record(op, fields)
        before = {k: g.copy() for k, g in guarded.items()}
        code = lib.kkt_debug_spectrum_op(h, C.byref(a))
        if code:
            assert b"kkt_debug_spectrum_op" in lib.kkt_last_error(h)
            # nothing was launched or touched: the allocations are as they went in, guards included
            for k, g in guarded.items():
                assert g.tobytes() == before[k].tobytes(), k
        return code

    st = ref.new_state(B, ms)
    dot = dict(mode=0, k=0, nmat=B, max_steps=ms, n=n, stride=stride, x=vec, y=vec,
               part=np.zeros(B * ref.REDUCE_BLOCKS), **st)
    assert rc("dot", **dot) == 0
    assert rc(99, **dot) == -1 and rc(-1, **dot) == -1
    assert lib.kkt_debug_spectrum_op(h, None) == -1
    assert lib.kkt_debug_spectrum_op(None, None) == -1
    for bad in (dict(mode=-1), dict(mode=5), dict(k=-1), dict(nmat=0), dict(nmat=-2), dict(nmat=65536),
                dict(n=0), dict(n=-5), dict(max_steps=0), dict(stride=stride + 1), dict(stride=n - 1),
                dict(stride=4), dict(stride=2 ** 31), dict(max_steps=2 ** 31 - 1),
                dict(na=[0, -1]), dict(nb=[-1, 0])):
        assert rc("dot", **dict(dot, **bad)) == -1, bad
    for name in ("x", "y", "part") + STATE:
        assert rc("dot", **dict(dot, **{name: None})) == -1, name
    assert rc("dot", **dict(dot, stride=6, x=vec[:12], y=vec[:12])) == 0       # even, n + 1
    upd = dict(mode=0, nmat=B, n=n, stride=stride, x=vec, v=vec, coef=st["coef"], active=st["active"])
    assert rc("update", **upd) == 0
    for bad in (dict(mode=-1), dict(mode=4), dict(nmat=0), dict(n=0), dict(stride=stride - 1),
                dict(stride=n - 1), dict(x=None), dict(v=None), dict(coef=None), dict(active=None)):
        assert rc("update", **dict(upd, **bad)) == -1, bad
    vals = np.arange(1.0, 2 * n + 1.0)
    t = np.array([1, 0, 2, -1, 4], dtype=np.int32)
    spl = dict(nmat=2, n=n, a=vals, tpos=t, h=np.zeros(2 * n), sk=np.zeros(2 * n),
               flag=np.zeros(2, dtype=np.uint32))
    assert rc("sym_skew", **spl) == 0
    for bad in (dict(nmat=0), dict(n=0), dict(nmat=65536), dict(n=2 ** 31), dict(a=None), dict(tpos=None),
                dict(h=None), dict(sk=None), dict(flag=None), dict(tpos=[1, 0, 2, -2, 4]),
                dict(tpos=[1, 0, 2, -1, 5])):
        assert rc("sym_skew", **dict(spl, **bad)) == -1, bad
    fp = dict(nmat=2, n=n, a=vals, words=np.zeros(2, dtype=np.uint64), fold=np.zeros(2, dtype=np.uint64))
    assert rc("fingerprint", **fp) == 0
    for bad in (dict(nmat=0), dict(n=0), dict(a=None), dict(words=None), dict(fold=None)):
        assert rc("fingerprint", **dict(fp, **bad)) == -1, bad
    pr = dict(nmat=2, n=n, npairs=2, a=vals, pair_a=[0, 1], pair_b=[1, 1], flag=np.zeros(2, dtype=np.uint32))
    assert rc("pairs_differ", **pr) == 0
    for bad in (dict(nmat=0), dict(n=0), dict(npairs=0), dict(npairs=65536), dict(a=None),
                dict(pair_a=None), dict(pair_b=None), dict(flag=None), dict(pair_a=[0, 2]),
                dict(pair_b=[-1, 1])):
        assert rc("pairs_differ", **dict(pr, **bad)) == -1, bad
