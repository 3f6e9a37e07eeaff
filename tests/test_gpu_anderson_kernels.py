"""The three kernels of the device Anderson mixer, one launch at a time through
``kkt_debug_anderson_op``, and ``kkt_anderson_step`` / ``_reset`` / ``_set`` on a small system of
identity blocks, against the independent reference ``tests/anderson_ref.py`` and the NumPy mirror
``control_amd/anderson.py``.

Lengths: 1, 2 (one pair), 63 .. 65 (a wave), 255 .. 257 (a workgroup of pairs is 512 elements:
these stay inside it, odd and even), 1023, 4097 (several workgroups, the odd tail), and lengths at
which the strided loops take a second trip.  The Gram pass has a fixed grid of 512 workgroups x
256 threads on pairs of elements: 131075 (a second trip had the kernel read single elements) and
262147 (a second trip as it is).  Push and mix launch up to 2048 workgroups x 256 threads on
pairs: their second trip begins above 2^20 elements, 1048579 here.  Columns 0, 1, 2, 3, 5, 8.

The Gram sums are fused multiply-adds summed in a fixed order: each within ``n u sum |a_i b_i|``
of the exact dot product, equal bits on repetition, exact on dyadic data.  Push and mix are bit
for bit NumPy's unfused arithmetic."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import anderson_ref as ref
import common
from control_amd import _lib
from control_amd.anderson import AndersonMixer, cholesky_gamma, mix

pytestmark = pytest.mark.gpu

GRID = 512 * 256
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097]
LONG = [GRID + 3, 2 * GRID + 3]
STREAM_LONG = 2 * 2048 * 256 + 3         # push and mix: one sweep of their largest grid, and 3
COLUMNS = [0, 1, 2, 3, 5, 8]
SLACK = 37
PAD = _lib.KRYLOV_PAD


@pytest.fixture(scope="module")
def handle():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0, lib.kkt_last_error(None)
    yield lib, h
    assert lib.kkt_destroy(h) == 0


def _ptr(a):
    return a.ctypes.data_as(_lib.c_f64p)


def _op(handle, name, **kw):
    lib, h = handle
    op = _lib.AndersonOp(op=_lib.ANDERSON_OPS[name], **kw)
    assert lib.kkt_debug_anderson_op(h, C.byref(op)) == 0, lib.kkt_last_error(h)
    assert op.inputs_changed == 0
    return op


def _data(n, c, seed):
    rng = np.random.default_rng(common.SEED + seed)
    return (rng.standard_normal(n), rng.standard_normal((c, n)), rng.standard_normal((c, n)))


def _padded(n, fill=None):
    a = np.full(n + SLACK, PAD)
    if fill is not None:
        a[:n] = fill
    return a


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ------------------------------------------------------------------------------ push
@pytest.mark.parametrize("n", SIZES + LONG + [STREAM_LONG])
def test_push(handle, n):
    f, prev, _ = _data(n, 1, 1)
    f_prev, out = _padded(n, prev[0]), _padded(n)
    _op(handle, "push", n=n, slack=SLACK, f=_ptr(f), f_prev=_ptr(f_prev), out=_ptr(out))
    assert _same_bits(out[:n], f - prev[0])
    assert _same_bits(f_prev[:n], f)                       # f_prev is replaced
    assert np.all(out[n:] == PAD) and np.all(f_prev[n:] == PAD)


# ------------------------------------------------------------------------------ gram
def _gram(handle, f, dF):
    c, n = dF.shape
    G, r = np.full((c, c), np.nan), np.full(c, np.nan)
    _op(handle, "gram", n=n, c=c, f=_ptr(f), dF=_ptr(dF), G=_ptr(G), r=_ptr(r))
    return G, r


GRAM_CASES = [(n, c) for n in SIZES for c in COLUMNS if c] + [(LONG[0], 3), (LONG[1], 1),
                                                              (LONG[1], 8)]


@pytest.mark.parametrize("n, c", GRAM_CASES)
def test_gram_on_dyadic_data_is_exact_and_repeats(handle, n, c):
    """Small integers over 8: every product and every partial sum is exact in double."""
    rng = np.random.default_rng(common.SEED + n + c)
    f = rng.integers(-16, 17, n) / 8.0
    dF = rng.integers(-16, 17, (c, n)) / 8.0
    G, r = _gram(handle, f, dF)
    assert _same_bits(G + 0.0, (dF @ dF.T) + 0.0) and _same_bits(r + 0.0, (dF @ f) + 0.0)
    G2, r2 = _gram(handle, f, dF)
    assert _same_bits(G, G2) and _same_bits(r, r2)


@pytest.mark.parametrize("n, c", [(n, c) for n in SIZES for c in (1, 3, 8)] + [(LONG[0], 2)])
def test_gram_within_the_dot_product_bound(handle, n, c):
    f, dF, _ = _data(n, c, 2)
    G, r = _gram(handle, f, dF)
    G2, r2 = _gram(handle, f, dF)
    assert _same_bits(G, G2) and _same_bits(r, r2)
    assert np.array_equal(G, G.T)
    for i in range(c):
        pairs = [(r[i], dF[i], f)] + [(G[i, j], dF[i], dF[j]) for j in range(i + 1)]
        for got, a, b in pairs:
            assert abs(Fraction(got) - ref.exact_dot(a, b)) <= ref.dot_bound(a, b)


def test_gram_without_columns_launches_nothing(handle):
    f = np.ones(5)
    _op(handle, "gram", n=5, c=0, f=_ptr(f))


# ------------------------------------------------------------------------------ mix
def _mix(handle, f, dX, dF, gamma, beta, alias=False):
    c, n = dF.shape
    s, slot = _padded(n), _padded(n)
    g = (C.c_double * 8)(*gamma)
    _op(handle, "mix", n=n, c=c, slack=SLACK, beta=beta, gamma=g, alias=int(alias), f=_ptr(f),
        dF=_ptr(dF), dX=_ptr(dX), out=_ptr(s), out2=_ptr(slot))
    assert np.all(s[n:] == PAD) and np.all(slot[n:] == PAD)
    assert _same_bits(s[:n], slot[:n])
    return s[:n]


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("n, c", [(n, c) for n in SIZES for c in COLUMNS] + [
    (LONG[0], 2), (LONG[1], 8), (STREAM_LONG, 0), (STREAM_LONG, 3)])
def test_mix_is_the_unfused_statement(handle, n, c, beta):
    f, dF, dX = _data(n, c, 3)
    gamma = np.random.default_rng(common.SEED + c).standard_normal(c)
    got = _mix(handle, f, dX, dF, gamma, beta)
    assert _same_bits(got, mix(f, dX, dF, gamma, beta))
    if n <= 257:
        assert _same_bits(got, ref.mix_unfused(f, dX, dF, gamma, beta))
    if c == 0 and beta == 1.0:
        assert _same_bits(got, f)                          # the plain Picard step: the input's bits
    if c:                 # a full ring: the new slot is the oldest pair's
        assert _same_bits(_mix(handle, f, dX, dF, gamma, beta, alias=True), got)


def test_mix_with_signed_zero_coefficients(handle):
    n = 65
    f, dF, dX = _data(n, 3, 4)
    f[:4] = [0.0, -0.0, 1.0, -1.0]
    for gamma in ([-0.0, 0.0, 1.5], [0.0, -0.0, -0.0], [-0.0, -0.0, -0.0]):
        assert _same_bits(_mix(handle, f, dX, dF, gamma, 1.0), mix(f, dX, dF, np.array(gamma), 1.0))


# ------------------------------------------------------------------------------ a system
class _System:
    """Two identity blocks of 128 and 129 rows: a finalized handle of local size 257."""

    def __init__(self, lib, nx=(128, 129), options=()):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.kkt_create(C.byref(self.h), 0) == 0
        for k, v in options:
            assert lib.kkt_set_option(self.h, k.encode(), v.encode()) == 0
        assert lib.kkt_set_layout(self.h, 1, 1, nx[0], nx[1], 0, -1, -1) == 0
        for q, n in ((0, nx[0]), (3, nx[1])):
            A = sp.identity(n, format="csr")
            ip, ix = _lib.i32(A.indptr), _lib.i32(A.indices)
            va = _lib.f64(A.data)
            assert lib.kkt_add_block(self.h, q, 0, 0, n, n, ip[1], ix[1], va[1], -1) == 0
        assert lib.kkt_finalize(self.h) == 0, lib.kkt_last_error(self.h)
        self.n = lib.kkt_local_size(self.h)
        self.d_u = C.c_void_p()
        assert lib.kkt_vec_alloc(self.h, C.byref(self.d_u)) == 0

    def step(self, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        assert self.lib.kkt_vec_upload(self.h, self.d_u, _ptr(f)) == 0
        info = _lib.AndersonInfo()
        rc = self.lib.kkt_anderson_step(self.h, self.d_u, C.byref(info))
        assert rc == 0, self.lib.kkt_last_error(self.h)
        s = np.empty(self.n)
        assert self.lib.kkt_vec_download(self.h, self.d_u, _ptr(s)) == 0
        return s, info

    def read(self, which, slot=0):
        out = np.full(self.n, np.nan)
        op = _lib.AndersonOp(op=_lib.ANDERSON_OPS["read"], which=which, slot=slot, out=_ptr(out))
        assert self.lib.kkt_debug_anderson_op(self.h, C.byref(op)) == 0
        return out, tuple(op.ring)

    def close(self):
        self.lib.kkt_vec_free(self.h, self.d_u)
        assert self.lib.kkt_destroy(self.h) == 0


@pytest.fixture()
def system():
    s = _System(_lib.load())
    yield s
    s.close()


def _updates(count, n, seed):
    rng = np.random.default_rng(common.SEED + seed)
    return [0.6 ** k * rng.standard_normal(n) for k in range(count)]


def test_sequence_of_eight_calls_at_depth_three(system):
    lib, n, depth = system.lib, system.n, 3
    assert n == 257
    assert lib.kkt_anderson_set(system.h, depth, 1.0, 1.0e7) == 0
    mirror = AndersonMixer(n, depth)
    fs, steps, drops = _updates(8, n, 5), [], []
    for k, f in enumerate(fs):
        mirror.step(f)
        s, info = system.step(f)
        c = info.columns
        assert (c, info.dropped) == (mirror.info["columns"], mirror.info["dropped"])
        G, r = np.array(info.G[:c * c]).reshape(c, c), np.array(info.r[:c])
        gamma = np.array(info.gamma[:c])
        if c:
            # gamma against the mirror's arithmetic on the device's own G, r ...
            dropped, mine = cholesky_gamma(G, r, 1.0e7)
            assert dropped == 0
            exact, ratio = ref.solve_mp(G, r)
            bound = ref.gamma_bound(c, ratio) * np.abs(exact).max()
            # the issue's bound, against the 60-digit solve of the device's own G, r; the
            # mirror's arithmetic on the same G, r obeys it too, so the two lie within twice it
            assert np.abs(gamma - exact).max() <= bound
            assert np.abs(mine - exact).max() <= bound
            assert np.abs(gamma - mine).max() <= 2.0 * bound
            for i in range(c):      # device and mirror sum the same dF in different orders:
                for j in range(c):  # each within the dot-product bound of exact, so twice apart
                    assert abs(G[i, j] - mirror.info["G"][i, j]) <= \
                        2.0 * ref.dot_bound(mirror.info["dF"][i], mirror.info["dF"][j])
        steps.append(s)
        drops.append(info.dropped)
        # the ring holds what the statement says, given the device's own steps
        dF, dX = ref.expected_ring(fs[:k + 1], steps[:k], depth, drops)
        head, count, have_prev, d = system.read(2)[1]
        assert (count, have_prev, d) == (c, 1, depth)
        for j in range(c):
            slot = (head - count + j) % depth
            assert _same_bits(system.read(0, slot)[0], dF[j])
            if slot != head:      # a full ring: the oldest pair's dX slot is the head, which
                assert _same_bits(system.read(1, slot)[0], dX[j])     # holds the step by now
        assert (c == depth) == any((head - count + j) % depth == head for j in range(c))
        assert _same_bits(system.read(1, head)[0], s)          # kept as the next dX
        assert _same_bits(system.read(2)[0], f)                # kept as f_prev
        # the step, given the device's gamma, is the unfused statement
        assert _same_bits(s, mix(f, dX, dF, gamma, 1.0))
    assert [system.read(2)[1][1]] == [3]


def test_reset_and_pass_through(system):
    lib = system.lib
    assert lib.kkt_anderson_reset(system.h) == -3            # no mixer yet
    assert lib.kkt_anderson_step(system.h, system.d_u, None) == -3
    assert lib.kkt_anderson_set(system.h, 2, 1.0, 1.0e7) == 0
    fs = _updates(3, system.n, 6)
    first, info = system.step(fs[0])
    assert _same_bits(first, fs[0]) and info.columns == 0
    second, info = system.step(fs[1])
    assert info.columns == 1
    assert lib.kkt_anderson_reset(system.h) == 0
    again, info = system.step(fs[0])
    assert _same_bits(again, first) and info.columns == 0
    again, info = system.step(fs[1])
    assert _same_bits(again, second) and info.columns == 1
    # equal consecutive updates: a zero pivot, the pair is dropped, the plain step again
    s, info = system.step(fs[1])
    assert (info.columns, info.dropped) == (0, 2) and _same_bits(s, fs[1])
    # damping
    assert lib.kkt_anderson_set(system.h, 2, 0.5, 1.0e7) == 0
    s, info = system.step(fs[2])
    assert _same_bits(s, 0.5 * fs[2])


def test_argument_errors(system):
    lib, h = system.lib, system.h
    for args, word in (((9, 1.0, 1.0e7), b"depth 9"), ((-1, 1.0, 1.0e7), b"depth -1"),
                       ((3, 1.0, 1.0), b"cond_max"), ((3, 1.0, 0.5), b"cond_max"),
                       ((3, 0.0, 1.0e7), b"beta"), ((3, float("nan"), 1.0e7), b"beta")):
        assert lib.kkt_anderson_set(h, *args) == -1
        assert word in lib.kkt_last_error(h)
    assert lib.kkt_anderson_set(h, 3, 1.0, 1.0e7) == 0
    assert lib.kkt_anderson_step(h, None, None) == -1
    bad = _lib.AndersonOp(op=7, n=4)
    assert lib.kkt_debug_anderson_op(h, C.byref(bad)) == -1
    bad = _lib.AndersonOp(op=_lib.ANDERSON_OPS["gram"], n=4, c=9, f=_ptr(np.ones(4)))
    assert lib.kkt_debug_anderson_op(h, C.byref(bad)) == -1


def test_a_sharded_handle_is_refused():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0
    try:
        assert lib.kkt_set_layout(h, 6, 6, 40, 40, 0, -1, -1) == 0
        assert lib.kkt_set_shard(h, 1, 3) == 0
        assert lib.kkt_anderson_set(h, 3, 1.0, 1.0e7) == -3
        assert b"time-sharded" in lib.kkt_last_error(h)
    finally:
        lib.kkt_destroy(h)


def test_depth_zero_frees_the_history():
    """Free device memory (``hipMemGetInfo``, as ``tests/test_gpu_device_memory.py`` reads it) on
    a system of 2 x 2^20 rows: a depth-8 history is 17 vectors of 16 MiB, and set / remove
    cycles must not accumulate it."""
    from test_gpu_device_memory import _free_once, _granule
    s = _System(_lib.load(), nx=(1 << 20, 1 << 20))
    try:
        granule = _granule()
        vec = 8 * s.n
        base = _free_once()
        held, levels = [], []
        for _ in range(4):
            assert s.lib.kkt_anderson_set(s.h, 8, 1.0, 1.0e7) == 0
            held.append(base - _free_once())
            assert s.lib.kkt_anderson_set(s.h, 0, 1.0, 1.0e7) == 0
            levels.append(_free_once())
        print(f"granule {granule} B, held while set {held} B (17 vectors: {17 * vec} B), free "
              f"after depth 0 minus before: {[v - base for v in levels]}")
        # the runtime hands freed memory back when it likes (the readings after depth 0 come in
        # two levels, one history apart), so what is held WHILE SET is the measure: a history
        # that depth 0 did not free would add 272 MiB to it with every cycle
        assert held[0] >= 17 * vec - granule
        assert all(h <= held[0] + granule for h in held[1:])
        assert all(v >= base - held[0] - granule for v in levels)
        # a new depth replaces the history: no more is held than by the larger one
        assert s.lib.kkt_anderson_set(s.h, 8, 1.0, 1.0e7) == 0
        assert s.lib.kkt_anderson_set(s.h, 2, 1.0, 1.0e7) == 0
        assert base - _free_once() <= held[0] + granule
    finally:
        s.close()


def test_stage_timers_report_the_three_kernels():
    s = _System(_lib.load(), options=(("stage_timers", "1"),))
    try:
        assert s.lib.kkt_anderson_set(s.h, 2, 1.0, 1.0e7) == 0
        fs = _updates(2, s.n, 7)
        _, info = s.step(fs[0])
        assert info.push_ms == 0.0 and info.gram_ms == 0.0 and info.mix_ms > 0.0
        _, info = s.step(fs[1])
        assert min(info.push_ms, info.gram_ms, info.mix_ms) > 0.0
    finally:
        s.close()
