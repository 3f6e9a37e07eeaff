"""The time-transform, nullspace and value set-up kernels against exact references, one launch at
a time through ``kkt_debug_block_op``: ``time_transform_kernel`` (kinds 1-4),
``time_transform_mask_kernel``, ``mask_blocks_kernel``, ``const_sums_kernel`` / ``const_shift_kernel``
(``launch_const_correct`` with ``second`` = 0, 1, 2 and ``launch_const_center``),
``csr_to_sell_kernel``, ``mask_columns_kernel``, ``vals_axpy_kernel``, ``vals_differ_kernel``,
``vals_sym_skew_kernel`` and ``extract_dinv_kernel<1 | 2>``.  References: ``tests/blockops_ref.py``
(checked on the host by ``tests/test_blockops_ref.py``).

Sizes -- each the smallest that reaches its regime, from the launch constants of ``kernels.hip``
(256 threads per workgroup everywhere):

    time_transform_mask   grid_for((nx + 1) / 2, 256, 256): one trip covers 256 x 256 x 2 = 131072
                          dofs.  1, 2, 3 (one thread, with and without the q = 1 break); 511, 512,
                          513 (one workgroup exactly, +-1); 131071, 131072, 131073, 131075 (the
                          second trip: absent, its first pair broken at q = 1, its second pair)
    time_transform        grid_for(nx), cap 2048 x 256 = 524288 per trip: 1, 255, 256, 257 and
                          524287, 524288, 524289
    mask_blocks,          grid_for(nx, 256, 64): 64 x 256 = 16384 per trip: 16383, 16384, 16385 and
    const_shift           40001 (a third trip) / 16385 and 50001 among the job lengths
    const_sums            one workgroup per job, `#pragma unroll 8` over chains of ceil(nx / 256):
                          1, 2, 255 (fewer elements than threads), 256, 257, 2047, 2048, 2049 (eight
                          per thread: the unrolled body once, with and without a remainder), 2305
    value arrays          grid_for(n): 1, 255, 256, 257; 524288, 524289 (second trip), 1048577 (third)
    extract_dinv          one thread per position, slices of 64 R: 1, 63, 64, 65, 127, 128, 129 and
                          1000 rows

What is asserted: every output bit for bit against the reference (``-0.0`` and ``+0.0`` differ); the
in-place calls the drivers make (``y == x`` under ``__restrict__``) give the bits of the
out-of-place ones; pieces of a transform run with the halo taken from the whole give the whole;
the sums of ``const_sums`` are the documented order's bit for bit and lie within
``gamma(ceil(nx / 256) + 8 + 1) sum |x|`` of the correctly rounded exact sum; every shifted element
is the rounded-product or the fused candidate, the same one throughout a launch; every launch gives
identical bits when repeated; the guard elements around every written array and all arrays a launch
only reads are as they were.

A row of ``extract_dinv`` without a stored diagonal gives 1.0 when none of its slots names the row
itself.  The library's own patterns pad a row with its own index and value 0, so there such a row,
if shorter than its slice, would read the padding's zero first; no matrix the drivers build has
such a row, and the cases here store the missing diagonal's row with ``-1`` padding.

Measured on an MI355X (gfx950): the shift of ``const_shift_kernel`` is the rounded-product
candidate in every launch in which the two differ (68 of 88; in the others, all with jobs of one or
two elements, they coincide).  Largest error / bound of a sum 0.092 (``nx`` = 256, one job; depth
9), 0.084 at 255 and 257, below 0.02 from 2047 on.  In-place and out-of-place launches of
``time_transform`` and ``mask_blocks`` agree in every case.  ``vals_axpy_kernel`` was found
contracted into a fused multiply-add (``c`` = 1/3: 16 % of the entries differed from the two
roundings its comment promises) and now runs under ``contract(off)``.  172 cases in 8 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import blockops_ref as ref
from control_amd import _lib

pytestmark = pytest.mark.gpu

G = _lib.BLOCK_GUARD
FILL = -1.2345e300          # what the array part of an output holds before a launch writes it
KINDS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def handle():
    """A created handle and nothing else: the entry does not depend on a layout."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0, lib.kkt_last_error(None)
    yield lib, h
    assert lib.kkt_destroy(h) == 0


# ------------------------------------------------------------------------------ the call
_TYPES = {"x": np.float64, "x2": np.float64, "lo_halo": np.float64, "hi_halo": np.float64,
          "mask": np.uint8, "has_mask": np.int32, "alpha": np.float64, "job_off": np.int64,
          "job_nx": np.int64, "job_c1": np.float64, "job_c2_one": np.float64,
          "job_c2_alpha": np.float64, "idx": np.int32, "idx2": np.int32, "idx3": np.int32}
_FIELD_TYPES = dict(_lib.BlockOp._fields_)


def _record(op, scalars, arrays, y, y2, flag):
    """``(BlockOp, [arrays kept alive], guarded y, guarded y2, guarded flag)``."""
    a = _lib.BlockOp()
    a.op = _lib.BLOCK_OPS[op] if isinstance(op, str) else op
    for k, v in scalars.items():
        setattr(a, k, v)
    keep = []
    for k, v in arrays.items():
        if v is None:
            continue
        v = np.ascontiguousarray(v, dtype=_TYPES[k])
        keep.append(v)
        setattr(a, k, v.ctypes.data_as(_FIELD_TYPES[k]))
    out = []
    for k, init in (("y", y), ("y2", y2)):
        if init is None:
            out.append(None)
            continue
        init = np.asarray(init, dtype=np.float64).ravel()
        g = np.full(len(init) + 2 * G, np.nan)
        g[G:G + len(init)] = init
        setattr(a, k, g.ctypes.data_as(_lib.c_f64p))
        out.append(g)
    gf = None
    if flag is not None:
        gf = np.zeros(2 * G + 1, dtype=np.uint32)
        gf[G] = flag
        a.flag = gf.ctypes.data_as(_lib.c_u32p)
    return a, keep, out[0], out[1], gf


def call(handle, op, *, y=None, y2=None, flag=None, kind=0, in_place=0, n=0, nx=0, length=0, c=0.0,
         **arrays):
    """One launch: ``(y, y2, flag)`` without their guards, which are checked here, as is the
    entry's comparison of every input with what it uploaded."""
    lib, h = handle
    a, keep, gy, gy2, gf = _record(op, dict(kind=kind, in_place=in_place, n=n, nx=nx, len=length, c=c),
                                   arrays, y, y2, flag)
    a.inputs_changed = -1
    rc = lib.kkt_debug_block_op(h, C.byref(a))
    if rc == -2:      # KKT_ERR_HIP: nothing more is started on a device that reported an error
        pytest.exit(f"HIP error in {op}: {lib.kkt_last_error(h)}", returncode=3)
    assert rc == 0, (op, rc, lib.kkt_last_error(h))
    assert a.inputs_changed == 0, (op, "an input array was written")
    res = []
    for g in (gy, gy2):
        if g is None:
            res.append(None)
            continue
        assert np.all(g[:G] == _lib.KRYLOV_PAD) and np.all(g[-G:] == _lib.KRYLOV_PAD), \
            (op, "guard elements were written")
        res.append(g[G:-G].copy())
    if gf is not None:
        assert np.all(gf[:G] == _lib.BLOCK_FLAG_PAD) and np.all(gf[G + 1:] == _lib.BLOCK_FLAG_PAD), \
            (op, "guard words of the flag were written")
        res.append(int(gf[G]))
    else:
        res.append(None)
    return res


def run(handle, op, **kw):
    """``call`` twice: identical bits."""
    first = call(handle, op, **kw)
    again = call(handle, op, **kw)
    for u, v in zip(first, again):
        if isinstance(u, np.ndarray):
            assert ref.same_bits(u, v), (op, "not reproducible")
        else:
            assert u == v, (op, "not reproducible")
    return first


@functools.lru_cache(maxsize=16)
def _levels(n, nx, seed):
    """Real data for n levels (cached: the kinds and forms of one size share it; read only)."""
    x = ref.real_data((n, nx), seed)
    x.setflags(write=False)
    return x


def _masks(n, nx, form, seed):
    """``(mask bytes or None, has_mask or None, list for the reference)``."""
    if form == "null":
        return None, None, [None] * n
    if form == "none_set":
        m = np.zeros((n, nx), dtype=np.uint8)
    elif form == "all":
        m = np.ones((n, nx), dtype=np.uint8)
    else:
        rng = np.random.default_rng([ref.SEED, n, nx, seed])
        m = (rng.random((n, nx)) < 0.3).astype(np.uint8)
        m[:, 0] = 1
        m[:, -1] = 1
        m *= rng.integers(1, 256, size=(n, nx), dtype=np.uint8)    # any non-zero byte masks
    return m, None, [m[i] != 0 for i in range(n)]


# --------------------------------------------------------------- the fused transform
@pytest.mark.parametrize("nx", (1, 2, 3, 511, 512, 513, 131071, 131072, 131073, 131075),
                         ids=lambda v: f"nx{v}")
@pytest.mark.parametrize("kind", (1, 2))
def test_time_transform_mask(handle, kind, nx):
    for n in (1, 2, 3, 7):
        t, xin = _levels(n, nx, 1), _levels(n, nx, 2)
        alpha = 0.5 + np.arange(n) * 1.25
        h = ref.real_data(nx, 3)
        for halo in (None, h):
            lo, hi = (halo, None) if kind == 2 else (None, halo)
            # (a halo on the side the kind does not read must not matter: given with every present one)
            other = None if halo is None else ref.real_data(nx, 4)
            glo, ghi = (halo, other) if kind == 2 else (other, halo)
            for form in ("null", "all", "none_set", "scattered"):
                m, _, mlist = _masks(n, nx, form, kind)
                want = ref.time_transform_mask(kind, t, xin, mlist, alpha, lo, hi)
                got = run(handle, "time_transform_mask", kind=kind, n=n, nx=nx, x=t, x2=xin, mask=m,
                          alpha=alpha, lo_halo=glo, hi_halo=ghi, y=np.full(n * nx, FILL))[0]
                assert ref.same_bits(got.reshape(n, nx), want), (n, halo is not None, form)
    # a level without a mask among masked ones, and xin absent when nothing is masked
    n = 3
    t, xin = _levels(n, nx, 1), _levels(n, nx, 2)
    m, _, mlist = _masks(n, nx, "scattered", 9)
    has = np.array([1, 0, 1], dtype=np.int32)
    mlist[1] = None
    alpha = np.array([2.0, 1e300, -3.0])
    want = ref.time_transform_mask(kind, t, xin, mlist, alpha)
    got = run(handle, "time_transform_mask", kind=kind, n=n, nx=nx, x=t, x2=xin, mask=m,
              has_mask=has, alpha=alpha, y=np.full(n * nx, FILL))[0]
    assert ref.same_bits(got.reshape(n, nx), want)
    got = run(handle, "time_transform_mask", kind=kind, n=n, nx=nx, x=t, y=np.full(n * nx, FILL))[0]
    assert ref.same_bits(got.reshape(n, nx), ref.time_transform(kind, t))


# ------------------------------------------------------------------- the transforms
@pytest.mark.parametrize("nx", (1, 255, 256, 257, 524287, 524288, 524289), ids=lambda v: f"nx{v}")
@pytest.mark.parametrize("kind", KINDS)
def test_time_transform(handle, kind, nx):
    """Out of place and in place (``pc_stokes.cpp`` calls ``launch_time_transform(st, h_, h_, ...)``):
    both bit for bit the reference."""
    for n in ((1, 2, 5) if nx < 10000 else (1, 2)):
        x = _levels(n, nx, 5)
        h = ref.real_data(nx, 6)
        for halo in (None, h):
            lo, hi = (halo, None) if kind in (2, 4) else (None, halo)
            other = None if halo is None else ref.real_data(nx, 7)
            glo, ghi = (halo, other) if kind in (2, 4) else (other, halo)
            want = ref.time_transform(kind, x, lo, hi)
            out = run(handle, "time_transform", kind=kind, n=n, nx=nx, x=x, lo_halo=glo, hi_halo=ghi,
                      y=np.full(n * nx, FILL))[0]
            assert ref.same_bits(out.reshape(n, nx), want), (n, halo is not None, "out of place")
            inp = run(handle, "time_transform", kind=kind, n=n, nx=nx, in_place=1, lo_halo=glo,
                      hi_halo=ghi, y=x)[0]
            assert ref.same_bits(inp.reshape(n, nx), want), (n, halo is not None, "in place")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_halo", (False, True), ids=("bare", "halo"))
def test_time_transform_pieces_give_the_whole(handle, kind, with_halo):
    """What a time shard computes: ``n`` = 6 levels cut at every place, each piece with the halo
    the whole provides -- the neighbour's raw level for ``T_1`` / ``T_2``, its finished one for the
    inverses."""
    n, nx = 6, 257
    x = _levels(n, nx, 8)
    h = ref.real_data(nx, 9) if with_halo else None
    lo, hi = (h, None) if kind in (2, 4) else (None, h)

    def dev(xp, lo_, hi_):
        return run(handle, "time_transform", kind=kind, n=len(xp), nx=nx, x=xp, lo_halo=lo_,
                   hi_halo=hi_, y=np.full(xp.size, FILL))[0].reshape(len(xp), nx)

    whole = dev(x, lo, hi)
    assert ref.same_bits(whole, ref.time_transform(kind, x, lo, hi))
    for cut in range(1, n):
        (lo_a, hi_a), (lo_b, hi_b) = ref.split_halos(kind, x, whole, cut, lo, hi)
        assert ref.same_bits(dev(x[:cut], lo_a, hi_a), whole[:cut]), cut
        assert ref.same_bits(dev(x[cut:], lo_b, hi_b), whole[cut:]), cut


# --------------------------------------------------------------------- mask_blocks
@pytest.mark.parametrize("nx", (1, 16383, 16384, 16385, 40001), ids=lambda v: f"nx{v}")
@pytest.mark.parametrize("nb", (1, 5), ids=lambda v: f"blocks{v}")
def test_mask_blocks(handle, nb, nx):
    """Out of place and in place (``system.cpp`` calls ``launch_mask_blocks(stream, d_y, d_y, ...)``);
    masked entries without ``mx`` are ``+0.0`` -- the comparison is on bits, and the data holds
    negative values and ``-0.0`` at masked places."""
    x = np.array(_levels(nb, nx, 10))
    mxv = _levels(nb, nx, 11)
    x[:, 0] = -0.0
    alpha = -1.5 + np.arange(nb) * 0.75
    for form in ("scattered", "all", "none_set", "null"):
        m, _, mlist = _masks(nb, nx, form, 12)
        has = None
        if form == "scattered" and nb > 1:
            has = np.ones(nb, dtype=np.int32)
            has[2] = 0                                  # one block with a null mask
            mlist[2] = None
        for mx in (None, mxv):
            want = ref.mask_blocks(x, mx, mlist, alpha)
            if mx is None and form in ("scattered", "all"):
                assert not np.any(np.signbit(want[0][mlist[0]]))
            out = run(handle, "mask_blocks", n=nb, nx=nx, x=x, x2=mx, mask=m, has_mask=has,
                      alpha=alpha, y=np.full(nb * nx, FILL))[0]
            assert ref.same_bits(out.reshape(nb, nx), want), (form, mx is not None, "out of place")
            inp = run(handle, "mask_blocks", n=nb, nx=nx, in_place=1, x2=mx, mask=m, has_mask=has,
                      alpha=alpha, y=x)[0]
            assert ref.same_bits(inp.reshape(nb, nx), want), (form, mx is not None, "in place")


# ------------------------------------------------------- ConstantNullspace corrections
CONST_NX = (1, 2, 255, 256, 257, 2047, 2048, 2049, 2305, 16385, 50001)


def _jobs(nx, njobs, exact):
    """Job lists: odd offsets, untouched ranges between the jobs; with four jobs the lengths
    differ and the longest is not the first.  ``exact``: coefficients that are powers of two (with
    integer data every product and sum is exact); else those of the drivers, ``-1 / nx``,
    ``1 / nx`` and ``alpha / nx``."""
    lens = [nx] if njobs == 1 else [max(1, nx // 3), nx, 1, max(1, nx - 1)]
    jobs, off = [], 3
    for j, ln in enumerate(lens):
        if exact:
            cs = (-0.25 * (j + 1), 0.5 * (j + 1), -2.0 * (j + 1))
        else:
            cs = (-1.0 / ln, 1.0 / ln, (0.7 + 0.1 * j) / ln)
        jobs.append((off, ln) + cs)
        off += ln + 5
        off += 1 - off % 2
    return jobs, off + 4


def _job_arrays(jobs):
    cols = list(zip(*jobs))
    return dict(job_off=cols[0], job_nx=cols[1], job_c1=cols[2], job_c2_one=cols[3],
                job_c2_alpha=cols[4])


def _const_case(handle, nx, njobs, second, center, y0, b, jobs, length):
    """One launch: ``(out, sums_a, sums_b)``."""
    ja = _job_arrays(jobs)
    if center:
        xc0 = np.full(length, FILL)
        out, sums, _ = run(handle, "const_center", n=njobs, length=length, x=y0, y=xc0,
                           y2=np.full(njobs, FILL), **ja)
        return out, sums, None
    out, sums, _ = run(handle, "const_correct", kind=second, n=njobs, length=length, y=y0,
                       x2=b if second else None, y2=np.full(2 * njobs, FILL), **ja)
    # (without the second term the launch sums `a` only: the other half is not written)
    if not second:
        assert ref.same_bits(sums[njobs:], np.full(njobs, FILL))
    return out, sums[:njobs], sums[njobs:] if second else None


VARIANTS = ((0, False), (1, False), (2, False), (0, True))   # (second, const_center)


@pytest.mark.parametrize("nx", CONST_NX, ids=lambda v: f"nx{v}")
@pytest.mark.parametrize("njobs", (1, 4), ids=lambda v: f"jobs{v}")
def test_const_corrections_are_exact_on_integer_data(handle, njobs, nx):
    jobs, length = _jobs(nx, njobs, True)
    y0, b = ref.int_data(length, 13), ref.int_data(length, 14)
    for second, center in VARIANTS:
        out, sa, sb = _const_case(handle, nx, njobs, second, center, y0, b, jobs, length)
        want_a = [float(y0[o:o + ln].astype(np.int64).sum()) for o, ln, *_ in jobs]
        assert ref.same_bits(sa, want_a)
        want = np.full(length, FILL) if center else y0.copy()
        for j, (o, ln, c1, c2_one, c2_alpha) in enumerate(jobs):
            want[o:o + ln] = y0[o:o + ln] + c1 * want_a[j]
            if second:
                s_b = float(b[o:o + ln].astype(np.int64).sum())
                assert sb[j] == s_b
                want[o:o + ln] += (c2_alpha if second == 2 else c2_one) * s_b
        # (exact: |values| < 2^9 + 8 * 2^9 * 50001 < 2^53 with nothing below 2^-2)
        assert ref.same_bits(out, want), (second, center)


@pytest.mark.parametrize("nx", CONST_NX, ids=lambda v: f"nx{v}")
@pytest.mark.parametrize("njobs", (1, 4), ids=lambda v: f"jobs{v}")
def test_const_corrections_on_real_data(handle, njobs, nx):
    """Sums: the documented order bit for bit, and within ``gamma(ceil(nx / 256) + 8 + 1) sum |x|``
    of the correctly rounded exact sum.  Outputs: the rounded-product or the fused candidate, one
    of them for the whole launch; everything outside the jobs keeps its bits."""
    jobs, length = _jobs(nx, njobs, False)
    y0, b = ref.real_data(length, 15), ref.real_data(length, 16)
    worst = 0.0
    for second, center in VARIANTS:
        out, sa, sb = _const_case(handle, nx, njobs, second, center, y0, b, jobs, length)
        for vec, got in ((y0, sa),) + (((b, sb),) if second else ()):
            assert ref.same_bits(got, ref.const_jobs_sums(vec, jobs)), (second, center, "order")
            for j, (o, ln, *_) in enumerate(jobs):
                bound = ref.gamma(ref.sum_depth(ln) + 1) * ref.exact_sum(np.abs(vec[o:o + ln]))
                err = abs(got[j] - ref.exact_sum(vec[o:o + ln]))
                worst = max(worst, err / bound)
                assert err <= bound, (second, center, j, err / bound)
        start = np.full(length, FILL) if center else y0
        rounded, fused = ref.shift_candidates(y0, start, jobs, sa, second, sb)
        is_r, is_f = ref.same_bits(out, rounded), ref.same_bits(out, fused)
        tell = "both" if is_r and is_f else "rounded" if is_r else "fused" if is_f else "neither"
        print(f"const nx{nx} jobs{njobs} second{second} center{int(center)}: candidate {tell}; "
              f"elements where the candidates differ {np.count_nonzero(rounded != fused)}")
        assert is_r or is_f, (second, center)
    print(f"const nx{nx} jobs{njobs}: largest sum error / bound {worst:.4f}")


# -------------------------------------------------------------------- value arrays
VAL_N = (1, 255, 256, 257, 524288, 524289, 1048577)


@pytest.mark.parametrize("n", VAL_N, ids=lambda v: f"n{v}")
def test_csr_to_sell_and_mask_columns(handle, n):
    rng = np.random.default_rng([ref.SEED, n, 17])
    ncsr = max(1, (2 * n) // 3)
    csr = ref.real_data(ncsr, 18)
    csr[0] = -0.0
    maps = {"permutation with padding": np.where(rng.random(n) < 0.25, -1,
                                                 rng.permutation(max(n, ncsr))[:n] % ncsr),
            "repeated sources": rng.integers(0, min(ncsr, 3), size=n),
            "padding only": np.full(n, -1)}
    maps["permutation with padding"][[0, -1]] = [ncsr - 1, -1] if n > 1 else [-1]
    for name, m in maps.items():
        got = run(handle, "csr_to_sell", nx=n, length=ncsr, x=csr, idx=m, y=np.full(n, FILL))[0]
        assert ref.same_bits(got, ref.csr_to_sell(csr, m)), name
    ncols = max(2, n // 5)
    col = rng.integers(0, ncols, size=n)
    col[0], col[-1] = 0, ncols - 1
    vals = ref.real_data(n, 19)
    for name, cm in (("first and last", np.zeros(ncols, dtype=np.uint8)),
                     ("none", np.zeros(ncols, dtype=np.uint8)),
                     ("scattered", (rng.random(ncols) < 0.4).astype(np.uint8) * 200)):
        if name == "first and last":
            cm[0] = cm[ncols - 1] = 1
        got = run(handle, "mask_columns", nx=n, length=ncols, idx=col, mask=cm, y=vals)[0]
        want = ref.mask_columns(vals, col, cm)
        assert ref.same_bits(got, want), name
        if name == "first and last":
            assert ref.bits(got[0]) == 0 and ref.bits(got[-1]) == 0       # +0.0


@pytest.mark.parametrize("n", VAL_N, ids=lambda v: f"n{v}")
def test_vals_axpy_keeps_two_roundings(handle, n):
    """``round(a + round(c b))``.  For ``c`` = 1/3 the fused result differs from it at a share of the
    entries that is checked to be non-zero here, so a contracted kernel could not pass."""
    a, b = ref.real_data(n, 20), ref.real_data(n, 21)
    for c in (0.0, 1.0, -0.5, 1.0 / 3.0):
        for av in (a, None):
            want = ref.vals_axpy(av, c, b)
            got = run(handle, "vals_axpy", nx=n, c=c, x=av, x2=b, y=np.full(n, FILL))[0]
            assert ref.same_bits(got, want), (c, av is not None)
    if n >= 255:
        fused = ref.vals_axpy_fused(a, 1.0 / 3.0, b)
        share = np.count_nonzero(ref.bits(fused) != ref.bits(ref.vals_axpy(a, 1.0 / 3.0, b))) / n
        assert share > 0.05, share


@pytest.mark.parametrize("n", VAL_N, ids=lambda v: f"n{v}")
def test_vals_differ(handle, n):
    a = ref.real_data(n, 22)
    a[n // 2] = np.nan

    def flag(u, v, start=0):
        return run(handle, "vals_differ", nx=n, x=u, x2=v, flag=start)[2]

    assert flag(a, a.copy()) == 0                        # equal, identical NaN bits included
    assert flag(a, a.copy(), 1) == 1                     # a set flag stays
    for p in sorted({0, n - 1, 524288} & set(range(n))):
        if p == n // 2:
            continue
        b = a.copy()
        b[p] = np.nextafter(b[p], np.inf)
        assert flag(a, b) == 1, p
        b = a.copy()
        b[p] = 0.0
        z = a.copy()
        z[p] = -0.0
        assert flag(z, b) == 1, ("zero signs", p)
    b = a.copy()
    b[n // 2] = (np.array([np.nan]).view(np.int64) ^ 1).view(np.float64)[0]     # another NaN
    assert flag(a, b) == 1


def _involution(n, seed):
    """A transpose map of ``n`` positions as a structurally symmetric pattern with padding gives
    it: pairs ``t[p] = q, t[q] = p``, fixed points (diagonal entries), ``-1`` (padding)."""
    rng = np.random.default_rng([ref.SEED, n, seed])
    t = np.arange(n, dtype=np.int32)
    order = rng.permutation(n)
    k = (n // 5) * 2                       # two fifths paired, a fifth padding, the rest diagonal
    t[order[0:k:2]], t[order[1:k:2]] = order[1:k:2], order[0:k:2]
    t[order[k:k + n // 5]] = -1
    return t


@pytest.mark.parametrize("n", VAL_N, ids=lambda v: f"n{v}")
def test_vals_sym_skew(handle, n):
    def dev(a, t, start=0):
        h, sk, f = run(handle, "vals_sym_skew", nx=n, x=a, idx=t, y=np.full(n, FILL),
                       y2=np.full(n, FILL), flag=start)
        wh, wsk, wf = ref.vals_sym_skew(a, t, start)
        assert ref.same_bits(h, wh) and ref.same_bits(sk, wsk)
        assert f == wf
        return f

    t = _involution(n, 23)
    a = ref.real_data(n, 24)
    a[a == 0.0] = 1.0
    paired = np.flatnonzero((t >= 0) & (t != np.arange(n)))
    assert dev(a, t) == (1 if len(paired) else 0)         # a general matrix on the pattern
    sym = a.copy()
    sym[t >= 0] = 0.5 * (a[t >= 0] + a[t[t >= 0]])
    assert ref.same_bits(sym[t >= 0], sym[t[t >= 0]])
    assert dev(sym, t) == 0                               # symmetric
    assert dev(sym, t, 1) == 1                            # a set flag stays
    if not len(paired):
        return
    for p in sorted({int(paired[0]), int(paired[-1])}):   # (the last pair lies in the last trip)
        q = int(t[p])
        for rel, want in ((2e-12, 1), (0.5e-12, 0)):
            m = sym.copy()
            m[q] = ref.apart(m[p], rel)
            assert dev(m, t) == want, (p, rel)
        m = sym.copy()
        m[q] = 0.0                                         # asymmetric, an exact zero on one side
        assert dev(m, t) == 0, p
        m[q] = -0.0
        assert dev(m, t) == 0, p


def test_vals_sym_skew_on_a_matrix_pattern(handle):
    """The transpose map of a structurally symmetric CSR pattern laid out with padding entries."""
    indptr, indices, _ = ref.random_csr(40, 25)
    pairs = {(r, int(c)) for r in range(40) for c in indices[indptr[r]:indptr[r + 1]]}
    pairs |= {(c, r) for r, c in pairs}
    rows = [sorted(c for r2, c in pairs if r2 == r) for r in range(40)]
    ip = np.cumsum([0] + [len(r) for r in rows])
    ix = np.array([c for r in rows for c in r])
    t = ref.transpose_map(ip, ix)
    # every third position of the padded array is padding
    n = len(ix) + len(ix) // 2
    pos = np.flatnonzero(np.arange(n) % 3 != 2)[:len(ix)]
    n = int(pos[-1]) + 2
    tp = np.full(n, -1, dtype=np.int32)
    tp[pos] = pos[t]
    a = np.zeros(n)
    a[pos] = ref.real_data(len(ix), 26)
    h, sk, f = run(handle, "vals_sym_skew", nx=n, x=a, idx=tp, y=np.full(n, FILL),
                   y2=np.full(n, FILL), flag=0)
    wh, wsk, wf = ref.vals_sym_skew(a, tp)
    assert ref.same_bits(h, wh) and ref.same_bits(sk, wsk) and f == wf == 1


# -------------------------------------------------------------------- extract_dinv
@pytest.mark.parametrize("nrows", (1, 63, 64, 65, 127, 128, 129, 1000), ids=lambda v: f"rows{v}")
@pytest.mark.parametrize("R", (1, 2), ids=lambda v: f"R{v}")
@pytest.mark.parametrize("permuted", (False, True), ids=("natural", "perm"))
def test_extract_dinv(handle, permuted, R, nrows):
    C_ = 64 * R
    rng = np.random.default_rng([ref.SEED, nrows, R, int(permuted)])
    nslices = -(-nrows // C_) + (1 if permuted else 0)
    perm = None
    if permuted:
        perm = np.full(nslices * C_, -1)
        perm[np.sort(rng.permutation(nslices * C_)[:nrows])] = rng.permutation(nrows)
    extra = (np.arange(nslices) + 1) % 3                 # slices of differing widths, with padding
    last = nrows - 1
    for no_diag, pad_self in (((), True), ((nrows // 2,), False)):
        indptr, indices, data = ref.random_csr(nrows, 27, no_diag=no_diag, diag_last=(last, 0))
        S = ref.build_sell(indptr, indices, data, R, perm, extra, pad_self=pad_self)
        assert last in no_diag or indices[indptr[last + 1] - 1] == last
        # (the entry takes more rows than the layout places: the others must keep their bits)
        length = nrows + (3 if permuted else 0)
        masks = [None, (rng.random(length) < 0.3).astype(np.uint8) * 7]
        if no_diag:
            masks[1][no_diag[0]] = 0
            m3 = masks[1].copy()
            m3[no_diag[0]] = 1
            masks.append(m3)
        for rowmask in masks:
            want = ref.extract_dinv(S, rowmask, init=np.full(length, FILL))
            got = run(handle, "extract_dinv", kind=R, n=S["nslices"], length=length,
                      nx=len(S["col"]), idx=S["col"], idx2=S["slice_off"], x=S["vals"],
                      idx3=S["perm"], mask=rowmask, y=np.full(length, FILL))[0]
            assert ref.same_bits(got, want), (no_diag, rowmask is not None)
            assert np.all(np.isfinite(got))
            if no_diag and (rowmask is None or not rowmask[no_diag[0]]):
                assert got[no_diag[0]] == 1.0
            if rowmask is not None:
                assert np.all(got[:nrows][rowmask[:nrows] != 0] == 1.0)
            if permuted:
                assert ref.same_bits(got[nrows:], np.full(3, FILL))


# --------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_rejected(handle):
    lib, h = handle
    x = np.arange(1.0, 13.0)

    def rc(op, y=x, y2=None, flag=None, **kw):
        scal = {k: kw.pop(k) for k in ("kind", "in_place", "n", "nx", "c") if k in kw}
        if "length" in kw:
            scal["len"] = kw.pop("length")
        a, keep, gy, gy2, gf = _record(op, scal, kw, y, y2, flag)
        code = lib.kkt_debug_block_op(h, C.byref(a))
        if code:
            assert b"kkt_debug_block_op" in lib.kkt_last_error(h)
            # nothing was launched or uploaded: the array parts are as they went in
            assert gy is None or ref.same_bits(gy[G:-G], np.asarray(y, dtype=np.float64).ravel())
        return code

    tt = dict(kind=1, n=3, nx=4, x=x)
    assert rc("time_transform", **tt) == 0
    assert rc(99, **tt) == -1 and rc(-1, **tt) == -1
    assert lib.kkt_debug_block_op(h, None) == -1
    assert lib.kkt_debug_block_op(None, None) == -1
    assert rc("time_transform", **dict(tt, kind=0)) == -1
    assert rc("time_transform", **dict(tt, kind=5)) == -1
    assert rc("time_transform", **dict(tt, n=0)) == -1
    assert rc("time_transform", **dict(tt, n=-3)) == -1
    assert rc("time_transform", **dict(tt, nx=-4)) == -1
    assert rc("time_transform", **dict(tt, x=None)) == -1
    assert rc("time_transform", **dict(tt, x=None, in_place=1)) == 0
    assert rc("time_transform", y=None, **tt) == -1
    m = np.ones(12, dtype=np.uint8)
    al = np.ones(3)
    assert rc("time_transform_mask", **dict(tt, x2=x, mask=m, alpha=al)) == 0
    assert rc("time_transform_mask", **dict(tt, kind=3, x2=x, mask=m, alpha=al)) == -1
    assert rc("time_transform_mask", **dict(tt, mask=m, alpha=al)) == -1          # masked, no xin
    assert rc("time_transform_mask", **dict(tt, x2=x, mask=m)) == -1              # no alpha
    assert rc("time_transform_mask", **dict(tt, x2=x, mask=m, alpha=al, in_place=1)) == -1
    assert rc("mask_blocks", n=3, nx=4, x=x, mask=m) == -1
    assert rc("mask_blocks", n=3, nx=4, x=None) == -1
    jobs = dict(job_off=[1, 7], job_nx=[5, 5], job_c1=[1.0, 1.0], job_c2_one=[1.0, 1.0],
                job_c2_alpha=[1.0, 1.0])
    s = np.zeros(4)
    assert rc("const_correct", kind=0, n=2, length=12, y2=s, **jobs) == 0
    assert rc("const_correct", kind=0, n=2, length=11, y2=s, **jobs) == -1        # off + nx past the end
    assert rc("const_correct", kind=0, n=2, length=12, y2=s, **dict(jobs, job_off=[-1, 7])) == -1
    assert rc("const_correct", kind=0, n=2, length=12, y2=s, **dict(jobs, job_nx=[5, 0])) == -1
    assert rc("const_correct", kind=3, n=2, length=12, y2=s, **jobs) == -1
    assert rc("const_correct", kind=1, n=2, length=12, y2=s, **jobs) == -1        # second without b
    assert rc("const_correct", kind=0, n=2, length=12, **jobs) == -1              # no sums
    assert rc("const_correct", kind=0, n=2, length=12, y2=s, **dict(jobs, job_c1=None)) == -1
    assert rc("const_center", n=2, length=12, y2=s, **jobs) == -1                 # no x
    assert rc("const_center", n=0, length=12, x=x, y2=s, **jobs) == -1
    assert rc("csr_to_sell", nx=12, length=3, x=x[:3], idx=[0, 1, 2] * 4) == 0
    assert rc("csr_to_sell", nx=12, length=3, x=x[:3], idx=[0, 1, 3] * 4) == -1
    assert rc("csr_to_sell", nx=12, length=3, x=x[:3], idx=[0, 1, -2] * 4) == -1
    assert rc("mask_columns", nx=12, length=3, idx=[0, 1, -1] * 4, mask=m[:3]) == -1
    assert rc("mask_columns", nx=12, length=3, idx=[0, 1, 3] * 4, mask=m[:3]) == -1
    assert rc("vals_axpy", nx=12, c=1.0) == -1
    assert rc("vals_axpy", nx=0, c=1.0, x2=x) == -1
    assert rc("vals_differ", y=None, nx=12, x=x, x2=x) == -1                       # no flag
    assert rc("vals_sym_skew", nx=12, x=x, idx=[12] * 12, y2=x, flag=0) == -1
    assert rc("vals_sym_skew", nx=12, x=x, idx=[0] * 12, flag=0) == -1            # no sk
    off = np.array([0, 1], dtype=np.int32)
    col = np.zeros(64, dtype=np.int32)
    v = np.ones(64)
    d = np.zeros(5)
    ed = dict(kind=1, n=1, length=5, nx=64, idx=col, idx2=off, x=v)
    assert rc("extract_dinv", y=d, **ed) == 0
    assert rc("extract_dinv", y=d, **dict(ed, kind=3)) == -1
    assert rc("extract_dinv", y=d, **dict(ed, length=65)) == -1                   # more rows than positions
    assert rc("extract_dinv", y=d, **dict(ed, nx=128)) == -1
    assert rc("extract_dinv", y=d, **dict(ed, idx2=[1, 2])) == -1
    assert rc("extract_dinv", y=d, **dict(ed, idx3=[5] * 64)) == -1               # perm past the rows
