"""The vector kernels of the Krylov loops against exact references, one operation at a time
through ``kkt_debug_krylov_op``: ``System::mdot`` (``mdot_stage1<NV>`` / ``mdot_stage2``),
``System::orthogonalise`` (the Gram-Schmidt step ``solve_once`` calls: the multi-dot, the grouped
``maxpy`` passes, ``maxpy_norm`` for the last group, ``norm2_finish``), ``System::maxpy_groups``
(the solution update of KSPGMRESBuildSoln), ``scale_inv``, ``axpby``, ``copy``, ``fill`` and
``System::norm2``.  References: ``tests/krylov_ref.py`` (checked on the host by
``tests/test_krylov_ref.py``).

Sizes -- each the smallest that reaches its regime of the reduction (``REDUCE_BLOCKS`` = 1024
chunks of ``(ceil(n / 1024) + 1) & ~1`` elements, ``double2`` pairs at stride 512 per workgroup,
a scalar tail for an odd last element) and of the elementwise grids (at most 2048 x 256 threads):

    1, 2, 3                    one workgroup with work, with and without the scalar tail
    2047, 2048, 2049           chunk 2 -> 4, the first workgroups whose chunk starts past n
    2421                       odd n at the size of the step-locked parity test
    65537                      a middle size, odd
    524287, 524288, 524289     chunk 512 -> 514: the second trip of the strided loop in thread 0,
                               the first grid-stride trip of the elementwise kernels
    1536001                    chunk 1502: two full trips and a ragged third, an empty last
                               workgroup, the scalar tail at an even thread offset

What is asserted: on integer data every result bit for bit against ``int64`` arithmetic; on real
data each inner product within ``gamma(dot_depth(n) + 1) sum |w_p v_p|`` of the correctly rounded
exact one (``gamma(k) = k u / (1 - k u)``, ``dot_depth`` counted from the launch constants, +1 for
the reference's own rounding: no further factor), the update bit for bit against the fused
multiply-add chain evaluated in ``Fraction`` arithmetic with the device's own coefficients, the
squared norm and ``tt`` against the exact norm of the downloaded vector; that ``maxpy_norm``
leaves the bits a separate ``mdot(w, w)`` and plain ``maxpy`` passes would; that every operation
gives identical bits when repeated; and that the basis vectors and the padding between the
vectors (set to ``KKT_KRYLOV_PAD`` by the entry) are as they were.

Measured on an MI355X (gfx950), real data: largest error / bound of an inner product 0.083
(``n`` = 2049 and 65537, 8 and 9 vectors; depth 23), of the squared norm after the step 0.057 and
of ``tt`` 0.084 (``n`` = 2421, 17 vectors); several results are the correctly rounded value
itself (ratio 0).  The worst-case bound is far from attained, as it should be for sums whose
errors do not line up; what it would catch is a lost, doubled or misplaced summand of visible
size, which the integer cases catch at any size.  213 cases in 17 s.
"""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_ref as ref
from control_amd import _lib

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 3, 2047, 2048, 2049, 2421]
LARGE = [65537, 524287, 524288, 524289, 1536001]
SIZES = SMALL + LARGE
# one pass; seven of eight; exactly one full group; 8 + 1; 8 + 8; 8 + 8 + 1; 24 + 1; 24 + 6
NV_ALL, NV_SMALL = [1, 2, 7, 8, 9], [16, 17, 25, 30]
CASES = [(n, nv) for n in SIZES for nv in NV_ALL] + [(n, nv) for n in SMALL for nv in NV_SMALL]
REAL_DOTS = [(n, nv) for n in (3, 2049, 2421, 65537) for nv in (1, 8, 9)] + [(1536001, 2)]
REAL_STEP = [(n, nv) for n in (3, 2049, 2421) for nv in (1, 8, 9)] + [(2421, 17), (2421, 30)]
U = ref.U


def _id(c):
    return f"n{c[0]}-nv{c[1]}"


@pytest.fixture(scope="module")
def handle():
    """A created handle and nothing else: the entry does not depend on a layout."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0, lib.kkt_last_error(None)
    yield lib, h
    assert lib.kkt_destroy(h) == 0


def _call(handle, op, w, V, coef, a, b):
    lib, h = handle
    n, nv = len(w), len(V)
    w, pw = _lib.f64(w)
    V, pV = _lib.f64(V)
    coef, pc = _lib.f64(np.zeros(nv) if coef is None else coef)
    w_out, scalars = np.full(n, np.nan), np.full(nv + 2, np.nan)
    arena = np.full((nv + 1, ref.stride(n)), np.nan)
    rc = lib.kkt_debug_krylov_op(h, _lib.KRYLOV_OPS[op], n, nv, pw, pV if nv else None, pc, a, b,
                                 _lib.f64(w_out)[1], _lib.f64(scalars)[1], _lib.f64(arena)[1])
    assert rc == 0, (op, n, nv, lib.kkt_last_error(h))
    return w_out, scalars, arena


def run(handle, op, w, V=(), coef=None, a=0.0, b=0.0):
    """``(w_out, scalars)`` of one operation -- run twice (identical bits), with the basis vectors
    and every padding element of the allocation checked against what went in."""
    V = np.asarray(V, dtype=np.float64).reshape(len(V), len(w))
    w_out, scalars, arena = _call(handle, op, w, V, coef, a, b)
    again = _call(handle, op, w, V, coef, a, b)
    for x, y in zip((w_out, scalars, arena), again):
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), (op, "not reproducible")
    n = len(w)
    assert np.array_equal(arena[0, :n].view(np.int64), w_out.view(np.int64))
    assert np.array_equal(arena[1:, :n].view(np.int64), V.view(np.int64)), (op, "V was written")
    assert np.all(arena[:, n:] == _lib.KRYLOV_PAD), (op, "padding was written")
    return w_out, scalars


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------ integer data
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_reductions_and_updates_are_exact_on_integer_data(handle, c):
    n, nv = c
    w, V = ref.int_data(n, nv, 0)
    wi, Vi = w.astype(np.int64), V.astype(np.int64)
    w_out, s = run(handle, "mdot", w, V)
    assert _same_bits(w_out, w)
    assert np.array_equal(s[:nv], Vi @ wi) and np.all(s[nv:] == 0)

    # KSPGMRESBuildSoln and the plain passes with the other sign
    coef = np.array([(-1) ** i * (1 + i % 8) for i in range(nv)], dtype=np.float64)
    upd = coef.astype(np.int64) @ Vi
    assert np.array_equal(run(handle, "build_solution", w, V, coef)[0], wi + upd)
    assert np.array_equal(run(handle, "maxpy", w, V, coef, a=-1.0)[0], wi - upd)

    # the Gram-Schmidt step, in the range that keeps ||w_out||^2 below 2^53
    w, V = ref.int_data(n, nv, 0, ref.orth_amp(n, nv, 0))
    h, want, sq = ref.int_orthogonalise(w, V)
    w_out, s = run(handle, "orthogonalise", w, V)
    assert np.array_equal(s[:nv], h), "h"
    assert np.array_equal(w_out, want), "w_out"
    assert 0 < sq < 2 ** 53 and s[nv + 1] == sq, "squared norm"
    assert abs(s[nv] - math.sqrt(sq)) <= 2 * U * math.sqrt(sq), "tt"


@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_elementwise_kernels_are_exact_on_integer_data(handle, n):
    w, V = ref.int_data(n, 1, 1)
    w_out, s = run(handle, "copy", w, V)
    assert _same_bits(w_out, V[0]) and np.all(s == 0)
    assert _same_bits(run(handle, "copy", w)[0], w)           # y == x: nothing is launched
    assert _same_bits(run(handle, "fill", w, V, a=-7.0)[0], np.full(n, -7.0))
    assert _same_bits(run(handle, "fill", w, a=0.0)[0], np.zeros(n))
    assert np.array_equal(run(handle, "axpby", w, V, a=3.0, b=-5.0)[0], 3 * V[0] - 5 * w)
    assert np.array_equal(run(handle, "axpby", w, V, a=-1.0, b=1.0)[0], w - V[0])
    assert np.array_equal(run(handle, "axpby", w, V, a=0.25, b=0.0)[0], V[0] / 4)
    assert _same_bits(run(handle, "scale_inv", w, a=4.0)[0], w / 4)
    w_out, s = run(handle, "norm2", w)
    sq = int(w.astype(np.int64) @ w.astype(np.int64))
    assert _same_bits(w_out, w) and s[1] == sq
    assert abs(s[0] - math.sqrt(sq)) <= 2 * U * math.sqrt(sq)


# --------------------------------------------------------------------------------- real data
@pytest.mark.parametrize("c", REAL_DOTS, ids=_id)
def test_inner_products_are_within_the_rounding_bound(handle, c):
    n, nv = c
    w, V = ref.real_data(n, nv, 0)
    got = run(handle, "mdot", w, V)[1][:nv]
    exact, scale = ref.exact_dots(w, V), ref.abs_dots(w, V)
    bound = ref.gamma(ref.dot_depth(n) + 1) * scale
    err = np.abs(got - exact)
    print(f"dots {_id(c)}: depth {ref.dot_depth(n)} largest error / bound {np.max(err / bound):.4f}")
    assert np.all(err <= bound), (err / bound).tolist()


@pytest.mark.parametrize("c", REAL_STEP, ids=_id)
def test_gram_schmidt_step_on_real_data(handle, c):
    n, nv = c
    w, V = ref.real_data(n, nv, 0)
    w_out, s = run(handle, "orthogonalise", w, V)
    h, tt, sq = s[:nv], s[nv], s[nv + 1]
    g = ref.gamma(ref.dot_depth(n) + 1)
    assert np.all(np.abs(h - ref.exact_dots(w, V)) <= g * ref.abs_dots(w, V))
    # the update: the documented chain with the device's own h, bit for bit
    assert _same_bits(w_out, ref.maxpy_exact(w, V, h, -1.0))
    if n >= nv:
        assert np.linalg.norm(w_out) < 1e-6 * np.linalg.norm(w)      # (the data cancels)
    # the norm of the vector the device holds (all summands >= 0: the bound is relative)
    sq_exact = ref.exact_dots(w_out, [w_out])[0]
    norm = float(np.sqrt(np.longdouble(sq_exact)))
    e_sq, e_tt = abs(sq - sq_exact) / sq_exact, abs(tt - norm) / norm
    print(f"step {_id(c)}: ||w_out|| / ||w|| {norm / np.linalg.norm(w):.1e}; squared norm error / "
          f"bound {e_sq / g:.4f}; tt error / bound {e_tt / (g / 2 + 2 * U):.4f}")
    assert e_sq <= g
    assert e_tt <= g / 2 + 2 * U
    # normalisation: the reciprocal rounded, then one product per element
    assert _same_bits(run(handle, "scale_inv", w_out, a=tt)[0], w_out * (1.0 / tt))


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_fused_norm_equals_separate_passes(handle, c):
    """``maxpy_norm`` "gives bitwise the norm a separate pass would give": the squared norm of the
    step equals ``mdot(w_out, w_out)`` of another call, and ``w_out`` equals what the plain
    ``maxpy`` passes make of the same ``h`` -- on data whose sums round at every step."""
    n, nv = c
    w, V = ref.real_data(n, nv, 1, orthonormal=False)
    w_out, s = run(handle, "orthogonalise", w, V)
    h = s[:nv]
    assert _same_bits(h, run(handle, "mdot", w, V)[1][:nv])
    assert np.all(np.isfinite(w_out)) and s[nv + 1] > 0
    assert _same_bits(run(handle, "mdot", w_out, [w_out])[1][0], s[nv + 1])
    assert _same_bits(run(handle, "norm2", w_out)[1], s[nv:nv + 2][:2])
    assert _same_bits(run(handle, "maxpy", w, V, h, a=-1.0)[0], w_out)


# --------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_rejected(handle):
    lib, h = handle
    x = np.ones(4)
    px = _lib.f64(x)[1]
    s = np.zeros(3)
    ps = _lib.f64(s)[1]
    op = _lib.KRYLOV_OPS["mdot"]
    call = lib.kkt_debug_krylov_op
    assert call(h, op, 0, 1, px, px, px, 0.0, 0.0, px, ps, None) == -1
    assert call(h, op, -4, 1, px, px, px, 0.0, 0.0, px, ps, None) == -1
    assert call(h, op, 4, -1, px, px, px, 0.0, 0.0, px, ps, None) == -1
    assert call(h, op, 4, 1, None, px, px, 0.0, 0.0, px, ps, None) == -1
    assert call(h, op, 4, 1, px, None, px, 0.0, 0.0, px, ps, None) == -1
    assert call(h, op, 4, 1, px, px, px, 0.0, 0.0, None, ps, None) == -1
    assert call(h, op, 4, 1, px, px, px, 0.0, 0.0, px, None, None) == -1
    assert call(h, _lib.KRYLOV_OPS["maxpy"], 4, 1, px, px, None, 1.0, 0.0, px, ps, None) == -1
    assert call(h, _lib.KRYLOV_OPS["orthogonalise"], 4, 0, px, None, None, 0.0, 0.0, px, ps, None) == -1
    assert call(h, 99, 4, 1, px, px, px, 0.0, 0.0, px, ps, None) == -1
    assert call(None, op, 4, 1, px, px, px, 0.0, 0.0, px, ps, None) == -1
    # and without the arena: the same results
    w, V = ref.int_data(4, 1, 3)
    out = np.zeros(4)
    assert call(h, op, 4, 1, _lib.f64(w)[1], _lib.f64(V)[1], None, 0.0, 0.0, _lib.f64(out)[1], ps,
                None) == 0
    assert s[0] == float(V[0] @ w) and _same_bits(out, w)
