"""The one Chebyshev coefficient function of the library (control_amd/csrc/chebyshev.hpp), bit for
bit against the two independent statements of the recurrence: ``oracle.kkt_oracle.
chebyshev_ellipse_coefficients`` for a spectrum inside an ellipse (``eimag > 0``, Manteuffel's form)
and ``tests/stokes_stage_ref.xp_cheb_coefficients`` evaluated in float64 for a real interval
(PETSc's form).  Every plain launch, interleaved step, tile program and pressure-space chain takes
its ``(c1, c2, c3)`` from this function, and the tile forms equal the plain forms bit for bit only
because they do.  tests/native/cheb_coefficients.cpp prints the function's doubles as words; it is
built with g++ at test time as the library's host code is (``-O3``, plain x86-64, so no fused
multiply-add), and the header is compiled without any HIP include path.  Host-only.

Degrees: 1 (none), 2 (one coefficient triple), 3, 8, 20, 80 and 600 (the most the K_p solve takes); intervals:
the mass solves' [0.25, 2], [emax / 30, emax] and the benchmark's Schur and K_p intervals up to
kappa = 1.05e4; ellipses with the imaginary semi-axis below and above the real one (``c^2 < 0``)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import stokes_stage_ref as ssr
from oracle.kkt_oracle import chebyshev_ellipse_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "cheb_coefficients.cpp")

DEGREES = (1, 2, 3, 8, 20, 80, 600)
INTERVALS = ((0.25, 2.0), (2.1 / 30, 2.1), (0.07, 2.1), (0.0007, 2.1), (0.0002, 2.1))
# (emin, emax, eimag): real semi-axes 1.015, 0.875 (eimag larger: c^2 < 0), 1.0499, 0.875
ELLIPSES = ((0.07, 2.1, 0.3), (0.25, 2.0, 1.5), (0.0002, 2.1, 0.05), (0.25, 2.0, 0.875))
CASES = ([(its, lo, hi, 0.0) for lo, hi in INTERVALS for its in DEGREES] +
         [(its, lo, hi, im) for lo, hi, im in ELLIPSES for its in DEGREES])


def word(x):
    return struct.pack(">d", float(x)).hex()


def build(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + extra + [SRC, "-o", exe])
    return exe


def run(exe):
    """{case: [scale, c1, c2, c3, c1, ...] as words}"""
    args = [a for its, lo, hi, im in CASES for a in (str(its), word(lo), word(hi), word(im))]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES) and all(ln.startswith("coef ") for ln in lines)
    return {c: ln.split()[1:] for c, ln in zip(CASES, lines)}


@pytest.fixture(scope="module")
def expected():
    """The references' coefficients as words, computed once."""
    out, xp = {}, ssr.XP
    ssr.XP = np.float64          # xp_cheb_coefficients "evaluated in float64"
    try:
        for case in CASES:
            its, lo, hi, im = case
            if im > 0.0:
                scale = 1.0 / (0.5 * (hi + lo))      # "p_1 = (1 / d) D^-1 b"
                coefs = chebyshev_ellipse_coefficients(lo, hi, im, its)
            else:
                scale, coefs = ssr.xp_cheb_coefficients(lo, hi, its)
                assert isinstance(scale, np.float64)
            assert len(coefs) == max(its - 1, 0)
            out[case] = [word(scale)] + [word(c) for triple in coefs for c in triple]
    finally:
        ssr.XP = xp
    return out


def compare(got, expected):
    triples = 0
    for case in CASES:
        g, e = got[case], expected[case]
        assert len(g) == len(e), case
        differ = [i for i in range(len(g)) if g[i] != e[i]]
        assert not differ, (case, "words that differ (0: scale, then c1 c2 c3 per step)", differ[:6])
        triples += (len(g) - 1) // 3
    assert triples == sum(max(its - 1, 0) for its, _, _, _ in CASES)


def test_negative_c2_case_is_present():
    lo, hi, im = ELLIPSES[1]
    assert (0.5 * (hi - lo)) ** 2 - im * im < 0.0


def test_coefficients_bit_for_bit(expected):
    compare(run(build(os.path.join(ROOT, "build", "cheb_coefficients"), ["-O3"])), expected)


def test_coefficients_are_clean_under_sanitizers(expected):
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    compare(run(build(os.path.join(ROOT, "build", "cheb_coefficients_san"),
                      ["-O1", "-g", "-fsanitize=address,undefined",
                       "-fno-sanitize-recover=undefined"])), expected)
