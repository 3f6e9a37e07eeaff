"""Regenerate ``schur_pc_definition.npz``: for every case of ``tests/schur_pc_cases.py`` with
explicit intervals and every input of it, the extended-precision reference of the Schur
preconditioner's application (``tests/schur_pc_ref.py``, 50 digits) as ``hi`` (float64) + ``lo``
(float32) per variable and level, and ``d``: the per-block distance of the float64 oracle
(``oracle/kkt_oracle.py``) from it.  The device test reads both; the host test recomputes them.

    python tests/golden/make_schur_pc_definition.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import schur_pc_cases as sc  # noqa: E402
import schur_pc_ref as ref  # noqa: E402


def entry(c, x, dps=None):
    """``(hi, lo, d)`` of one case and input: reference ``(2, m, nx)`` and oracle distance."""
    x0, x1 = sc.split(c, x)
    u0, u1 = sc.reference(c, dps=dps).apply(x0, x1)
    (h0, l0), (h1, l1) = ref.to_pairs(u0), ref.to_pairs(u1)
    d = sc.distance(c, sc.oracle_apply(c, x), h0, l0, h1, l1)
    return np.stack([h0, h1]), np.stack([l0, l1]).astype(np.float32), d


def main():
    out = {}
    for c in sc.CASES:
        for name, x in sc.inputs(c).items():
            hi, lo, d = entry(c, x)
            k = sc.case_id(c) + "/" + name
            out[k + "/hi"], out[k + "/lo"], out[k + "/d"] = hi, lo, np.float64(d)
            print(f"{k:48s} d_case {d:.2e}", flush=True)
    np.savez_compressed(sc.golden_path(), **out)
    print(f"{sc.golden_path()}: {os.path.getsize(sc.golden_path())} bytes")


if __name__ == "__main__":
    main()
