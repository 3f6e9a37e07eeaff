"""``tests/tile_level_ref.py`` without a GPU: the reference of the tile program's two-grid levels
against

* the CPU emulation of the kernel's scheme (``tests/native/tile_coarse_emu.cpp --dump``), bit for
  bit -- two restatements that agree before any GPU is involved: the emulator goes through the
  plan and ``build_tile_coarse_lists``, the reference is written from the definitions and is given
  only the rows each tile owns;
* the same recurrence in ``numpy.longdouble``, within the componentwise bound of
  ``structures.componentwise_ok`` for the roundings on its longest path;
* itself on one tile: the partition enters the bits of exactly the coarse functions that more than
  one tile touches.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import structures as st
import tile_level_ref as tl
from test_tile_coarse_plan import GRIDS, ROOT, build

DEPTHS, ITS, CYCLES = (1, 3), (4, 6), (1, 2, 3)


@pytest.fixture(scope="module")
def emu():
    return build(os.path.join(ROOT, "build", "tile_coarse_emu"), ["-O2"])


@pytest.fixture(scope="module")
def emu_sanitized():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    return build(os.path.join(ROOT, "build", "tile_coarse_emu_san"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def load_dump(path):
    """The arrays of ``tile_coarse_emu --dump`` (its header comment gives the layout)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"TCEMU01\0"
    at = [8]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a
    n, nc, nnz, nnzp, tiles, nlev, its, cycles, depth, W = (int(v) for v in take("<i4", 10))
    indptr, indices, mask = take("<i4", n + 1), take("<i4", nnz), take("u1", n).astype(bool)
    csr = lambda v: sp.csr_matrix((v, indices, indptr), shape=(n, n))
    lev = [dict(A=csr(take("<f8", nnz)), U=csr(take("<f8", nnz)), dinv=take("<f8", n),
                b=take("<f8", n), einv=take("<f8", nc * nc).reshape(nc, nc)) for _ in range(nlev)]
    coef = np.stack([take("<f8", its) for _ in range(3)], axis=1)
    ca, cy, post1, post2 = take("<f8", 4)
    p_ip = take("<i4", n + 1)
    p_ix = take("<i4", nnzp)
    P = sp.csr_matrix((take("<f8", nnzp), p_ix, p_ip), shape=(n, nc))
    own_ptr = take("<i4", tiles + 1)
    own_rows = take("<i4", int(own_ptr[-1]))
    own = [own_rows[own_ptr[t]:own_ptr[t + 1]] for t in range(tiles)]
    out = [take("<f8", n) for _ in range(nlev)]
    assert at[0] == len(raw)
    for l, L in enumerate(lev):
        L.update(coef=coef, post1=post1, post2=post2)
        if l == 0:
            del L["U"]             # the emulator's first level is a solo level
        else:
            L.update(ca=ca, cy=cy)
    return dict(levels=lev, mask=mask, P=P, own=own, its=its, cycles=cycles, depth=depth, W=W,
                out=out)


def dump(exe, grid, depth, its, cycles, path):
    nx, ny, nz, tiles, comps = grid
    args = [str(a) for a in (nx, ny, nz, tiles, depth, its, cycles, comps)] + ["--dump", str(path)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
    return load_dump(path)


def reference(d, **kw):
    # (the emulator applies whole rows of its dense stand-in for the coarse inverse)
    return tl.run(d["levels"], d["mask"], d["P"], d["own"], d["its"], d["cycles"], rows="full", **kw)


@pytest.mark.parametrize("grid", GRIDS)
def test_reference_equals_the_emulated_kernel_bit_for_bit(emu, grid, tmp_path):
    for depth in DEPTHS:
        for its in ITS:
            for cycles in CYCLES:
                d = dump(emu, grid, depth, its, cycles, tmp_path / "run.bin")
                assert d["depth"] == depth and len(d["levels"]) == 2
                for l, (x, _) in enumerate(reference(d)):
                    assert np.array_equal(x, d["out"][l]) and not np.signbit(x[d["mask"]]).any(), \
                        (grid, depth, its, cycles, l, np.flatnonzero(x != d["out"][l])[:8])
                    assert np.isfinite(x).all() and np.abs(x).max() > 0


@pytest.mark.parametrize("grid", GRIDS)
def test_sanitized_emulator_dumps_the_same_run(emu, emu_sanitized, grid, tmp_path):
    a = dump(emu, grid, 3, 4, 2, tmp_path / "a.bin")
    b = dump(emu_sanitized, grid, 3, 4, 2, tmp_path / "b.bin")
    assert open(tmp_path / "a.bin", "rb").read() == open(tmp_path / "b.bin", "rb").read()
    assert all(np.array_equal(x, y) for x, y in zip(a["out"], b["out"]))


@pytest.mark.parametrize("grid", GRIDS)
def test_reference_within_the_componentwise_bound_of_the_exact_recurrence(emu, grid, tmp_path):
    """|x - x*| <= (k + 2) u m + u |x*| per row, with x* the recurrence in extended precision, m its
    majorant (absolute values everywhere, subtractions added) and k the roundings on the longest
    path: the bound of structures.componentwise_ok with the majorant in the place of |A||x|."""
    for depth, its, cycles in ((1, 4, 1), (3, 6, 3)):
        d = dump(emu, grid, depth, its, cycles, tmp_path / "run.bin")
        args = (d["levels"], d["mask"], d["P"], d["own"], d["its"], d["cycles"])
        exact, major = tl.run_exact(*args), tl.run_exact(*args, majorant=True)
        for l, ((x, _), (xs, k), (m, _)) in enumerate(zip(reference(d), exact, major)):
            ratio = st.componentwise_ok(x, xs.astype(np.float64), m.astype(np.float64), k)
            assert ratio <= 1.0, (grid, depth, its, cycles, ratio)
            # The majorant of a recurrence grows with every sweep (it is the recurrence of the
            # absolute values, which does not contract), so the bound says most on a short level:
            # on one cycle of four sweeps it must lie below the 1e-10 to which the GPU tests hold
            # the two-grid tile form against the oracle, or it would add nothing to them.
            if (its, cycles, l) == (4, 1, 0):
                assert ((k + 2) * st.U * m.astype(np.float64)).max() < 1e-10 * np.abs(x).max()


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2], GRIDS[3]])
def test_the_partition_enters_the_bits_only_through_shared_coarse_functions(emu, grid, tmp_path):
    """One tile that owns every row, in the order of the tiles' lists one after the other: the
    restriction lists of a coarse function that a single tile touches are then the same, so its
    coarse residual is; a function that several tiles touch is summed lane-strided over one long
    list instead of tile by tile.  This states that the partition enters the bits -- it is not a
    weakness of the reference."""
    nx, ny, nz, _, comps = grid
    d = dump(emu, grid, 1, 4, 1, tmp_path / "run.bin")
    # tiles of this test's own making: slabs of the first coordinate, cut between coarse nodes, so
    # that the coarse functions around a node inside a slab belong to that slab alone
    rows = np.flatnonzero(~d["mask"])
    i = (rows // comps) % nx
    cut = 8 if nx > 9 else 4
    own = [rows[i < cut], rows[i >= cut]]
    one = [np.concatenate(own)]
    args = (d["levels"][:1], d["mask"], d["P"])
    t_many, t_one = [], []
    many = tl.run(*args, own, d["its"], 1, rows="full", trace=t_many)
    single = tl.run(*args, one, d["its"], 1, rows="full", trace=t_one)
    shared = tl.Restriction(d["P"], own).shared()
    alone = np.setdiff1d(np.arange(d["P"].shape[1]), shared)
    touched = np.flatnonzero(np.diff(sp.csc_matrix(d["P"]).indptr) > 0)
    alone = np.intersect1d(alone, touched)
    assert len(shared) and len(alone)
    rc_many, rc_one = t_many[0][2], t_one[0][2]
    assert np.array_equal(rc_many[alone], rc_one[alone])
    assert (rc_many[shared] != rc_one[shared]).any()
    rel = np.abs(rc_many - rc_one).max() / np.abs(rc_one).max()
    assert rel < 64 * st.U
    assert not np.array_equal(many[0][0], single[0][0])
    assert np.abs(many[0][0] - single[0][0]).max() < 1e-12 * np.abs(single[0][0]).max()
