"""The spectrum estimates of a preconditioner build in lock-step batches (option
``spectrum_batch``, csrc/spectrum.cpp, csrc/spectrum_kernels.hip) against the one-matrix path
(``spectrum_batch = 0``).

A batch runs, per matrix, the one-matrix loop's arithmetic in its order, so the contract is
equality: ``pc_solves()`` and ``pc_matrices()`` -- every field compared as bits: intervals,
semi-axes, degrees, the estimate kind, the Lanczos and power step counts, the twin a matrix shares
with, creation order -- and one ``pc_apply`` of the same vector are identical under batch sizes 1
(single-matrix batches), 3 (does not divide the counts) and 64 (larger than any count).  The
collection pass must have covered every matrix the build solved with: ``fallbacks == 0``.

Near-twins (case 2b): ``share=False`` copies of one level matrix of which one level differs in a
single diagonal value, by one ulp or by a factor two.  Which records are estimated and which
share, the interval each runs with, ``spectrum_stats()["matrices"]`` and, with a coarse space and
given intervals, the number of coarse inverses are held against the value sets counted on the
host (``spectrum_ref.value_key``): a comparison that took a near-twin for a twin would solve with
another matrix's interval or inverse.

The saving itself is asserted from ``spectrum_stats()``, without a clock: a batched Lanczos run
takes at most ceil(400 / 10) + 4 host synchronisations and the twin search at most 2 per build,
whatever the number of matrices.
"""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import common
import sharded_spectrum_worker as worker
import spectrum_ref
import test_gpu_sharded as base
from control_amd import picard
from control_amd.blocks import instationary_blocks
from control_amd.coarse import multilinear_coarse_space
from control_amd.fem import unit_square_p1
from test_gpu_coarse_setup import _convection_problem
from test_gpu_spectrum_estimates import _mms_convection_problem

pytestmark = pytest.mark.gpu

AUTO = (-1, 0.0, 0.0)
MASS = (20, 0.5, 2.0)
BATCHES = (1, 3, 64)
LANCZOS_STEPS = 400
LANCZOS_SYNCS = math.ceil(LANCZOS_STEPS / 10) + 4
TWIN_SYNCS = 2


def bits(records):
    """The records with every float as its bit pattern (so -0.0, NaN payloads and the last bit count)."""
    def one(v):
        return float(v).hex() if isinstance(v, (float, np.floating)) else v
    return [{k: one(v) for k, v in r.items()} for r in records]


def opts(nbatch):
    return {"spectrum_batch": str(nbatch)}


def heat_run(p, nbatch, coarse=None):
    g = common.gpu_system(p, options=opts(nbatch))
    y = g.pc_apply(common.rng_vector(g.local_size), common.gpu_pc(p, MASS, AUTO, coarse=coarse))
    out = dict(solves=g.pc_solves(), mats=g.pc_matrices(), stats=g.spectrum_stats(), y=y.tobytes())
    g.close()
    return out


def check_stats(name, nbatch, run, serial):
    st, n_est = run["stats"], sum(m["estimate"] == "lanczos" for m in serial["mats"])
    print(f"{name} spectrum_batch={nbatch}: {st}")
    assert st["fallbacks"] == 0, (name, nbatch, st)
    assert st["matrices"] == n_est, (name, nbatch, st)
    assert st["batches"] == math.ceil(n_est / nbatch), (name, nbatch, st)
    assert st["lanczos_steps"] == sum(m["lanczos"] for m in serial["mats"]), (name, nbatch, st)
    assert st["power_steps"] == sum(m["power"] for m in serial["mats"]), (name, nbatch, st)
    assert st["lanczos_syncs_max"] <= LANCZOS_SYNCS, (name, nbatch, st)
    assert st["twin_syncs"] <= TWIN_SYNCS, (name, nbatch, st)
    assert st["batch_bytes"] > 0 and st["launches"] > 0


def check_equal(name, runs):
    """runs: {nbatch: run}, 0 the one-matrix path."""
    serial = runs[0]
    assert serial["stats"]["batches"] == 0 and serial["stats"]["fallbacks"] == 0, serial["stats"]
    assert any(m["estimate"] == "lanczos" for m in serial["mats"]), name
    for nbatch, run in runs.items():
        if nbatch == 0:
            continue
        assert bits(run["mats"]) == bits(serial["mats"]), (name, nbatch)
        assert bits(run["solves"]) == bits(serial["solves"]), (name, nbatch)
        assert run["y"] == serial["y"], (name, nbatch, "pc_apply differs")
        check_stats(name, nbatch, run, serial)


def check_masking(name, serial):
    """The matrices of one batch (batch size 64: all of them) stop at different steps, so the
    `active` words are exercised: asserted on the one-matrix path's own records."""
    steps = [m["lanczos"] for m in serial["mats"] if m["estimate"] == "lanczos"]
    print(f"{name}: Lanczos steps per estimated matrix {steps}")
    assert len(set(steps)) >= 2, (name, steps)


def reaction_levels_problem(n=24, n_t=6, CN=False, beta=1e-4, growth=500.0):
    """``heat_problem(time_dependent=True)`` with a reaction term that grows 5 000 times faster,
    K_i = K + 500 i M: with the builder's 0.1 i M every level matrix stops its Lanczos run at the
    same step (60 on 24 x 24, measured on the one-matrix path), here they stop at 40, 50 and 60."""
    sd = unit_square_p1(n)
    tau = 2.0 / (n_t - 1.0)
    K = [sd.K + (growth * i) * sd.M for i in range(n_t)]
    b00, b01, b10, b11, m = instationary_blocks(sd.M, K, tau, beta, n_t, CN, share=True)
    return dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=sd.boundary)


@functools.lru_cache(maxsize=None)
def time_dependent_runs(CN, n_t=6, batches=(0,) + BATCHES):
    p = reaction_levels_problem(n_t=n_t, CN=CN)
    return {nb: heat_run(p, nb) for nb in batches}


# ---- case 1: every level its own matrix; 529 interior rows, chunks of 2 in the dot
@pytest.mark.parametrize("CN", [False, True], ids=["BE", "CN"])
def test_time_dependent_levels(CN):
    name = f"time-dependent p1 24 x 6 {'CN' if CN else 'BE'}"
    runs = time_dependent_runs(CN)
    check_equal(name, runs)
    check_masking(name, runs[0])


# ---- case 2: mode-G copies with equal values: every twin is found
def test_equal_copies_share_one_estimate():
    p = common.heat_problem(n=16, n_t=6, beta=1e-4, share=False)
    runs = {nb: heat_run(p, nb) for nb in (0,) + BATCHES}
    check_equal("share=False p1 16 x 6", runs)
    distinct = spectrum_ref.distinct_solved_matrices(p)
    for nb, run in runs.items():
        assert sum(m["estimate"] == "lanczos" for m in run["mats"]) == distinct, nb
        assert sum(m["estimate"] == "shared" for m in run["mats"]) > 0, nb
        assert run["stats"]["matrices"] == distinct, (nb, run["stats"])


# ---- case 2b: near-twins -- level matrices equal but for one stored value of one level.  Only the
# bit-for-bit comparison of the twin search stands between such a level and a shared interval or
# a shared coarse inverse.
NEAR_TWINS = ("first interior diagonal", "last interior diagonal", "dirichlet diagonal",
              "doubled diagonal")
NEAR_LEVEL = 2          # a level whose shift its neighbours have too (BE: 1 .. n_t - 2; CN: all)


def near_twin_problem(CN, variant):
    """``heat_problem(share=False)`` -- every level its own copy of the same values -- with one
    diagonal entry of level ``NEAR_LEVEL``'s matrices moved by one ulp (``doubled``: times two): of
    the first or last interior row, or of a Dirichlet row, which the boundary conditions remove."""
    p = common.heat_problem(n=16, n_t=6, beta=1e-4, CN=CN, share=False)
    nodes = np.asarray(p["nodes"])
    interior = np.setdiff1d(np.arange(p["sd"].n_dofs), nodes)
    row = int({NEAR_TWINS[0]: interior[0], NEAR_TWINS[1]: interior[-1], NEAR_TWINS[2]: nodes[0],
               NEAR_TWINS[3]: interior[len(interior) // 2]}[variant])
    for quadrant in (1, 2):
        blk = p["blocks"][quadrant][(NEAR_LEVEL, NEAR_LEVEL)]
        assert sp.isspmatrix_csr(blk)
        others = [b for key, b in p["blocks"][quadrant].items() if b is not None and key != (NEAR_LEVEL,) * 2]
        assert all(b is not blk and not np.shares_memory(b.data, blk.data) for b in others)
        lo, hi = blk.indptr[row], blk.indptr[row + 1]
        k = lo + int(np.flatnonzero(blk.indices[lo:hi] == row)[0])
        blk.data[k] = 2.0 * blk.data[k] if variant == NEAR_TWINS[3] else np.nextafter(blk.data[k], np.inf)
    return p


def solve_keys(p):
    """The identity of the values each sub-solve's matrix has after assembly, in emission order."""
    kind = "CN" if p["CN"] else "BE"
    return [spectrum_ref.value_key(spectrum_ref.assembled(blk, c, p["sd"].M, p["nodes"]), c)
            for _, _, blk, c in spectrum_ref.schur_solve_map(kind, p["blocks"], p["m"], p["tau"], p["beta"])]


def check_twins(name, run, keys, estimated):
    """The records against the host's value sets: the first matrix of a set is estimated, every
    later one shares -- with THAT matrix: all solves of a set run with one interval.  Returns
    ``({value set: its first matrix}, {first matrix: interval bits})``."""
    solves, mats = run["solves"], run["mats"]
    assert len(solves) == len(keys), name
    key_of = {}
    for s, k in zip(solves, keys):
        assert key_of.setdefault(s["matrix"], k) == k, (name, "one matrix record for two value sets")
    first = {}
    for m, rec in enumerate(mats):
        if m not in key_of:      # multiplied with only
            assert rec["solves"] == 0 and rec["estimate"] == "none", (name, m, rec)
            continue
        k = key_of[m]
        want = ("shared" if k in first else "lanczos") if estimated else "given"
        assert rec["estimate"] == want, (name, m, rec, want)
        first.setdefault(k, m)
    interval = {}
    for s in solves:
        iv = tuple(float(s[f]).hex() for f in ("emin", "emax", "eimag"))
        assert interval.setdefault(first[key_of[s["matrix"]]], iv) == iv, (name, s)
    return first, interval


def near_twin_counts(CN, variant, keys):
    """The number of value sets, from the host: one more than the unperturbed problem's, but for
    the Dirichlet entry."""
    base = spectrum_ref.distinct_solved_matrices(common.heat_problem(n=16, n_t=6, beta=1e-4, CN=CN,
                                                                      share=False))
    distinct = len(set(keys))
    assert distinct == base + (0 if variant == NEAR_TWINS[2] else 1), (variant, base, distinct)
    return distinct


@pytest.mark.parametrize("variant", NEAR_TWINS, ids=lambda v: v.replace(" ", "-"))
@pytest.mark.parametrize("CN", [False, True], ids=["BE", "CN"])
def test_near_twins_are_not_twins(CN, variant):
    name = f"near-twin {variant} {'CN' if CN else 'BE'}"
    p = near_twin_problem(CN, variant)
    keys = solve_keys(p)
    distinct = near_twin_counts(CN, variant, keys)
    runs = {nb: heat_run(p, nb) for nb in (0,) + BATCHES}
    check_equal(name, runs)
    for nb, run in runs.items():
        first, interval = check_twins(f"{name} batch {nb}", run, keys, True)
        assert len(first) == distinct
        assert run["stats"]["matrices"] == distinct, (nb, run["stats"])
        assert run["stats"]["fallbacks"] == 0
        if variant == NEAR_TWINS[3]:      # a false twin would also show in the interval
            assert interval[first[keys[NEAR_LEVEL]]] != interval[first[keys[NEAR_LEVEL - 1]]], nb


@pytest.mark.parametrize("variant", NEAR_TWINS, ids=lambda v: v.replace(" ", "-"))
@pytest.mark.parametrize("CN", [False, True], ids=["BE", "CN"])
def test_near_twins_do_not_share_a_coarse_inverse(CN, variant):
    """Two-grid sub-solves with given intervals: nothing is estimated, the twin search alone
    decides which matrices share a coarse inverse."""
    name = f"near-twin two-grid {variant} {'CN' if CN else 'BE'}"
    p = near_twin_problem(CN, variant)
    keys = solve_keys(p)
    distinct = near_twin_counts(CN, variant, keys)
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=4))
    runs = {}
    for nb in (0,) + BATCHES:
        g = common.gpu_system(p, options=opts(nb))
        y = g.pc_apply(common.rng_vector(g.local_size), common.gpu_pc(p, MASS, (4, 0.3, 1.9), coarse=(P, 2)))
        runs[nb] = dict(solves=g.pc_solves(), mats=g.pc_matrices(), stats=g.spectrum_stats(),
                        coarse=g.coarse_setup_stats()["matrices"], y=y.tobytes())
        g.close()
    for nb, run in runs.items():
        assert bits(run["mats"]) == bits(runs[0]["mats"]), (name, nb)
        assert bits(run["solves"]) == bits(runs[0]["solves"]), (name, nb)
        assert run["y"] == runs[0]["y"], (name, nb, "pc_apply differs")
        first, _ = check_twins(f"{name} batch {nb}", run, keys, False)
        assert len(first) == distinct
        assert run["coarse"] == distinct, (name, nb, run["coarse"], distinct)
        assert run["stats"]["fallbacks"] == 0 and run["stats"]["matrices"] == 0, (nb, run["stats"])
        assert all(m["coarse"] for m in run["mats"] if m["solves"]), nb


# ---- case 3: width 15, and ragged rows with perm
@pytest.mark.parametrize("space,n,n_t", [("p1_3d", 12, 6), ("q2", 16, 6)])
def test_other_structures(space, n, n_t):
    p = common.heat_problem(space=space, n=n, n_t=n_t, beta=1e-4)
    check_equal(f"{space} {n} x {n_t}", {nb: heat_run(p, nb) for nb in (0,) + BATCHES})


# ---- case 4: non-symmetric blocks, batched power iteration
def convection_reaction_problem(N, CN, n_t=10, growth=200.0):
    """The operators of ``test_gpu_spectrum_estimates._mms_convection_problem`` -- K + (wind(t_i) .
    grad) per level on ``rectangle_p1(N, N, 2, 2)``, beta = 1 -- plus a reaction term 200 i M.  The
    MMS problem itself has one symmetric part for all levels (the wind is divergence-free), so all
    its Lanczos runs stop at one step (40 at N = 16, 60 at N = 24, measured on the one-matrix
    path); with the reaction term at N = 24 they stop at 40, 50 and 60."""
    from control_amd.fem import rectangle_p1
    disc = rectangle_p1(N, N, 2.0, 2.0)
    beta, T = 1.0, 2.0
    tau = T / (n_t - 1.0)

    def wind(X, t):
        x, y = X[:, 0] - 1.0, X[:, 1] - 1.0
        return np.cos(0.5 * np.pi * t) * np.stack([2.0 * y * (1.0 - x * x), -2.0 * x * (1.0 - y * y)], 1)
    Ks = [(disc.K + disc.convection(lambda Xq, t=i * tau: wind(Xq, t)) + (growth * i) * disc.M).tocsr()
          for i in range(n_t)]
    b00, b01, b10, b11, m = instationary_blocks(disc.M, Ks, tau, beta, n_t, CN, share=True)
    return dict(sd=disc, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                nodes=disc.boundary)


@pytest.mark.parametrize("CN", [False, True], ids=["BE", "CN"])
def test_convection_diffusion_mms(CN):
    """The MMS problem as it is (N = 16, n_t = 10), and its variant whose runs stop at different steps."""
    name = f"convection-diffusion MMS 16 {'CN' if CN else 'BE'}"
    runs = {nb: heat_run(_mms_convection_problem(16, CN), nb) for nb in (0,) + BATCHES}
    check_equal(name, runs)
    assert any(r["eimag"] > 0.0 for r in runs[0]["solves"])
    name = f"convection-diffusion-reaction 24 {'CN' if CN else 'BE'}"
    p = convection_reaction_problem(24, CN)
    runs = {nb: heat_run(p, nb) for nb in (0,) + BATCHES}
    check_equal(name, runs)
    assert any(r["eimag"] > 0.0 for r in runs[0]["solves"])
    assert all(m["power"] > 0 for m in runs[0]["mats"] if m["estimate"] == "lanczos")
    check_masking(name, runs[0])


# ---- case 5: component blocks, the inner handle of StokesPC, coarse inverses
@pytest.mark.parametrize("multigrid", [False, True], ids=["plain", "two-grid"])
def test_navier_stokes_cavity(multigrid):
    pb, v_init, _ = common.navier_stokes_cavity_problem(n=8, n_t=10)
    v = v_init + 0.5 * pb.v_d
    D = [pb.D_v(v[i]) for i in range(pb.n_t)]
    Dp = [pb.D_p(v[i]) for i in range(pb.n_t)]
    runs = {}
    for nb in (0,) + BATCHES:
        gls = picard.GpuLinearSolver(pb, Multigrid=multigrid, kp=AUTO, options=opts(nb))
        gls._build(gls._blocks(D, Dp))
        y = gls.outer.pc_apply(common.rng_vector(gls.outer.local_size), gls.pc)
        runs[nb] = dict(solves=gls.inner.pc_solves() + gls.outer.pc_solves(), mats=gls.inner.pc_matrices(),
                        stats=gls.inner.spectrum_stats(), y=y.tobytes(),
                        coarse=gls.inner.coarse_setup_stats()["matrices"])
    check_equal(f"cavity 8{' two-grid' if multigrid else ''}", runs)
    assert any(r.get("eimag", 0.0) > 0.0 for r in runs[0]["solves"])
    for nb in BATCHES:
        assert runs[nb]["coarse"] == runs[0]["coarse"]
        assert (runs[nb]["coarse"] > 0) == multigrid
        assert all(m["coarse"] == multigrid for m in runs[nb]["mats"] if m["solves"])


# ---- case 6: product-only matrices stay `none`
def test_cn_product_only_matrices_stay_unestimated():
    p = common.heat_problem(n=8, n_t=10, CN=True, beta=1.0)
    runs = {nb: heat_run(p, nb) for nb in (0,) + BATCHES}
    check_equal("CN p1 8 beta 1", runs)
    for run in runs.values():
        product_only = [m for m in run["mats"] if m["solves"] == 0]
        assert len(product_only) >= 2
        assert all(m["estimate"] == "none" and not m["coarse"] and m["lanczos"] == 0 and m["power"] == 0
                   for m in product_only)


# ---- case 7: a rebuild on new values
def test_rebuild_equals_a_fresh_handle():
    variants = [_convection_problem(n=16), _convection_problem(n=16, scale=2.0)]
    p, q = variants
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=4))
    x = common.rng_vector(2 * p["m"] * p["sd"].n_dofs)

    def read(g, y):
        return dict(solves=g.pc_solves(), mats=g.pc_matrices(), stats=g.spectrum_stats(), y=y.tobytes())
    fresh, rebuilt = {}, {}
    for nb in (0,) + BATCHES:
        g = common.gpu_system(q, options=opts(nb))
        fresh[nb] = read(g, g.pc_apply(x, common.gpu_pc(q, MASS, AUTO, coarse=(P, 2))))
        g.close()
        g = common.gpu_system(p, options=opts(nb))
        pc = common.gpu_pc(p, MASS, AUTO, coarse=(P, 2))
        first = g.pc_apply(x, pc)
        for i in range(p["n_t"]):
            for quadrant in (1, 2):      # the level matrices of both sweeps
                g.update_block_values(quadrant, i, i, q["blocks"][quadrant][(i, i)])
        rebuilt[nb] = read(g, g.pc_apply(x, pc))
        assert rebuilt[nb]["y"] != first.tobytes()
        g.close()
    check_equal("fresh two-grid handle", fresh)
    check_equal("rebuilt two-grid handle", rebuilt)
    for nb in (0,) + BATCHES:
        assert bits(rebuilt[nb]["mats"]) == bits(fresh[0]["mats"]), nb
        assert bits(rebuilt[nb]["solves"]) == bits(fresh[0]["solves"]), nb
        assert rebuilt[nb]["y"] == fresh[0]["y"], nb


# ---- case 8: a time shard of 2 ranks on one GPU
def test_time_shards():
    res = base.launch(2, False, None, target=functools.partial(worker.run_spectrum_batch, CN=False, m=7))
    assert sorted(res) == [0, 1] and [res[r]["levels"] for r in (0, 1)] == [4, 3]
    for r in (0, 1):
        runs = res[r]["runs"]
        assert sorted(runs) == sorted(worker.BATCHES)
        check_equal(f"time shard, rank {r}", runs)
        # a rank estimates its own levels only: the middle level's matrix is one of the sweeps'
        assert len(runs[0]["mats"]) == 2 * res[r]["levels"]


# ---- the saving: synchronisations do not grow with the number of matrices
def test_synchronisations_do_not_depend_on_the_matrix_count():
    small = time_dependent_runs(False, 6, (0, 64))
    large = time_dependent_runs(False, 12, (0, 64))
    check_equal("time-dependent p1 24 x 12 BE", large)
    n_small, n_large = (r[64]["stats"]["matrices"] for r in (small, large))
    assert n_large >= 2 * n_small, (n_small, n_large)
    # one batch: the twin search (2), the symmetric / skew split (1), one Lanczos run
    whole = TWIN_SYNCS + 1 + LANCZOS_SYNCS
    for r in (small, large):
        st = r[64]["stats"]
        assert st["batches"] == 1 and st["power_steps"] == 0
        assert st["twin_syncs"] <= TWIN_SYNCS and st["lanczos_syncs_max"] <= LANCZOS_SYNCS
        assert st["syncs"] <= whole, st
    # the one-matrix path: at least one round trip per Lanczos step and matrix
    assert large[0]["stats"]["lanczos_steps"] > 10 * whole
