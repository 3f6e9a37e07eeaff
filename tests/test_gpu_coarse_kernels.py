"""The coarse set-up and correction kernels of the two-grid sub-solves, one by one, against the
exact references of ``tests/coarse_ref.py`` (run with -m gpu on an MI355X).

* ``galerkin_kernel`` and the column path: every kept matrix paired one to one with ``P^T At P`` of
  the matrices the sub-solves solve with -- integer data bit for bit, real data within the depth
  of the kernel's chains -- on every storage form (uniform, ragged, row-sorted, R = 1 and 2,
  masked and unmasked, component blocks), each case asserting the form from the launch constants.
* ``gj_init_kernel`` / ``gj_panel_kernel`` / ``gj_update_kernel``: exact families bit for bit, real
  ones against an extended-precision inverse within 8 times what float64 attains, at sizes around
  the 32-column panels, the 64-column update tiles and the 1 024 threads of the panel kernel, and
  at the benchmark's 1 089; the threshold, the flags, the tie rule.
* ``coarse_block_scatter_kernel``, the deflated K_p inverse, the column path's inverse.
* ``coarse_restrict_kernel`` / ``coarse_dense_kernel`` / ``coarse_prolong_kernel`` and their batched
  forms through ``kkt_debug_coarse_correction``: each stage on its own device inputs, in the
  second trips of the strided loops and the grid-stride trips of the prolongations.

``einv_outside_kernel`` is not covered: its only effect is the width of the tile plan's column
ranges, which no hook reports.
"""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_ref as ref
import common
import spectrum_ref
import structures as st
import test_gpu_sweep_forms as forms
from control_amd.blocks import conform_to, instationary_blocks
from control_amd.coarse import multilinear_coarse_space

pytestmark = pytest.mark.gpu

MASS = (8, 0.5, 2.0)
SCHUR = (8, 2.1 / 30, 2.1)
EPS = 2.0 ** -10              # sqrt(EPS) tau / sqrt(beta), the last level's shift, is a power of two
_WORST = {}


def _note(what, ratio):
    _WORST[what] = max(_WORST.get(what, 0.0), float(ratio))
    print(f"[coarse kernels] {what}: ratio {ratio:.3g} (largest so far {_WORST[what]:.3g})")


# ------------------------------------------------------------------------------ problems
def _on(values, like):
    return sp.csr_matrix((values, like.indices, like.indptr), shape=like.shape)


def _integers(like, seed):
    """Small non-zero integers on the structure of ``like``, the diagonal pushed away from 0."""
    rng = np.random.default_rng([ref.SEED, seed])
    v = rng.integers(1, 5, size=like.nnz) * rng.choice([-1.0, 1.0], size=like.nnz)
    rows = np.repeat(np.arange(like.shape[0]), np.diff(like.indptr))
    v[like.indices == rows] += 40.0
    return _on(v, like)


def heat(space, n, integer, n_t=3, sd=None):
    """BE heat-control blocks with one non-symmetric forward operator per level (K + 0.1 i M +
    0.3 (1 + i) C, C the skew part of K's values), mass and stiffness on one structure: the forward
    and the adjoint sweep solve with different matrices on every level.  tau = 1; ``integer``:
    integer values and beta = 1/16, so every ``blk + c M`` the sub-solves form holds multiples of
    1/8 (shifts 0, 4 and 1/8)."""
    sd = forms.spatial(space, n) if sd is None else sd
    like = sp.csr_matrix(abs(sp.csr_matrix(sd.K)) + abs(sp.csr_matrix(sd.M)))
    like.sort_indices()
    K, M = conform_to(sd.K, like), conform_to(sd.M, like)
    if integer:
        M = _integers(K, 1)
        Ks = [_integers(K, 2 + i) for i in range(n_t)]
        beta = 2.0 ** -4
    else:
        rows = np.repeat(np.arange(like.shape[0]), np.diff(like.indptr))
        skew = np.sign(like.indices - rows) * K.data
        Ks = [_on(K.data + (0.1 * i) * M.data + (0.3 * (1 + i)) * skew, K) for i in range(n_t)]
        beta = 1e-2
    tau = 2.0 / (n_t - 1.0)
    b00, b01, b10, b11, m = instationary_blocks(M, Ks, tau, beta, n_t, False, share=True)
    sd = dataclasses.replace(sd, M=M)
    return dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=False, m=m, blocks=(b00, b01, b10, b11),
                nodes=sd.boundary)


def dyadic(P, bits=6):
    """``P`` with its weights rounded to multiples of 2^-bits."""
    P = sp.csr_matrix(P, copy=True)
    P.data = np.round(np.ldexp(P.data, bits)) * 2.0 ** -bits
    return P


def build(p, P, options=None, cycles=1):
    """A handle whose preconditioner -- two-grid sub-solves on ``P`` -- is built."""
    g = common.gpu_system(p, options={"coarse_keep": "1", "persistent": "0", **(options or {})})
    pc = dataclasses.replace(common.gpu_pc(p, MASS, SCHUR, coarse=(P, cycles)), epsilon=EPS)
    g.pc_apply(common.rng_vector(g.local_size), pc)
    return g


def solved_matrices(p):
    """The distinct ``(blk, c)`` the sub-solves of one application solve with."""
    out, seen = [], set()
    for _, _, blk, c in spectrum_ref.schur_solve_map("BE", p["blocks"], p["m"], p["tau"],
                                                     p["beta"], EPS):
        blk = sp.csr_matrix(blk)
        key = (np.float64(c).tobytes(), blk.indices.tobytes(), blk.data.tobytes())
        if key not in seen:
            seen.add(key)
            out.append((blk, c))
    return out


def _masked(A, nodes, n):
    free = np.ones(n)
    free[np.asarray(nodes, dtype=np.int64)] = 0.0
    D = sp.diags(free)
    return sp.csr_matrix(D @ sp.csr_matrix(A) @ D)


def galerkin_reference(blk, c, M, nodes, P):
    """``(E, G, At)`` of ``At = D (blk + c M) D``: E from the unrounded ``blk + c M`` (the device
    forms it with one rounding, which the bound's + 10 holds), G from the rounded one."""
    n = P.shape[0]
    Ab, Am = _masked(blk, nodes, n), _masked(M, nodes, n)
    At = Ab if c == 0.0 else _masked(sp.csr_matrix(blk) + c * sp.csr_matrix(M), nodes, n)
    E, _ = ref.galerkin_exact(Ab, P)
    _, G = ref.galerkin_exact(At, P)
    if c != 0.0:
        E = E + np.longdouble(c) * ref.galerkin_exact(Am, P)[0]
    return E, G, At


def pair_one_to_one(kept, match):
    """``match(b, r)`` for kept matrix b and reference r: the pairing must be a bijection."""
    table = np.array([[bool(match(b, r)) for r in range(len(kept))] for b in range(len(kept))])
    assert (table.sum(axis=1) == 1).all(), ("kept matrices without exactly one reference", table)
    assert (table.sum(axis=0) == 1).all(), ("references matched by several kept matrices", table)
    return table.argmax(axis=1)


def check_galerkin(g, p, P, integer, what):
    """Every kept matrix of the handle against the references of ``p``; returns the worst ratio."""
    P = sp.csr_matrix(P)
    kept = g.coarse_matrices()
    solved = solved_matrices(p)
    refs = [galerkin_reference(blk, c, p["sd"].M, p["nodes"], P) for blk, c in solved]
    assert len(kept) == len(refs) == g.coarse_setup_stats()["matrices"]
    shape = g.coarse_shape()
    if integer:
        exact = [(P.T @ At @ P).toarray() for _, _, At in refs]        # float64 SciPy
        for (E, _, _), x in zip(refs, exact):
            assert np.array_equal(E.astype(np.float64), x)             # no rounding anywhere
        pair_one_to_one(kept, lambda b, r: np.array_equal(kept[b], exact[r]))
        return 0.0
    width = shape["uniform_w"] if shape["uniform_w"] >= 0 else int(st.row_widths(solved[0][0]).max())
    depth = ref.galerkin_depth(width, np.diff(P.T.tocsr().indptr))[:, None]
    worst = np.zeros((len(kept), len(refs)))
    for b, Eb in enumerate(kept):
        for r, (E, G, _) in enumerate(refs):
            err = np.abs(Eb.astype(np.longdouble) - E).astype(np.float64)
            bound = depth * ref.U * G
            with np.errstate(divide="ignore", invalid="ignore"):
                worst[b, r] = np.max(np.where(err == 0, 0.0, err / bound))     # 0 bound: inf
    order = pair_one_to_one(kept, lambda b, r: worst[b, r] <= 1.0)
    for b, r in enumerate(order):
        assert not kept[b][refs[r][1] == 0.0].any()       # outside the structure: exact zeros
    ratio = max(worst[b, r] for b, r in enumerate(order))
    _note(f"Galerkin {what}", ratio)
    return ratio


# ----------------------------------------------------------------------- Galerkin matrices
# (space, n, coarse cells): the structures and coarse spaces of test_gpu_sweep_forms.py.  The
# unsorted slices of Q2 on 6^2 and of P2 on 6^2 are all as wide as their widest row; Q2 on 8^2
# (slices 25, 25, 15 wide) is the unsorted ragged structure.
SPACES = {"fd5": ("fd5", 24, 4), "q1": ("q1", 16, 4), "p1": ("p1", 16, 4), "p1_3d": ("p1_3d", 6, 3),
          "q2": ("q2", 6, 3), "p2v": ("p2v", 6, 3), "q2_8": ("q2", 8, 4)}
RAGGED = ("q2", "p2v", "q2_8")
GALERKIN_CASES = [(s, r, so) for s in SPACES for r in ("2", "1")
                  for so in (("1", "0") if s in RAGGED else ("1",))]


_GALERKIN_FORMS = {}


def galerkin_case(space, sell_r, sell_sort):
    """Integer and real data on the batched and on the column path; returns the launch constants
    of the batched set-up."""
    key = (space, sell_r, sell_sort)
    if key in _GALERKIN_FORMS:
        return _GALERKIN_FORMS[key]
    fem_space, n, cells = SPACES[space]
    opts = {"sell_r": sell_r, "sell_sort": sell_sort}
    for integer in (True, False):
        p = heat(fem_space, n, integer)
        P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells)
        P = dyadic(P) if integer else sp.csr_matrix(P)
        for columns in (False, True):
            g = build(p, P, {**opts, **({"coarse_setup": "columns"} if columns else {})})
            shape, stats = g.coarse_shape(), g.coarse_setup_stats()
            assert shape["n_coarse"] == P.shape[1] and shape["n"] == P.shape[0]
            if space == "p2v" and not columns:      # two components: the block form of the launch
                assert shape["block_n"] * 2 == P.shape[1] and stats["blocks"] == 2
            else:
                assert stats["blocks"] == 1
            what = (f"{space} R={shape['R']} w={shape['uniform_w']} sorted={shape['sorted']} "
                    f"{'columns' if columns else 'batched'} {'integer' if integer else 'real'}")
            assert check_galerkin(g, p, P, integer, what) <= 1.0, what
            if not columns:
                _GALERKIN_FORMS[key] = shape
    return _GALERKIN_FORMS[key]


@pytest.mark.parametrize("space,sell_r,sell_sort", GALERKIN_CASES)
def test_galerkin_matrices_on_every_storage_form(space, sell_r, sell_sort):
    shape = galerkin_case(space, sell_r, sell_sort)
    # the form this case is named after
    assert shape["R"] == int(sell_r) and shape["masked"] == 1
    if sell_sort == "0":
        assert shape["sorted"] == 0
    if space == "q2_8":
        assert shape["uniform_w"] == -1, shape


def test_every_galerkin_branch_is_reached():
    """Uniform width, ragged slices unsorted and row-sorted, each at R = 1 and R = 2."""
    reached = set()
    for case in GALERKIN_CASES:
        shape = galerkin_case(*case)
        kind = "uniform" if shape["uniform_w"] >= 0 else ("sorted" if shape["sorted"] else "ragged")
        reached.add((kind, shape["R"]))
    want = {(k, r) for k in ("uniform", "ragged", "sorted") for r in (1, 2)}
    assert not want - reached, sorted(want - reached)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("n,cells", [(68, 4), (36, 18)])
def test_galerkin_second_trips(n, cells, integer):
    """P1 with coarse supports of 33^2 rows (the strided loop over a row of P^T takes five trips)
    and with 361 coarse functions (more than 256 of anything indexed by them)."""
    p = heat("p1", n, integer)
    P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells)
    P = dyadic(P) if integer else sp.csr_matrix(P)
    g = build(p, P)
    shape = g.coarse_shape()
    if cells == 4:
        assert shape["pt_longest"] > 4 * ref.REDUCE_THREADS
    else:
        assert shape["n_coarse"] > ref.REDUCE_THREADS
    assert check_galerkin(g, p, P, integer, f"p1 {n}^2, {cells} cells") <= 1.0


@pytest.mark.parametrize("blocks", ["1", "0"])
def test_galerkin_component_blocks(blocks):
    """The two-component convection problem of test_gpu_multigrid_drivers.py: ``block_n`` > 0 writes
    each diagonal block as a matrix of its own; ``coarse_blocks`` = 0 the whole matrix."""
    import test_gpu_multigrid_drivers as drivers
    p, P = drivers._two_component_convection_problem(n=24, n_t=4)
    g = build(p, P, {"coarse_blocks": blocks}, cycles=2)
    stats, shape = g.coarse_setup_stats(), g.coarse_shape()
    assert shape["block_n"] * 2 == P.shape[1]
    assert stats["blocks"] == (2 if blocks == "1" else 1)
    assert check_galerkin(g, p, P, False, f"two components, coarse_blocks={blocks}") <= 1.0
    # the scatter: each diagonal block of the kept inverse against the reference of its own block,
    # exact zeros outside
    E, inv = g.coarse_matrices(), g.coarse_inverses()
    h = shape["block_n"]
    assert not inv[:, :h, h:].any() and not inv[:, h:, :h].any()
    for b in (0, len(E) - 1):
        for k in range(2):
            s = slice(k * h, (k + 1) * h)
            check_inverse(E[b][s, s], inv[b][s, s], f"component block {k}, coarse_blocks={blocks}")


def test_galerkin_unmasked_and_the_deflated_inverse():
    """The K_p solve of the Stokes preconditioner: no masked rows; the kept inverse is that of
    ``E + fl(trace(E) / n_c^2)``, the trace summed in index order."""
    p = common.stokes_problem(n=8, n_t=4)
    th = p["th"]
    Pp = sp.csr_matrix(multilinear_coarse_space(th.coords_p, (), cells=3))
    specs = dict(common.STOKES_SPECS, kp=(6, 0.15, 2.1))
    outer, gpc = common.stokes_gpu(p, specs, options={"coarse_keep": "1"}, kp_coarse=(Pp, 2))
    outer.pc_apply(common.rng_vector(2 * p["m"] * (th.n_v + th.n_p)), gpc)
    shape = outer.coarse_shape()
    assert shape["masked"] == 0 and shape["n_coarse"] == Pp.shape[1] and shape["n"] == th.n_p
    kept = outer.coarse_matrices()
    assert len(kept) == 1
    Kp = sp.csr_matrix(th.K_p)
    E, G = ref.galerkin_exact(Kp, Pp)
    width = shape["uniform_w"] if shape["uniform_w"] >= 0 else int(st.row_widths(Kp).max())
    bound = ref.galerkin_depth(width, np.diff(Pp.T.tocsr().indptr))[:, None] * ref.U * G
    err = np.abs(kept[0].astype(np.longdouble) - E).astype(np.float64)
    assert (err <= bound).all() and not kept[0][G == 0.0].any()
    _note("Galerkin K_p (unmasked)", np.max(err[bound > 0] / bound[bound > 0]))
    nc = Pp.shape[1]
    tr = 0.0
    for v in np.diag(kept[0]):
        tr += v
    check_inverse(kept[0] + tr / (float(nc) * float(nc)), outer.coarse_inverses()[0],
                  "deflated K_p inverse")


# -------------------------------------------------------------------------- dense inverse
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1089)
_HANDLE = []


def handle():
    """Any finalized handle serves ``debug_dense_inverse``."""
    if not _HANDLE:
        _HANDLE.append(common.gpu_system(common.heat_problem(n=8, n_t=4)))
    return _HANDLE[0]


def check_inverse(A, X, what):
    """The device inverse ``X`` of ``A`` against ``inverse_columns`` on the sampled columns, and its
    residual over all entries, each within 8 times what float64 attains on ``A`` (the larger of
    the figures of ``gauss_jordan_f64`` and ``numpy.linalg.inv``)."""
    r_d, r_rho, change = ref.inverse_ratios(A, X)
    assert change <= 2.0 ** -60, (what, change)
    _note(f"inverse {what}: distance", r_d)
    _note(f"inverse {what}: residual", r_rho)
    assert r_d <= 8 and r_rho <= 8, (what, r_d, r_rho)


@pytest.mark.parametrize("n", SIZES)
def test_dense_inverse_exact_families(n):
    """Bit for bit, in batches of 1 and 3.  Above n = 1 024 every row loop of the panel kernel
    takes its second trip; ``tie_blocks`` is exact under the tie rule only."""
    g = handle()
    for name, fam in ref.EXACT_FAMILIES.items():
        A, X = fam(n)
        inv, bad = g.debug_dense_inverse(A[None])
        assert bad.tolist() == [n] and np.array_equal(inv[0], X), (name, 1)
        three = [fam(n, seed) for seed in (1, 2, 3)]
        inv, bad = g.debug_dense_inverse(np.stack([a for a, _ in three]))
        assert bad.tolist() == [n] * 3
        for b, (_, x) in enumerate(three):
            assert np.array_equal(inv[b], x), (name, 3, b)


_REAL = {}


def _device_real(n):
    """The four real matrices of size n and their device inverses: ``normal`` alone, the other
    three as one batch."""
    if n not in _REAL:
        _REAL.clear()
        g = handle()
        A = {name: ref.real_family(name, n) for name in ref.REAL_FAMILIES}
        inv, bad = g.debug_dense_inverse(A["normal"][None])
        assert bad.tolist() == [n]
        out = {"normal": (A["normal"], inv[0])}
        rest = ref.REAL_FAMILIES[1:]
        inv, bad = g.debug_dense_inverse(np.stack([A[name] for name in rest]))
        assert bad.tolist() == [n] * 3
        for b, name in enumerate(rest):
            out[name] = (A[name], inv[b])
        _REAL[n] = out
    return _REAL[n]


@pytest.mark.parametrize("name", ref.REAL_FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_dense_inverse_real_families(n, name):
    A, X = _device_real(n)[name]
    check_inverse(A, X, f"{name} n={n}")


@pytest.mark.parametrize("columns", [False, True])
def test_kept_inverses_of_a_real_build(columns):
    """36 coarse functions on the 40^2 P1 heat problem: every kept inverse against the reference of
    its kept Galerkin matrix, on the batched path and on the column path (four launches per
    pivot, ``gj_pivot_kernel`` and its kin)."""
    p = heat("p1", 40, False, n_t=4)
    P = sp.csr_matrix(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=5))
    assert P.shape[1] == 36
    g = build(p, P, {"coarse_setup": "columns"} if columns else None)
    E, inv = g.coarse_matrices(), g.coarse_inverses()
    assert len(E) == len(inv) >= 3
    for b in range(len(E)):
        check_inverse(E[b], inv[b], f"kept Galerkin matrix, {'columns' if columns else 'batched'}")


def _diag_with(n, at, value):
    d = np.ones(n)
    d[at] = value
    return np.diag(d)


@pytest.mark.parametrize("n,at", [(40, 17), (1089, 1030)])
def test_dense_inverse_threshold(n, at):
    """1e-13 max|diag| lies between 2^-44 and 2^-43: a factor 2 from the knife edge on either side."""
    g = handle()
    inv, bad = g.debug_dense_inverse(np.stack([_diag_with(n, at, 2.0 ** -43),
                                               _diag_with(n, at, 2.0 ** -44)]))
    assert bad.tolist() == [n, at]
    assert np.array_equal(inv[0], _diag_with(n, at, 2.0 ** 43))


def test_dense_inverse_reports_the_smallest_bad_column():
    g = handle()
    n = 100
    A = _diag_with(n, 70, 0.0)
    A[33, 33] = 2.0 ** -50
    B = _diag_with(n, 5, 2.0 ** -60)
    B[99, 99] = 0.0
    good = ref.real_family("dominant", n)
    inv, bad = g.debug_dense_inverse(np.stack([good, A, good, B]))
    assert bad.tolist() == [n, 33, n, 5]
    alone, _ = g.debug_dense_inverse(good[None])
    assert np.array_equal(inv[0], alone[0]) and np.array_equal(inv[2], alone[0])


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_dense_inverse_flags_non_finite_input(value):
    """One non-finite entry -- in a dense matrix, and above the diagonal of a sparse one, where no
    pivot search ever meets it -- flags its matrix and leaves the neighbours in the batch alone."""
    g = handle()
    n = 70
    good = ref.real_family("dominant", n)
    dense = good.copy()
    dense[50, 12] = value
    sparse = [np.eye(n), np.eye(n)]
    sparse[0][3, 20] = value        # same panel as its row: the multipliers under pivot 20 are 0
    sparse[1][3, 40] = value        # a later panel
    diagonal = np.eye(n)
    diagonal[37, 37] = value
    inv, bad = g.debug_dense_inverse(np.stack([good, dense, good, *sparse, diagonal, good]))
    assert bad[0] == bad[2] == bad[6] == n
    assert bad[1] < n and bad[3] == 20 and bad[4] == 40 and bad[5] < n, bad
    alone, _ = g.debug_dense_inverse(good[None])
    for b in (0, 2, 6):
        assert np.array_equal(inv[b], alone[0])


@pytest.mark.parametrize("n", [2, 64, 1090])
def test_dense_inverse_of_an_antidiagonal_permutation(n):
    """max|diag| = 0: the threshold is 0 and every pivot, 1, passes it."""
    g = handle()
    A = np.fliplr(np.eye(n))
    inv, bad = g.debug_dense_inverse(A[None])
    assert bad.tolist() == [n] and np.array_equal(inv[0], A)


# ------------------------------------------------------------------- correction kernels
_SPACES = {}


def correction_handle(kind):
    """``(g, P)``: small -- 25 coarse functions, rows of P^T below 256 entries; wide -- 324
    functions of more than 256 rows (second trips of the restriction and of the dense product); large --
    fd5 on 725^2 points, more rows than one pass of either prolongation covers."""
    if kind not in _SPACES:
        _SPACES.clear()
        space, n, cells = {"small": ("p1", 16, 4), "wide": ("p1", 153, 17),
                           "large": ("fd5", 724, 4)}[kind]
        p = heat(space, n, False)
        P = dyadic(multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=cells))
        _SPACES[kind] = (build(p, P), P)
    return _SPACES[kind]


def _vectors(n, nb, vstride, integer, seed):
    rng = np.random.default_rng([ref.SEED, seed, n, nb])
    draw = (lambda k: rng.integers(-8, 9, size=k).astype(np.float64)) if integer else \
        rng.standard_normal
    r, x_in = draw(nb * vstride), draw(nb * vstride)
    prior = np.full(nb * vstride, -7.0)
    return r, x_in, prior


def _einv(nc, integer, seed):
    rng = np.random.default_rng([ref.SEED, seed, nc])
    return rng.integers(-4, 5, size=(nc, nc)).astype(np.float64) if integer else \
        rng.standard_normal((nc, nc))


def check_stages(P, einv, r, x_in, rc, ec, x_out, integer, what):
    """Each stage against the exact result on the inputs the device gave it."""
    Pt = sp.csr_matrix(P.T)
    stages = [("restriction", rc, Pt, r, ref.reduce_depth(np.diff(Pt.indptr)), None),
              ("dense product", ec, sp.csr_matrix(einv), rc,
               ref.reduce_depth(np.full(len(einv), len(einv))), None),
              ("prolongation", x_out, P, ec, None, x_in)]
    for name, y, A, x, terms, plus in stages:
        ratio, equal = ref.stage_ok(y, A, x, terms=terms, plus=plus)
        _note(f"{what} {name}", ratio)
        assert ratio <= 1.0, (what, name, ratio)
        if integer:
            assert equal, (what, name)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("kind", ["small", "wide"])
def test_correction_stages(kind, integer):
    g, P = correction_handle(kind)
    n, nc = P.shape
    shape = g.coarse_shape()
    if kind == "small":
        assert nc == 25 and shape["pt_longest"] < ref.REDUCE_THREADS
    else:
        assert nc == 324 > ref.REDUCE_THREADS and shape["pt_longest"] > ref.REDUCE_THREADS
    einv = _einv(nc, integer, 1)
    r, x_in, _ = _vectors(n, 1, n, integer, 2)
    for with_x in (True, False):
        rc, ec, x_out = g.debug_coarse_correction(r, einv, x_in=x_in if with_x else None)
        check_stages(P, einv, r, x_in if with_x else None, rc[0], ec[0], x_out, integer,
                     f"correction {kind}")


@pytest.mark.parametrize("nb", [1, 3, 5])
@pytest.mark.parametrize("kind", ["small", "wide"])
def test_batched_correction_equals_the_one_vector_launches(kind, nb):
    """Bit for bit per vector, at a stride above n; the gaps between the vectors keep their
    prior contents."""
    g, P = correction_handle(kind)
    n, nc = P.shape
    vstride = n + 37
    einv = _einv(nc, False, 3)
    r, x_in, prior = _vectors(n, nb, vstride, False, 4)
    for with_x in (True, False):
        rc, ec, x_out = g.debug_coarse_correction(r, einv, x_in=x_in if with_x else None,
                                                  x_out=prior, nb=nb, vstride=vstride, batched=True)
        x_out = x_out.reshape(nb, vstride)
        assert np.array_equal(x_out[:, n:], prior.reshape(nb, vstride)[:, n:])
        for b in range(nb):
            s = slice(b * vstride, b * vstride + n)
            one = g.debug_coarse_correction(r[s], einv, x_in=x_in[s] if with_x else None)
            assert np.array_equal(rc[b], one[0][0]) and np.array_equal(ec[b], one[1][0])
            assert np.array_equal(x_out[b, :n], one[2])
    # ... and the batched stages on their own, against the exact results
    rc, ec, x_out = g.debug_coarse_correction(r, einv, x_in=x_in, x_out=prior, nb=nb,
                                              vstride=vstride, batched=True)
    b = nb - 1
    s = slice(b * vstride, b * vstride + n)
    check_stages(P, einv, r[s], x_in[s], rc[b], ec[b], x_out[s], False, f"batched correction {kind}")


def test_prolongations_beyond_one_pass():
    """725^2 rows: the grid-stride loop of ``coarse_prolong_kernel`` (one pass: 524 288 rows) and of
    the batched form (65 536) take further trips, and the restriction sums 131 000 entries per
    coarse function.  Integer data and dyadic weights: every stage is exact in float64, so plain
    NumPy products are the reference."""
    g, P = correction_handle("large")
    n, nc = P.shape
    assert n > ref.PROLONG_ROWS > ref.PROLONG_BATCHED_ROWS and g.coarse_shape()["n"] == n
    einv = _einv(nc, True, 5)
    nb, vstride = 2, n + 11
    r, x_in, prior = _vectors(n, nb, vstride, True, 6)
    Pt = sp.csr_matrix(P.T)
    rc, ec, x_out = g.debug_coarse_correction(r, einv, x_in=x_in, x_out=prior, nb=nb,
                                              vstride=vstride, batched=True)
    x_out = x_out.reshape(nb, vstride)
    assert np.array_equal(x_out[:, n:], prior.reshape(nb, vstride)[:, n:])
    for b in range(nb):
        s = slice(b * vstride, b * vstride + n)
        want_rc = Pt @ r[s]
        want_ec = einv @ want_rc
        want_x = x_in[s] + P @ want_ec
        assert np.abs(want_x).max() < 2.0 ** 50            # (far from any rounding)
        assert np.array_equal(rc[b], want_rc) and np.array_equal(ec[b], want_ec)
        assert np.array_equal(x_out[b, :n], want_x)
        one = g.debug_coarse_correction(r[s], einv, x_in=x_in[s])
        assert np.array_equal(one[0][0], want_rc) and np.array_equal(one[1][0], want_ec)
        assert np.array_equal(one[2], want_x)
    rc, ec, x_out = g.debug_coarse_correction(r[:n], einv)                  # no x_in
    assert np.array_equal(x_out, P @ (einv @ (Pt @ r[:n])))


def test_correction_hook_refuses_bad_arguments():
    from control_amd._lib import KktError
    g, P = correction_handle("small")
    n, nc = P.shape
    with pytest.raises(KktError):
        handle().coarse_shape()                                  # no two-grid preconditioner
    with pytest.raises(KktError):
        g.debug_coarse_correction(np.zeros(2 * n), np.eye(nc), nb=2)        # nb != 1, not batched
    with pytest.raises(KktError):
        g.debug_coarse_correction(np.zeros(n - 1), np.eye(nc), vstride=n - 1, batched=True)
