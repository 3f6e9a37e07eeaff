"""The kernels of the scalar reaction re-linearisation (``reaction_kernels.hip`` and the gather and
composition of ``relin_kernels.hip`` on this plan) one by one, read back through
``kkt_debug_reaction_array`` / ``kkt_debug_block_values``:

* element matrices against the exact rational sums of ``tests/reaction_ref.py`` (``32 u S``);
* the ordered gather, the composition into block values, the right-hand side and the update bit
  for bit against numpy statements of the same sums;
* the residual against correctly rounded rows built from the *downloaded* ``D`` (componentwise
  bound), with the host's ``non_linear_res_eval`` held to the same bound;
* the tails of the grid-stride loops: every small shape is no multiple of 256, and
  ``rectangle_p1(362, 362)`` with five levels crosses every launcher's cap -- the element kernel's
  (1024 workgroups over ``ne n_t``), the gather's (16384 over ``nnz n_t``), the composition's (256
  over a block's padded slots), the residual's (512 over the rows) and those of the right-hand side
  and the update (2048 over ``2 m n``).  No cap is out of reach.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import common
import reaction_ref
import structures
from control_amd import _lib, blocks, fem, reaction, relinearise
from control_amd.control import GpuBackend, Instationary, _apply_T_1, _apply_T_2
from control_amd.multiblock import DirichletBCNullspace, MultiBlockSystem
from test_gpu_relin_kernels import _Vec, _exact_rows, _ratio, _transposed

pytestmark = pytest.mark.gpu

U = structures.U
BAR = reaction_ref.ELEMENT_BAR          # tests/reaction_ref.py derives it
MESHES = {"square": (2, 2, 2.0, 2.0), "anisotropic": (3, 2, 3.0, 1.0)}
ITERATES = ("normal", "decades", "zero_level")
COEFFICIENTS = [(2.0, 0.0, 0.5), (2.0, 0.0, 1.5), (1.25, -0.75, 0.5, -2.0, 0.375)]
BETA = 2.0 ** -6
ELEMENT_CAP = 1024 * 256       # launch_reaction_elements, over ne * n_t
GATHER_CAP = 16384 * 256       # launch_relin_gather_one, over nnz * n_t
COMPOSE_CAP = 256 * 256        # launch_relin_compose, over the padded slots of a block
RESIDUAL_CAP = 512 * 256       # launch_reaction_residual, over the rows of a row block
VECTOR_CAP = 2048 * 256        # launch_reaction_rhs / launch_reaction_update, over 2 m n


# --------------------------------------------------------------------------------- problems
def _wind(X):
    return np.stack([1.0 + X[:, 1], -0.5 - X[:, 0]], axis=1)


def _control(mesh, n_t, CN, coefficients=COEFFICIENTS[0], tau=0.5, skew=False, lifted=False,
             seed=0):
    """``tau``, ``tau / 2`` and ``tau / beta`` are powers of two; random desired states and forces
    per level: every data row is non-trivial.  ``skew``: a non-symmetric linear part; ``lifted``:
    inhomogeneous boundary values and a non-zero initial condition."""
    disc = fem.rectangle_p1(*mesh) if isinstance(mesh, tuple) else mesh
    rng = np.random.default_rng(common.SEED + seed)
    tables = rng.standard_normal((2, n_t, disc.n_dofs))
    v_0 = rng.standard_normal(disc.n_dofs)

    def level(t):
        return int(round(t / tau))
    term = fem.ReactionTerm(disc, coefficients,
                            linear=disc.K + disc.convection(_wind) if skew else None)
    kw = {}
    if lifted:
        kw = dict(bcs_v=lambda Xb, t: 0.25 * (1.0 + t) + Xb[:, 0],
                  initial_condition=lambda X: v_0)
    return Instationary(disc, term, desired_state=lambda X, t: tables[0][level(t)],
                        force_f=lambda X, t: tables[1][level(t)], beta=BETA, CN=CN, n_t=n_t,
                        time_interval=(0.0, tau * (n_t - 1)), **kw)


def _iterate(kind, disc, n_t=3):
    rng = np.random.default_rng(common.SEED + ITERATES.index(kind))
    v = rng.standard_normal((n_t, disc.n_dofs))
    if kind == "decades":
        v = np.sign(v) * 10.0 ** rng.uniform(-6.0, 6.0, size=v.shape)
    elif kind == "zero_level":
        v[1] = 0.0
    return v


def _device(ctl):
    """The pattern-only block system of the device loop with the plan on it; nothing composed."""
    plan = reaction.ReactionPlan(ctl)
    system, quads, full = reaction.build_system(ctl, GpuBackend(), plan)
    return system, reaction.DeviceReaction(ctl, system, plan=plan), full


def _state(ctl, rng, v=None):
    """Random iterate; zeta is non-zero on the Dirichlet dofs too."""
    shape = (ctl._n_t, ctl._disc.n_dofs)
    return (rng.standard_normal(shape) if v is None else v), rng.standard_normal(shape)


def _residual(system, dev, rhs):
    with _Vec(system) as d:
        norm = dev.residual(d.d, rhs=rhs)
        return d.get(), norm


# ----------------------------------------------------------------------- element matrices
_EXACT = {}


def _exact_elements(mesh_name, kind, c):
    """Exact element matrices and scales per level, computed once per (mesh, iterate, c)."""
    key = (mesh_name, kind, c)
    if key not in _EXACT:
        disc = fem.rectangle_p1(*MESHES[mesh_name])
        term = fem.ReactionTerm(disc, c)
        _EXACT[key] = [(reaction_ref.exact_element_matrices(term, w), reaction_ref.scales(term, w))
                       for w in _iterate(kind, disc)]
    return _EXACT[key]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("kind", ITERATES)
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_element_kernel_against_the_exact_reference(mesh_name, kind, CN):
    for c in COEFFICIENTS:
        ctl = _control(MESHES[mesh_name], 3, CN, c)
        v = _iterate(kind, ctl._disc)
        system, dev, _ = _device(ctl)
        dev.set_state(*_state(ctl, np.random.default_rng(common.SEED), v))
        dev.assemble()
        E = dev.debug_array("E")
        worst = 0.0
        for l, (X, S) in enumerate(_exact_elements(mesh_name, kind, c)):
            worst = max(worst, reaction_ref.worst_ratio(E[l], X, S))
        same = all(np.array_equal(E[l], ctl._forward.element_matrices(v[l])) for l in range(3))
        print(f"{mesh_name} {kind} CN={CN} c={c}: device worst err / (u S) = {worst:.2f}; "
              f"bit for bit the host statement: {same}")
        assert worst <= BAR


# --------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_gather_bit_for_bit(mesh_name, skew):
    ctl = _control(MESHES[mesh_name], 3, skew, COEFFICIENTS[2], skew=skew)
    term = ctl._forward
    rng = np.random.default_rng(common.SEED + 1)
    system, dev, _ = _device(ctl)
    for kind in ITERATES:
        dev.set_state(*_state(ctl, rng, _iterate(kind, ctl._disc)))
        dev.assemble()
        E, D = dev.debug_array("E"), dev.debug_array("D")
        for l in range(3):
            assert np.array_equal(D[l], term.L.data + relinearise.gather(E[l], *dev.plan.lists)), l
        dev.assemble()            # the same state again: the same bits
        assert np.array_equal(dev.debug_array("E"), E) and np.array_equal(dev.debug_array("D"), D)


# -------------------------------------------------------------------------------- compose
def _composed(dev, D, level, alpha, transpose, gamma):
    """``fl(fl(alpha D(^T)) + fl(gamma M))`` (``blocks._axpby``; ``alpha = 0``: ``gamma M``) in
    the stored CSR order of a block, Dirichlet columns zeroed."""
    M = dev.plan.term.M
    if alpha == 0.0:
        e = gamma * M.data
    else:
        e = alpha * (_transposed(D[level], M) if transpose else D[level]) + gamma * M.data
    e[np.isin(M.indices, dev.ctl._disc.boundary)] = 0.0
    return e


def _check_blocks(dev, system, recipes, D):
    for (q, i, j, level, alpha, transpose, gamma) in recipes:
        got, padding_zero = system.block_values(q, i, j)
        assert np.array_equal(got, _composed(dev, D, level, alpha, transpose, gamma)), (q, i, j)
        assert padding_zero, (q, i, j)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_compose_bit_for_bit(mesh_name, CN):
    """The linear part is ``K + convection``: ``D`` is not symmetric, so the transposed blocks
    really read through the permutation."""
    ctl = _control(MESHES[mesh_name], 3, CN, skew=True)
    rng = np.random.default_rng(common.SEED + 2)
    system, dev, full = _device(ctl)
    dev.set_state(*_state(ctl, rng, _iterate("decades", ctl._disc)))
    dev.assemble()
    D = dev.debug_array("D")
    M = dev.plan.term.M
    assert np.any(_transposed(D[1], M) != D[1])
    assert any(r[4] == 0.0 for r in full) and any(r[5] for r in full)
    dev.relinearise(recipes=full)
    _check_blocks(dev, system, full, D)
    for (q, i, j, level, alpha, transpose, gamma) in full:
        if alpha == 0.0:
            got, _ = system.block_values(q, i, j)
            keep = ~np.isin(M.indices, ctl._disc.boundary)
            assert np.array_equal(got[keep], (gamma * M.data)[keep])
            assert np.all(got[~keep] == 0.0) and (~keep).any()
    # the plain transpose, and non-dyadic coefficients (a contracted alpha D + (gamma M) would
    # round once less)
    for once in ([(1, 0, 0, 1, 1.0, True, 0.0)], [(1, 0, 0, 2, 0.7, False, 0.3)]):
        dev.relinearise(recipes=once)
        _check_blocks(dev, system, once, D)
    # the loop's own list after another assembly
    dev.set_state(*_state(ctl, rng))
    dev.assemble()
    dev.relinearise()
    relin = blocks.instationary_relinearisation_recipes(dev.plan.tau, BETA, 3, CN)["inner"]
    _check_blocks(dev, system, relin, dev.debug_array("D"))


def test_a_shared_value_array_becomes_private():
    """Host-built blocks share one value array per ``mass(c)`` object; a recipe on one of them
    must leave the others as they were."""
    ctl = _control(MESHES["anisotropic"], 4, False)
    disc, n_t = ctl._disc, 4
    plan = reaction.ReactionPlan(ctl)
    M = plan.term.M
    b00, b01, b10, b11, m = blocks.instationary_blocks(M, [ctl._forward(np.zeros(disc.n_dofs), 0.0)]
                                                       * n_t, plan.tau, BETA, n_t, False)
    assert b01[(0, 1)] is b01[(1, 2)]
    ns = (DirichletBCNullspace(disc.boundary),) * m
    system = MultiBlockSystem(disc.n_dofs, disc.n_dofs, b00, b01, b10, b11, n_blocks_00=m,
                              n_blocks_11=m, nullspace_0=ns, nullspace_1=ns)
    dev = reaction.DeviceReaction(ctl, system, plan=plan)
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED + 3)))
    dev.assemble()
    D = dev.debug_array("D")
    arrays = system.info()["n_value_arrays"]
    before, _ = system.block_values(1, 1, 2)
    once = [(1, 0, 1, 2, 0.7, False, 0.3)]
    dev.relinearise(recipes=once)
    _check_blocks(dev, system, once, D)
    assert np.array_equal(system.block_values(1, 1, 2)[0], before)
    assert np.array_equal(before, _composed(dev, D, 0, 0.0, False, -1.0))
    assert system.info()["n_value_arrays"] == arrays + 1


# ------------------------------------------------------------------------------- residual
# Roundings of reaction_residual_kernel beyond the stored entries of the row sums; tau, tau / 2
# and tau / beta are dyadic (their products are exact).  BE: tau D z + M z; d - tau M v; - (.);
# + M z': 4 (the state rows alike).  CN: v_i + v_i+1 inside the row sum; d - h (.);
# h D^T z + M z; - (.); h D^T z' - M z'; - (.): 6 (the state rows alike).
def _c_roundings(CN):
    return 6 if CN else 4


def _row_terms(ctl, plan, D, state, fam, i, cache):
    """The products of row block (fam, i) as ``(A, x)`` with the row ``data - sum A x``, from
    ``Instationary.non_linear_res_eval``; the dyadic coefficients are folded into ``x``."""
    v, zeta = state
    tau, beta, n_t = plan.tau, plan.beta, plan.n_t
    M = plan.term.M

    def Dl(l, transpose=False):
        if (l, transpose) not in cache:
            data = _transposed(D[l], M) if transpose else D[l]
            cache[(l, transpose)] = sp.csr_matrix((data, M.indices, M.indptr), shape=M.shape)
        return cache[(l, transpose)]
    if not plan.CN:
        if fam == 0:
            t = [(Dl(i, True), tau * zeta[i]), (M, zeta[i])]
            if i < n_t - 1:
                t += [(M, tau * v[i]), (M, -zeta[i + 1])]
            return t
        t = [(Dl(i), tau * v[i]), (M, v[i])]
        if i >= 1:
            t += [(M, -v[i - 1]), (M, -(tau / beta) * zeta[i])]
        return t
    h = 0.5 * tau
    if fam == 0:
        return [(M, h * v[i]), (M, h * v[i + 1]), (Dl(i, True), h * zeta[i]), (M, zeta[i]),
                (Dl(i + 1, True), h * zeta[i + 1]), (M, -zeta[i + 1])]
    return [(Dl(i), h * v[i]), (M, -v[i]), (Dl(i + 1), h * v[i + 1]), (M, v[i + 1]),
            (M, -(h / beta) * zeta[i]), (M, -(h / beta) * zeta[i + 1])]


def _check_residual(ctl, dev, state, r, host, rows=None):
    """Every row block of the device residual ``r`` and of the host's against the exact rows;
    returns the worst ratios (device, host) of error to bound."""
    plan, disc = dev.plan, ctl._disc
    m, n = plan.m, disc.n_dofs
    D = dev.debug_array("D")
    c = _c_roundings(plan.CN)
    bc = np.zeros(n, dtype=bool)
    bc[disc.boundary] = True
    pick = np.arange(n) if rows is None else rows
    worst, cache = [0.0, 0.0], {}
    for rb in range(2 * m):
        fam, i = divmod(rb, m)
        data = plan.data[rb]
        if not plan.CN and fam == 0 and i == plan.n_t - 1:
            data = np.zeros(n)                    # the last adjoint row has no data term
        ref, absum, k = _exact_rows(data, _row_terms(ctl, plan, D, state, fam, i, cache), rows)
        free = ~bc[pick]
        for w, vec in enumerate((r, host)):
            got = vec[rb * n:(rb + 1) * n][pick]
            assert np.all(got[~free] == 0.0), (rb, w)          # Dirichlet rows
            worst[w] = max(worst[w], _ratio(got[free], ref[free], absum[free], k[free], c,
                                            data[pick][free]))
    return worst


def _host_residual(ctl, state):
    disc = ctl._disc
    v_0 = (np.zeros(disc.n_dofs) if ctl._initial_condition is None
           else np.asarray(ctl._initial_condition(disc.coords), dtype=np.float64))
    r0, r1 = ctl.non_linear_res_eval(state[0], state[1], v_0, ctl.construct_v_d(),
                                     ctl.construct_f())
    return np.concatenate([np.ravel(r0), np.ravel(r1)])


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [2, 3, 5])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_residual_against_correctly_rounded_rows(mesh_name, n_t, CN):
    """Inhomogeneous boundary values, a non-zero ``v_0`` and a non-symmetric linear part."""
    ctl = _control(MESHES[mesh_name], n_t, CN, lifted=True, skew=n_t == 3)
    rng = np.random.default_rng(common.SEED + 3 + n_t)
    state = _state(ctl, rng)
    system, dev, _ = _device(ctl)
    dev.set_state(*state)
    with pytest.raises(_lib.KktError) as err:                  # nothing assembled yet
        _residual(system, dev, rhs=False)
    assert err.value.code == -3
    dev.assemble()
    r, norm = _residual(system, dev, rhs=False)
    if not CN:
        assert np.any(dev.plan.data[dev.plan.m] != 0.0)        # the initial-condition row
    worst = _check_residual(ctl, dev, state, r, _host_residual(ctl, state))
    print(f"{mesh_name} n_t={n_t} CN={CN}: worst error / bound = {worst[0]:.3f} (device), "
          f"{worst[1]:.3f} (host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    ref = np.linalg.norm(r)
    assert abs(norm - ref) <= 1e-12 * ref


# ------------------------------------------------------------------------ right-hand side
def _host_rhs(r, m, CN):
    r0, r1 = r[:r.size // 2].reshape(m, -1), r[r.size // 2:].reshape(m, -1)
    if CN:
        r0, r1 = _apply_T_1(r0), _apply_T_2(r1)
    return np.concatenate([np.ravel(r0), np.ravel(r1)])


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("tau", [0.5, 0.3])
def test_right_hand_side(tau, CN):
    ctl = _control(MESHES["anisotropic"], 4, CN, tau=tau)
    system, dev, _ = _device(ctl)
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED + 4)))
    dev.assemble()
    r, norm_r = _residual(system, dev, rhs=False)
    b, norm_b = _residual(system, dev, rhs=True)
    assert np.array_equal(b, _host_rhs(r, dev.plan.m, CN))
    assert np.array_equal(b, r) != CN
    assert norm_b == norm_r                            # the norm of r, not of b
    assert abs(norm_r - np.linalg.norm(r)) <= 1e-12 * np.linalg.norm(r)


# --------------------------------------------------------------------------------- update
def _check_update(ctl, system, dev, rng):
    disc, m, cn = ctl._disc, dev.plan.m, int(dev.plan.CN)
    n, nodes = disc.n_dofs, disc.boundary
    old = _state(ctl, rng)
    assert np.all(old[1][:, nodes] != 0.0)
    dev.set_state(*old)
    u = rng.standard_normal(system.local_size)
    assert u.size == 2 * m * n
    u0, u1 = u[:m * n].reshape(m, n), u[m * n:].reshape(m, n)
    with _Vec(system, u) as d:
        dev.update(d.d)
        left = d.get()
    v, zeta = dev.get_state()
    want_v = old[0].copy()
    want_v[cn:cn + m] += u0                 # unknown block i: v at level i (CN: i + 1)
    want_v[:, nodes] = old[0][:, nodes]     # the boundary values stay
    want_z = old[1].copy()
    want_z[:m] += u1
    want_z[:m, nodes] = 0.0                 # (CN: the last level is not an unknown; the loop
    assert np.array_equal(v, want_v)        #  keeps it at zero)
    if cn:
        assert np.array_equal(v[0], old[0][0])
        assert np.array_equal(zeta[m], old[1][m])
    assert np.array_equal(zeta, want_z)
    assert np.array_equal(left, np.zeros_like(left))


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [2, 4])
def test_update(n_t, CN):
    ctl = _control(MESHES["anisotropic"], n_t, CN)
    system, dev, _ = _device(ctl)
    _check_update(ctl, system, dev, np.random.default_rng(common.SEED + 5))


# ----------------------------------------------------------------------- grid-stride tails
def test_tails_past_every_launch_cap():
    """362 x 362, five levels, CN: every launcher's range exceeds its cap (the module docstring
    lists them).  Bitwise references where the kernels have them; the element matrices against the
    host statement within twice the bar (both lie within the bar of the exact sum), and the
    residual rows past the cap against correctly rounded rows."""
    ctl = _control((362, 362, 2.0, 2.0), 5, True)
    disc, term = ctl._disc, ctl._forward
    system, dev, full = _device(ctl)
    plan = dev.plan
    m, n, ne, nnz = plan.m, disc.n_dofs, len(term.cells), term.M.nnz
    assert ne * 5 > ELEMENT_CAP and nnz * 5 > GATHER_CAP and nnz > COMPOSE_CAP
    assert n > RESIDUAL_CAP and 2 * m * n > VECTOR_CAP
    assert n % 256 and (ne * 5) % 256 and (2 * m * n) % 256
    rng = np.random.default_rng(common.SEED + 6)
    state = _state(ctl, rng)
    dev.set_state(*state)
    dev.assemble()
    E, D = dev.debug_array("E"), dev.debug_array("D")
    for l in (0, 4):
        host = term.element_matrices(state[0][l])
        S = reaction_ref.scales(term, state[0][l])
        ratio = float((np.abs(E[l] - host) / (U * S)).max())
        print(f"level {l}: device against host element matrices, worst {ratio:.2f} u S")
        assert ratio <= 2 * BAR
        assert np.array_equal(D[l], term.L.data + relinearise.gather(E[l], *plan.lists))
    assert np.any(E[4][-1] != 0.0) and np.any(D[4][-8:] != 0.0)
    recipe = [(1, 0, 0, 0, 0.5 * plan.tau, True, 1.0), (2, m - 1, m - 1, 4, 0.7, False, 0.3)]
    dev.relinearise(recipes=recipe)
    _check_blocks(dev, system, recipe, D)
    r, norm = _residual(system, dev, rhs=False)
    host = _host_residual(ctl, state)
    assert common.rel_err(r, host) <= 1e-12
    assert abs(norm - np.linalg.norm(r)) <= 1e-12 * np.linalg.norm(r)
    tail = np.arange(RESIDUAL_CAP, n)
    worst = _check_residual(ctl, dev, state, r, host, rows=tail)
    print(f"rows past the cap: worst error / bound = {worst[0]:.3f} (device), {worst[1]:.3f} "
          f"(host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    b, _ = _residual(system, dev, rhs=True)
    assert np.array_equal(b, _host_rhs(r, m, True)) and np.any(b[VECTOR_CAP:] != r[VECTOR_CAP:])
    _check_update(ctl, system, dev, rng)


# --------------------------------------------------------------------------------- errors
def test_errors():
    ctl = _control(MESHES["square"], 3, False)
    system, dev, full = _device(ctl)
    lib, h = system._lib, system.handle
    # a second plan of the other kind on this handle; and the other way round
    assert lib.kkt_set_relinearisation(h, C.byref(_lib.RelinDesc())) == -3
    from test_gpu_relin_kernels import _bare, _problem
    outer, _ = _bare(_problem((2, 2, 2.0, 2.0), 3, False))
    d, keep = dev.plan.descriptor()
    assert lib.kkt_set_reaction_relinearisation(outer.handle, C.byref(d)) == -3
    # the descriptor on a layout that is not its own
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.n_t = 4
    fresh = reaction.build_system(ctl, GpuBackend(), dev.plan)[0]
    assert lib.kkt_set_reaction_relinearisation(fresh.handle, C.byref(bad)) == -1
    assert b"scalar instationary system" in lib.kkt_last_error(fresh.handle)
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.degree = 5
    assert lib.kkt_set_reaction_relinearisation(fresh.handle, C.byref(bad)) == -1
    # state: nothing assembled yet
    out = np.empty(dev.plan.term.M.nnz * 3)
    assert lib.kkt_debug_reaction_array(h, 1, out.ctypes.data_as(_lib.c_f64p), out.size) == -3
    with pytest.raises(_lib.KktError) as err:
        dev.relinearise(recipes=full)
    assert err.value.code == -3
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED)))
    dev.assemble()
    # cap too small, no such array
    assert lib.kkt_debug_reaction_array(h, 1, out.ctypes.data_as(_lib.c_f64p), out.size - 1) == -1
    assert lib.kkt_debug_reaction_array(h, 4, out.ctypes.data_as(_lib.c_f64p), out.size) == -1
    assert lib.kkt_debug_reaction_array(h, 1, out.ctypes.data_as(_lib.c_f64p), out.size) == 0
    # recipes outside the layout: no such block, a level that does not exist, another space
    for recipe in ([(1, 0, 2, 0, 0.5, False, 1.0)], [(1, 0, 0, 3, 0.5, False, 1.0)]):
        with pytest.raises(_lib.KktError) as err:
            dev.relinearise(recipes=recipe)
        assert err.value.code == -1
    arr = relinearise._recipe_array([(1, 0, 0, 0, 0.5, False, 1.0)], 1)
    assert lib.kkt_reaction_relinearise(h, h, 0, 1, arr) == -1
    # nothing was written by the refused calls: the blocks are still unset
    with pytest.raises(_lib.KktError):
        system.mult(np.zeros(system.local_size))
    del keep
