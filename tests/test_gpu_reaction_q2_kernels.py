"""The kernels of the scalar reaction re-linearisation on Q2 quadrilaterals (``nq = 25``, ``nv =
9``), by the scheme of ``tests/test_gpu_reaction_p2_kernels.py`` and with the helpers of
``tests/test_gpu_reaction_kernels.py``, on two meshes of ``fem.rectangle_q2`` (a 2 x 2 square of
equal cells -- 4 cells, 25 dofs, 9 of them interior -- and a 3 x 1/2 rectangle of 6 stretched
ones, which tells ``nx`` from ``ny`` and one local order from another), ``n_t`` 2 and 3: the
smallest shapes at which a wrong node order, a wrong lane-to-row map or a wrong level stride shows.

* the Q2 element kernel (three lanes per (element, level), lane ``p`` owning the rows ``p``,
  ``p + 3``, ``p + 6``, the stores staged through LDS in three rounds) bit for bit
  against the host statement and against the exact rational sums of ``tests/reaction_q2_ref.py``
  (``128 u S``), Picard and Gauss-Newton coefficients;
* the ordered gather (up to four contributions a position), the composition on the 25-wide
  pattern, the right-hand side and the update bit for bit against numpy statements of the same
  sums -- code that is unchanged, on rows it has not seen;
* the residual against correctly rounded rows built from the downloaded ``D`` (rows of up to 25
  stored entries), the host's residual held to the same bound;
* the tail of the element kernel's grid-stride loop: ``rectangle_q2(67, 67)`` with 20 levels is
  89 780 (element, level) pairs, 269 340 lanes -- past the launcher's cap of 262 144 lanes
  (87 381 pairs and a third) and a multiple of neither 64 nor 256, so the last wave and the last
  block are partly idle and one pair straddles two passes;
* what the descriptor refuses: an ``nv`` that is no element, and one that contradicts ``nq``.
"""
import ctypes as C

import numpy as np
import pytest

import common
import reaction_q2_ref as ref
from control_amd import _lib, blocks, fem, reaction, relinearise
from control_amd.control import GpuBackend, Instationary
from test_gpu_reaction3d_kernels import _skew_linear
from test_gpu_reaction_kernels import (ELEMENT_CAP, _check_blocks, _check_residual, _check_update,
                                       _device, _host_residual, _host_rhs, _residual, _state)
from test_gpu_relin_kernels import _transposed

pytestmark = pytest.mark.gpu

U = ref.U
BAR = ref.ELEMENT_BAR_Q2                # tests/reaction_q2_ref.py derives it
BETA = 2.0 ** -6


def _control(mesh, n_t, CN, coefficients=ref.COEFFICIENTS[0], tau=0.5, skew=False, lifted=False,
             seed=0):
    """``_control`` of the P1 file on a Q2 mesh: ``tau``, ``tau / 2`` and ``tau / beta`` are powers
    of two; random desired states and forces per level.  ``skew``: the stored values of ``K``
    perturbed entry by entry (there is no ``convection`` on the Q2 space)."""
    disc = fem.rectangle_q2(*mesh)
    rng = np.random.default_rng(common.SEED + seed)
    tables = rng.standard_normal((2, n_t, disc.n_dofs))
    v_0 = rng.standard_normal(disc.n_dofs)

    def level(t):
        return int(round(t / tau))
    term = fem.ReactionTerm(disc, coefficients, linear=_skew_linear(disc, seed) if skew else None)
    kw = {}
    if lifted:
        kw = dict(bcs_v=lambda Xb, t: 0.25 * (1.0 + t) + Xb[:, 0] - Xb[:, 1],
                  initial_condition=lambda X: v_0)
    return Instationary(disc, term, desired_state=lambda X, t: tables[0][level(t)],
                        force_f=lambda X, t: tables[1][level(t)], beta=BETA, CN=CN, n_t=n_t,
                        time_interval=(0.0, tau * (n_t - 1)), **kw)


def _iterate(kind, disc, n_t=3):
    return ref.iterate(kind, disc, n_t, seed=common.SEED)


def test_the_meshes():
    sizes = {}
    for name, mesh in ref.MESHES.items():
        disc = fem.rectangle_q2(*mesh)
        sizes[name] = (len(disc.cells), disc.n_dofs, disc.n_dofs - len(disc.boundary))
    assert sizes == {"square": (4, 25, 9), "stretched": (6, 35, 15)}


# ----------------------------------------------------------------------- element matrices
@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("kind", ref.ITERATES)
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_element_kernel_against_the_exact_reference(mesh, kind, CN):
    for c in ref.COEFFICIENTS:
        ctl = _control(ref.MESHES[mesh], 3, CN, c)
        v = _iterate(kind, ctl._disc)
        system, dev, _ = _device(ctl)
        dev.set_state(*_state(ctl, np.random.default_rng(common.SEED), v))
        dev.assemble()
        E = dev.debug_array("E")
        assert E.shape == (3, len(ctl._forward.cells), 9, 9)
        worst = 0.0
        for l, (X, S) in enumerate(ref.exact_elements(mesh, kind, c, common.SEED)):
            worst = max(worst, ref.worst_ratio(E[l], X, S))
        same = all(np.array_equal(E[l], ctl._forward.element_matrices(v[l])) for l in range(3))
        print(f"{mesh} {kind} CN={CN} c={c}: device worst err / (u S) = {worst:.2f}; "
              f"bit for bit the host statement: {same}")
        assert same and worst <= BAR


# --------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_gather_bit_for_bit(mesh, skew):
    ctl = _control(ref.MESHES[mesh], 3, skew, ref.COEFFICIENTS[2], skew=skew)
    term = ctl._forward
    assert (abs(term.L - term.L.T).max() > 1e-3) == skew
    assert np.diff(reaction.ReactionPlan(ctl).lists[0]).max() == 4
    rng = np.random.default_rng(common.SEED + 1)
    system, dev, _ = _device(ctl)
    for kind in ref.ITERATES:
        dev.set_state(*_state(ctl, rng, _iterate(kind, ctl._disc)))
        dev.assemble()
        E, D = dev.debug_array("E"), dev.debug_array("D")
        for l in range(3):
            assert np.array_equal(D[l], term.L.data + relinearise.gather(E[l], *dev.plan.lists)), l
        dev.assemble()            # the same state again: the same bits
        assert np.array_equal(dev.debug_array("E"), E) and np.array_equal(dev.debug_array("D"), D)


# -------------------------------------------------------------------------------- compose
@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_compose_bit_for_bit(mesh, CN):
    """On the 25-wide pattern, with a non-symmetric ``D``: the transposed blocks really read
    through the permutation.  ``_check_blocks`` also asserts the padding slots zero, and
    ``_composed`` the Dirichlet columns."""
    ctl = _control(ref.MESHES[mesh], 3, CN, skew=True)
    rng = np.random.default_rng(common.SEED + 2)
    system, dev, full = _device(ctl)
    dev.set_state(*_state(ctl, rng, _iterate("decades", ctl._disc)))
    dev.assemble()
    D = dev.debug_array("D")
    M = dev.plan.term.M
    assert np.diff(M.indptr).max() == 25
    assert np.any(_transposed(D[1], M) != D[1])
    assert full == blocks.instationary_build_recipes(dev.plan.tau, BETA, 3, CN)["inner"]
    assert any(r[4] == 0.0 for r in full) and any(r[5] for r in full)
    dev.relinearise(recipes=full)
    _check_blocks(dev, system, full, D)
    dirichlet = np.isin(M.indices, ctl._disc.boundary)
    assert dirichlet.any() and not dirichlet.all()
    for (q, i, j, *_) in full:
        got, padding_zero = system.block_values(q, i, j)
        assert padding_zero and np.all(got[dirichlet] == 0.0) and np.any(got[~dirichlet] != 0.0)
    # two non-dyadic recipes, one of them transposed (a contracted alpha D + (gamma M) would
    # round once less)
    for once in ([(1, 0, 0, 1, 0.7, True, 0.3)], [(1, 0, 0, 2, 0.3, False, 0.7)]):
        dev.relinearise(recipes=once)
        _check_blocks(dev, system, once, D)


# ------------------------------------------------------------------------------- residual
@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [2, 3])
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_residual_against_correctly_rounded_rows(mesh, n_t, CN):
    """Inhomogeneous boundary values, a non-zero ``v_0`` and a non-symmetric linear part."""
    ctl = _control(ref.MESHES[mesh], n_t, CN, lifted=True, skew=n_t == 3)
    rng = np.random.default_rng(common.SEED + 3 + n_t)
    state = _state(ctl, rng)
    system, dev, _ = _device(ctl)
    dev.set_state(*state)
    dev.assemble()
    r, norm = _residual(system, dev, rhs=False)
    if not CN:
        assert np.any(dev.plan.data[dev.plan.m] != 0.0)        # the initial-condition row
    worst = _check_residual(ctl, dev, state, r, _host_residual(ctl, state))
    print(f"{mesh} n_t={n_t} CN={CN}: worst error / bound = {worst[0]:.3f} (device), "
          f"{worst[1]:.3f} (host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert abs(norm - np.linalg.norm(r)) <= 1e-12 * np.linalg.norm(r)


# ----------------------------------------------------------- right-hand side and update
def test_right_hand_side():
    ctl = _control(ref.MESHES["stretched"], 4, True, lifted=True)
    system, dev, _ = _device(ctl)
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED + 4)))
    dev.assemble()
    r, norm_r = _residual(system, dev, rhs=False)
    b, norm_b = _residual(system, dev, rhs=True)
    assert np.array_equal(b, _host_rhs(r, dev.plan.m, True)) and not np.array_equal(b, r)
    assert norm_b == norm_r                            # the norm of r, not of b


def test_update():
    ctl = _control(ref.MESHES["stretched"], 4, True, lifted=True)
    system, dev, _ = _device(ctl)
    _check_update(ctl, system, dev, np.random.default_rng(common.SEED + 5))


# ------------------------------------------------------------------ Gauss-Newton coefficients
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_gauss_newton_coefficients_reach_the_kernel(mesh):
    c = ref.COEFFICIENTS[2]
    newton = tuple((k + 1) * ck for k, ck in enumerate(c))
    ctl = _control(ref.MESHES[mesh], 3, False, c)
    ctl.set_Gauss_Newton()
    term = ctl._forward
    v = _iterate("normal", ctl._disc)
    system, dev, _ = _device(ctl)
    assert dev.plan.coefficients == newton
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED), v))
    dev.assemble()
    E, D = dev.debug_array("E"), dev.debug_array("D")
    for l in range(3):
        X = ref.exact_element_matrices(term, v[l], newton)
        ratio = ref.worst_ratio(E[l], X, ref.scales(term, v[l], newton))
        picard = ref.worst_ratio(E[l], ref.exact_elements(mesh, "normal", c, common.SEED)[l][0],
                                 ref.scales(term, v[l], newton))
        print(f"{mesh} level {l}: against (k + 1) c_k {ratio:.2f} u S, against c_k {picard:.3g}")
        assert ratio <= BAR and picard > 1e6
        assert np.array_equal(D[l], term.L.data + relinearise.gather(E[l], *dev.plan.lists))
        assert common.rel_err(D[l], term.jacobian(v[l], 0.0).data) <= 1e-13


# ----------------------------------------------------------------------- grid-stride tail
def test_tail_past_the_element_launch_cap():
    """67 x 67 cells, 20 levels, BE: every pair, those of the second pass and the one that
    straddles the passes included, is the host statement bit for bit.  The device array holds
    exactly the pairs' doubles, so what lies behind the last pair is checked where it can be seen:
    the debug download into a longer host buffer leaves the doubles behind the last pair as they
    were."""
    n_t, lanes = 20, 3
    ctl = _control((67, 67, 1.0, 1.0), n_t, False)
    term = ctl._forward
    ne = len(term.cells)
    pairs = ne * n_t
    assert ne == 4489 and pairs == 89780 and lanes * pairs == 269340 > ELEMENT_CAP == 262144
    assert ELEMENT_CAP % lanes and (lanes * pairs) % 64 and (lanes * pairs) % 256
    system, dev, _ = _device(ctl)
    state = _state(ctl, np.random.default_rng(common.SEED + 6))
    dev.set_state(*state)
    dev.assemble()
    guard = 4096
    out = np.full(pairs * 81 + guard, -7.25)
    assert system._lib.kkt_debug_reaction_array(system.handle, 0, out.ctypes.data_as(_lib.c_f64p),
                                                out.size) == 0
    assert np.all(out[pairs * 81:] == -7.25)
    E = out[:pairs * 81].reshape(n_t, ne, 9, 9)
    same = [np.array_equal(E[l], term.element_matrices(state[0][l])) for l in range(n_t)]
    print(f"levels bit for bit the host statement: {sum(same)} of {n_t}")
    assert all(same)
    D = dev.debug_array("D")
    for l in (0, n_t - 1):
        assert np.array_equal(D[l], term.L.data + relinearise.gather(E[l], *dev.plan.lists))
    assert np.all(E[n_t - 1][-1] != 0.0)


# --------------------------------------------------------------------------------- errors
def test_errors():
    ctl = _control(ref.MESHES["square"], 3, False)
    plan = reaction.ReactionPlan(ctl)
    system = reaction.build_system(ctl, GpuBackend(), plan)[0]
    lib, h = system._lib, system.handle
    d, keep = plan.descriptor()
    assert d.nq == 25 and d.nv == 9
    ne, n = len(plan.term.cells), ctl._disc.n_dofs

    def unset():                 # nothing was written: the blocks are still unset
        with pytest.raises(_lib.KktError):
            system.mult(np.zeros(system.local_size))
    for nv, nq in ((9, 7), (5, 25), (6, 15)):
        bad = _lib.ReactionDesc.from_buffer_copy(d)
        bad.nv, bad.nq = nv, nq
        assert lib.kkt_set_reaction_relinearisation(h, C.byref(bad)) == -1
        assert b"nv" in lib.kkt_last_error(h), (nv, nq)
        unset()
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.nq = 8
    assert lib.kkt_set_reaction_relinearisation(h, C.byref(bad)) == -1
    message = lib.kkt_last_error(h)
    assert b"triangles" in message and b"tetrahedra" in message
    unset()
    cells = plan.term.cells.copy()
    cells[-1, 8] = n
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.cells = cells.ctypes.data_as(_lib.c_i32p)
    assert lib.kkt_set_reaction_relinearisation(h, C.byref(bad)) == -1
    assert b"cells" in lib.kkt_last_error(h)
    unset()
    # the plan itself, then a buffer one double short of the element matrices
    dev = reaction.DeviceReaction(ctl, system, plan=plan)
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED)))
    dev.assemble()
    out = np.empty(3 * ne * 81)
    assert lib.kkt_debug_reaction_array(h, 0, out.ctypes.data_as(_lib.c_f64p), out.size - 1) == -1
    assert lib.kkt_debug_reaction_array(h, 0, out.ctypes.data_as(_lib.c_f64p), out.size) == 0
    assert np.array_equal(out.reshape(3, -1, 9, 9), dev.debug_array("E"))
    del keep


def test_nv_zero_with_25_points_is_still_the_p2_plan():
    """A descriptor of the earlier layout: ``nv = 0`` leaves the element to ``nq``."""
    disc = fem.rectangle_p2(2, 2, 2.0, 2.0)
    rng = np.random.default_rng(common.SEED + 7)
    tables = rng.standard_normal((2, 3, disc.n_dofs))
    term = fem.ReactionTerm(disc, ref.COEFFICIENTS[0])
    ctl = Instationary(disc, term, desired_state=lambda X, t: tables[0][int(round(2 * t))],
                       force_f=lambda X, t: tables[1][int(round(2 * t))], beta=BETA, n_t=3,
                       time_interval=(0.0, 1.0))
    plan = reaction.ReactionPlan(ctl)
    system = reaction.build_system(ctl, GpuBackend(), plan)[0]
    d, keep = plan.descriptor()
    assert d.nv == 6
    old = _lib.ReactionDesc.from_buffer_copy(d)
    old.nv = 0
    assert system._lib.kkt_set_reaction_relinearisation(system.handle, C.byref(old)) == 0
    v = ref.iterate("normal", disc, seed=common.SEED)
    out = np.empty(3 * len(term.cells) * 36)
    lib, h = system._lib, system.handle
    zeta = np.zeros_like(v)
    assert lib.kkt_reaction_state(h, 0, v.ctypes.data_as(_lib.c_f64p),
                                  zeta.ctypes.data_as(_lib.c_f64p)) == 0
    assert lib.kkt_reaction_relinearise(h, h, 1, 0, None) == 0
    assert lib.kkt_debug_reaction_array(h, 0, out.ctypes.data_as(_lib.c_f64p), out.size) == 0
    E = out.reshape(3, -1, 6, 6)
    assert all(np.array_equal(E[l], term.element_matrices(v[l])) for l in range(3))
    del keep
