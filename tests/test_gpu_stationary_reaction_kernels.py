"""The scalar reaction re-linearisation on the stationary system (``n_t = 1``,
``Stationary.non_linear_solve(device=True)``) kernel by kernel, by the scheme of
``tests/test_gpu_reaction_kernels.py`` and with its helpers, on its two triangle meshes and on the
boxes of ``tests/test_gpu_reaction3d_kernels.py``:

* element matrices and ``D`` of the one-level launch bit for bit against the host statement
  (``ReactionTerm.element_matrices``, ``reaction_values`` + ``L``); the instationary files hold
  the same kernels to the exact rational sums;
* the composed blocks bit for bit against the numpy statement for both recipe lists, and the
  system's ``mult`` against the host-built system's;
* the new residual kernel against correctly rounded rows built from the downloaded ``D``, the
  host's ``non_linear_res_eval`` held to the same bound;
* the update bit for bit;
* the tails of the grid-stride loops on ``rectangle_p1(512, 512)``;
* what the descriptor and the recipes refuse.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import common
import reaction3d_ref as ref3
from control_amd import _lib, blocks, fem, reaction, relinearise
from control_amd.control import GpuBackend, Stationary
from control_amd.multiblock import DirichletBCNullspace, MultiBlockSystem
from test_gpu_reaction3d_kernels import _skew_linear
from test_gpu_reaction_kernels import (ELEMENT_CAP, MESHES, RESIDUAL_CAP, VECTOR_CAP,
                                       _check_blocks, _device, _residual, _wind)
from test_gpu_reaction_kernels import _control as _instationary_control
from test_gpu_relin_kernels import _Vec, _exact_rows, _ratio, _transposed

pytestmark = pytest.mark.gpu

BETA = 2.0 ** -6
COEFFICIENTS = (1.25, -0.75, 0.5, -2.0, 0.375)
CASES = {"square": MESHES["square"], "anisotropic": MESHES["anisotropic"],
         "cube": ref3.BOXES["cube"], "flat": ref3.BOXES["flat"]}
SKEW = ("anisotropic", "flat")          # the cases with a non-symmetric ``linear=``


def _disc(name):
    return fem.rectangle_p1(*CASES[name]) if len(CASES[name]) == 4 else fem.box_p1(*CASES[name])


def _control(name, coefficients=COEFFICIENTS, newton=False, seed=0, disc=None):
    """Random desired state and force, inhomogeneous boundary values; ``1 / beta`` is a power of
    two."""
    disc = _disc(name) if disc is None else disc
    rng = np.random.default_rng(common.SEED + seed)
    tables = rng.standard_normal((2, disc.n_dofs))
    linear = None
    if name in SKEW:
        linear = (disc.K + disc.convection(_wind) if disc.cells.shape[1] == 3
                  else _skew_linear(disc, seed))
    term = fem.ReactionTerm(disc, coefficients, linear=linear)
    ctl = Stationary(disc, term, desired_state=lambda X: tables[0], force_f=lambda X: tables[1],
                     beta=BETA, bcs_v=lambda Xb: 0.25 + Xb[:, 0] - Xb[:, -1])
    if newton:
        ctl.set_Gauss_Newton()
    return ctl


def _state(ctl, rng):
    """Random iterate ``(1, n)``; zeta is non-zero on the Dirichlet dofs too."""
    n = ctl._disc.n_dofs
    return rng.standard_normal((1, n)), rng.standard_normal((1, n))


def _assembled(name, seed, newton=False):
    ctl = _control(name, newton=newton)
    rng = np.random.default_rng(common.SEED + seed)
    system, dev, full = _device(ctl)
    state = _state(ctl, rng)
    dev.set_state(*state)
    return ctl, system, dev, full, state, rng


# ------------------------------------------------------------- element matrices and D
@pytest.mark.parametrize("newton", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_elements_and_D_at_one_level(name, newton):
    ctl, system, dev, full, state, rng = _assembled(name, 1, newton)
    term, plan = ctl._forward, dev.plan
    assert dev.window == {"v": (0, 1), "zeta": (0, 1), "D": (0, 1), "blocks": (0, 1)}
    assert np.array_equal(dev.debug_array("v"), state[0])
    assert np.array_equal(dev.debug_array("zeta"), state[1])
    for _ in range(2):                       # a second iterate on the same plan
        dev.assemble()
        E, D = dev.debug_array("E"), dev.debug_array("D")
        nv = term.cells.shape[1]
        assert E.shape == (1, len(term.cells), nv, nv) and D.shape == (1, term.M.nnz)
        c = plan.coefficients
        assert c == (term.jacobian_coefficients if newton else term.coefficients)
        assert np.array_equal(E[0], term.element_matrices(state[0][0], c))
        assert np.array_equal(D[0], term.L.data + relinearise.gather(E[0], *plan.lists))
        assert np.array_equal(D[0], term.L.data + term.reaction_values(state[0][0], c))
        assert np.array_equal(D[0], ctl.construct_D_v(state[0][0]).data)
        state = _state(ctl, rng)
        dev.set_state(*state)


# ------------------------------------------------------------------------- composition
def _host_system(ctl, D):
    disc = ctl._disc
    M = ctl._forward.M
    ns = (DirichletBCNullspace(disc.boundary),)
    Dm = sp.csr_matrix((D, M.indices, M.indptr), shape=M.shape)
    return MultiBlockSystem(disc.n_dofs, disc.n_dofs, *blocks.stationary_blocks(M, Dm, ctl._beta),
                            nullspace_0=ns, nullspace_1=ns)


@pytest.mark.parametrize("name", list(CASES))
def test_compose_bit_for_bit(name):
    ctl, system, dev, full, state, rng = _assembled(name, 2)
    dev.assemble()
    D = dev.debug_array("D")
    M = dev.plan.term.M
    # (a symmetric linear part still leaves roundings between (wg la) lb and (wg lb) la)
    assert (np.abs(_transposed(D[0], M) - D[0]).max() > 1e-3) == (name in SKEW)
    assert full == blocks.stationary_build_recipes(BETA)
    dev.relinearise(recipes=full)
    _check_blocks(dev, system, full, D)
    dirichlet = np.isin(M.indices, ctl._disc.boundary)
    assert dirichlet.any() and not dirichlet.all()
    for (q, i, j, *_) in full:
        got, padding_zero = system.block_values(q, i, j)
        assert padding_zero and np.all(got[dirichlet] == 0.0) and np.any(got[~dirichlet] != 0.0)
    x = rng.standard_normal(system.local_size)
    host = _host_system(ctl, D[0])
    for (q, i, j, *_) in full:
        assert np.array_equal(system.block_values(q, i, j)[0], host.block_values(q, i, j)[0]), q
    assert common.rel_err(system.mult(x), host.mult(x)) <= 1e-13
    # the loop's own list after another assembly: D^T and D move, the mass blocks stay
    mass = [system.block_values(q, 0, 0)[0] for q in (0, 3)]
    dev.set_state(*_state(ctl, rng))
    dev.assemble()
    dev.relinearise()
    D2 = dev.debug_array("D")
    assert np.any(D2 != D)
    _check_blocks(dev, system, blocks.stationary_relinearisation_recipes(BETA), D2)
    assert all(np.array_equal(system.block_values(q, 0, 0)[0], a) for q, a in zip((0, 3), mass))
    assert common.rel_err(system.mult(x), _host_system(ctl, D2[0]).mult(x)) <= 1e-13


# ---------------------------------------------------------------------------- residual
# Roundings of reaction_stationary_residual_kernel beyond the stored entries of the row sums
# (ib = 1 / beta is a power of two: its product is exact, and the issue's count keeps it).
# Adjoint rows: d - M v; - D^T zeta: 2.  State rows: d - D v; ib (M zeta); + (.): 3.
C_ROUNDINGS = (2, 3)


def _row_terms(plan, D, state, fam):
    """The products of family ``fam`` as ``(A, x)`` with the row ``data - sum A x``, from
    ``Stationary.non_linear_res_eval``; the dyadic ``ib`` is folded into ``x``."""
    M = plan.term.M
    v, zeta = state[0][0], state[1][0]

    def mat(data):
        return sp.csr_matrix((data, M.indices, M.indptr), shape=M.shape)
    if fam == 0:
        return [(M, v), (mat(_transposed(D[0], M)), zeta)]
    return [(mat(D[0]), v), (M, -(1.0 / plan.beta) * zeta)]


def _host_residual(ctl, state):
    v, zeta = state[0][0], state[1][0]
    r0, r1 = ctl.non_linear_res_eval(*ctl._data(), v, zeta, ctl.construct_D_v(v))
    return np.concatenate([r0, r1])


def _check_residual(ctl, dev, state, r, host, rows=None):
    """Both families of the device residual ``r`` and of the host's against the exact rows;
    returns the worst ratios (device, host) of error to bound."""
    plan, disc = dev.plan, ctl._disc
    n = disc.n_dofs
    D = dev.debug_array("D")
    bc = np.zeros(n, dtype=bool)
    bc[disc.boundary] = True
    pick = np.arange(n) if rows is None else rows
    free = ~bc[pick]
    worst = [0.0, 0.0]
    for fam in range(2):
        data = plan.data[fam]
        exact, absum, k = _exact_rows(data, _row_terms(plan, D, state, fam), rows)
        for w, vec in enumerate((r, host)):
            got = vec[fam * n:(fam + 1) * n][pick]
            assert np.all(got[~free] == 0.0), (fam, w)             # Dirichlet rows
            worst[w] = max(worst[w], _ratio(got[free], exact[free], absum[free], k[free],
                                            C_ROUNDINGS[fam], data[pick][free]))
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_residual_against_correctly_rounded_rows(name):
    ctl, system, dev, full, state, rng = _assembled(name, 3)
    with pytest.raises(_lib.KktError) as err:                  # nothing assembled yet
        _residual(system, dev, rhs=False)
    assert err.value.code == -3
    dev.assemble()
    r, norm = _residual(system, dev, rhs=False)
    assert r.size == 2 * ctl._disc.n_dofs
    assert np.any(dev.plan.data[0] != 0.0) and np.any(dev.plan.data[1] != 0.0)
    worst = _check_residual(ctl, dev, state, r, _host_residual(ctl, state))
    print(f"{name}: worst error / bound = {worst[0]:.3f} (device), {worst[1]:.3f} (host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    expect = np.linalg.norm(r)
    assert abs(norm - expect) <= 1e-12 * expect
    b, norm_b = _residual(system, dev, rhs=True)               # the rows are the right-hand side
    assert np.array_equal(b, r) and norm_b == norm


# ------------------------------------------------------------------------------ update
def _check_update(ctl, system, dev, rng):
    disc = ctl._disc
    n, nodes = disc.n_dofs, disc.boundary
    old = _state(ctl, rng)
    assert np.all(old[1][0, nodes] != 0.0)
    dev.set_state(*old)
    u = rng.standard_normal(system.local_size)
    assert u.size == 2 * n
    with _Vec(system, u) as d:
        dev.update(d.d)
        left = d.get()
    v, zeta = dev.get_state()
    want_v = old[0] + u[:n]
    want_v[0, nodes] = old[0][0, nodes]          # the boundary values stay
    want_z = old[1] + u[n:]
    want_z[0, nodes] = 0.0
    assert np.array_equal(v, want_v) and np.array_equal(zeta, want_z)
    assert np.array_equal(left, np.zeros_like(left))


@pytest.mark.parametrize("name", ["anisotropic", "flat"])
def test_update(name):
    ctl = _control(name)
    system, dev, _ = _device(ctl)
    _check_update(ctl, system, dev, np.random.default_rng(common.SEED + 5))


# ------------------------------------------------------------------- grid-stride tails
def test_tails_past_the_launch_caps():
    """512 x 512 at one level -- 263 169 nodes, 524 288 triangles -- is the smallest mesh past the
    element kernel's cap (1024 x 256 over ``ne``), the residual's (512 x 256 rows) and the vector
    cap of the update (2048 x 256 over ``2 n``).  The gather's cap (16 384 x 256 over ``nnz``)
    is out of reach of a seconds-long one-level case: that kernel is unchanged, and
    ``tests/test_gpu_reaction_kernels.py::test_tails_past_every_launch_cap`` pins it past its cap.
    Elements, ``D`` and the blocks whole and bit for bit; the residual on sampled rows past the
    cap (every 97th, and the last 300) against correctly rounded rows."""
    ctl = _control("square", coefficients=(2.0, 0.0, 0.5), disc=fem.rectangle_p1(512, 512))
    disc, term = ctl._disc, ctl._forward
    system, dev, full = _device(ctl)
    plan = dev.plan
    n, ne = disc.n_dofs, len(term.cells)
    assert (n, ne) == (263169, 524288)
    assert ne > ELEMENT_CAP and n > RESIDUAL_CAP and 2 * n > VECTOR_CAP and n % 256
    rng = np.random.default_rng(common.SEED + 6)
    state = _state(ctl, rng)
    dev.set_state(*state)
    dev.assemble()
    E, D = dev.debug_array("E"), dev.debug_array("D")
    assert np.array_equal(E[0], term.element_matrices(state[0][0]))
    assert np.array_equal(D[0], term.L.data + relinearise.gather(E[0], *plan.lists))
    assert np.any(E[0][-1] != 0.0) and np.any(D[0][-8:] != 0.0)
    dev.relinearise(recipes=full)
    _check_blocks(dev, system, full, D)
    r, norm = _residual(system, dev, rhs=False)
    host = _host_residual(ctl, state)
    assert common.rel_err(r, host) <= 1e-12
    assert abs(norm - np.linalg.norm(r)) <= 1e-12 * np.linalg.norm(r)
    tail = np.unique(np.concatenate([np.arange(RESIDUAL_CAP, n, 97), np.arange(n - 300, n)]))
    worst = _check_residual(ctl, dev, state, r, host, rows=tail)
    print(f"rows past the cap: worst error / bound = {worst[0]:.3f} (device), {worst[1]:.3f} "
          f"(host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    _check_update(ctl, system, dev, rng)


# ------------------------------------------------------------------------------ errors
def test_errors():
    ctl = _control("square")
    plan = reaction.ReactionPlan(ctl)
    system = reaction.build_system(ctl, GpuBackend(), plan)[0]
    lib, h = system._lib, system.handle
    d, keep = plan.descriptor()
    assert (d.n_t, d.cn) == (1, 0)

    def unset(s=system):         # nothing was written: the blocks are still unset
        with pytest.raises(_lib.KktError):
            s.mult(np.zeros(s.local_size))
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.cn = 1
    assert lib.kkt_set_reaction_relinearisation(h, C.byref(bad)) == -1
    assert b"cn == 0" in lib.kkt_last_error(h)
    unset()
    bad = _lib.ReactionDesc.from_buffer_copy(d)
    bad.n_t = 2                  # an instationary descriptor on the stationary handle
    assert lib.kkt_set_reaction_relinearisation(h, C.byref(bad)) == -1
    assert b"scalar instationary system" in lib.kkt_last_error(h)
    unset()
    # the stationary descriptor on an instationary handle of the same space
    inst = _instationary_control(MESHES["square"], 3, False)
    other = reaction.build_system(inst, GpuBackend(), reaction.ReactionPlan(inst))[0]
    assert lib.kkt_set_reaction_relinearisation(other.handle, C.byref(d)) == -1
    assert b"stationary system" in lib.kkt_last_error(other.handle)
    unset(other)
    with pytest.raises(_lib.KktError) as err:       # and no plan was left behind
        other._ck(lib.kkt_reaction_window(other.handle, (C.c_int * 8)()))
    assert err.value.code == -3
    # the plan itself; a recipe at a level the one-level plan does not have
    dev = reaction.DeviceReaction(ctl, system, plan=plan)
    dev.set_state(*_state(ctl, np.random.default_rng(common.SEED)))
    dev.assemble()
    with pytest.raises(_lib.KktError) as err:
        dev.relinearise(recipes=[(1, 0, 0, 1, 1.0, True, 0.0)])
    assert err.value.code == -1
    assert b"level" in lib.kkt_last_error(h)
    unset()
    # the Navier-Stokes plan on a handle that carries this one
    assert lib.kkt_set_relinearisation(h, C.byref(_lib.RelinDesc())) == -3
    unset()
    dev.relinearise(recipes=blocks.stationary_build_recipes(BETA))
    system.mult(np.zeros(system.local_size))
    del keep
