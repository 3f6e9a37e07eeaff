"""The device re-linearisation kernels (``relin_kernels.hip``) one by one, read back through
``kkt_debug_relin_array`` / ``kkt_debug_block_values``:

* element matrices against the exact rational reference of ``tests/relin_ref.py`` (``32 u S``);
* the ordered gather, the composition into block values, the right-hand side (dyadic ``tau``) and
  the update bit for bit against numpy statements of the same sums;
* the residual against a correctly rounded reference built from the *downloaded* ``D2``
  (componentwise bound), with the host path held to the same bound;
* the tails of the grid-stride loops at the smallest shapes that cross the launchers' caps.

Not covered: the caps of the element kernel and of the gather over ``Ep`` (16384 * 256 threads
over ``ne n_t`` / ``nnz1 n_t``) are out of reach of a small shape.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import common
import relin_ref
import structures
from control_amd import _lib, blocks, fem, picard, relinearise
from control_amd.multiblock import (ConstantNullspace, DirichletBCNullspace, MultiBlockSystem,
                                    PatternOnly)

pytestmark = pytest.mark.gpu

U = structures.U
ELEMENT_BAR = 32          # tests/test_relin_ref.py derives it
MESHES = {"square": (2, 2, 2.0, 2.0), "anisotropic": (3, 2, 3.0, 1.0)}
WINDS = ("normal", "decades", "zero_level", "zero_component")
BETA = 2.0 ** -6
# grid_of(n, cap) in compose.hpp: min(ceil(n / 256), cap) workgroups of 256 threads
RHS_UPDATE_CAP = 2048 * 256      # launch_relin_rhs / launch_relin_update (the default cap)
COMPOSE_CAP = 256 * 256          # launch_relin_compose, over the padded slots of a block
RESIDUAL_CAP = 512 * 256         # launch_relin_residual, over the rows of a row block
GATHER_CAP = 16384 * 256         # launch_relin_gather, over nnz * n_t


# --------------------------------------------------------------------------------- problems
def _problem(mesh, n_t, CN, tau=0.5, seed=0):
    """``tau``, ``tau / 2`` and ``tau / beta`` are powers of two unless ``tau`` says otherwise;
    random desired states and forces: every data row is non-trivial."""
    th = fem.rectangle_p2p1(*mesh) if isinstance(mesh, tuple) else mesh
    rng = np.random.default_rng(common.SEED + seed)
    return picard.NavierStokesControl(disc=th, nu=0.1, beta=BETA, n_t=n_t, T=tau * (n_t - 1),
                                      v_d=rng.standard_normal((n_t, th.n_v)),
                                      f=rng.standard_normal((n_t, th.n_v)), CN=CN)


def _winds(kind, th, n_t=3):
    rng = np.random.default_rng(common.SEED + WINDS.index(kind))
    v = rng.standard_normal((n_t, th.n_v))
    n2 = th.n_v // 2
    if kind == "decades":
        v = np.sign(v) * 10.0 ** rng.uniform(-6.0, 6.0, size=v.shape)
    elif kind == "zero_level":
        v[1] = 0.0
    elif kind == "zero_component":
        v[:2, n2:] = 0.0
        v[2, :n2] = 0.0
    return v


def _state(pb, rng, v=None):
    """Random iterate; zeta is non-zero on the Dirichlet dofs too."""
    th, n_t = pb.disc, pb.n_t
    m = n_t - 1 if pb.CN else n_t
    return (rng.standard_normal((n_t, th.n_v)) if v is None else v,
            rng.standard_normal((n_t, th.n_v)), rng.standard_normal((m, th.n_p)),
            rng.standard_normal((m, th.n_p)))


def _full(pb, state):
    """The three systems of a device build, every block composed; no preconditioner."""
    ls = picard.GpuLinearSolver(pb, relinearise="device", build="device")
    ls._build_device(*state)
    return ls, ls.device_plan()


def _bare(pb, velocity_blocks=((0, 0),)):
    """What ``kkt_set_relinearisation`` requires and no more: the outer layout with the
    ``tau B`` couplings and the given velocity blocks as patterns."""
    th = pb.disc
    plan = relinearise.RelinearisationPlan(pb)
    m = plan.m
    none = {(i, j): None for i in range(2 * m) for j in range(2 * m)}
    b00, b01, b10 = dict(none), dict(none), dict(none)
    for key in velocity_blocks:
        b00[key] = PatternOnly(*plan.velocity_pattern(), (th.n_v, th.n_v))
    tB = blocks._csr(pb.tau * sp.csr_matrix(th.B))
    tBT = blocks._csr(tB.T)
    for i in range(2 * m):
        b01[(i, i)], b10[(i, i)] = tBT, tB
    kw = dict(sub_n_blocks_00_0=m, sub_n_blocks_11_0=m) if pb.CN else {}
    outer = MultiBlockSystem(th.n_v, th.n_p, b00, b01, b10, dict(none), n_blocks_00=2 * m,
                             n_blocks_11=2 * m,
                             nullspace_0=(DirichletBCNullspace(th.boundary_v),) * (2 * m),
                             nullspace_1=tuple(ConstantNullspace() for _ in range(2 * m)),
                             CN=pb.CN, **kw)
    dev = relinearise.DeviceRelinearisation(pb, outer, {"outer": [], "inner": [],
                                                        "commutator": []}, plan=plan)
    return outer, dev


class _Vec:
    """A device vector of the outer handle."""

    def __init__(self, system, host=None):
        self.s, self.d = system, C.c_void_p()
        system._ck(system._lib.kkt_vec_alloc(system.handle, C.byref(self.d)))
        if host is not None:
            host = np.ascontiguousarray(host, dtype=np.float64)
            assert host.size == system.local_size
            system._ck(system._lib.kkt_vec_upload(system.handle, self.d,
                                                  host.ctypes.data_as(C.POINTER(C.c_double))))

    def get(self):
        out = np.empty(self.s.local_size)
        self.s._ck(self.s._lib.kkt_vec_download(self.s.handle, self.d,
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.s._lib.kkt_vec_free(self.s.handle, self.d)


def _residual(outer, dev, rhs):
    with _Vec(outer) as d:
        norm = dev.residual(d.d, rhs=rhs)
        return d.get(), norm


# ----------------------------------------------------------------------- element matrices
_EXACT = {}


def _exact_elements(mesh_name, kind):
    """Exact element matrices and scales per level, computed once per (mesh, wind)."""
    key = (mesh_name, kind)
    if key not in _EXACT:
        th = fem.rectangle_p2p1(*MESHES[mesh_name])
        v = _winds(kind, th)
        _EXACT[key] = [relin_ref.mesh_element_matrices(th, w)
                       + relin_ref.scales(th.elem, th.n_v // 2, w) for w in v]
    return _EXACT[key]


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("kind", WINDS)
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_element_kernel_against_the_exact_reference(mesh_name, kind, CN):
    pb = _problem(MESHES[mesh_name], 3, CN)
    th = pb.disc
    v = _winds(kind, th)
    outer, dev = _bare(pb)
    dev.set_state(*_state(pb, np.random.default_rng(common.SEED), v))
    dev.assemble()
    Ev, Ep = dev.debug_array("Ev"), dev.debug_array("Ep")
    worst_v = worst_p = 0.0
    for l, (Xv, Xp, Sv, Sp) in enumerate(_exact_elements(mesh_name, kind)):
        worst_v = max(worst_v, relin_ref.worst_ratio(Ev[l], Xv, Sv))
        worst_p = max(worst_p, relin_ref.worst_ratio(Ep[l], Xp, Sp))
        if not v[l].any():
            assert np.array_equal(Ev[l], np.zeros_like(Ev[l]))
            assert np.array_equal(Ep[l], np.zeros_like(Ep[l]))
    print(f"{mesh_name} {kind} CN={CN}: device worst err / (u S) = {worst_v:.2f} (velocity), "
          f"{worst_p:.2f} (pressure)")
    assert worst_v <= ELEMENT_BAR and worst_p <= ELEMENT_BAR


# --------------------------------------------------------------------------------- gather
def _check_gather(dev, Ev, Ep, D2, Dp):
    plan, nu = dev.plan, dev.pb.nu
    for l in range(dev.pb.n_t):
        want = nu * plan.K2.data + relinearise.gather(Ev[l], *plan.v_lists)
        assert np.array_equal(D2[l], want), l
        want = nu * plan.Kp.data + relinearise.gather(Ep[l], *plan.p_lists)
        assert np.array_equal(Dp[l], want), l


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_gather_bit_for_bit(mesh_name, CN):
    pb = _problem(MESHES[mesh_name], 3, CN)
    th = pb.disc
    rng = np.random.default_rng(common.SEED + 1)
    outer, dev = _bare(pb)
    names = ("Ev", "Ep", "D2", "Dp")
    for kind in ("zero_level", "decades"):
        v = _winds(kind, th)
        dev.set_state(*_state(pb, rng, v))
        dev.assemble()
        first = [dev.debug_array(n) for n in names]
        _check_gather(dev, *first)
        if kind == "zero_level":
            assert np.array_equal(first[2][1], pb.nu * dev.plan.K2.data)
            assert np.array_equal(first[3][1], pb.nu * dev.plan.Kp.data)
        dev.assemble()            # the same state again: the same bits
        for a, n in zip(first, names):
            assert np.array_equal(dev.debug_array(n), a), n
    dev.set_state(*_state(pb, rng))
    dev.assemble()
    for a, n in zip(first, names):
        b = dev.debug_array(n)
        assert all(np.any(b[l] != a[l]) for l in range(pb.n_t)), n


# -------------------------------------------------------------------------------- compose
def _transposed(data, like):
    """Values of the transpose on the (symmetric, sorted) structure of ``like``, by scipy."""
    T = sp.csr_matrix((data, like.indices, like.indptr), shape=like.shape).T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, like.indices) and np.array_equal(T.indptr, like.indptr)
    return T.data


def _composed(dev, space, D, level, alpha, transpose, gamma, masked):
    """``fl(fl(alpha D(^T)) + fl(gamma M))`` in the stored CSR order of a block."""
    plan = dev.plan
    K, M = (plan.K2, plan.M2) if space == 0 else (plan.Kp, plan.Mp)
    if alpha == 0.0:
        e = gamma * M.data
    else:
        d = _transposed(D[level], K) if transpose else D[level]
        e = alpha * d + gamma * M.data
    if space == 1:
        return e
    e = np.concatenate([e, e])                  # both components from the one scalar array
    if masked:
        cols = plan.velocity_pattern()[1]
        e[np.isin(cols, dev.pb.disc.boundary_v)] = 0.0
    return e


def _check_blocks(dev, system, recipes, space, D, masked):
    for (q, i, j, level, alpha, transpose, gamma) in recipes:
        got, padding_zero = system.block_values(q, i, j)
        want = _composed(dev, space, D, level, alpha, transpose, gamma, masked)
        assert np.array_equal(got, want), (q, i, j)
        assert padding_zero, (q, i, j)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_compose_bit_for_bit(mesh_name, CN):
    pb = _problem(MESHES[mesh_name], 3, CN)
    th = pb.disc
    rng = np.random.default_rng(common.SEED + 2)
    ls, dev = _full(pb, _state(pb, rng, _winds("decades", th)))
    D2, Dp = dev.debug_array("D2"), dev.debug_array("Dp")
    full = blocks.instationary_build_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
    assert any(r[4] == 0.0 for r in full["inner"]) and any(r[5] for r in full["inner"])
    # every velocity-space column block of the outer and inner systems carries the Dirichlet
    # nullspace: their value arrays have the column mask; the pressure space has none
    systems = (("outer", ls.outer, 0, D2, True), ("inner", ls.inner, 0, D2, True),
               ("commutator", ls.comm, 1, Dp, False))
    for name, system, space, D, masked in systems:
        _check_blocks(dev, system, full[name], space, D, masked)
    # one-off recipes: the plain transpose, and non-dyadic coefficients (a contracted
    # alpha D + (gamma M) would round once less)
    for name, system, space, D, masked in systems:
        q = 0 if name == "outer" else 1
        once = [(q, 0, full["m"] if name == "outer" else 0, 1, 1.0, True, 0.0)]
        dev.relinearise(system, name, recipes=once)
        _check_blocks(dev, system, once, space, D, masked)
        got, _ = system.block_values(*once[0][:3])
        want = _transposed(D[1], dev.plan.K2 if space == 0 else dev.plan.Kp)
        if space == 1:
            assert np.array_equal(got, want)
        else:
            keep = ~np.isin(dev.plan.velocity_pattern()[1], th.boundary_v)
            assert np.array_equal(got[keep], np.concatenate([want, want])[keep])
            assert np.all(got[~keep] == 0.0) and (~keep).any()
        odd = [(once[0][0], once[0][1], once[0][2], 2, 0.7, False, 0.3)]
        dev.relinearise(system, name, recipes=odd)
        _check_blocks(dev, system, odd, space, D, masked)


# ------------------------------------------------------------------------------- residual
def _exact_rows(data, terms, rows=None):
    """``data - sum_j A_j x_j`` correctly rounded per row (error-free products, ``math.fsum``,
    as ``structures.rows_exact``), ``sum_j |A_j| |x_j|`` and the stored entries summed."""
    n = len(data) if rows is None else len(rows)
    d = data if rows is None else data[rows]
    parts = [[np.array([x])] for x in d]
    absum, k = np.zeros(n), np.zeros(n, dtype=np.int64)
    for A, x in terms:
        A = sp.csr_matrix(A)
        if rows is not None:
            A = A[rows]
        p, e = structures.two_prod(A.data, np.asarray(x, np.float64)[A.indices])
        for r in range(n):
            s = slice(A.indptr[r], A.indptr[r + 1])
            parts[r].append(-p[s])
            parts[r].append(-e[s])
        absum += abs(A) @ np.abs(x)
        k += np.diff(A.indptr)
    return np.array([math.fsum(np.concatenate(q)) for q in parts]), absum, k


# Roundings of relin_residual_v_kernel beyond the stored entries of the row sums, tau, tau / 2,
# tau / beta dyadic (their products are exact).  BE: tau D z + M z; d - (.); -tau M v + M z';
# out += (.); out -= tau B^T mu: 5 (the state rows alike).  CN: M v0 + M v1; d - h (.);
# h D^T z0 + M z0; - (.); h D^T z1 - M z1; - (.); - tau B^T mu: 7 (the state rows alike).
def _c_roundings(CN):
    return 7 if CN else 5


def _velocity_terms(pb, plan, D2, state, fam, i, cache):
    """The products of velocity row block (fam, i) as ``(A, x)`` with the row ``data - sum A x``,
    from picard.non_linear_res_eval; the dyadic coefficients are folded into ``x``.  ``cache``
    keeps the level matrices built from ``D2``."""
    v, zeta, p, mu = state
    tau, beta, n_t = pb.tau, pb.beta, pb.n_t
    I2 = sp.identity(2, format="csr")
    K2 = plan.K2

    def D(l, transpose=False):
        if (l, transpose) not in cache:
            data = _transposed(D2[l], K2) if transpose else D2[l]
            cache[(l, transpose)] = sp.kron(
                I2, sp.csr_matrix((data, K2.indices, K2.indptr), shape=K2.shape), format="csr")
        return cache[(l, transpose)]
    M = pb.disc.M_v
    BT = sp.csr_matrix(pb.disc.B.T)
    if not pb.CN:
        if fam == 0:
            t = [(D(i, True), tau * zeta[i]), (M, zeta[i])]
            if i < n_t - 1:
                t += [(M, tau * v[i]), (M, -zeta[i + 1])]
            return t + [(BT, tau * mu[i])]
        t = [(D(i), tau * v[i]), (M, v[i])]
        if i >= 1:
            t += [(M, -v[i - 1]), (M, -(tau / beta) * zeta[i])]
        return t + [(BT, tau * p[i])]
    h = 0.5 * tau
    if fam == 0:
        return [(M, h * v[i]), (M, h * v[i + 1]), (D(i, True), h * zeta[i]), (M, zeta[i]),
                (D(i + 1, True), h * zeta[i + 1]), (M, -zeta[i + 1]), (BT, tau * mu[i])]
    return [(D(i), h * v[i]), (M, -v[i]), (D(i + 1), h * v[i + 1]), (M, v[i + 1]),
            (M, -(h / beta) * zeta[i]), (M, -(h / beta) * zeta[i + 1]), (BT, tau * p[i])]


def _ratio(got, ref, absum, k, c, data):
    bound = (k + c) * U * absum + U * np.abs(data)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.inf)).max())


def _check_residual(pb, dev, state, r, host, rows=None):
    """Every row block of the device residual ``r`` and of the host's against the exact rows;
    returns the worst ratios (device, host) of error to bound."""
    th, plan = pb.disc, dev.plan
    m, nv, n1 = plan.m, th.n_v, th.n_p
    D2 = dev.debug_array("D2")
    v, zeta = state[0], state[1]
    c = _c_roundings(pb.CN)
    bc = np.zeros(nv, dtype=bool)
    bc[th.boundary_v] = True
    pick = np.arange(nv) if rows is None else rows
    worst, cache = [0.0, 0.0], {}
    for rb in range(2 * m):
        fam, i = divmod(rb, m)
        data = plan.data[rb]
        ref, absum, k = _exact_rows(data, _velocity_terms(pb, plan, D2, state, fam, i, cache),
                                    rows)
        free = ~bc[pick]
        for w, vec in enumerate((r, host)):
            got = vec[rb * nv:(rb + 1) * nv][pick]
            assert np.all(got[~free] == 0.0), (rb, w)          # Dirichlet rows
            worst[w] = max(worst[w], _ratio(got[free], ref[free], absum[free], k[free], c,
                                            data[pick][free]))
    if rows is not None:         # (a subset of the velocity rows: the pressure rows are not asked)
        return worst
    off = 2 * m * nv
    for rb in range(2 * m):      # -B v (CN: the level i + 1) and -B zeta
        fam, i = divmod(rb, m)
        x = zeta[i] if fam else v[i + 1 if pb.CN else i]
        ref, absum, k = _exact_rows(np.zeros(n1), [(th.B, x)])
        for w, vec in enumerate((r, host)):
            got = vec[off + rb * n1:off + (rb + 1) * n1]
            worst[w] = max(worst[w], _ratio(got, ref, absum, k, 0, np.zeros(n1)))
    return worst


def _host_residual(pb, state):
    D = [pb.D_v(x) for x in state[0]]
    return np.concatenate([np.ravel(x) for x in picard.non_linear_res_eval(pb, D, *state)])


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [2, 3, 5])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_residual_against_correctly_rounded_rows(mesh_name, n_t, CN):
    pb = _problem(MESHES[mesh_name], n_t, CN)
    rng = np.random.default_rng(common.SEED + 3 + n_t)
    state = _state(pb, rng)
    outer, dev = _bare(pb)
    dev.set_state(*state)
    dev.assemble()
    r, norm = _residual(outer, dev, rhs=False)
    worst = _check_residual(pb, dev, state, r, _host_residual(pb, state))
    print(f"{mesh_name} n_t={n_t} CN={CN}: worst error / bound = {worst[0]:.3f} (device), "
          f"{worst[1]:.3f} (host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    ref = np.linalg.norm(r)
    assert abs(norm - ref) <= 4 * U * np.sqrt(r.size) * ref


# ------------------------------------------------------------------------ right-hand side
def _host_rhs(pb, r, m):
    """The rows the host loop hands to the linear solve (picard.incompressible_non_linear_solve):
    pressure rows times tau, CN: T_1 / T_2 with its pairing.  Also the two summands of every
    entry (the second zero where nothing is added)."""
    nv, n1 = pb.disc.n_v, pb.disc.n_p
    r0 = r[:2 * m * nv].reshape(2 * m, nv)
    r1 = r[2 * m * nv:].reshape(2 * m, n1)
    r00, r01, s10, s11 = r0[:m], r0[m:], pb.tau * r1[:m], pb.tau * r1[m:]
    parts = [r00, r01, s10, s11]
    if pb.CN:
        out = [picard._apply_T_1(r00), picard._apply_T_2(r01), picard._apply_T_2(s10),
               picard._apply_T_1(s11)]
    else:
        out = parts
    b = np.concatenate([np.ravel(x) for x in out])
    a = np.concatenate([np.ravel(x) for x in parts])
    return b, a, b - a


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("tau", [0.5, 0.3])
def test_right_hand_side(tau, CN):
    pb = _problem(MESHES["anisotropic"], 4, CN, tau=tau)
    if tau == 0.3:
        assert math.frexp(pb.tau)[0] != 0.5            # not a power of two
    rng = np.random.default_rng(common.SEED + 4)
    outer, dev = _bare(pb)
    dev.set_state(*_state(pb, rng))
    dev.assemble()
    r, norm_r = _residual(outer, dev, rhs=False)
    b, norm_b = _residual(outer, dev, rhs=True)
    m, nv = dev.plan.m, pb.disc.n_v
    want, first, second = _host_rhs(pb, r, m)
    assert np.any(r[2 * m * nv:] != 0.0)
    if tau == 0.5:
        assert np.array_equal(b, want)
    else:
        # tau r + (tau r') may be contracted into one fma: one rounding less on one product
        assert np.all(np.abs(b - want) <= U * (np.abs(first) + np.abs(second)))
    if not CN:
        assert np.array_equal(b[:2 * m * nv], r[:2 * m * nv])
        assert np.array_equal(b[2 * m * nv:], pb.tau * r[2 * m * nv:])
    else:
        assert np.any(b[:2 * m * nv] != r[:2 * m * nv])
    assert norm_b == norm_r                            # the norm of r, not of b
    assert abs(norm_b - np.linalg.norm(r)) <= 4 * U * np.sqrt(r.size) * np.linalg.norm(r)
    assert np.linalg.norm(b) != np.linalg.norm(r)


# --------------------------------------------------------------------------------- update
def _check_update(pb, outer, dev, rng):
    th, m = pb.disc, dev.plan.m
    nv, n1, cn = th.n_v, th.n_p, int(pb.CN)
    old = _state(pb, rng)
    assert np.all(old[1][:, th.boundary_v] != 0.0)
    dev.set_state(*old)
    u = rng.standard_normal(outer.local_size)
    assert u.size == 2 * m * (nv + n1)
    u0 = u[:2 * m * nv].reshape(2 * m, nv)
    u1 = u[2 * m * nv:].reshape(2 * m, n1)
    with _Vec(outer, u) as d:
        dev.update(d.d)
        left = d.get()
    v, zeta, p, mu = dev.get_state()
    want_v = old[0].copy()
    want_v[cn:cn + m] += u0[:m]              # unknown block i: v at level i (CN: i + 1)
    want_z = old[1].copy()
    want_z[:m] += u0[m:]
    want_z[:, th.boundary_v] = 0.0           # every level, also the last one under CN
    assert np.array_equal(v, want_v)
    if cn:
        assert np.array_equal(v[0], old[0][0])
    assert np.array_equal(zeta, want_z)
    assert np.array_equal(mu, old[3] + u1[:m]) and np.array_equal(p, old[2] + u1[m:])
    assert np.array_equal(left, np.zeros_like(left))


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("n_t", [2, 4])
def test_update(n_t, CN):
    pb = _problem(MESHES["anisotropic"], n_t, CN)
    outer, dev = _bare(pb)
    _check_update(pb, outer, dev, np.random.default_rng(common.SEED + 5))


# ----------------------------------------------------------------------- grid-stride tails
def test_tails_of_rhs_update_and_compose():
    """n = 32, n_t = 28 (BE): the rhs / update range and one velocity block's padded slots
    exceed their launch caps; bitwise references only."""
    pb = _problem((32, 32, 2.0, 2.0), 28, False)
    th = pb.disc
    outer, dev = _bare(pb, velocity_blocks=((0, 0),))
    m, nv, n1 = dev.plan.m, th.n_v, th.n_p
    assert 2 * m * (nv + n1) > RHS_UPDATE_CAP
    assert 2 * dev.plan.K2.nnz > COMPOSE_CAP          # the padded slots hold every entry
    rng = np.random.default_rng(common.SEED + 6)
    dev.set_state(*_state(pb, rng))
    dev.assemble()
    r, _ = _residual(outer, dev, rhs=False)
    b, _ = _residual(outer, dev, rhs=True)
    assert np.array_equal(b, _host_rhs(pb, r, m)[0])
    assert np.any(b[RHS_UPDATE_CAP:] != 0.0)
    recipe = [(0, 0, 0, 27, pb.tau, True, 1.0)]
    dev.relinearise(outer, "outer", recipes=recipe)
    _check_blocks(dev, outer, recipe, 0, dev.debug_array("D2"), True)
    _check_update(pb, outer, dev, rng)


def test_tails_of_gather_and_residual():
    """n = 128, n_t = 6 (BE): the rows of a residual row block and the gather's range exceed
    their launch caps."""
    pb = _problem((128, 128, 2.0, 2.0), 6, False)
    th = pb.disc
    outer, dev = _bare(pb)
    nv = th.n_v
    assert nv > RESIDUAL_CAP and dev.plan.K2.nnz * pb.n_t > GATHER_CAP
    rng = np.random.default_rng(common.SEED + 7)
    state = _state(pb, rng)
    dev.set_state(*state)
    dev.assemble()
    Ev, D2 = dev.debug_array("Ev"), dev.debug_array("D2")
    for l in range(pb.n_t):
        want = pb.nu * dev.plan.K2.data + relinearise.gather(Ev[l], *dev.plan.v_lists)
        assert np.array_equal(D2[l], want), l
    r, norm = _residual(outer, dev, rhs=False)
    host = _host_residual(pb, state)
    assert common.rel_err(r, host) <= 1e-12
    tail = np.arange(RESIDUAL_CAP, nv)
    worst = _check_residual(pb, dev, state, r, host, rows=tail)
    print(f"n = 128 rows past the cap: worst error / bound = {worst[0]:.3f} (device), "
          f"{worst[1]:.3f} (host)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


# -------------------------------------------------------------------------------- refusals
def test_errors():
    """What ``kkt_relinearise_device`` refuses, and that a refused call writes nothing."""
    pb = _problem(MESHES["square"], 3, False)
    good = (0, 0, 0, 0, pb.tau, False, 1.0)
    # composing before any assembly; the block stays unset
    outer, dev = _bare(pb)
    with pytest.raises(_lib.KktError) as err:
        dev.relinearise(outer, "outer", recipes=[good])
    assert err.value.code == -3
    with pytest.raises(_lib.KktError) as err:
        outer.mult(np.zeros(outer.local_size))
    assert err.value.code == -3

    ls, dev = _full(pb, _state(pb, np.random.default_rng(common.SEED + 8)))
    full = blocks.instationary_build_recipes(pb.tau, pb.beta, pb.n_t, pb.CN)
    lib, plan_handle = ls.outer._lib, ls.outer.handle
    for name, system in (("outer", ls.outer), ("inner", ls.inner), ("commutator", ls.comm)):
        space = 1 if name == "commutator" else 0
        q, i, j, level, alpha, transpose, gamma = full[name][0]
        before, _ = system.block_values(q, i, j)
        assert np.any(before != 0.0)

        def refused(recipe, as_space=space):
            arr = relinearise._recipe_array([recipe], as_space)
            code = lib.kkt_relinearise_device(system.handle, plan_handle, None, 1, arr)
            message = lib.kkt_last_error(system.handle)
            assert np.array_equal(system.block_values(q, i, j)[0], before)   # nothing written
            return code, message

        code, message = refused((q, i, 99, level, 0.7, transpose, 0.3))
        assert code == -1 and message.startswith(b"kkt_relinearise_device: recipe 0: no such block")
        assert refused((q, i, j, level, 0.7, transpose, 0.3), as_space=2)[0] == -1
        assert refused((q, i, j, pb.n_t, 0.7, transpose, 0.3))[0] == -1
        assert refused((q, i, j, -1, 0.7, transpose, 0.3))[0] == -1
        # a block of the other space: its pattern is not the plan's pattern of the space asked for
        code, message = refused((q, i, j, level, 0.7, transpose, 0.3), as_space=1 - space)
        assert code == -1 and (b"velocity pattern", b"pressure pattern")[1 - space] in message
