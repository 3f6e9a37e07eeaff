"""The NumPy mirror of the Anderson mixer (``control_amd/anderson.py``) against the independent
reference ``tests/anderson_ref.py``, its properties, the drivers' refusals and the host loops with
``anderson=``.  No GPU: the host loops run on the CPU oracle backend."""
from fractions import Fraction

import numpy as np
import pytest

import anderson_ref as ref
import common
from control_amd import fem, picard
from control_amd.anderson import AndersonMixer, HostAnderson, check_anderson
from control_amd.control import Stationary

N = 257


def _vectors(count, n=N, seed=0):
    """Updates of a contracting iteration: decaying, with fresh directions."""
    rng = np.random.default_rng(common.SEED + seed)
    return [0.6 ** k * rng.standard_normal(n) for k in range(count)]


def _run(mixer, fs):
    steps, infos = [], []
    for f in fs:
        steps.append(mixer.step(f))
        infos.append(mixer.info)
    return steps, infos


# ------------------------------------------------------------------ against the reference
def test_gram_entries_against_exact_dots():
    fs = _vectors(6)
    m = AndersonMixer(N, 3)
    for f, info in zip(fs, _run(m, fs)[1]):
        c = info["columns"]
        G, r = ref.gram_exact(info["dF"], f)
        for i in range(c):
            assert abs(Fraction(info["r"][i]) - r[i]) <= ref.dot_bound(info["dF"][i], f)
            for j in range(c):
                assert abs(Fraction(info["G"][i, j]) - G[i][j]) <= \
                    ref.dot_bound(info["dF"][i], info["dF"][j])


def test_gamma_within_the_cholesky_bound_of_the_solve_of_its_own_system():
    fs = _vectors(8, seed=1)
    m = AndersonMixer(N, 3)
    seen = 0
    for info in _run(m, fs)[1]:
        c = info["columns"]
        if c == 0:
            continue
        want, ratio = ref.solve_mp(info["G"], info["r"])
        assert ratio <= 1.0e3          # the data keeps the factor's diagonal within 1e3
        err = np.abs(info["gamma"] - want).max() / np.abs(want).max()
        assert err <= ref.gamma_bound(c, ratio)
        seen += 1
    assert seen == 7


@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_step_is_the_unfused_statement_bit_for_bit(beta):
    fs = _vectors(6, seed=2)
    m = AndersonMixer(N, 3, beta=beta)
    steps, infos = _run(m, fs)
    for f, s, info in zip(fs, steps, infos):
        want = ref.mix_unfused(f, info["dX"], info["dF"], info["gamma"], beta)
        assert np.array_equal(s, want)
    assert np.array_equal(steps[0], beta * fs[0])
    assert [i["columns"] for i in infos] == [0, 1, 2, 3, 3, 3]


# ------------------------------------------------------------------ properties
def test_finite_termination_on_an_affine_map():
    """``x -> A x + b`` in dimension 5, ``||A||_2 = 0.9``, depth 5: after 5 + 1 steps the update
    ``A x + b - x`` is at round-off; plain iteration has reduced it by 0.9^6 at best.  Bar: 1e3 x
    the update norm at the direct solve's solution (measured: 5.4e-16, so the bar is 5.4e-13; the
    accelerated iteration reaches 3.9e-16, the plain one 2.8e-2)."""
    d = 5
    rng = np.random.default_rng(common.SEED + 3)
    Q1, _ = np.linalg.qr(rng.standard_normal((d, d)))
    Q2, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = Q1 @ np.diag([0.9, 0.7, 0.5, 0.3, 0.1]) @ Q2
    b = rng.standard_normal(d)
    x_star = np.linalg.solve(np.eye(d) - A, b)
    bar = 1.0e3 * np.linalg.norm(A @ x_star + b - x_star)

    def iterate(mixer):
        x = np.zeros(d)
        for _ in range(d + 1):
            f = A @ x + b - x
            x = x + (mixer.step(f) if mixer else f)
        return np.linalg.norm(A @ x + b - x)
    plain, mixed = iterate(None), iterate(AndersonMixer(d, d))
    print(f"direct {bar / 1e3:.2e}, accelerated {mixed:.2e}, plain {plain:.2e}")
    assert mixed <= bar < plain


def test_ring_wraps_at_depth_two():
    fs = _vectors(6, seed=4)
    m = AndersonMixer(N, 2)
    steps, infos = [], []
    for k, f in enumerate(fs):
        steps.append(m.step(f))
        infos.append(m.info)
        dF, dX = ref.expected_ring(fs[:k + 1], steps[:k], 2, [i["dropped"] for i in infos])
        assert len(m.info["dF"]) == len(dF) == min(k, 2)
        for a, b in zip(m.info["dF"] + m.info["dX"], dF + dX):
            assert np.array_equal(a, b)
    assert [i["columns"] for i in infos] == [0, 1, 2, 2, 2, 2]


def test_equal_consecutive_updates_drop_the_zero_column():
    f = _vectors(1, seed=5)[0]
    m = AndersonMixer(N, 3)
    m.step(f)
    s = m.step(f.copy())
    assert (m.info["columns"], m.info["dropped"]) == (0, 1)
    assert np.array_equal(s, f)                      # the plain step again
    m.step(0.5 * f)
    assert (m.info["columns"], m.info["dropped"]) == (1, 0)


@pytest.mark.parametrize("factor, dropped", [(2.0, 1), (0.5, 0)])
def test_near_parallel_columns_around_cond_max(factor, dropped):
    """Columns ``e_1`` and ``e_1 + eps e_2``: ``L = [[1, 0], [1, eps]]``, diagonal ratio
    ``1 / eps`` -- twice above ``cond_max`` the older column goes, twice below both stay."""
    cond_max = 1.0e7
    eps = 1.0 / (factor * cond_max)
    e1, e2 = np.eye(N)[0], np.eye(N)[1]
    m = AndersonMixer(N, 3, cond_max=cond_max)
    for f in (np.zeros(N), e1, 2.0 * e1 + eps * e2):
        m.step(f)
    assert (m.info["columns"], m.info["dropped"]) == (2 - dropped, dropped)
    assert ref.solve_mp(np.array([[1.0, 1.0], [1.0, 1.0 + eps * eps]]), [1.0, 1.0])[1] == \
        pytest.approx(factor * cond_max, rel=0.1)


def test_pass_through_and_reset():
    fs = _vectors(4, seed=6)
    m = AndersonMixer(N, 3)
    first = m.step(fs[0])
    assert first.tobytes() == fs[0].tobytes()        # beta = 1, no pairs: the input's bits
    second = m.step(fs[1])
    m.reset()
    assert m.step(fs[0]).tobytes() == first.tobytes() and m.info["columns"] == 0
    assert m.step(fs[1]).tobytes() == second.tobytes() and m.info["columns"] == 1


def test_damping_one_half():
    fs = _vectors(3, seed=7)
    m = AndersonMixer(N, 2, beta=0.5)
    s0 = m.step(fs[0])
    assert np.array_equal(s0, 0.5 * fs[0])
    m.step(fs[1])
    assert np.array_equal(m.info["dX"][0], s0) and np.array_equal(m.info["dF"][0], fs[1] - fs[0])


# ------------------------------------------------------------------ refusals
class _TwoRanks:
    world = 2


def _scalar(CN=True, n=6):
    from test_gpu_reaction_p2_picard import reaction_heat_control_p2
    return reaction_heat_control_p2(CN, n=n)


@pytest.mark.parametrize("device", [False, True])
def test_the_drivers_refuse_before_any_work(device):
    ctl = _scalar()
    with pytest.raises(ValueError, match="0..8"):
        ctl.non_linear_solve(device=device, anderson=9)
    with pytest.raises(ValueError, match="0..8"):
        ctl.non_linear_solve(device=device, anderson=-1)
    with pytest.raises(ValueError, match="time shards"):
        ctl.non_linear_solve(device=True, comm=_TwoRanks(), anderson=3)
    ctl.set_Gauss_Newton()
    with pytest.raises(ValueError, match="Gauss_Newton"):
        ctl.non_linear_solve(device=device, anderson=3)
    disc = fem.unit_square_p1(4)
    st = Stationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)),
                    desired_state=lambda X: X[:, 0], beta=1.0)
    with pytest.raises(ValueError, match="0..8"):
        st.non_linear_solve(device=device, anderson=9)
    st.set_Gauss_Newton()
    with pytest.raises(ValueError, match="Gauss_Newton"):
        st.non_linear_solve(device=device, anderson=2)
    pb = common.navier_stokes_problem()
    solver = common.OracleLinearSolver(pb)
    with pytest.raises(ValueError, match="0..8"):
        picard.incompressible_non_linear_solve(pb, solver, anderson=9, device=device)
    solver.dist = _TwoRanks()            # what a time-sharded GpuLinearSolver carries
    with pytest.raises(ValueError, match="time shards"):
        picard.incompressible_non_linear_solve(pb, solver, anderson=2, device=device)
    from test_control_driver import _stationary_navier_stokes_control
    ns = _stationary_navier_stokes_control()[0]
    with pytest.raises(ValueError, match="0..8"):
        ns.incompressible_non_linear_solve(device=device, anderson=-2)
    with pytest.raises(ValueError, match="0..8"):
        ns.incompressible_non_linear_solve(device=device, anderson=2.5)


def test_the_mixers_argument_errors():
    """The arguments ``kkt_anderson_set`` refuses with ``KKT_ERR_ARG`` (the C-ABI needs a GPU to
    make a handle: ``tests/test_gpu_anderson_kernels.py``), refused alike by the mirror."""
    for kw in (dict(depth=9), dict(depth=0), dict(depth=3, cond_max=1.0), dict(depth=3, beta=0.0),
               dict(depth=3, cond_max=0.5)):
        with pytest.raises(ValueError):
            AndersonMixer(N, **kw)
    assert check_anderson(0, 1.0, _TwoRanks(), True) == 0    # off: nothing to refuse


# ------------------------------------------------------------------ the host loops
def _field_distance(a, b):
    return max(np.abs(x - y).max() for x, y in zip(a, b))


def test_host_loop_scalar_crank_nicolson():
    """``unit_square_p2(6)`` x 4 levels, Crank-Nicolson, coefficients (2, 0, 0.5), non-linear rtol
    1e-9, through the CPU oracle backend: plain Picard takes 29 iterations, ``anderson=3`` takes 8
    (measured here).  Fields: within ten times the distance between the plain loop's fields at
    rtol 1e-9 and 1e-11 (that distance: 2.2e-9, the accelerated loop's distance to the plain
    fields at 1e-9: 2.5e-9)."""
    from test_gpu_reaction_p2_picard import KAT_SP, MASS, SCHUR

    def loop(rtol, **kw):
        ctl = _scalar(True)
        norms = ctl.non_linear_solve(solver_parameters=KAT_SP, lambda_v_bounds=MASS,
                                     relative_non_linear_tol=rtol, absolute_non_linear_tol=0.0,
                                     backend=common.OracleBackend(schur=SCHUR),
                                     max_non_linear_iter=60, **kw)
        return norms, (ctl._v.copy(), ctl._zeta.copy()), getattr(ctl, "non_linear_info", None)
    plain, fields, _ = loop(1.0e-9)
    _, tighter, _ = loop(1.0e-11)
    mixed, got, info = loop(1.0e-9, anderson=3)
    bar = 10.0 * _field_distance(fields, tighter)
    print(f"Picard iterations plain {len(plain) - 1}, anderson=3 {len(mixed) - 1}; bar {bar:.2e}, "
          f"distance {_field_distance(got, fields):.2e}")
    assert mixed[-1] <= 1.0e-9 * mixed[0]
    assert len(mixed) < len(plain)
    assert _field_distance(got, fields) <= bar
    assert len(info["anderson"]) == len(mixed) - 1
    assert all(c <= min(k, 3) for k, (c, _) in enumerate(info["anderson"]))
    nodes = _scalar()._disc.boundary
    assert np.all(got[1][:, nodes] == 0.0) and np.array_equal(got[0][:, nodes], fields[0][:, nodes])


def test_host_loop_cavity():
    """The cavity of ``tests/test_picard.py`` (8 x 8, n_t = 10, nu = 1/100, backward Euler, rtol
    1e-5, budget 10): plain needs 6 iterations, so ``anderson=3`` must converge within the budget
    in no more (measured: 6 and 6).  Fields: within ten times the distance between the plain
    loop's fields at rtol 1e-5 and at 1e-7 -- how far an iterate converged to this case's
    tolerance still moves (measured: 1.3e-5 apart, bar 1.3e-4; accelerated to plain 1.4e-5)."""
    from test_picard import NS_SPECS, _cavity

    def loop(rtol=1.0e-5, **kw):
        pb, v_init, _ = _cavity(8, 10, False)
        return picard.incompressible_non_linear_solve(
            pb, common.OracleLinearSolver(pb, specs=NS_SPECS), v=v_init, max_non_linear_iter=10,
            relative_non_linear_tol=rtol, print_error_non_linear=False, **kw)
    names = ("v", "zeta", "p", "mu")
    plain, tighter, mixed = loop(), loop(1.0e-7), loop(anderson=3)
    bar = 10.0 * _field_distance([plain[k] for k in names], [tighter[k] for k in names])
    dist = _field_distance([mixed[k] for k in names], [plain[k] for k in names])
    print(f"Picard iterations plain {len(plain['norms']) - 1}, anderson=3 "
          f"{len(mixed['norms']) - 1}; bar {bar:.2e}, distance {dist:.2e}")
    assert plain["converged"] and mixed["converged"]
    assert len(mixed["norms"]) <= len(plain["norms"]) <= 11
    assert dist <= bar
    assert len(mixed["anderson"]) == len(mixed["norms"]) - 1
    th = _cavity(8, 10, False)[0].disc
    assert np.array_equal(mixed["v"][:, th.boundary_v], plain["v"][:, th.boundary_v])
    assert np.all(mixed["zeta"][:, th.boundary_v] == 0.0)


def test_host_loops_stationary():
    """The two stationary host loops with the keyword.  Scalar: ``unit_square_p1(8)``, desired
    state of amplitude 8, beta = 1e-2, rtol 1e-9 -- plain 21 iterations, ``anderson=3`` 7.
    Navier-Stokes: the problem of ``tests/test_control_driver.py`` (N = 4, nu = 1, rtol 1e-8) --
    plain 5, ``anderson=2`` 4 (asserted: no more than plain)."""
    from test_control_driver import MMS_STOKES_SP, _stationary_navier_stokes_control
    from test_gpu_reaction_p2_picard import KAT_SP
    disc = fem.unit_square_p1(8)

    def v_d(X):
        return 8.0 * np.prod(np.sin(np.pi * X), axis=1) * np.exp(X[:, 0] + X[:, 1])

    def scalar(**kw):
        ctl = Stationary(disc, fem.ReactionTerm(disc, (2.0, 0.0, 0.5)), desired_state=v_d,
                         beta=1.0e-2)
        norms = ctl.non_linear_solve(solver_parameters=KAT_SP, lambda_v_bounds=(0.5, 2.0),
                                     relative_non_linear_tol=1.0e-9, absolute_non_linear_tol=0.0,
                                     max_non_linear_iter=60,
                                     backend=common.OracleBackend(schur=(40, 0.02, 2.2)), **kw)
        return norms, ctl

    def navier_stokes(**kw):
        ctl, th, D_p = _stationary_navier_stokes_control()
        norms = ctl.incompressible_non_linear_solve(
            forward_operator_p=D_p, solver_parameters=MMS_STOKES_SP,
            lambda_v_bounds=(0.3924, 2.0598), lambda_p_bounds=(0.5, 2.0), max_non_linear_iter=20,
            relative_non_linear_tol=1.0e-8, absolute_non_linear_tol=0.0,
            backend=common.OracleBackend(schur=(40, 0.01, 2.25)), **kw)
        return norms, ctl
    for loop, depth, rtol in ((scalar, 3, 1.0e-9), (navier_stokes, 2, 1.0e-8)):
        plain, _ = loop()
        mixed, ctl = loop(anderson=depth)
        print(f"{loop.__name__}: Picard iterations plain {len(plain) - 1}, anderson={depth} "
              f"{len(mixed) - 1}")
        assert mixed[-1] <= rtol * mixed[0] and len(mixed) <= len(plain)
        hist = ctl.non_linear_info["anderson"]
        assert len(hist) == len(mixed) - 1 and all(c <= depth for c, _ in hist)
        assert np.all(ctl._zeta[ctl._disc.boundary] == 0.0)


def test_host_mixer_keeps_the_blocks_shapes():
    h = HostAnderson(2)
    a, b = np.arange(6.0).reshape(2, 3), np.arange(4.0)
    x, y = h.step(a, b)
    assert x.shape == a.shape and y.shape == b.shape
    assert np.array_equal(x, a) and np.array_equal(y, b) and h.history == [(0, 0)]
