"""The host plan of the scalar device loop (``control_amd.reaction.ReactionPlan``, no GPU): its
contribution lists reproduce the host assembly bit for bit, its data rows are the residual at the
zero iterate, and everything ``non_linear_solve(device=True)`` refuses is refused before the GPU
is touched."""
import numpy as np
import pytest

import common
import reaction_ref
from control_amd import fem, relinearise
from control_amd.control import Instationary
from control_amd.reaction import ReactionPlan


@pytest.mark.parametrize("mesh", [(2, 2, 2.0, 2.0), (3, 2, 3.0, 1.0), (8, 8, 1.0, 1.0)])
def test_lists_reproduce_the_host_assembly(mesh):
    disc = fem.rectangle_p1(*mesh)
    term = fem.ReactionTerm(disc, (1.25, -0.75, 0.5, -2.0, 0.375))
    plan = ReactionPlan(Instationary(disc, term, desired_state=lambda X, t: X[:, 0], n_t=3))
    cptr, clist = plan.lists
    assert cptr[-1] == len(clist) == 9 * len(term.cells)
    rng = np.random.default_rng(common.SEED)
    for _ in range(2):
        v = rng.standard_normal(disc.n_dofs)
        E = term.element_matrices(v)
        assert np.array_equal(relinearise.gather(E, cptr, clist), term.reaction_values(v))
    M = term.M
    assert np.array_equal(M.data[plan.tperm], M.T.tocsr().sorted_indices().data)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("newton", [False, True])
def test_data_rows_are_the_residual_at_the_zero_iterate(CN, newton):
    ctl = reaction_ref.reaction_heat_control(
        CN, force_f=lambda X, t: (1.0 + t) * X[:, 1],
        initial_condition=lambda X: np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]),
        bcs_v=lambda Xb, t: 0.1 * (1.0 + t) * np.ones(len(Xb)))
    ctl.set_Gauss_Newton(newton)
    plan = ReactionPlan(ctl)
    assert plan.coefficients == ((2.0, 0.0, 1.5) if newton else (2.0, 0.0, 0.5))
    disc = ctl._disc
    z = np.zeros((ctl._n_t, disc.n_dofs))
    v_0 = np.asarray(ctl._initial_condition(disc.coords))
    r0, r1 = ctl.non_linear_res_eval(z, z.copy(), v_0, ctl.construct_v_d(), ctl.construct_f())
    assert plan.data.shape == (2 * plan.m, disc.n_dofs)
    assert np.array_equal(plan.data, np.concatenate([r0, r1]))
    assert np.any(plan.data[plan.m] != 0.0) or CN         # backward Euler's initial-condition row


def test_what_is_refused_is_refused_without_a_gpu():
    with pytest.raises(ValueError):
        fem.ReactionTerm(fem.unit_square_q2(2), (2.0, 0.0, 0.5))
    with pytest.raises(ValueError):
        fem.ReactionTerm(fem.unit_cube_p1(2), (2.0, 0.0, 0.5))
    disc = fem.unit_square_p1(4)
    with pytest.raises(ValueError):
        fem.ReactionTerm(disc, (1.0, 0.0, 0.0, 0.0, 0.0, 1.0))        # degree 5
    with pytest.raises(ValueError):
        fem.ReactionTerm(disc, ())
    ctl = reaction_ref.reaction_heat_control(False, declared=False, n=4, n_t=3)
    with pytest.raises(ValueError, match="ReactionTerm"):
        ctl.non_linear_solve(device=True)
    ctl = reaction_ref.reaction_heat_control(False, n=4, n_t=3)
    with pytest.raises(ValueError, match="P="):
        ctl.non_linear_solve(device=True, P=lambda *a: None)
    th = fem.rectangle_p2p1(2, 2)
    ctl = Instationary(th, None, desired_state=lambda X, t: np.zeros(th.n_v), n_t=3)
    with pytest.raises(ValueError):
        ctl.non_linear_solve(device=True)
