"""The device re-linearisation kernels on Q2-Q1 quadrilaterals, by the scheme of
``tests/test_gpu_relin_kernels.py`` (whose helpers and bit-for-bit tests take any plan):

* ``relin_elements_q2q1_kernel`` against the exact rational reference of
  ``tests/relin_q2_ref.py`` within ``ELEMENT_BAR_Q2 u S`` (that file derives the number; the host
  statement is held to the same one in ``tests/test_relin_q2_ref.py``), a zero level exactly zero;
* the ordered gather (``D2``, ``Dp`` = ``nu K + relinearise.gather(downloaded E)``), the composed
  block values, the right-hand side (dyadic ``tau``) and the update bit for bit, and the residual
  by the correctly rounded rows from the downloaded ``D2`` -- the triangles' tests, run on
  ``fem.rectangle_q2q1`` discretisations put in the place of their meshes;
* one shape whose pairs fill one workgroup and part of a second;
* the descriptor checks of ``kkt_set_relinearisation`` on ``nv``.

Pairs per workgroup: the element kernel gives three lanes to an (element, level) pair, so a
workgroup of 256 lanes holds 85 pairs and the first lane of the 86th.  6 x 5 cells x 3 levels are
90 pairs: workgroup 0 works on pairs 0..84 and on row block 0 of pair 85, workgroup 1 (14 live
lanes) on the rest of pair 85 and on pairs 86..89.
"""
import ctypes as C

import numpy as np
import pytest

import common
import relin_q2_ref as ref
import test_gpu_relin_kernels as p2p1
from control_amd import fem

pytestmark = pytest.mark.gpu

BAR = ref.ELEMENT_BAR_Q2
MESHES = {"square": (2, 2, 2.0, 2.0), "anisotropic": (3, 2, 3.0, 1.0)}
WINDS = p2p1.WINDS
KKT_ERR_ARG = -1
_DISCS = {}


def _disc(mesh_name):
    if mesh_name not in _DISCS:
        _DISCS[mesh_name] = fem.rectangle_q2q1(*MESHES[mesh_name])
    return _DISCS[mesh_name]


@pytest.fixture(autouse=True)
def _quadrilaterals(monkeypatch):
    """The triangles' tests build their problems through ``_problem(MESHES[name], ...)``, which
    takes a discretisation as it is."""
    monkeypatch.setattr(p2p1, "MESHES", {name: _disc(name) for name in MESHES})


# ----------------------------------------------------------------------- element matrices
def _check_elements(dev, v, exact):
    Ev, Ep = dev.debug_array("Ev"), dev.debug_array("Ep")
    ne = len(dev.plan.V)
    assert Ev.shape == (len(v), ne, 9, 9) and Ep.shape == (len(v), ne, 4, 4)
    worst_v = worst_p = 0.0
    for l, (Xv, Xp, Sv, Sp) in enumerate(exact):
        worst_v = max(worst_v, ref.worst_ratio(Ev[l], Xv, Sv))
        worst_p = max(worst_p, ref.worst_ratio(Ep[l], Xp, Sp))
        if not v[l].any():
            assert np.array_equal(Ev[l], np.zeros_like(Ev[l]))
            assert np.array_equal(Ep[l], np.zeros_like(Ep[l]))
    return worst_v, worst_p


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("kind", WINDS)
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_element_kernel_against_the_exact_reference(mesh_name, kind, CN):
    th = _disc(mesh_name)
    pb = p2p1._problem(th, 3, CN)
    v = p2p1._winds(kind, th)
    outer, dev = p2p1._bare(pb)
    dev.set_state(*p2p1._state(pb, np.random.default_rng(common.SEED), v))
    dev.assemble()
    worst_v, worst_p = _check_elements(dev, v,
                                       ref.exact_elements(MESHES[mesh_name], kind, p2p1._winds))
    print(f"{mesh_name} {kind} CN={CN}: device worst err / (u S) = {worst_v:.2f} (velocity), "
          f"{worst_p:.2f} (pressure), bar {BAR}")
    assert worst_v <= BAR and worst_p <= BAR


def test_one_workgroup_and_part_of_a_second():
    """90 pairs (see the module's docstring): every pair against the exact reference, the pair
    split between the two workgroups included, and the arrays around ``Ev`` / ``Ep`` in the plan's
    memory as they should be after the assembly: ``D2`` / ``Dp`` the gather of what was
    downloaded, the iterate's windows untouched."""
    th = fem.rectangle_q2q1(6, 5, 3.0, 2.5)
    pb = p2p1._problem(th, 3, False)
    ne = len(th.elem["V"])
    assert ne * 3 == 90 and 256 < 3 * 90 < 512 and 256 % 3 == 1
    v = p2p1._winds("normal", th)
    state = p2p1._state(pb, np.random.default_rng(common.SEED + 1), v)
    outer, dev = p2p1._bare(pb)
    dev.set_state(*state)
    dev.assemble()
    exact = [ref.mesh_element_matrices(th, w) + ref.scales(th.elem, th.n_v // 2, w) for w in v]
    worst_v, worst_p = _check_elements(dev, v, exact)
    print(f"6 x 5 x 3 levels: device worst err / (u S) = {worst_v:.2f} (velocity), "
          f"{worst_p:.2f} (pressure), bar {BAR}")
    assert worst_v <= BAR and worst_p <= BAR
    Ev, Ep = dev.debug_array("Ev"), dev.debug_array("Ep")
    # pair 85 = (level 2, element 25): its rows 0, 3, 6 come from workgroup 0, the rest from 1
    split = Ev.reshape(90, 9, 9)[85]
    assert np.all(split != 0.0) and np.all(Ep.reshape(90, 4, 4)[85:] != 0.0)
    # the same state again, and after another one: no slot keeps a stale value
    dev.assemble()
    assert np.array_equal(dev.debug_array("Ev"), Ev) and np.array_equal(dev.debug_array("Ep"), Ep)
    p2p1._check_gather(dev, Ev, Ep, dev.debug_array("D2"), dev.debug_array("Dp"))
    assert np.array_equal(dev.debug_array("v"), state[0])
    assert np.array_equal(dev.debug_array("zeta"), state[1])
    got = dev.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(got, state))


# --------------------------------------------- gather, compose, residual, rhs, update
@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_gather_bit_for_bit(mesh_name, CN):
    p2p1.test_gather_bit_for_bit(mesh_name, CN)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_compose_bit_for_bit(mesh_name, CN):
    p2p1.test_compose_bit_for_bit(mesh_name, CN)


@pytest.mark.parametrize("CN", [False, True])
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_residual_against_correctly_rounded_rows(mesh_name, CN):
    p2p1.test_residual_against_correctly_rounded_rows(mesh_name, 3, CN)


@pytest.mark.parametrize("CN", [False, True])
def test_right_hand_side(CN):
    p2p1.test_right_hand_side(0.5, CN)


@pytest.mark.parametrize("CN", [False, True])
def test_update(CN):
    p2p1.test_update(3, CN)


def test_the_borrowed_tests_ran_on_quadrilaterals():
    pb = p2p1._problem(p2p1.MESHES["anisotropic"], 3, False)
    assert pb.disc.elem["kind"] == "q2q1" and pb.disc is _disc("anisotropic")
    outer, dev = p2p1._bare(pb)
    assert dev.plan.kind == "q2q1" and dev.plan.V.shape[1] == 9


# -------------------------------------------------------------------------------- refusals
def _set(outer, d):
    lib = outer._lib
    code = lib.kkt_set_relinearisation(outer.handle, C.byref(d))
    return code, lib.kkt_last_error(outer.handle)


def test_descriptor_checks_on_nv():
    th = _disc("square")
    pb = p2p1._problem(th, 3, False)
    v = p2p1._winds("normal", th)
    outer, dev = p2p1._bare(pb)
    dev.set_state(*p2p1._state(pb, np.random.default_rng(common.SEED), v))
    dev.assemble()
    Ev = dev.debug_array("Ev")
    for nv, nq in ((9, 7), (6, 16), (9, 25)):
        d, keep = dev.plan.descriptor()
        assert (d.nv, d.nq) == (9, 16)
        d.nv, d.nq = nv, nq
        code, message = _set(outer, d)
        assert code == KKT_ERR_ARG and b"nv" in message, (nv, nq, message)
    d, keep = dev.plan.descriptor()
    d.jinv = None
    code, message = _set(outer, d)
    assert code == KKT_ERR_ARG and b"nv" in message and b"jinv" in message, message
    # a refused descriptor leaves the plan that stands as it is
    dev.assemble()
    assert np.array_equal(dev.debug_array("Ev"), Ev)


def test_a_triangle_descriptor_with_nv_zero_is_still_accepted():
    tri = fem.rectangle_p2p1(2, 2, 2.0, 2.0)
    pb = p2p1._problem(tri, 3, False)
    outer, dev = p2p1._bare(pb)
    d, keep = dev.plan.descriptor()              # what _bare has just set on the handle
    assert (d.nv, d.nq) == (0, 7) and not d.jinv
    d.nq = 16
    code, message = _set(outer, d)
    assert code == KKT_ERR_ARG and b"nq must be 7" in message      # the message as it was
    dev.set_state(*p2p1._state(pb, np.random.default_rng(common.SEED)))
    dev.assemble()
    assert dev.debug_array("Ev").shape == (3, len(tri.elem["V"]), 6, 6)
    assert dev.debug_array("Ep").shape == (3, len(tri.elem["V"]), 3, 3)
