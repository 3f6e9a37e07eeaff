"""The stopping rules of the device Krylov loops (``System::solve_once`` / ``solve_minres``)
through ``MultiBlockSystem.solve``: the case table of ``krylov_stop_cases.py`` against the
independent 60-digit reference of ``krylov_stop_ref.py``.  Reasons, counts and history lengths are
also compared with the oracle's and must be equal exactly.

Worst relative deviation from the reference over every compared entry (bar
``10 N u kappa r_0 / r_k``, compared where it is under 1e-8):
  oracle on the CPU   history 1.6e-13, iterate 2.7e-15
  device on MI355X    history 2.5e-13, iterate 3.6e-15
"""
import ctypes as C

import numpy as np
import pytest

import krylov_stop_cases as kc
from test_gpu_edge_cases import pair

pytestmark = pytest.mark.gpu

ORACLE = kc.OracleBackend()


class DeviceBackend:
    name = "device"

    def handle(self, s, diagonal=False):
        g, _ = pair(s.nx, s.nx, s.diag_blocks() if diagonal else s.blocks(), s.m, s.m,
                    None, None, None, None)
        return g

    def pointer(self):
        return DevicePointerBackend()

    def solve(self, h, s, spec, pc="id", x0=None, b=None):
        x = np.array(s.guesses["zero"] if x0 is None else x0, dtype=np.float64)
        b = s.b if b is None else b
        r = h.solve(*s.split(x), *s.split(b), solver_parameters=spec.parameters(),
                    pc_fn=kc.make_pc(s, pc))
        return kc.Result(int(r.reason), int(r.its), np.array(r.history, dtype=np.float64), x,
                         int(r.info["last_op_applies"]))


class DevicePointerBackend(DeviceBackend):
    """The same solves through ``kkt_solve_device`` on vectors of the handle."""

    def solve(self, h, s, spec, pc="id", x0=None, b=None):
        lib, f64p = h._lib, C.POINTER(C.c_double)
        x = np.array(s.guesses["zero"] if x0 is None else x0, dtype=np.float64)
        b = np.ascontiguousarray(s.b if b is None else b, dtype=np.float64)
        d_b, d_u = C.c_void_p(), C.c_void_p()
        h._ck(lib.kkt_vec_alloc(h.handle, C.byref(d_b)))
        h._ck(lib.kkt_vec_alloc(h.handle, C.byref(d_u)))
        try:
            h._ck(lib.kkt_vec_upload(h.handle, d_b, b.ctypes.data_as(f64p)))
            h._ck(lib.kkt_vec_upload(h.handle, d_u, x.ctypes.data_as(f64p)))
            r = h.solve_device(d_b, d_u, solver_parameters=spec.parameters(),
                               pc_fn=kc.make_pc(s, pc))
            h._ck(lib.kkt_vec_download(h.handle, d_u, x.ctypes.data_as(f64p)))
        finally:
            lib.kkt_vec_free(h.handle, d_b)
            lib.kkt_vec_free(h.handle, d_u)
        return kc.Result(int(r.reason), int(r.its), np.array(r.history, dtype=np.float64), x,
                         int(r.info["last_op_applies"]))


DEVICE = DeviceBackend()


def both(check, *args):
    """The check on the device, then on the oracle: codes, counts and lengths equal exactly."""
    dev = check(DEVICE, *args)
    ora = check(ORACLE, *args)
    assert len(dev) == len(ora)
    for d, o in zip(dev, ora):
        assert (d.reason, d.its, len(d.history)) == (o.reason, o.its, len(o.history))
    return dev


@pytest.mark.parametrize("name,form,pc,m", kc.A_COMBOS)
def test_a_step_counts_at_restart_boundaries(name, form, pc, m):
    both(kc.check_a, name, form, pc, m)


@pytest.mark.parametrize("name,form,pc,guess", kc.B_COMBOS)
def test_b_thresholds_fire_at_their_step(name, form, pc, guess):
    both(kc.check_b, name, form, pc, guess)


def test_b_minres_history_and_threshold():
    both(kc.check_minres_values)


@pytest.mark.parametrize("form,pc", [(f, "diag") for f in kc.GMRES_FORMS + ("minres",)]
                         + [("left", "id")])
def test_c_divergence_limit(form, pc):
    both(kc.check_c, form, pc)


@pytest.mark.parametrize("form,pc", [(f, "diag") for f in kc.GMRES_FORMS + ("minres",)]
                         + [("left", "id")])
def test_d_zero_rhs_zero_guess(form, pc):
    both(kc.check_d, form, pc)


@pytest.mark.parametrize("form,pc", [(f, "id") for f in kc.GMRES_FORMS]
                         + [(f, "diag") for f in kc.GMRES_FORMS])
def test_e_exact_happy_step(form, pc):
    both(kc.check_e, form, pc)


@pytest.mark.parametrize("form", kc.GMRES_FORMS)
def test_e_zero_norm_vector_does_not_leak_into_the_next_solve(form):
    """The happy step divides the next basis vector by a zero norm.  A solve on the same handle
    afterwards, long enough to use that slot, equals a fresh handle's bit for bit."""
    two, s = kc.system("two"), kc.system("eig5")
    assert np.array_equal(two.A != 0, s.A != 0)         # the same structure: one handle for both
    h = DEVICE.handle(two, diagonal=True)
    kc.check_e(_OnHandle(h), form, "id")
    spec = kc.Spec(form, restart=5, rtol=1e-10, max_it=40)
    _set_diagonal(h, s)
    after = DEVICE.solve(h, s, spec, "id")
    fresh = DEVICE.solve(DEVICE.handle(s, diagonal=True), s, spec, "id")
    assert after.reason == 2 and np.isfinite(after.x).all() and after.same_bits(fresh)


class _OnHandle(DeviceBackend):
    def __init__(self, h):
        self.h = h

    def handle(self, s, diagonal=False):
        return self.h


def _set_diagonal(h, s):
    b00, _, _, b11 = s.diag_blocks()
    h.update_block_values(0, 0, 0, b00[(0, 0)])
    h.update_block_values(3, 0, 0, b11[(0, 0)])


@pytest.mark.parametrize("form", kc.GMRES_FORMS)
def test_f_singular_breakdown(form):
    both(kc.check_f, form)


@pytest.mark.parametrize("form,d", [(f, d) for f in kc.GMRES_FORMS for d in (3, 5)]
                         + [("minres", 6)])
def test_g_finite_termination(form, d):
    both(kc.check_g_terminates, form, d)


@pytest.mark.parametrize("form", kc.GMRES_FORMS)
def test_g_six_eigenvalues_against_restart_five(form):
    both(kc.check_g_restarted, form)


@pytest.mark.parametrize("form", kc.GMRES_FORMS)
def test_g_restart_longer_than_the_system(form):
    both(kc.check_g_long_restart, form)


@pytest.mark.parametrize("form,call", sorted(kc.H_NAN_STEPS))
def test_h_nan_from_the_preconditioner(form, call):
    both(kc.check_h_nan, form, call)


def test_h_nan_then_another_solver_on_the_handle():
    both(kc.check_h_nan_then_other_solver)


@pytest.mark.parametrize("form", kc.GMRES_FORMS + ("minres",))
def test_h_inf_in_the_right_hand_side(form):
    both(kc.check_h_inf, form)


def test_i_minres_singular_operator():
    both(kc.check_i)


def test_j_one_handle_many_solvers():
    both(kc.check_j)


@pytest.mark.parametrize("name,guess,form,m,max_it", [
    ("A24", "far", "left", 3, 7), ("A24", "far", "flexible", 10, 11), ("A24", "far", "right", 3, 4),
    ("S24", "zero", "minres", 10, 6)])
def test_k_device_pointer_path(name, guess, form, m, max_it):
    s = kc.system(name)
    spec = kc.Spec(form, restart=m, max_it=max_it)
    host = DEVICE.solve(DEVICE.handle(s), s, spec, "diag", x0=s.guesses[guess])
    dev = DevicePointerBackend().solve(DEVICE.handle(s), s, spec, "diag", x0=s.guesses[guess])
    assert (host.reason, host.its) == (-3, max_it)
    assert dev.same_bits(host) and dev.op_applies == host.op_applies


@pytest.mark.parametrize("reason", sorted(kc.l_cases()))
def test_l_python_layer_raises_or_returns(reason):
    both(kc.check_l, reason)


def test_report_worst_device_deviation():
    """Not an assertion of the table's: the figures for the record (run after the table)."""
    print(f"worst relative deviation from the reference: {kc.WORST}")
    w = kc.WORST.get("device")
    assert w is None or (w["history"] < kc.BAR_CAP and w["iterate"] < kc.BAR_CAP)
