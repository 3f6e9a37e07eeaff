"""The host half of the batched spectrum estimates (control_amd/csrc/spectrum_host.hpp): the
lock-step controller -- device-side alpha / beta bookkeeping and break rules, the host's Ritz
check every 10 steps, tridiag_eigenvalues -- against the one-matrix loop on small dense matrices
in plain C++ (tests/native/spectrum_lockstep_emu.cpp).  Matrices that stop at different steps,
two that break down at step 0, one that never starts and one that reaches max_steps: step counts
and intervals must be identical bit for bit.
Host-only: the device side is compared in tests/test_gpu_spectrum_batch.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "native", "spectrum_lockstep_emu.cpp")]


def build(exe, extra):
    # the header is free of HIP: nothing of it is read or linked
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "control_amd", "csrc")]
                          + extra + SRC + ["-o", exe])
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spectrum lock-step: 0 failures" in r.stdout, r.stdout
    assert "DIFFERENT" not in r.stdout, r.stdout
    return r.stdout


def test_lock_step_equals_the_one_matrix_loop():
    print(run(build(os.path.join(ROOT, "build", "spectrum_lockstep_emu"), ["-O2"])))


def test_lock_step_is_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build(os.path.join(ROOT, "build", "spectrum_lockstep_emu_san"),
              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
