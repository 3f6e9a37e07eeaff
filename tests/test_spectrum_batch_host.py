"""The host half of the batched spectrum estimates (control_amd/csrc/spectrum_host.hpp): the
lock-step controller -- device-side alpha / beta bookkeeping and break rules, the host's Ritz
check every 10 steps, tridiag_eigenvalues -- against the one-matrix loop on small dense matrices
in plain C++ (tests/native/spectrum_lockstep_emu.cpp).  Matrices that stop at different steps,
two that break down at step 0, one that never starts and one that reaches max_steps: step counts
and intervals must be identical bit for bit.

The grouping of the twin search (group_twins / twin_classes, what SchurPC::collect_matrices makes
its pairs and classes with) on forged fingerprints (tests/native/twin_groups.cpp): no twins, all
twins, equal fingerprints under different shifts, and a collision -- equal fingerprints, different
bits -- which no real build reaches: the colliding candidates end without a class.
Host-only: the device side is compared in tests/test_gpu_spectrum_batch.py and
tests/test_gpu_spectrum_kernels.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCKSTEP = ("spectrum_lockstep_emu", "spectrum lock-step: 0 failures")
TWINS = ("twin_groups", "twin groups: 0 failures")


def build(name, suffix, extra):
    # the header is free of HIP: nothing of it is read or linked
    exe = os.path.join(ROOT, "build", name + suffix)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "control_amd", "csrc")]
                          + extra + [os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    return exe


def run(exe, verdict):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert verdict in r.stdout, r.stdout
    assert "DIFFERENT" not in r.stdout, r.stdout
    return r.stdout


SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_lock_step_equals_the_one_matrix_loop():
    print(run(build(LOCKSTEP[0], "", ["-O2"]), LOCKSTEP[1]))


def test_lock_step_is_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build(LOCKSTEP[0], "_san", SANITIZE), LOCKSTEP[1])


def test_twin_grouping_on_forged_fingerprints():
    out = run(build(TWINS[0], "", ["-O2"]), TWINS[1])
    print(out)
    # the collision case ran: B and C without a class, A with its own
    assert "collision  candidate 1: shift 1 fingerprint 5 values 1 -> class -1 (expected -1)" in out
    assert "collision  candidate 2: shift 1 fingerprint 5 values 1 -> class -1 (expected -1)" in out
    assert "collision  candidate 0: shift 1 fingerprint 5 values 0 -> class 0 (expected 0)" in out


def test_twin_grouping_is_clean_under_sanitizers():
    run(build(TWINS[0], "_san", SANITIZE), TWINS[1])
