"""The host-side checks both device re-linearisation plans share (control_amd/csrc/plan_checks.cpp):
the validators of a descriptor's CSR pattern, transpose permutation, contribution lists and index
arrays, and the proof that a target block's pattern is a plan's space once per component.
tests/native/plan_checks.cpp drives them on the P1 pattern of a 3 x 3-node mesh: the correct
arrays pass, one fault each is refused with KKT_ERR_ARG and the caller's prefix.
Host-only: the composition that relies on them is compared in tests/test_gpu_relin_kernels.py and
tests/test_gpu_reaction_kernels.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "native", "plan_checks.cpp"),
       os.path.join(ROOT, "control_amd", "csrc", "plan_checks.cpp")]


def build(exe, extra):
    # nothing of HIP is called: its headers are read, its library is not linked
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include"] + extra + SRC + ["-o", exe])
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan checks: 0 failures" in r.stdout, r.stdout


def test_validators_and_pattern_proof():
    run(build(os.path.join(ROOT, "build", "plan_checks"), ["-O2"]))


def test_validators_and_pattern_proof_are_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build(os.path.join(ROOT, "build", "plan_checks_san"),
              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
