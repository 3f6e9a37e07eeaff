"""The run partition of the preconditioner program (control_amd/csrc/program_partition.hpp): how
SchurPC::fuse_programs cuts the emitted steps into pieces that stay plain launches, become row
programs or go to the tile form, on hand-written step lists with their expected piece lists in
plain C++ (tests/native/program_partition.cpp) -- short runs, runs of levels the tile form takes
or refuses, an ineligible level, two-grid levels, the data-flow chain cut, the one-level time
shard, and the steps that end a run.
Host-only: the forms that run are read back on the device in tests/test_gpu_sweep_forms.py and
tests/test_gpu_sharded_forms.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, VERDICT = "program_partition", "program partition: 0 failures"
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(suffix, extra):
    # the header is free of HIP: nothing of it is read or linked
    exe = os.path.join(ROOT, "build", NAME + suffix)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "control_amd", "csrc")]
                          + extra + [os.path.join(ROOT, "tests", "native", NAME + ".cpp"), "-o", exe])
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert VERDICT in r.stdout, r.stdout
    assert "DIFFERENT" not in r.stdout, r.stdout
    return r.stdout


def test_partition_of_hand_written_step_lists():
    out = run(build("", ["-O2"]))
    print(out)
    # the cases ran: the one-level shard gives its level to the tile form, the steps around it stay
    assert "one-level shard                    plain[0,2) tiles[2,8) plain[8,9)  asked [2,8)" in out
    assert "chain breaks after step 2 of 9     plain[0,2) program[2,9)" in out


def test_partition_is_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build("_san", SANITIZE))
