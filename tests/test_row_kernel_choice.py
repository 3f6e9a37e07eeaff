"""Which kernel family and instantiation a launch of the preconditioner's row steps gets
(``rows_kernel``, ``shared_kernel``, ``il_kernel`` of control_amd/csrc/kernels.hpp): the functions
``launch_rowops`` (tag 1), ``launch_rowops_shared`` and ``launch_rowops_il`` dispatch on, which
``kkt_debug_row_step`` and ``kkt_debug_pc_forms`` report.  tests/native/row_kernel_choice.cpp holds
the table -- written out from the launchers' former switch statements, not computed with the
functions -- for R = 1 and 2, the widths -4 .. 17, 20, 24, 38 and 0 .. 64 ops: R = 1 and the widths
0, 17, 20, -1 run the slot loop (width 0), 1 .. 16 their own instantiation; the shared form declines
R = 1 and fewer than four ops, runs ``pc_rows_shared<W>`` for 1 .. 8 and ``pc_rows_shared_g`` (4)
otherwise; interleaved steps run ``pc_rows_il<8>`` for 1 .. 8, else ``pc_rows_il<4>``.
Host-only: that the launchers run what the functions say is pinned per launch by
tests/test_gpu_row_steps.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "row_kernel_choice.cpp")


def build(exe, extra):
    # nothing of HIP is called: its headers are read, its library is not linked
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include"] + extra + [SRC, "-o", exe])
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "row kernel choice: 0 failures" in r.stdout, r.stdout


def test_kernel_choice_table():
    run(build(os.path.join(ROOT, "build", "row_kernel_choice"), ["-O2"]))


def test_kernel_choice_table_is_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build(os.path.join(ROOT, "build", "row_kernel_choice_san"),
              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
