"""The launch schedule of the batched mass solves on tiles (control_amd/csrc/mass_tile_kernels.hip,
planned in csrc/pc_lower.cpp) on a real tile plan of control_amd/csrc/tiles.cpp, emulated on the CPU by
tests/native/mass_tile_emu.cpp: ceil(its / K) launches of at most K steps out of a tile's local
vectors, the older iterate overwritten in place, the iterates between launches in two pairs of
global vectors.  Against the global three-term recurrence bit for bit; no local row read while
its value belongs to another step; the Dirichlet rows of the result +0.0.
Host-only: the GPU kernel is compared in tests/test_gpu_mass_tiles.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "native", "mass_tile_emu.cpp"),
       os.path.join(ROOT, "control_amd", "csrc", "tiles.cpp")]


def build(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
        + extra + SRC + ["-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def emu():
    return build(os.path.join(ROOT, "build", "mass_tile_emu"), ["-O2"])


@pytest.fixture(scope="module")
def emu_sanitized():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    return build(os.path.join(ROOT, "build", "mass_tile_emu_san"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


# nx, ny, nz
GRIDS = [(17, 17, 1), (33, 33, 1), (9, 9, 9)]
TILES = (1, 8, 16)
DEPTHS = (1, 2, 3, 4, 5)


def degrees(K):
    return sorted({2, 3, K, K + 1, 2 * K - 1, 2 * K, 20} - {0})


def run_cases(exe, grid):
    nx, ny, nz = grid
    cut_short = 0
    for tiles in TILES:
        for K in DEPTHS:
            for its in degrees(K):
                args = [str(a) for a in (nx, ny, nz, tiles, K, its)]
                r = subprocess.run([exe] + args, capture_output=True, text=True)
                assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
                assert f"mismatches: 0 of {nx * ny * nz}, stale reads: 0, boundary rows not +0: 0" \
                    in r.stdout, r.stdout
                assert f"launches: {-(-its // K)};" in r.stdout, r.stdout
                got = int(r.stdout.split("plan: ")[1].split()[0])
                assert got == tiles, r.stdout
                if tiles > 1:
                    cut_short += int(r.stdout.split("cut short: ")[1].split()[0])
    # tiles whose rings reach the mesh boundary before distance K were among the cases
    assert cut_short > 0


@pytest.mark.parametrize("grid", GRIDS)
def test_launch_schedule_equals_global_recurrence(emu, grid):
    run_cases(emu, grid)


@pytest.mark.parametrize("grid", GRIDS)
def test_plan_and_emulation_are_clean_under_sanitizers(emu_sanitized, grid):
    run_cases(emu_sanitized, grid)
