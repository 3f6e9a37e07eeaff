"""The lists of the coarse corrections inside the tile sweep program (control_amd/csrc/tiles.cpp,
build_tile_coarse_lists) and the scheme of the two-grid levels of its kernel, emulated on the CPU
by tests/native/tile_coarse_emu.cpp: the form in which a tile prolongs a correction onto its ring
rows itself against the form with a hand-off after every correction, both against the global
recurrence, bit for bit; no ring entry read while stale; the ring form's hand-off count.
Host-only: the GPU kernel is compared in tests/test_gpu_coarse_rings.py.

Hand-offs per level: the ring form drops the one after each correction; in front of a later
cycle's residual it takes one always, the other form only where the sweeps used the rings up
(`depth` divides `its`).  So a two-cycle level runs exactly two hand-offs fewer where the depth
divides the sweep count and one fewer elsewhere -- the program asserts cycles, respectively 1,
for every case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "native", "tile_coarse_emu.cpp"),
       os.path.join(ROOT, "control_amd", "csrc", "tiles.cpp")]


def build(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
        + extra + SRC + ["-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def emu():
    return build(os.path.join(ROOT, "build", "tile_coarse_emu"), ["-O2"])


@pytest.fixture(scope="module")
def emu_sanitized():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    return build(os.path.join(ROOT, "build", "tile_coarse_emu_san"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


# nx, ny, nz, tiles, components
GRIDS = [(17, 17, 1, 8, 1), (33, 33, 1, 16, 1), (17, 17, 1, 8, 2), (9, 9, 9, 8, 1)]
SCHEMES = [(depth, its, cycles) for depth in (1, 2, 3, 4) for its in (4, 6, 8) for cycles in (1, 2, 3)]


def run_cases(exe, grid):
    nx, ny, nz, tiles, comps = grid
    for depth, its, cycles in SCHEMES:
        args = [str(a) for a in (nx, ny, nz, tiles, depth, its, cycles, comps)]
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
        assert "mismatches: 0 of" in r.stdout and "stale reads: 0 0 0" in r.stdout, r.stdout
        assert "list errors: 0, hand-off count errors: 0" in r.stdout, r.stdout
        rings = int(r.stdout.split("rings ")[1].split()[0])
        assert rings == (0 if nz > 1 else 1), r.stdout     # 3-D: the builder leaves the flag off
        if rings:
            base, ring = (int(x) for x in
                          r.stdout.split("hand-offs per level: ")[1].split(" (")[0].split(", ring form "))
            assert base - ring == (cycles if its % depth == 0 else 1), r.stdout
            if cycles == 2 and its % depth == 0:
                assert base - ring == 2


@pytest.mark.parametrize("grid", GRIDS)
def test_ring_form_equals_handoff_form_and_global_recurrence(emu, grid):
    run_cases(emu, grid)


@pytest.mark.parametrize("grid", GRIDS)
def test_list_builder_and_emulation_are_clean_under_sanitizers(emu_sanitized, grid):
    run_cases(emu_sanitized, grid)
