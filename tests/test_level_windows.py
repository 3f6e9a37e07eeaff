"""The level windows of both device re-linearisation plans as the library's own code computes them
(control_amd/csrc/levels.hpp): which levels of v, zeta and D a rank holds, whether their ends are
halos, the neighbours it trades them with, the slot of the level it sends up and the levels it
downloads.  tests/native/level_windows.cpp prints them for every rank of 1, 2, 3, 5 and 6 ranks on
six unknown blocks (BE n_t = 6, CN n_t = 7; 6 ranks: one-block shards) and for the stationary plan
(n_t = 1); every line is compared with the NumPy restatement tests/reaction_shard_ref.py, which
tests/test_reaction_shard_ref.py holds to the rules on the host.
Host-only: the plans that carry these windows are held to the one-rank plan on 2, 3 and 5 ranks in
tests/test_gpu_sharded_relin.py and tests/test_gpu_sharded_reaction.py."""
import os
import subprocess

import reaction_shard_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "level_windows.cpp")
M = ref.M_BLOCKS
WORLDS = (1, 2, 3, 5, 6)


def build(exe, extra):
    # the header alone: nothing of HIP, nothing of the library is linked
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + extra + [SRC, "-o", exe])
    return exe


def expected_line(m, CN, rank, world):
    """The program's line for one rank, from the reference alone."""
    w = ref.shard_windows(m, CN, rank, world)
    lo, hi = ref.shard_range(m, rank, world)
    own_v, own_z = ref.owned_levels(m, CN, rank, world)
    # an end of a window past the rank's own levels is a halo, and comes from the next rank on
    # that side; the level sent up is the last v level the rank owns
    v_halo, z_halo = int(rank > 0), int(rank < world - 1)
    up, dn = (rank + 1 if z_halo else -1), (rank - 1 if v_halo else -1)
    numbers = [*w["v"], *w["zeta"], *w["D"], *w["blocks"]]
    return ("window " + " ".join(map(str, numbers)) + f" halo {v_halo} {z_halo}"
            f" neighbours {up} {dn} v_last {own_v[-1] - w['v'][0]}"
            f" owned {own_v.start} {own_v.stop} {own_z.start} {own_z.stop}")


def cases():
    """``(n_t, CN, rank, world)`` of every rank of every world, both schemes, then the stationary
    plan."""
    out = [(M + 1 if CN else M, CN, rank, world)
           for CN in (False, True) for world in WORLDS for rank in range(world)]
    return out + [(1, False, 0, 1)]


def run(exe):
    args, want = [], []
    for n_t, CN, rank, world in cases():
        m = n_t - 1 if CN else n_t
        lo, hi = ref.shard_range(m, rank, world)
        args += [n_t, int(CN), lo, hi, rank]
        want.append(expected_line(m, CN, rank, world))
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(want) == 2 * sum(WORLDS) + 1
    for case, g, w in zip(cases(), got, want):
        assert g == w, f"(n_t, CN, rank, world) = {case}: library\n  {g}\nreference\n  {w}"
    # the stationary plan: one level of everything, nobody to trade with
    assert got[-1] == ("window 0 1 0 1 0 1 0 1 halo 0 0 neighbours -1 -1 v_last 0 "
                       "owned 0 1 0 1")


def test_windows_match_the_reference():
    run(build(os.path.join(ROOT, "build", "level_windows"), ["-O2"]))


def test_windows_are_clean_under_sanitizers():
    # host code with a main of its own: the sanitizer runtimes are linked in, nothing is preloaded
    run(build(os.path.join(ROOT, "build", "level_windows_san"),
              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
