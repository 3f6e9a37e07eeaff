"""The harness of the sharded stopping-rule test, proven without a GPU.

``sharded_stop_worker.run_cases`` with the oracle behind the shard wrappers: 2, 3 and 5 ranks
(processes) over real pipes, every rank solving the whole system with ``oracle.kkt_oracle`` and
then going through the slicing of the time levels, the wrapping of the callback preconditioner
and the gathering that the device ranks go through.  So on a CPU-only machine this shows that the
wrappers are exact (every result is the plain oracle's bit for bit), that a failing assert -- one
wrong expectation seeded into a copy of a case -- is reported by every rank while the ranks stay
in step for the cases after it, and that the case loop ends.
"""
import functools

import numpy as np
import pytest

import krylov_stop_cases as kc
import sharded_stop_worker as worker
from test_gpu_sharded import launch

WORLDS = [2, 3, 5]        # 5: one level per rank on L5, which the device test does not run yet
SEEDED_AFTER = 3
_cache = {}


def results(world):
    """One launch per world; a failed launch is not repeated."""
    if world not in _cache:
        try:
            _cache[world] = launch(world, False, None, target=functools.partial(
                worker.run_cases, engine="oracle", seeded_after=SEEDED_AFTER, bits=True,
                trajectories=reference()))
        except BaseException as e:
            _cache[world] = e
    if isinstance(_cache[world], BaseException):
        raise _cache[world]
    return _cache[world]


@functools.lru_cache(maxsize=None)
def reference():
    return kc.layer_trajectories()


@functools.lru_cache(maxsize=None)
def plain_oracle():
    oracle = kc.OracleBackend()
    return {case[0]: [(r.reason, r.its, r.history.tobytes(), r.x.tobytes())
                      for r in kc.run_case(oracle, case)] for case in kc.layer_cases()}


def test_levels_are_those_of_the_issue():
    owned = {(m, w): [hi - lo for lo, hi in (worker.levels_of(m, r, w) for r in range(w))]
             for m in (5, 7) for w in (2, 3, 5)}
    assert owned == {(5, 2): [3, 2], (5, 3): [2, 2, 1], (5, 5): [1] * 5,
                     (7, 2): [4, 3], (7, 3): [3, 2, 2], (7, 5): [2, 2, 1, 1, 1]}
    for (m, w), n in owned.items():
        assert worker.levels_of(m, 0, w)[0] == 0 and worker.levels_of(m, w - 1, w)[1] == m


def test_local_callback_is_the_global_one_on_its_rows():
    s = kc.system("L7")
    rng = np.random.default_rng(3)
    B0, B1 = rng.standard_normal((2, s.m, s.nx))
    U0, U1 = np.zeros((2, s.m, s.nx))
    kc.diag_pc(s)(U0, U1, B0, B1)
    for world in (2, 3, 5):
        for rank in range(world):
            lo, hi = worker.levels_of(s.m, rank, world)
            u_0, u_1 = np.full((2, hi - lo, s.nx), np.nan)
            worker.local_pc(s, kc.diag_pc(s), lo, hi)(u_0, u_1, B0[lo:hi], B1[lo:hi])
            assert u_0.tobytes() == U0[lo:hi].tobytes() and u_1.tobytes() == U1[lo:hi].tobytes()
    # the NaN of nan_pc lands on the rank that owns its level and on no other
    lo, hi = worker.levels_of(s.m, 1, 3)
    for level, hit in ((0, False), (3, True), (6, False)):
        u_0, u_1 = np.zeros((2, hi - lo, s.nx))
        worker.local_pc(s, kc.nan_pc(s, 1, entry=2, level=level), lo, hi)(u_0, u_1, B0[lo:hi],
                                                                           B1[lo:hi])
        assert bool(np.isnan(u_0).any()) == hit and not np.isnan(u_1).any()
        if hit:
            assert np.argwhere(np.isnan(u_0)).tolist() == [[level - lo, 2]]


@pytest.mark.parametrize("world", WORLDS)
def test_every_case_ran_on_every_rank_and_the_loop_ended(world):
    res = results(world)
    want = [c[0] for c in kc.layer_cases()]
    want.insert(SEEDED_AFTER, worker.SEEDED[0])
    assert sorted(res) == list(range(world))
    for r in range(world):
        assert res[r]["order"] == want and sorted(res[r]["records"]) == sorted(want)


@pytest.mark.parametrize("world", WORLDS)
def test_seeded_wrong_expectation_is_reported_by_every_rank(world):
    res = results(world)
    for r in range(world):
        rec = res[r]["records"][worker.SEEDED[0]]
        assert rec["status"] == "failed" and "'seeded', -3, 4" in rec["message"], rec
        # the ranks stayed in step: every case after it, and before it, passed
        bad = {k: v["message"] for k, v in res[r]["records"].items()
               if v["status"] != "ok" and k != worker.SEEDED[0]}
        assert not bad, (r, bad)


@pytest.mark.parametrize("world", WORLDS)
def test_wrappers_are_exact(world):
    """Slicing, callback wrapping and gathering change no bit: every result of every rank is the
    plain oracle's."""
    res, plain = results(world), plain_oracle()
    for r in range(world):
        for case_id, want in plain.items():
            assert res[r]["records"][case_id]["bits"] == want, (r, case_id)
