"""The stopping rules of the device Krylov loops on time shards, rank by rank (run with -m gpu on
an MI355X).

On a time-sharded handle every branch of ``System::solve_once`` and ``System::solve_minres``
(csrc/krylov.cpp) is taken from scalars that went through ``Comm::allreduce_sum``: ``rnorm0``, the
first residual, the Gram-Schmidt column with ``tt`` and the time-out flag behind it, MINRES'
``alpha`` and ``dp``.  2 and 3 ranks (processes) share GPU 0 over the host-staged pipe
transport of tests/test_gpu_sharded.py, which sums in rank order on every rank.  One launch per
world: the ranks go through ``krylov_stop_cases.layer_cases()`` in-process
(tests/sharded_stop_worker.py) on the layered systems ``L5`` (5 time levels: 3 + 2 and 2 + 2 + 1)
and ``L7`` (4 + 3 and 3 + 2 + 2) with 5 unknowns per level and variable, so local vectors of 10
to 40 doubles.

NOT RUN: 5 ranks (one level per rank on ``L5``, 2 + 2 + 1 + 1 + 1 on ``L7``: the only world with
a one-level rank in the middle, whose single block row reads both halos).  The same launch with
5 ranks did not finish on the MI355X: after 240 s no rank had reported, all five were alive and
none had printed an error, while 2 and 3 ranks finished the same list in 6.5 s and 8.0 s then and the
oracle harness of tests/test_sharded_stop_worker_cpu.py finishes it with 5 ranks.  Whether that
is a deadlock of the ranks' collectives or the shared GPU serving six processes too slowly is not
known; the world is left out until it is, and it is the first thing to add here.

Asserted on every rank against the 60-digit reference of ``krylov_stop_ref.py`` and the table,
never against another backend: the checks of ``krylov_stop_cases.py``, unchanged.  Every solve
gathers all ranks' reasons, counts and histories and fails unless they are identical in every
bit.  Codes, counts and history lengths are compared across the worlds, with one rank of the
device and with the oracle, and must be equal exactly (the values are not: the sums are formed
rank by rank).  tests/test_sharded_stop_worker_cpu.py proves the harness without a GPU.

Worst relative deviation from the reference over every compared entry (bar
``10 N u kappa r_0 / r_k``, compared where it is under 1e-8), next to the one-rank figures of
tests/test_gpu_krylov_stopping.py (history 2.5e-13, iterate 3.6e-15 on the one-block systems):
  one rank  history 7.7e-14, iterate 3.8e-15     (the same layered cases, in this process)
  2 ranks   history 1.0e-13, iterate 2.9e-15     launch 5.7 s (4.6 s in the case loop)
  3 ranks   history 1.1e-13, iterate 2.8e-15     launch 6.7 s (6.0 s in the case loop)
One launch of tests/test_gpu_sharded.py::test_sharded_matches_oracle takes 1.0 to 1.4 s on the
same machine.  A launch here is 407 solves per rank, most on a handle of their own, at 2 to 3 ms
a step (every collective of a step is staged through the host and a pipe); the 60-digit
reference is computed once in this process and handed to the ranks (it cost every rank 1 to 2 s
more).
"""
import functools
import time

import pytest

import krylov_stop_cases as kc
import sharded_stop_worker as worker
import test_gpu_sharded as base
from test_gpu_krylov_stopping import ORACLE, DeviceBackend, DevicePointerBackend

pytestmark = pytest.mark.gpu


class LayeredPointer(DevicePointerBackend):
    name = "device, layered"          # its own line in kc.WORST, apart from the one-block table


class LayeredDevice(DeviceBackend):
    name = "device, layered"

    def pointer(self):
        return LayeredPointer()


DEVICE = LayeredDevice()

WORLDS = (2, 3)
LAUNCH_SECONDS = 120          # a launch takes 6 to 7 s
CASES = kc.layer_cases()
_cache, _wall = {}, {}


def results(world):
    """One launch per world, shared by the tests below; a failed launch is not repeated."""
    if world not in _cache:
        t0 = time.perf_counter()
        try:
            _cache[world] = base.launch(
                world, False, None, timeout=LAUNCH_SECONDS,
                target=functools.partial(worker.run_cases, engine="gpu", trajectories=reference()))
        except BaseException as e:
            _cache[world] = e
        _wall[world] = time.perf_counter() - t0
    if isinstance(_cache[world], BaseException):
        raise _cache[world]
    return _cache[world]


@functools.lru_cache(maxsize=None)
def reference():
    """The 60-digit reference, computed once here and handed to the ranks of every world."""
    return kc.layer_trajectories()


def summary(out):
    return [(r.reason, r.its, len(r.history)) for r in out]


@functools.lru_cache(maxsize=None)
def one_rank(case_id):
    """The case on one rank of the device and on the oracle: (reason, count, length) of every
    solve, equal exactly."""
    case = next(c for c in CASES if c[0] == case_id)
    dev, ora = summary(kc.run_case(DEVICE, case)), summary(kc.run_case(ORACLE, case))
    assert dev == ora, (case_id, dev, ora)
    return dev


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_layered_case_on_one_rank(case):
    assert one_rank(case[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("world", WORLDS)
def test_case_on_every_rank(world, case):
    """The check of the table passed on every rank; the ranks report the same codes, counts and
    lengths (that their histories agree in every bit is asserted inside every solve), and these
    are the ones of one rank and of the oracle."""
    res = results(world)
    assert sorted(res) == list(range(world))
    for r in range(world):
        rec = res[r]["records"][case[0]]
        assert rec["status"] == "ok", (world, r, case[0], rec["message"])
    for r in range(world):
        assert res[r]["records"][case[0]]["results"] == one_rank(case[0]), (world, r, case[0])


def test_worst_deviation_per_world():
    """The figures for the record (the module text), printed before they are asserted: every
    compared entry was under its a-priori bar inside check_values already."""
    for world in WORLDS:
        res = results(world)
        for r in range(world):
            print(f"world {world} rank {r}: worst relative deviation {res[r]['worst']}, "
                  f"{res[r]['seconds']:.1f} s in the worker, launch {_wall[world]:.1f} s; slowest "
                  f"cases {sorted(((v['seconds'], k) for k, v in res[r]['records'].items()))[-3:]}")
    print(f"one rank, the same cases: worst relative deviation {kc.WORST.get(DEVICE.name)}")
    for world in WORLDS:
        res = results(world)
        for r in range(world):
            w = res[r]["worst"]
            assert w == res[0]["worst"]          # the gathered results are the same on every rank
            assert w["history"] < kc.BAR_CAP and w["iterate"] < kc.BAR_CAP


def test_every_case_ran_on_every_world():
    """Fails if any case of the list was not run, or did not pass, on some rank of some world."""
    want = [c[0] for c in CASES]
    assert len(want) == len(set(want)) > 100
    missing = []
    for world in WORLDS:
        res = results(world)
        for r in range(world):
            assert res[r]["order"] == want, (world, r)
            missing += [(world, r, k) for k in want
                        if res[r]["records"].get(k, {}).get("status") != "ok"]
    assert not missing, missing
