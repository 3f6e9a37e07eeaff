"""Anderson acceleration of the Picard loops in update space.

Call ``k = 0, 1, ...`` of a mixer receives ``f_k``, the update the linearised solve produced, and
returns the step ``s_k`` the loop adds to its iterate:

* history: for ``k >= 1`` the pair ``dF = f_k - f_{k-1}``, ``dX = s_{k-1}`` enters a ring of at most
  ``depth`` pairs; the oldest falls out;
* Gram system: ``G = dF^T dF`` and ``r = dF^T f_k`` of the pairs kept, every entry recomputed at
  every call;
* condition rule: ``G = L L^T`` by unpivoted Cholesky in double, columns oldest first, accepted
  when every pivot is positive and ``max L_ii / min L_ii <= cond_max``; otherwise the oldest pair
  leaves the ring and the rest is factored again;
* ``gamma`` from the two triangular solves;
* step: ``s = beta f``, then ``t = dX_j + beta dF_j``, ``s = s - gamma_j t`` for ``j`` = oldest ..
  newest, every product and sum rounded on its own.  Without pairs ``s = beta f``: the plain
  Picard step for ``beta = 1``, bit for bit.

``AndersonMixer`` is the statement in NumPy, operation by operation: the reference the device
mixer (``kkt_anderson_step``, ``DeviceAnderson``) is tested against, and what the host loops mix
with.  Not offered on time shards and not under ``set_Gauss_Newton()``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

__all__ = ["AndersonMixer", "DeviceAnderson", "HostAnderson", "check_anderson", "cholesky_gamma",
           "MAX_DEPTH"]

MAX_DEPTH = _lib.ANDERSON_MAX_DEPTH


def check_anderson(anderson, anderson_beta=1.0, comm=None, gauss_newton=False):
    """The drivers' refusals (``ValueError``, before any GPU work); returns the depth."""
    if isinstance(anderson, bool) or not isinstance(anderson, (int, np.integer)) \
            or not 0 <= anderson <= MAX_DEPTH:
        raise ValueError(f"anderson={anderson!r}: the depth is an integer in 0..{MAX_DEPTH}")
    if anderson == 0:
        return 0
    if not math.isfinite(anderson_beta) or anderson_beta == 0.0:
        raise ValueError(f"anderson_beta={anderson_beta!r} must be finite and not zero")
    if comm is not None and getattr(comm, "world", 1) > 1:
        raise ValueError("anderson > 0 is not offered on time shards (comm of more than one rank): "
                         "the Gram sums would have to be all-reduced")
    if gauss_newton:
        raise ValueError("anderson > 0 is not offered under set_Gauss_Newton(): Anderson "
                         "acceleration is for the Picard iteration")
    return int(anderson)


def cholesky_gamma(G, r, cond_max):
    """The condition rule on ``G`` (c x c, oldest first) and ``r``: ``(dropped, gamma)`` with
    ``gamma`` of the ``c - dropped`` newest columns.  Plain Python floats, in the library's order
    of operations."""
    c0 = len(r)
    for d in range(c0):
        c = c0 - d
        L = [[0.0] * c for _ in range(c)]
        lmin, lmax, ok = math.inf, 0.0, True
        for i in range(c):
            for j in range(i + 1):
                s = float(G[d + i][d + j])
                for k in range(j):
                    s -= L[i][k] * L[j][k]
                if j < i:
                    L[i][j] = s / L[j][j]
                elif not s > 0.0 or not math.isfinite(s):
                    ok = False
                    break
                else:
                    L[i][i] = math.sqrt(s)
                    lmin, lmax = min(lmin, L[i][i]), max(lmax, L[i][i])
            if not ok:
                break
        if not ok or not lmax / lmin <= cond_max:
            continue
        y = [0.0] * c
        for i in range(c):
            s = float(r[d + i])
            for k in range(i):
                s -= L[i][k] * y[k]
            y[i] = s / L[i][i]
        gamma = [0.0] * c
        for i in range(c - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, c):
                s -= L[k][i] * gamma[k]
            gamma[i] = s / L[i][i]
        return d, np.array(gamma)
    return c0, np.zeros(0)


def mix(f, dX, dF, gamma, beta):
    """The step statement, unfused: every product and sum rounded on its own."""
    s = beta * f
    for j in range(len(gamma)):
        t = dX[j] + beta * dF[j]
        s = s - gamma[j] * t
    return s


class AndersonMixer:
    """The statement in NumPy on flat vectors of length ``n``.  ``info`` after a call: ``columns``
    and ``dropped``, ``G``, ``r`` and ``gamma`` of the pairs used, and ``dF`` / ``dX`` (the pairs
    used, oldest first)."""

    def __init__(self, n, depth, beta=1.0, cond_max=1.0e7):
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) \
                or not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth {depth!r} is outside 1..{MAX_DEPTH}")
        if not math.isfinite(beta) or beta == 0.0:
            raise ValueError(f"beta={beta!r} must be finite and not zero")
        if not cond_max > 1.0:
            raise ValueError(f"cond_max={cond_max!r} must be above 1")
        self.n, self.depth, self.beta, self.cond_max = int(n), int(depth), float(beta), float(cond_max)
        self.reset()

    def reset(self):
        """The next call behaves as the first."""
        self._dF, self._dX, self._f_prev, self._s_prev = [], [], None, None
        self.info = None

    def step(self, u):
        f = np.array(u, dtype=np.float64).reshape(-1)
        if f.size != self.n:
            raise ValueError(f"vector of length {f.size}, expected {self.n}")
        if self._f_prev is not None:
            self._dF.append(f - self._f_prev)
            self._dX.append(self._s_prev)
            del self._dF[:-self.depth], self._dX[:-self.depth]
        c0 = len(self._dF)
        G = np.array([[np.dot(a, b) for b in self._dF] for a in self._dF]).reshape(c0, c0)
        r = np.array([np.dot(a, f) for a in self._dF])
        dropped, gamma = cholesky_gamma(G, r, self.cond_max) if c0 else (0, np.zeros(0))
        del self._dF[:dropped], self._dX[:dropped]
        s = mix(f, self._dX, self._dF, gamma, self.beta)
        self._f_prev, self._s_prev = f, s
        self.info = {"columns": c0 - dropped, "dropped": dropped, "gamma": gamma,
                     "G": G[dropped:, dropped:].copy(), "r": r[dropped:].copy(),
                     "dF": list(self._dF), "dX": list(self._dX)}
        return s.copy()


class DeviceAnderson:
    """The device mixer on a block system (``kkt_anderson_set`` on its handle): ``step(d_u)`` turns
    the solver's update into the accelerated step in place, between ``solve`` and ``update`` of
    ``relinearise.device_picard_loop``.  ``history``: per call ``(columns, dropped)``."""

    def __init__(self, system, depth, beta=1.0, cond_max=1.0e7):
        self._system, self._lib, self.depth = system, system._lib, int(depth)
        system._ck(self._lib.kkt_anderson_set(system.handle, int(depth), float(beta),
                                               float(cond_max)))
        self.history, self.info = [], None

    def step(self, d_u):
        rec = _lib.AndersonInfo()
        self._system._ck(self._lib.kkt_anderson_step(self._system.handle, d_u, C.byref(rec)))
        c = rec.columns
        self.info = {"columns": c, "dropped": rec.dropped, "gamma": np.array(rec.gamma[:c]),
                     "G": np.array(rec.G[:c * c]).reshape(c, c), "r": np.array(rec.r[:c])}
        self.history.append((c, rec.dropped))

    def reset(self):
        self._system._ck(self._lib.kkt_anderson_reset(self._system.handle))

    def close(self):
        """Release the history (the system's ``close`` releases it as well)."""
        if self._system.handle:
            self._system._ck(self._lib.kkt_anderson_set(self._system.handle, 0, 1.0, 1.0e7))


class HostAnderson:
    """What the host loops mix with: the flat concatenation of the update blocks through an
    ``AndersonMixer`` (made at the first call), back in the blocks' shapes."""

    def __init__(self, depth, beta=1.0):
        self.depth, self.beta, self.mixer, self.history = depth, beta, None, []

    def step(self, *blocks):
        flat = np.concatenate([np.ravel(b) for b in blocks])
        if self.mixer is None:
            self.mixer = AndersonMixer(flat.size, self.depth, self.beta)
        s = self.mixer.step(flat)
        self.history.append((self.mixer.info["columns"], self.mixer.info["dropped"]))
        out, at = [], 0
        for b in blocks:
            out.append(s[at:at + b.size].reshape(np.shape(b)))
            at += b.size
        return out

    def step_fields(self, nodes, fields, others=()):
        """``step`` on a driver's update as its loop takes it: ``fields`` (velocity-like, dofs on
        the last axis) count with zeros on the Dirichlet dofs ``nodes``, where the loop keeps the
        iterate's boundary values whatever the linearised solve left there -- the device update
        ignores ``d_u`` on those dofs likewise --, ``others`` as they are."""
        fields = [np.array(f, dtype=np.float64) for f in fields]
        for f in fields:
            f[..., nodes] = 0.0
        return self.step(*fields, *others)

    def reset(self):
        if self.mixer is not None:
            self.mixer.reset()
