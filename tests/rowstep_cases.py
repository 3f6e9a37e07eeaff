"""The launches of ``tests/test_gpu_row_steps.py`` as plain data, so that ``tests/test_rowstep_ref.py``
can check on the host that every data set separates the contraction candidates.  A launch names its
vectors by index into a table and its matrices by block number; ``ref_ops`` turns it into the ops
of ``rowstep_ref``, the GPU test into the records of ``kkt_debug_row_step``.

Structures (``tests/structures.py`` generators; R = 2 unless said): fixed widths 1, 5, 7, 9, 15, 16
(``pc_rows<2, n>``), uniform width 20 (the ``uniform_w`` slot loop), ``ragged`` (slices of 9 / 15 /
25, the widths of Q2 rows, unsorted: the ``slice_off`` path), ``sorted`` (rows of 9 / 15 / 25 mixed
inside every slice, row-sorted storage: ``perm``), ``r1`` (width 7 at R = 1).

Coefficients of the real-data sets are non-dyadic (``c1 = -0.91, c2 = 1.37, c3 = 0.81 * 1.37, ca =
-0.37, cy = 0.77, cz = 0.43``, the level factors ``post1`` / ``post2`` differ per level): with
production's ``cy = 1`` or ``ca = -1`` the candidates coincide.  The integer sets use powers of two
and integer vectors and matrices, so that every candidate is exact.
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

import rowstep_ref as ref
import structures as st

MAX_TERMS = 8
NBLOCKS = 8
ROWS_SMALL = (1, 63, 64, 65, 127, 128, 129)     # positions past nrows inside a slice, R = 1 and 2
ROWS_WAVE4 = (511, 512, 513)                    # the fourth wave of a workgroup
ROWS_XCD = 4225                                 # R = 2: 34 slices, nine workgroups
FIXED_WIDTHS = (1, 5, 7, 9, 15, 16)
IL_STEPS = ("first", "second", "middle", "last", "last2")
IL_BLOCK = 5                                    # the matrix of the interleaved steps


@dataclass
class OpSpec:
    mode: str
    terms: list = field(default_factory=list)     # (block, vector)
    y: int = -1
    y2: int = -1
    yin: int = -1
    z: int = -1
    mx: int = -1
    b: int = -1
    pkm1: int = -1
    pk: int = -1
    ca: float = 1.0
    cy: float = 0.0
    cz: float = 0.0
    malpha: float = 0.0
    c1: float = 0.0
    c2: float = 0.0
    c3: float = 0.0
    post1: float = 1.0
    post2: float = 1.0


@dataclass
class Launch:
    name: str
    form: str                     # rows | single | shared | interleaved
    kind: str                     # real | int
    ops: list
    vecs: list
    mask: object
    dinv: object
    xcd: int = 1
    last: bool = False            # interleaved: the step writes the levels' outputs
    data: str = ""                # names the data set (launches with pc_xcd on and off share one)


# ------------------------------------------------------------------------------ structures
def structure(name, n):
    """``(CSR pattern with values, options)`` of a structure at ``n`` rows."""
    opts = {"sell_r": "2", "sell_sort": "0"}
    if name.startswith("w"):
        A = st.banded(n, min(int(name[1:]), n), seed=3)
    elif name == "r1":
        opts["sell_r"] = "1"
        A = st.banded(n, min(7, n), seed=4)
    elif name == "ragged":
        ns = (n + st.SLICE - 1) // st.SLICE
        sw = np.resize(np.array([9, 25, 15, 9, 15]), ns)
        A = st.banded(n, np.minimum(st.slice_row_widths(sw, nrows=n), n), seed=5)
    elif name == "sorted":
        opts["sell_sort"] = "1"
        rng = np.random.default_rng([ref.SEED, n, 6])
        A = st.banded(n, np.minimum(rng.choice([9, 9, 9, 15, 25], size=n), n), seed=6)
    else:
        raise KeyError(name)
    return A, opts


def matrices(A, kind):
    """The NBLOCKS term matrices on the structure of ``A``."""
    return [st.with_values(A, 100 + k, integer=kind == "int") for k in range(NBLOCKS)]


def block_coords(k, kind):
    """Block number -> (quadrant, i, j) on the 2 x 2 layout: real values in Q00 / Q01, integer ones
    in Q10 / Q11."""
    return (k // 4 + (2 if kind == "int" else 0), (k % 4) // 2, k % 2)


# ----------------------------------------------------------------------------- the builder
COEF = {
    "real": dict(c1=-0.91, c2=1.37, c3=0.81 * 1.37, ca=-0.37, cy=0.77, cz=0.43, malpha=0.63,
                 post=((0.9, 1.1), (1.3, 0.7), (0.6, 1.9), (1.7, 0.3), (1.21, 0.83), (0.47, 2.3),
                       (1.9, 1.9), (0.11, 0.7))),
    "int": dict(c1=-0.5, c2=2.0, c3=0.25, ca=-2.0, cy=0.5, cz=4.0, malpha=-2.0,
                post=((2.0, 0.5), (4.0, 0.25), (0.5, 0.5), (8.0, 2.0), (2.0, 2.0), (0.25, 4.0),
                      (1.0, 2.0), (0.5, 1.0))),
}


# Launches whose first draw of vectors left two candidates of some op closer than the 5 % that
# tests/test_rowstep_ref.py asks of every data set (small sets: a few dozen unmasked rows; keyed
# by the data set's name), with
# the draw that separates them.
SALT = {"single-w7-63-12": 1, "rows-r1-63": 5, "rows-w7-65": 1, "rows-w7-129": 1,
        "single-w7-129-11": 1, "rows-w16-257": 2, "single-w16-257-12": 1, "rows-w20-513": 1,
        "shared-w9-129-5": 1, "shared-w9-129-8": 1, "shared-w15-257-8": 1, "il-w7-129-last": 1,
        "il-w9-129-last": 2, "il-w15-257-middle": 1, "il-w15-257-last": 1}


class _Table:
    def __init__(self, n, kind, name):
        # (seeded by the launch's name and its draw)
        key = zlib.crc32(f"{name}#{SALT.get(name, 0)}".encode())
        self.n, self.kind, self.key, self.vecs = n, kind, key, []

    def new(self, data=True):
        """Index of a new vector: data, or the fill an output holds before the launch."""
        k = len(self.vecs)
        if not data:
            v = np.full(self.n, -1.2345e300)
        elif self.kind == "int":
            v = ref.int_vec(self.n, self.key, k)
        else:
            v = ref.real_vec(self.n, self.key, k)
        self.vecs.append(v)
        return k


def _dinv(n, kind, key):
    return ref.pow2_vec(n, key) if kind == "int" else 0.5 + np.abs(ref.real_vec(n, key, 99))


def menu(n, kind, key, one_block=None, R=2):
    """The ops of the emitters, one of each operand set, as one launch's worth: ``(ops, table)``.
    ``one_block``: every op has exactly one term, of that block (what the shared kernels take)."""
    c = COEF[kind]
    T = _Table(n, kind, key)
    ops = []

    def terms(k):
        if one_block is not None:
            return [(one_block, T.new())]
        return [((3 * t + 1) % NBLOCKS, T.new()) for t in range(k)]

    def lin(k, yin=False, z=False, mx=False, y2=False, inplace=True):
        o = OpSpec("lin", terms(k), ca=c["ca"], cy=c["cy"] if yin else 0.0,
                   cz=c["cz"] if z else 0.0, c3=c["c3"], malpha=c["malpha"] if mx else 0.0)
        if yin:
            o.yin = T.new()
        o.y = o.yin if (yin and inplace) else T.new(False)
        if z:
            o.z = T.new()
        if mx:
            o.mx = T.new()
        if y2:
            o.y2 = T.new(False)
        ops.append(o)

    def cheb(pk=False, pkm1=False, post=None):
        o = OpSpec("cheb", c1=c["c1"] if pkm1 else 0.0, c2=c["c2"] if pk else 0.0, c3=c["c3"],
                   b=T.new(), y=T.new(False))
        if pk or one_block is not None:
            o.terms = terms(1)
        if pk:
            o.pk = o.terms[0][1]
        if pkm1:
            o.pkm1 = T.new()
        if post is not None:
            o.post1, o.post2 = c["post"][post]
        ops.append(o)

    if one_block is None:
        lin(0, yin=True, z=True)              # B = B - b1 in place, no matrix
        lin(1)                                # y = ca A x
        lin(1, z=True)                        # r = b - A x
        lin(1, yin=True)                      # the level update, in place
        lin(2, yin=True, y2=True)             # ... with two terms and the first Chebyshev step
        lin(1, yin=True, y2=True, inplace=False)
        lin(MAX_TERMS, yin=True, z=True)
        lin(2, mx=True, y2=True)              # a masked row's second output
        cheb()                                # first step / Jacobi application
        cheb(post=0)
        cheb(pk=True)                         # second step
        cheb(pk=True, pkm1=True)              # a middle step
        cheb(pk=True, pkm1=True, post=1)      # the last step
        cheb(pk=True, post=2)
    else:
        lin(1)
        cheb(pk=True, pkm1=True)
        lin(1, z=True)
        cheb(pk=True)
        lin(1, yin=True, y2=True)
        cheb(pk=True, pkm1=True, post=3)
        lin(1, yin=True, z=True, inplace=False)
        cheb(pk=True, post=4)
    return ops, T


def rows_launch(name, n, kind, R=2, form="rows", pick=None):
    ops, T = menu(n, kind, name, R=R)
    if pick is not None:
        ops = [ops[pick]]
    return Launch(name, form, kind, ops, T.vecs, ref.row_mask(n, R, 1), _dinv(n, kind, 1),
                  data=name)


def shared_launch(name, n, kind, nops, xcd=1):
    ops, T = menu(n, kind, name, one_block=2)
    return Launch(f"{name}-x{xcd}", "shared", kind, ops[:nops], T.vecs, ref.row_mask(n, 2, 2),
                  _dinv(n, kind, 2), xcd=xcd, data=name)


def il_launch(name, n, kind, step, nlev=6, xcd=1):
    """One interleaved step of ``nlev`` levels: ``first`` (no p_k), ``second`` (no p_{k-1}),
    ``middle``, ``last`` (writes the levels' outputs with their own factors) and ``last2`` (the last
    step of a solve of degree two: the outputs and factors of ``last`` without p_{k-1})."""
    c = COEF[kind]
    T = _Table(n, kind, name)
    ops = []
    for l in range(nlev):
        o = OpSpec("cheb", c1=c["c1"] if step in ("middle", "last") else 0.0,
                   c2=c["c2"] if step != "first" else 0.0, c3=c["c3"], b=T.new())
        if step != "first":
            o.pk = T.new()
            o.terms = [(IL_BLOCK, o.pk)]
        if step in ("middle", "last"):
            o.pkm1 = T.new()
        if step in ("last", "last2"):
            o.y = T.new(False)
            o.post1, o.post2 = c["post"][l]
        ops.append(o)
    return Launch(f"{name}-x{xcd}", "interleaved", kind, ops, T.vecs, ref.row_mask(n, 2, 3),
                  _dinv(n, kind, 3), xcd=xcd, last=step in ("last", "last2"), data=name)


# ------------------------------------------------------------------------------- reference
def ref_ops(L, mats):
    """The launch's ops as ``rowstep_ref.Op`` (operands: the table's vectors before the launch)."""
    v = L.vecs
    out = []
    for o in L.ops:
        def get(k):
            return None if k < 0 else v[k]
        out.append(ref.Op(o.mode, [(mats[b], v[x]) for b, x in o.terms], mask=L.mask, dinv=L.dinv,
                          ca=o.ca, cy=o.cy, cz=o.cz, malpha=o.malpha, yin=get(o.yin), z=get(o.z),
                          mx=get(o.mx), y2=o.y2 >= 0, c1=o.c1, c2=o.c2, c3=o.c3, post1=o.post1,
                          post2=o.post2, b=get(o.b), pkm1=get(o.pkm1), pk=get(o.pk)))
    return out


# ---------------------------------------------------------------------------- the case list
def cases():
    """``(structure, n, [launch makers])``: every launch of the GPU test, per handle.  A maker is
    called with the data kind."""
    out = []

    def add(sname, n, makers):
        out.append((sname, n, makers))

    def plain(s, n, R=2, singles=(3, 4, 6, 8, 11, 12)):
        m = [lambda kind: rows_launch(f"rows-{s}-{n}", n, kind, R)]
        m += [lambda kind, p=p: rows_launch(f"single-{s}-{n}-{p}", n, kind, R, "single", p)
              for p in singles]
        return m

    for n in ROWS_SMALL + ROWS_WAVE4:
        add("w7" if n > 1 else "w1", n, plain("w7" if n > 1 else "w1", n))
        add("r1", n, plain("r1", n, R=1, singles=(4, 12)))
    for w in FIXED_WIDTHS:
        if w != 7:
            add(f"w{w}", 257, plain(f"w{w}", 257, singles=(4, 12)))
    for s in ("w20", "ragged", "sorted"):
        add(s, 513, plain(s, 513, singles=(4, 12)))
    # shared: pc_rows_shared<7>, pc_rows_shared_g on widths 9 and 15, ragged and row-sorted storage
    for s, sizes in (("w7", (129, ROWS_XCD)), ("w9", (129, ROWS_XCD)), ("w15", (257,)),
                     ("ragged", (513,)), ("sorted", (513,))):
        for n in sizes:
            m = [lambda kind, s=s, n=n, k=k, x=x: shared_launch(f"shared-{s}-{n}-{k}", n, kind, k, x)
                 for k in (4, 5, 8) for x in ((0, 1) if n == ROWS_XCD or k == 5 else (1,))]
            m.append(lambda kind, s=s, n=n: shared_launch(f"shared-{s}-{n}-3", n, kind, 3))
            add(s, n, m)
    # interleaved: pc_rows_il<8> at width 7, <4> at widths 9 and 15, ragged and row-sorted
    for s, sizes in (("w7", (129, ROWS_XCD)), ("w9", (129, ROWS_XCD)), ("w15", (257,)),
                     ("ragged", (513,)), ("sorted", (513,))):
        for n in sizes:
            add(s, n, [lambda kind, s=s, n=n, step=step, x=x:
                       il_launch(f"il-{s}-{n}-{step}", n, kind, step, xcd=x)
                       for step in IL_STEPS
                       for x in ((0, 1) if n == ROWS_XCD else (1,))])
    return out
