"""The preconditioner's row steps bit for bit, one production launch at a time, through
``kkt_debug_row_step``: the two epilogues of ``RowOp`` (``EPI_LIN``, ``EPI_CHEB``) as ``pc_rows``,
``pc_row_step``, ``pc_rows_shared<W>``, ``pc_rows_shared_g``, ``pc_rows_il<8>`` and ``pc_rows_il<4>``
run them.  Reference: ``tests/rowstep_ref.py``; the launches and their data: ``tests/rowstep_cases.py``
(both checked on the host by ``tests/test_rowstep_ref.py``).  The hook fills the ops, builds the launch
and runs it with the functions of ``csrc/rowlaunch.hpp`` that ``SchurPC`` and ``StokesPC`` use, and the
family and width it reports are the answer the launcher itself dispatches on (``rows_kernel``,
``shared_kernel``, ``il_kernel`` of ``csrc/kernels.hpp``), which ``run_case`` holds against its own table.

Sizes -- each the smallest that reaches its regime (256 threads = 4 waves = 4 slices per workgroup):
1, 63, 64, 65, 127, 128, 129 rows (positions past ``nrows`` inside a slice, R = 1 and R = 2); 511, 512,
513 (the fourth wave); 4225 rows for the shared and interleaved kernels with ``pc_xcd`` on and off
(R = 2: 34 slices, nine workgroups, so every XCD eighth is non-empty and the grid is rounded up to
16; at 129 rows seven eighths are empty).  Patterns: fixed widths 1, 5, 7, 9, 15, 16; uniform width
20 (the ``uniform_w`` slot loop); ragged slices of 9 / 15 / 25 (``slice_off``); row-sorted storage
(``perm``); R = 1.  Shared form: 4, 5, 8 ops (and 3, which the launcher declines); interleaved: 6
levels (a group of two), first / second / middle / last step with per-level factors, and the
last step of a solve of degree two (outputs and factors without ``pkm1``).  Operand sets:
every one ``emit_lin`` / ``emit_cheb`` / ``emit_solves_interleaved`` / ``StokesPC`` produce, the level
update in place (``y == yin``) among them, and a masked-row source ``mx`` with ``y2``.  No production
caller of these launchers addresses a vector through ``Bases`` (all pass absolute pointers), so no
case does.

Asserted per launch: (a) guards and every array the launch only reads are untouched, outputs of
positions past ``nrows`` do not exist to be written; (b) integer data with power-of-two
coefficients: bit for bit (all candidates coincide); (c) real data: every output of an op equals ONE
contraction candidate of ``rowstep_ref`` on every element; (d) independently, every output lies
inside ``roundings * u * sum |.|``.  The closing test asserts that the candidate of an operand set
is the same in every case and every kernel family and instantiation, and that every launcher
branch listed above ran.

Measured on an MI355X (gfx950): all six kernels run candidate ``ff`` of both modes -- the first
product rounded, every further addend one fma (``uf`` without ``pkm1``, ``fu`` with one of ``yin`` /
``z``, ``uu`` where nothing is added) -- which is the chain ``csrc/epilogue.hpp`` writes out, fma by
fma, for every kernel, and the closing test asserts (``EXPECTED``).  Largest error / bound 0.714.  42 cases of 416 launches and the closing test: 3.5 s,
the slowest case (4225 rows, interleaved, ``pc_xcd`` on and off) 0.34 s.  A library whose
``pc_rows_il`` takes ``post1[0]`` for every level fails the seven interleaved cases (the last step's
second level matches no candidate, 3e14 times the bound) and the closing test.
A library whose ``rowops_body`` rounds ``c2 pk`` before adding it passes every case (``uf`` is a
correct step) and fails the closing test: ``pc_rows`` / ``pc_row_step`` at ``uf``, the others at ``ff``.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import rowstep_cases as rc
import rowstep_ref as ref
from control_amd import _lib

pytestmark = pytest.mark.gpu

G = _lib.BLOCK_GUARD
CASES = rc.cases()
FOUND = {}        # operand set -> {(family, width): candidates that matched every launch so far}
REACHED = set()
WORST = {"ratio": 0.0}
_handles = {}
_done = {}


# ------------------------------------------------------------------------------- the handle
def _ck(lib, h, rc_):
    if rc_ == -2:     # KKT_ERR_HIP: nothing more is started on a device that reported an error
        pytest.exit(f"HIP error: {lib.kkt_last_error(h)}", returncode=3)
    assert rc_ == 0, lib.kkt_last_error(h)


def handle(sname, n):
    """A finalized handle whose sixteen blocks share the structure: real values in Q00 / Q01,
    integer ones in Q10 / Q11 (``rowstep_cases.block_coords``)."""
    if (sname, n) in _handles:
        return _handles[sname, n]
    lib = _lib.load()
    A, opts = rc.structure(sname, n)
    h = C.c_void_p()
    assert lib.kkt_create(C.byref(h), 0) == 0, lib.kkt_last_error(None)
    for k, v in opts.items():
        _ck(lib, h, lib.kkt_set_option(h, k.encode(), v.encode()))
    _ck(lib, h, lib.kkt_set_layout(h, 2, 2, n, n, 0, -1, -1))
    mats = {}
    indptr, indices = _lib.i32(A.indptr)[0], _lib.i32(A.indices)[0]
    for kind in ("real", "int"):
        mats[kind] = rc.matrices(A, kind)
        for k, M in enumerate(mats[kind]):
            q, i, j = rc.block_coords(k, kind)
            data = np.ascontiguousarray(M.data, np.float64)
            _ck(lib, h, lib.kkt_add_block(h, q, i, j, n, n, indptr.ctypes.data_as(_lib.c_i32p),
                                          indices.ctypes.data_as(_lib.c_i32p),
                                          data.ctypes.data_as(_lib.c_f64p), -1))
    _ck(lib, h, lib.kkt_finalize(h))
    _handles[sname, n] = (lib, h, mats)
    return _handles[sname, n]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for lib, h, _ in _handles.values():
        lib.kkt_destroy(h)
    _handles.clear()


# --------------------------------------------------------------------------------- the call
def launch(lib, h, L, n):
    """One launch: ``(report, vectors after, interleaved output or None)``; (a) is asserted here."""
    nvec, slot = len(L.vecs), n + 2 * G
    table = np.full(nvec * slot, np.nan)
    for k, v in enumerate(L.vecs):
        table[k * slot + G:k * slot + G + n] = v
    ops = (_lib.RowStepOp * len(L.ops))()
    for rec, o in zip(ops, L.ops):
        rec.mode = _lib.ROWSTEP_LIN if o.mode == "lin" else _lib.ROWSTEP_CHEB
        il = L.form == "interleaved"
        # (every interleaved step names its matrix, the first too, which has no term to multiply)
        terms = [(rc.IL_BLOCK, 0)] if il else o.terms
        rec.nterms = len(terms)
        for t, (blk, x) in enumerate(terms):
            rec.term_q[t], rec.term_i[t], rec.term_j[t] = rc.block_coords(blk, L.kind)
            rec.term_x[t] = x
        for f in ("y", "y2", "yin", "z", "mx", "b"):
            setattr(rec, f, getattr(o, f))
        # (interleaved levels hand their iterates over in il_x / il_pkm1, not by index)
        rec.pk, rec.pkm1 = (-1, -1) if il else (o.pk, o.pkm1)
        for f in ("ca", "cy", "cz", "malpha", "c1", "c2", "c3", "post1", "post2"):
            setattr(rec, f, getattr(o, f))
    a = _lib.RowStep()
    a.form = _lib.ROWSTEP_FORMS[L.form]
    a.q, a.i, a.j = rc.block_coords(0, L.kind)
    a.nops, a.pc_xcd, a.nvec = len(L.ops), L.xcd, nvec
    a.ops = ops
    a.vecs = table.ctypes.data_as(_lib.c_f64p)
    mask = np.ascontiguousarray(np.where(L.mask, 1 + (np.arange(n) % 255), 0), np.uint8)
    dinv = np.ascontiguousarray(L.dinv, np.float64)
    a.rowmask = mask.ctypes.data_as(_lib.c_u8p)      # any non-zero byte masks
    a.dinv = dinv.ctypes.data_as(_lib.c_f64p)
    keep, il_y = [mask, dinv], None
    if L.form == "interleaved":
        for f, idx in (("il_x", [o.pk for o in L.ops]), ("il_pkm1", [o.pkm1 for o in L.ops])):
            if idx[0] >= 0:
                buf = ref.interleave([L.vecs[k] for k in idx], n)
                keep.append(buf)
                setattr(a, f, buf.ctypes.data_as(_lib.c_f64p))
        if not L.last:
            il_y = np.full((len(L.ops) + 3) // 4 * 4 * n + 2 * G, -1.2345e300)
            a.il_y = il_y.ctypes.data_as(_lib.c_f64p)
    a.inputs_changed = -1
    _ck(lib, h, lib.kkt_debug_row_step(h, C.byref(a)))
    assert a.inputs_changed == 0, (L.name, "an array the launch only reads was written")
    table = table.reshape(nvec, slot)
    assert np.all(table[:, :G] == _lib.KRYLOV_PAD) and np.all(table[:, -G:] == _lib.KRYLOV_PAD), \
        (L.name, "guard elements were written")
    if il_y is not None:
        assert np.all(il_y[:G] == _lib.KRYLOV_PAD) and np.all(il_y[-G:] == _lib.KRYLOV_PAD), L.name
        il_y = il_y[G:-G]
    return a, table[:, G:-G], il_y


_reference = {}


def reference(L, mats):
    """Per op ``(op, acc, exact y, exact y2)``, computed once per data set: the launches with
    ``pc_xcd`` on and off, and the shared launches of 4, 5 and 8 ops' common ops, read the same."""
    key = (L.data, L.kind, len(L.ops))
    if key not in _reference:
        _reference.clear()          # (launches of a data set follow one another)
        _reference[key] = [(op, ref.accumulate(op)) + ref.exact(op) for op in rc.ref_ops(L, mats)]
    return _reference[key]


def check(L, mats, report, after, il_y, n):
    """(b), (c), (d) for every op of the launch."""
    fam = (_lib.ROWSTEP_FAMILIES[report.family], report.width)
    levels = None
    if il_y is not None:
        levels, rest = ref.deinterleave(il_y, len(L.ops), n)
        # the unused levels of the last group: zero iterates and right-hand sides give +0.0
        assert ref.same_bits(rest, np.zeros(len(rest))), (L.name, "unused levels")
    for k, (o, (op, acc, tri, tri2)) in enumerate(zip(L.ops, reference(L, mats))):
        y = levels[k] if levels is not None else after[o.y]
        y2 = after[o.y2] if o.y2 >= 0 else None
        match = ref.matching(op, y, y2, acc)
        un = ~op.mask
        ratio = ref.bound_ratio(y, tri, un)
        if y2 is not None:
            ratio = max(ratio, ref.bound_ratio(y2, tri2, un))
        WORST["ratio"] = max(WORST["ratio"], ratio)
        inside = "inside" if ratio <= 1.0 else "OUTSIDE"
        assert match, (L.name, k, op.operands(), fam,
                       f"no candidate gives these bits; error / bound {ratio:.3f}: {inside} the bound")
        assert ratio <= 1.0, (L.name, k, fam, ratio)                               # (d)
        if L.kind == "int":
            assert match == list(ref.candidates(op)), (L.name, k)                  # (b)
        else:
            slot = FOUND.setdefault(op.operands(), {})
            slot[fam] = slot.get(fam, set(ref.candidates(op))) & set(match)        # (c)
            assert slot[fam], (L.name, k, fam, "another candidate than earlier launches of this kernel")
        REACHED.add((fam[0], "terms0" if not op.terms else f"terms{len(op.terms)}", op.mode))
        REACHED.add((fam[0], op.operands()))
        if o.y2 >= 0:
            REACHED.add((fam[0], "y2"))
        if o.mode == "lin" and o.y == o.yin:
            REACHED.add((fam[0], "in place"))
        if o.mode == "cheb":
            REACHED.add((fam[0], "post" if (o.post1, o.post2) != (1.0, 1.0) else "no post"))


def run_case(idx):
    if idx in _done:
        return
    sname, n, makers = CASES[idx]
    lib, h, mats = handle(sname, n)
    for mk in makers:
        for kind in ("int", "real"):
            L = mk(kind)
            report, after, il_y = launch(lib, h, L, n)
            fam = _lib.ROWSTEP_FAMILIES[report.family]
            if L.form == "shared" and len(L.ops) < 4:
                # the launcher declines fewer than four ops (replay then runs pc_rows): nothing ran
                assert report.launched == 0
                for o in L.ops:
                    assert ref.same_bits(after[o.y], L.vecs[o.y])
                REACHED.add(("shared declined",))
                continue
            assert report.launched == 1, L.name
            # the case ran the form it is named after
            want = {"rows": "pc_rows", "single": "pc_row_step", "interleaved": "pc_rows_il"}.get(L.form)
            if L.form == "shared":
                want = "pc_rows_shared" if sname in ("w1", "w5", "w7") else "pc_rows_shared_g"
            assert fam == want, (L.name, fam)
            assert report.R == (1 if sname == "r1" else 2)
            assert report.sorted == (1 if sname == "sorted" else 0), (L.name, "storage")
            if sname.startswith("w"):
                assert report.uniform_w == min(int(sname[1:]), n)
            else:
                assert report.uniform_w == (min(7, n) if sname == "r1" else -1)
            if fam in ("pc_rows", "pc_row_step"):
                w = report.uniform_w if (report.R == 2 and 1 <= report.uniform_w <= 16) else 0
                assert report.width == w
                path = ("R1" if report.R == 1 else "perm" if report.sorted else
                        "slice_off" if report.uniform_w < 0 else "uniform_w loop")
                REACHED.add((fam, report.width if w else path))
            else:
                REACHED.add((fam, report.width, "perm" if report.sorted else
                             "slice_off" if report.uniform_w < 0 else "uniform"))
                REACHED.add((fam, report.width, "xcd" if L.xcd else "dispatch order",
                             "nine workgroups" if n == rc.ROWS_XCD else "few"))
                REACHED.add((fam, "ops", len(L.ops)))
            if L.form == "interleaved":
                REACHED.add((fam, report.width, L.data.split("-")[3]))
            check(L, mats[L.kind], report, after, il_y, n)
    _done[idx] = True


@pytest.mark.parametrize("idx", range(len(CASES)),
                         ids=[f"{s}-{n}-{m[0]('int').form}" for s, n, m in CASES])
def test_row_steps(idx):
    run_case(idx)


# ------------------------------------------------------------------------ the whole table
EXPECTED = {("cheb", False, False): "uu", ("cheb", False, True): "uf", ("cheb", True, True): "ff",
            ("lin", False, False, True): "uu", ("lin", False, True, True): "fu",
            ("lin", True, False, True): "fu", ("lin", True, True, False): "uf",
            ("lin", True, True, True): "ff"}


def required():
    need = set()
    for fam in ("pc_rows", "pc_row_step"):
        need |= {(fam, w) for w in rc.FIXED_WIDTHS}
        need |= {(fam, p) for p in ("R1", "perm", "slice_off", "uniform_w loop")}
        need |= {(fam, "in place"), (fam, "y2"), (fam, "post"), (fam, "no post"),
                 (fam, "terms0", "cheb"), (fam, "terms1", "cheb"), (fam, "terms2", "lin"),
                 (fam, f"terms{rc.MAX_TERMS}", "lin"),
                 (fam, ("cheb", False, False)), (fam, ("cheb", True, True)),
                 (fam, ("lin", True, False, True)), (fam, ("lin", True, True, True))}
    need |= {("pc_rows", "terms0", "lin"), ("pc_rows", "terms1", "lin"),
             ("pc_rows", ("cheb", False, True)), ("pc_rows", ("lin", False, False, True)),
             ("pc_rows", ("lin", False, True, True)), ("pc_rows", ("lin", True, True, False))}
    for fam, w, paths in (("pc_rows_shared", 7, ("uniform",)),
                          ("pc_rows_shared_g", 4, ("uniform", "slice_off", "perm")),
                          ("pc_rows_il", 8, ("uniform",)),
                          ("pc_rows_il", 4, ("uniform", "slice_off", "perm"))):
        need |= {(fam, w, p) for p in paths}
        need |= {(fam, w, x, "nine workgroups") for x in ("xcd", "dispatch order")}
        need.add((fam, w, "xcd", "few"))
        if fam == "pc_rows_il":
            need |= {(fam, w, step) for step in rc.IL_STEPS}
            need |= {(fam, "ops", 6), (fam, "post"), (fam, "no post"),
                     (fam, ("cheb", False, False)), (fam, ("cheb", False, True)),
                     (fam, ("cheb", True, True))}
        else:
            need |= {(fam, "ops", k) for k in (4, 5, 8)}
            need |= {(fam, "in place"), (fam, "y2"), (fam, "post"), (fam, "no post"),
                     (fam, ("cheb", False, True)), (fam, ("cheb", True, True)),
                     (fam, ("lin", False, False, True)), (fam, ("lin", False, True, True)),
                     (fam, ("lin", True, False, True)), (fam, ("lin", True, True, True))}
    need.add(("shared declined",))
    return need


def test_every_row_step_branch_is_reached_with_one_candidate():
    """Every launcher branch of the table above ran, and every operand set has ONE candidate: the
    same in every case, kernel family and instantiation.  (Runs the cases that have not run.)"""
    for idx in range(len(CASES)):
        run_case(idx)
    missing = required() - REACHED
    assert not missing, sorted(map(str, missing))
    chosen = {}
    for operands, per_kernel in sorted(FOUND.items(), key=str):
        common = functools.reduce(set.intersection, per_kernel.values())
        assert len(common) == 1, (operands, {k: sorted(v) for k, v in per_kernel.items()})
        chosen[operands] = common.pop()
    print("candidate per operand set:", chosen)
    # the chain csrc/epilogue.hpp writes: every product after the first fused into
    # its add ("ff"), reduced to "u" where the operand set leaves the letter no choice
    assert chosen == EXPECTED, chosen
    print(f"largest error / bound: {WORST['ratio']:.3f}")
