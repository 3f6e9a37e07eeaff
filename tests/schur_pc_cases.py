"""The cases of the Schur preconditioner's definition tests: one table for the host test
(tests/test_schur_pc_ref.py: extended reference against the oracle) and the device test
(tests/test_gpu_schur_pc_definition.py: the library against the extended reference).

Sizes are the smallest at which first, middle and last level differ: P1 on the unit square with
6 x 6 cells (49 dofs, 25 free), the convection-diffusion operators of the MMS problem on
``rectangle_p1(6, 6, 2, 2)`` and the P2 velocity blocks of ``rectangle_p2p1(2, 2, 1, 1)`` (50 dofs
in two components, 18 free, ragged rows).  BE runs n_t = 4 and 5, CN n_t = 4 and 6 (3 and 5
levels), the stationary form one level.  Schur degrees 0, 1, 2, 3 and 6 on (0.05, 2.1) are the
degrees at which the emission changes shape; mass degrees 0 and 20 on (0.25, 2.0).

The references of the cases with explicit intervals are in ``tests/golden/schur_pc_definition.npz``
(``tests/golden/make_schur_pc_definition.py``) with the oracle's distance ``d_case`` from them; the
cases with estimated intervals take their intervals from the device's records and are computed
where they run.
"""
import numpy as np

SEED = 20250917
MASS20 = (20, 0.25, 2.0)
MASS0 = (0, 0.0, 0.0)
INTERVAL = (0.05, 2.1)
EPSILON = 1.0e-3
U = 1.1e-16
IMPULSES = ("b0_level", "b1_level", "b0_node", "b1_node")


def case(kind, n_t=1, schur=6, mass=20, beta=1e-2, disc="p1", td=False, eimag=0.0, coarse=0,
         estimated=False, impulses=False, short=False):
    """``schur``: degree (two-grid: sweeps per cycle); ``coarse``: cycles (0: none); ``td``: every
    level its own matrix; ``estimated``: intervals and degree estimated on the device; ``short``:
    no run of four single-block steps, or a stationary two-grid solve -- the library has no sweep
    program for either (``SchurPC::fuse_programs``), so default options run plain launches too."""
    return dict(kind=kind, n_t=n_t, schur=schur, mass=mass, beta=beta, disc=disc, td=td,
                eimag=eimag, coarse=coarse, estimated=estimated, impulses=impulses, short=short)


def case_id(c):
    s = f"{c['kind']}{c['n_t'] if c['kind'] != 'stationary' else ''}-{c['disc']}"
    s += f"-m{c['mass']}-s{'auto' if c['estimated'] else c['schur']}-b{c['beta']:g}"
    if c["td"]:
        s += "-td"
    if c["eimag"]:
        s += f"-e{c['eimag']:g}"
    if c["coarse"]:
        s += f"-mg{c['coarse']}"
    return s


def family(c):
    if c["coarse"]:
        return "two-grid"
    if c["disc"] == "conv":
        return "ellipse"
    return c["kind"]


CASES = [
    # ---- backward Euler, shared blocks: every degree, both n_t, both beta
    case("BE", 4, 6, impulses=True), case("BE", 5, 6), case("BE", 5, 0, mass=0, impulses=True),
    case("BE", 4, 1), case("BE", 4, 2), case("BE", 5, 3), case("BE", 5, 6, beta=1e-4),
    case("BE", 4, 3, beta=1e-4, mass=0),
    # ---- ... every level its own matrix
    case("BE", 4, 6, td=True), case("BE", 5, 3, td=True, beta=1e-4),
    # ---- Crank-Nicolson: 3 and 5 levels
    case("CN", 4, 6, impulses=True), case("CN", 6, 6), case("CN", 6, 0, mass=0, impulses=True),
    case("CN", 4, 1, short=True), case("CN", 6, 2), case("CN", 4, 3), case("CN", 6, 6, beta=1e-4),
    case("CN", 6, 6, td=True), case("CN", 4, 2, td=True, beta=1e-4, mass=0),
    # ---- stationary
    case("stationary", schur=6, impulses=True), case("stationary", schur=0, mass=0, short=True),
    case("stationary", schur=1, beta=1e-4), case("stationary", schur=2),
    case("stationary", schur=3, beta=1e-4),
    # ---- convection-diffusion, explicit ellipses: eimag below the real semi-axis (1.025) and above
    case("BE", 4, 6, disc="conv", beta=1.0, eimag=0.3, impulses=True),
    case("BE", 5, 6, disc="conv", beta=1.0, eimag=1.5),
    case("BE", 5, 1, disc="conv", beta=1.0, eimag=1.5),
    case("BE", 4, 2, disc="conv", beta=1.0, eimag=0.3),
    case("BE", 4, 3, disc="conv", beta=1.0, eimag=1.5),
    case("CN", 4, 6, disc="conv", beta=1.0, eimag=1.5),
    case("CN", 6, 3, disc="conv", beta=1.0, eimag=0.3),
    # ---- two-grid: cycles 1 and 2, sweeps 1, 2 and 4
    case("BE", 4, 1, coarse=1), case("BE", 5, 2, coarse=1),
    case("BE", 4, 4, coarse=1, impulses=True),
    case("BE", 5, 1, coarse=2), case("BE", 4, 2, coarse=2), case("BE", 5, 4, coarse=2),
    case("CN", 4, 4, coarse=1), case("CN", 6, 2, coarse=2, impulses=True),
    case("CN", 6, 1, coarse=1, beta=1e-4), case("stationary", schur=4, coarse=2, short=True),
    case("BE", 4, 4, coarse=1, disc="conv", beta=1.0, eimag=0.3),
    # ---- the P2 velocity blocks of the Stokes inner system
    case("BE", 4, 6, disc="p2v", impulses=True), case("CN", 4, 3, disc="p2v"),
    case("BE", 4, 4, disc="p2v", coarse=1),
]

# intervals and degree estimated on the device: the reference runs every sub-solve with what
# pc_solves() reports for it
ESTIMATED = [
    case("BE", 5, estimated=True, beta=1e-4), case("CN", 4, estimated=True),
    case("BE", 4, estimated=True, disc="conv", beta=1.0), case("stationary", estimated=True),
    case("BE", 4, estimated=True, td=True),
]


# ------------------------------------------------------------------------------ problems
_PROBLEMS = {}


def problem(c):
    """``dict(sd, tau, beta, n_t, CN, m, blocks, nodes)`` as ``problems.heat_problem`` returns."""
    key = (c["kind"], c["n_t"], c["beta"], c["disc"], c["td"])
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    from control_amd.blocks import instationary_blocks, stationary_blocks
    from control_amd.fem import SpatialDiscretisation, rectangle_p2p1, unit_square_p1
    kind, n_t, beta, CN = c["kind"], c["n_t"], c["beta"], c["kind"] == "CN"
    if c["disc"] == "conv":
        from test_gpu_spectrum_estimates import _mms_convection_problem
        assert beta == 1.0 and kind != "stationary" and not c["td"]
        p = _mms_convection_problem(6, CN, n_t=n_t)
    else:
        if c["disc"] == "p2v":
            th = rectangle_p2p1(2, 2, 1.0, 1.0)
            sd = SpatialDiscretisation(M=th.M_v, K=th.K_v, coords=np.vstack([th.coords_v] * 2),
                                       boundary=th.boundary_v, name="p2v")
        else:
            sd = unit_square_p1(6)
        if kind == "stationary":
            b00, b01, b10, b11 = stationary_blocks(sd.M, sd.K, beta)
            p = dict(sd=sd, tau=1.0, beta=beta, n_t=1, CN=False, m=1, blocks=(b00, b01, b10, b11),
                     nodes=sd.boundary)
        else:
            tau = 2.0 / (n_t - 1.0)
            K = [sd.K + (0.1 * i) * sd.M for i in range(n_t)] if c["td"] else sd.K
            b00, b01, b10, b11, m = instationary_blocks(sd.M, K, tau, beta, n_t, CN, share=True)
            p = dict(sd=sd, tau=tau, beta=beta, n_t=n_t, CN=CN, m=m, blocks=(b00, b01, b10, b11),
                     nodes=sd.boundary)
    p["nodes"] = np.asarray(p["nodes"], dtype=np.int64)
    _PROBLEMS[key] = p
    return p


_COARSE = {}


def coarse_space(c):
    """The multilinear coarse space with the fewest cells that leave >= 4 coarse functions: one
    cell (4 functions; two components: 8)."""
    if not c["coarse"]:
        return None
    if c["disc"] not in _COARSE:
        from control_amd.coarse import multilinear_coarse_space
        p = problem(c)
        P = multilinear_coarse_space(p["sd"].coords, p["nodes"], cells=1)
        assert P.shape[1] >= 4
        _COARSE[c["disc"]] = P
    return _COARSE[c["disc"]]


def specs(c):
    """``(mass, schur)`` as ``(its, emin, emax, eimag)`` tuples."""
    mass = MASS20 if c["mass"] == 20 else MASS0
    assert c["mass"] in (0, 20)
    if c["estimated"]:
        return mass + (0.0,), (-1, 0.0, 0.0, 0.0)
    return mass + (0.0,), (c["schur"],) + INTERVAL + (c["eimag"],)


def steps(c, its=None):
    """Dependent row steps on the longest path through one application: the mass solve, then per
    sweep and level the sub-solve (``cycles`` x [correction, sweeps]) and the product that feeds
    the next level, and the two products between the stages."""
    its = c["schur"] if its is None else its
    sub = c["coarse"] * (its + 1) if c["coarse"] else max(its, 1)
    return max(c["mass"], 1) + 2 * problem(c)["m"] * (sub + 1) + 2


def inputs(c):
    """``{name: flat vector}``: a seeded random vector; with ``impulses``: ``b_0`` (``b_1``)
    non-zero on a single level, and on a single boundary node."""
    p = problem(c)
    m, nx = p["m"], p["sd"].n_dofs
    rng = np.random.default_rng(SEED)
    out = {"random": rng.standard_normal(2 * m * nx)}
    if c["impulses"]:
        node = int(p["nodes"][len(p["nodes"]) // 3])
        for name in IMPULSES:
            x = np.zeros((2, m, nx))
            var = 0 if name.startswith("b0") else 1
            level = (m // 2) if var == 0 else m - 1
            if name.endswith("level"):
                x[var, level] = rng.standard_normal(nx)
            else:
                x[var, level, node] = 1.0 + rng.random()
            out[name] = x.ravel()
    return out


def split(c, x):
    """``(x_0, x_1)``, each ``(m, nx)``."""
    p = problem(c)
    return np.asarray(x).reshape(2, p["m"], p["sd"].n_dofs)


# ------------------------------------------------------------------------------ the three sides
def _dense(blocks):
    return {k: (None if A is None else A.toarray()) for k, A in blocks.items()}


def reference(c, dps=None, wrong=None, records=None):
    """The extended-precision reference of the case.  ``records``: ``pc_solves()`` of a device
    run -- every sub-solve then runs with the interval and degree its record reports."""
    import schur_pc_ref as ref
    p = problem(c)
    mass, schur = specs(c)
    P = coarse_space(c)
    Pd = None if P is None else P.toarray()

    def spec(its, emin, emax, eimag):
        s = dict(its=int(its), emin=emin, emax=emax, eimag=eimag)
        if Pd is not None:
            s.update(P=Pd, cycles=c["coarse"])
        return s

    if records is None:
        assert not c["estimated"]
        sch = spec(*schur)
    else:
        table = {(r["sweep"], r["level"]): spec(r["its"], r["emin"], r["emax"], r["eimag"])
                 for r in records}
        assert len(table) == len(records)

        def sch(sweep, level):
            return table[(sweep, level)]
    b00, b01, b10, b11 = p["blocks"]
    return ref.Reference(c["kind"], p["sd"].M.toarray(), _dense(b01), _dense(b10), p["nodes"],
                         p["beta"], dict(its=mass[0], emin=mass[1], emax=mass[2]), sch,
                         n_t=p["n_t"], tau=p["tau"], epsilon=EPSILON,
                         dps=ref.DPS if dps is None else dps, wrong=wrong)


def oracle_apply(c, x):
    """The float64 oracle's application (``oracle/kkt_oracle.py``)."""
    from oracle import kkt_oracle as ko
    p = problem(c)
    mass, schur = specs(c)
    sd, m = p["sd"], p["m"]
    b00, b01, b10, b11 = p["blocks"]
    ns = tuple(ko.DirichletBCNullspace(p["nodes"]) for _ in range(m))
    osys = ko.OracleSystem(sd.n_dofs, sd.n_dofs, b00, b01, b10, b11, n_blocks_00=m, n_blocks_11=m,
                           nullspace_0=ns, nullspace_1=ns, CN=p["CN"])
    sch = ko.ChebSpec(*schur)
    P = coarse_space(c)
    if P is not None:
        sch.coarse = ko.CoarseSpace(P, c["coarse"])
    ms = ko.ChebSpec(*mass)
    if c["kind"] == "stationary":
        pc = ko.pc_stationary(sd.M, b10[(0, 0)], b01[(0, 0)], p["beta"], p["nodes"], ms, sch)
    elif c["kind"] == "CN":
        pc = ko.pc_instationary_CN(sd.M, b01, b10, p["n_t"], p["tau"], p["beta"], p["nodes"], ms,
                                   sch)
    else:
        pc = ko.pc_instationary_BE(sd.M, b01, b10, p["n_t"], p["tau"], p["beta"], p["nodes"], ms,
                                   sch, epsilon=EPSILON)
    return osys.pc_apply(pc, x)


def gpu_handle(c, options=None):
    """``(system, SchurPC)`` on a fresh handle."""
    from control_amd.multiblock import (ChebSpec, CoarseSpace, DirichletBCNullspace,
                                        MultiBlockSystem, SchurPC)
    p = problem(c)
    mass, schur = specs(c)
    sd, m = p["sd"], p["m"]
    ns = tuple(DirichletBCNullspace(p["nodes"]) for _ in range(m))
    g = MultiBlockSystem(sd.n_dofs, sd.n_dofs, *p["blocks"], n_blocks_00=m, n_blocks_11=m,
                         nullspace_0=ns, nullspace_1=ns, CN=p["CN"], options=options)
    if getattr(sd, "coords", None) is not None:
        g.set_tile_coordinates(sd.coords)
    sch = ChebSpec(*schur)
    P = coarse_space(c)
    if P is not None:
        sch.coarse = CoarseSpace(P, c["coarse"])
    pc = SchurPC(kind=c["kind"], M=sd.M, beta=p["beta"], bc_nodes=p["nodes"], mass=ChebSpec(*mass),
                 schur=sch, n_t=p["n_t"], tau=p["tau"], epsilon=EPSILON)
    return g, pc


# ------------------------------------------------------------------------------ the fixture
def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "schur_pc_definition.npz")


_GOLDEN = []


def golden():
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(golden_path())))
    return _GOLDEN[0]


def golden_reference(c, name):
    """``(hi_0, lo_0, hi_1, lo_1, d_case)`` of one case and input from the fixture: the extended
    reference per variable as ``hi + lo`` and the oracle's distance from it."""
    g, k = golden(), case_id(c) + "/" + name
    hi, lo = g[k + "/hi"], g[k + "/lo"].astype(np.float64)
    return hi[0], lo[0], hi[1], lo[1], float(g[k + "/d"])


def distance(c, y, hi0, lo0, hi1, lo1):
    """Per-block distance of an output from a reference: the larger of the two variables'."""
    import schur_pc_ref as ref
    y0, y1 = split(c, y)
    return max(ref.block_distance(y0, hi0, lo0), ref.block_distance(y1, hi1, lo1))


def zero_blocks_are_plus_zero(c, y, hi0, lo0, hi1, lo1):
    """Every output level that is exactly zero in the reference is ``+0.0`` in every bit."""
    ok = True
    for got, hi, lo in zip(split(c, y), (hi0, hi1), (lo0, lo1)):
        for g, h, l in zip(got, hi, lo):
            if not h.any() and not l.any():
                ok = ok and not g.view(np.uint64).any()
    return ok
