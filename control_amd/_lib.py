"""ctypes binding of ``libkkt.so`` (``include/kkt.h``).  No PyTorch, no fallbacks.

The library is built in-tree by ``make -C control_amd/csrc`` (``__graft_entry__.build``).
Loading fails loudly when it is missing; creating a system fails loudly when there is no
GPU -- the product has no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (KKT_LIB: another build of the same library, for same-box A/B measurements of a kernel change)
LIB_PATH = os.environ.get("KKT_LIB") or os.path.join(_HERE, "libkkt.so")

c_i32p = C.POINTER(C.c_int32)
c_f64p = C.POINTER(C.c_double)


class KktError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkkt error {code}: {msg}")
        self.code = code


class PcDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("n_t", C.c_int), ("tau", C.c_double),
                ("beta", C.c_double), ("epsilon", C.c_double), ("nx", C.c_int64),
                ("m_indptr", c_i32p), ("m_indices", c_i32p), ("m_values", c_f64p),
                ("n_bc", C.c_int64), ("bc_idx", c_i32p),
                ("mass_its", C.c_int), ("mass_emin", C.c_double), ("mass_emax", C.c_double),
                ("schur_its", C.c_int), ("schur_emin", C.c_double),
                ("schur_emax", C.c_double), ("schur_eimag", C.c_double),
                ("coarse_cycles", C.c_int), ("n_coarse", C.c_int64),
                ("p_indptr", c_i32p), ("p_indices", c_i32p), ("p_values", c_f64p)]


class PcStokesDesc(C.Structure):
    _fields_ = [("n_p_blocks", C.c_int), ("cn", C.c_int), ("nv", C.c_int64), ("np", C.c_int64),
                ("b_scale", C.c_double), ("post_scale", C.c_double),
                ("b_indptr", c_i32p), ("b_indices", c_i32p), ("b_values", c_f64p),
                ("kp_indptr", c_i32p), ("kp_indices", c_i32p), ("kp_values", c_f64p),
                ("mp_indptr", c_i32p), ("mp_indices", c_i32p), ("mp_values", c_f64p),
                ("kp_its", C.c_int), ("kp_emin", C.c_double), ("kp_emax", C.c_double),
                ("mp_its", C.c_int), ("mp_emin", C.c_double), ("mp_emax", C.c_double),
                ("kp_coarse_cycles", C.c_int), ("kp_n_coarse", C.c_int64),
                ("kp_p_indptr", c_i32p), ("kp_p_indices", c_i32p), ("kp_p_values", c_f64p)]


class Info(C.Structure):
    _fields_ = [(n, C.c_int64) for n in
                ("n_local", "n_blocks_stored", "n_value_arrays", "n_patterns",
                 "nnz_blocks", "rows_blocks", "bytes_algorithmic",
                 "bytes_device_values", "bytes_device_index", "bytes_streamed")] + \
               [("last_solve_ms", C.c_double), ("last_pc_applies", C.c_int64),
                ("last_op_applies", C.c_int64), ("program_fallbacks", C.c_int64)] + \
               [(n, C.c_int64) for n in
                ("sweep_form", "sweep_tiles", "sweep_threads", "sweep_depth", "sweep_row_slots",
                 "sweep_its", "apply_launches", "apply_switched", "blocks_unset")]

    def as_dict(self):
        return {n: getattr(self, n) for cls in reversed(type(self).__mro__)
                for n, _ in cls.__dict__.get("_fields_", ())}


class InfoRings(Info):
    """``kkt_info`` as the library fills it today: the fields of ``Info`` (whose list is pinned
    where it stood when ``blocks_unset`` was appended) followed by what was appended since."""
    _fields_ = [("sweep_coarse_rings", C.c_int64), ("sweep_coarse_cache", C.c_int64),
                ("sweep_coarse_ew", C.c_int64)]


class StageTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("operator_ms", "pc_ms", "orth_ms", "allreduce_ms",
                                          "other_ms", "total_ms")] + \
               [(n, C.c_int64) for n in ("iterations", "operator_applies", "pc_applies")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PcStageTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("sweeps_ms", "batched_ms", "comm_ms", "total_ms")] + \
               [(n, C.c_int64) for n in ("sweep_launches", "sweep_phases", "batched_launches",
                                         "comm_steps")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CoarseStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("matrices", "launches", "n_coarse")] + [("ms", C.c_double)]
                + [(n, C.c_int64) for n in ("blocks", "block_n")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SpectrumStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("matrices", "batches", "lanczos_steps", "power_steps", "launches",
                                          "syncs", "twin_syncs", "lanczos_syncs_max", "fallbacks",
                                          "batch_bytes")] + [("ms", C.c_double)] +
                [(n, C.c_int64) for n in ("alias_blocks", "aliased")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class StepLock(C.Structure):
    _fields_ = [("n_steps", C.c_int), ("restart", C.c_int), ("V", c_f64p), ("h", c_f64p),
                ("v_next", c_f64p)]


class RelinDesc(C.Structure):
    # kkt_relin_desc; nv (it fills the padding before ne) selects the element: 0 P2-P1 triangles
    # (nq = 7), 9 Q2-Q1 quadrilaterals (nq = 16: gphi / glam are the reference tables, jinv the
    # cells' 1 / hx, 1 / hy)
    _fields_ = ([("n_t", C.c_int), ("cn", C.c_int), ("nq", C.c_int), ("nv", C.c_int),
                 ("ne", C.c_int64), ("n2", C.c_int64), ("n1", C.c_int64),
                 ("nu", C.c_double), ("tau", C.c_double), ("beta", C.c_double),
                 ("V", c_i32p)] + [(n, c_f64p) for n in ("W", "phi", "gphi", "lam", "glam")]
                + [("nnz2", C.c_int64)]
                + [(n, c_i32p) for n in ("v_indptr", "v_indices", "v_tperm", "v_cptr", "v_clist")]
                + [("K2", c_f64p), ("M2", c_f64p), ("nnz1", C.c_int64)]
                + [(n, c_i32p) for n in ("p_indptr", "p_indices", "p_tperm", "p_cptr", "p_clist")]
                + [("Kp", c_f64p), ("Mp", c_f64p), ("nnz_b", C.c_int64),
                   ("b_indptr", c_i32p), ("b_indices", c_i32p), ("b_values", c_f64p),
                   ("n_bc", C.c_int64), ("bc_idx", c_i32p), ("data", c_f64p), ("jinv", c_f64p)])


class RelinRecipe(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("quadrant", "i", "j", "space", "level", "transpose")] + \
               [("alpha", C.c_double), ("gamma", C.c_double)]


class ReactionDesc(C.Structure):
    # kkt_reaction_desc; nq selects the element: 7 P1 triangles, 15 P1 tetrahedra, 25 P2 triangles
    # or, with nv = 9, Q2 quadrilaterals (nv = 0: inferred from nq; the field fills the padding
    # before ne); lam: the nq x nv values of the shape functions at the points
    _fields_ = ([("n_t", C.c_int), ("cn", C.c_int), ("nq", C.c_int), ("nv", C.c_int),
                 ("ne", C.c_int64),
                 ("n1", C.c_int64), ("tau", C.c_double), ("beta", C.c_double),
                 ("cells", c_i32p), ("W", c_f64p), ("lam", c_f64p), ("nnz", C.c_int64)]
                + [(n, c_i32p) for n in ("indptr", "indices", "tperm", "cptr", "clist")]
                + [("L", c_f64p), ("M", c_f64p), ("degree", C.c_int), ("c", C.c_double * 5),
                   ("n_bc", C.c_int64), ("bc_idx", c_i32p), ("data", c_f64p)])


# kkt_debug_krylov_op: the operations (KKT_KRYLOV_*) and the padding value (KKT_KRYLOV_PAD)
KRYLOV_OPS = {name: k for k, name in enumerate(
    ("mdot", "orthogonalise", "build_solution", "scale_inv", "axpby", "copy", "fill", "norm2",
     "maxpy"))}
KRYLOV_PAD = -6.02214076e23

# kkt_debug_block_op: the operations (KKT_BLOCK_*), the guard elements around every written array
# (KKT_BLOCK_GUARD, set to KRYLOV_PAD; the flag's to BLOCK_FLAG_PAD) and the argument record
BLOCK_OPS = {name: k for k, name in enumerate(
    ("time_transform", "time_transform_mask", "mask_blocks", "const_correct", "const_center",
     "csr_to_sell", "mask_columns", "vals_axpy", "vals_differ", "vals_sym_skew", "extract_dinv"))}
BLOCK_GUARD = 64
BLOCK_FLAG_PAD = 0xA5A5A5A5
c_u8p = C.POINTER(C.c_uint8)
c_i64p = C.POINTER(C.c_int64)
c_u32p = C.POINTER(C.c_uint32)


class BlockOp(C.Structure):
    _fields_ = ([(n, C.c_int) for n in ("op", "kind", "in_place", "n")]
                + [("nx", C.c_int64), ("len", C.c_int64), ("c", C.c_double)]
                + [(n, c_f64p) for n in ("x", "x2", "lo_halo", "hi_halo")]
                + [("mask", c_u8p), ("has_mask", c_i32p), ("alpha", c_f64p),
                   ("job_off", c_i64p), ("job_nx", c_i64p)]
                + [(n, c_f64p) for n in ("job_c1", "job_c2_one", "job_c2_alpha")]
                + [(n, c_i32p) for n in ("idx", "idx2", "idx3")]
                + [("y", c_f64p), ("y2", c_f64p), ("flag", c_u32p), ("inputs_changed", C.c_int32)])


# kkt_debug_spectrum_op: the operations (KKT_SPECTRUM_*), the modes of DOT, the kinds of UPDATE and
# the argument record; guards as for kkt_debug_block_op
SPECTRUM_OPS = {name: k for k, name in enumerate(
    ("dot", "update", "sym_skew", "fingerprint", "pairs_differ"))}
SPECTRUM_DOT_MODES = {name: k for k, name in enumerate(("start", "pap", "rz", "norm0", "norm"))}
SPECTRUM_UPDATES = {name: k for k, name in enumerate(("r", "p", "scale", "copy"))}
c_u64p = C.POINTER(C.c_uint64)


class SpectrumOp(C.Structure):
    _fields_ = ([(n, C.c_int) for n in ("op", "mode", "k", "nmat", "max_steps", "npairs")]
                + [("n", C.c_int64), ("stride", C.c_int64)]
                + [("x", c_f64p), ("y", c_f64p), ("v", c_f64p), ("active", c_u32p),
                   ("na", c_i32p), ("nb", c_i32p)]
                + [(n, c_f64p) for n in ("rz", "coef", "last", "mu2", "alpha", "beta", "part")]
                + [("a", c_f64p), ("tpos", c_i32p), ("h", c_f64p), ("sk", c_f64p),
                   ("pair_a", c_i32p), ("pair_b", c_i32p), ("flag", c_u32p),
                   ("words", c_u64p), ("fold", c_u64p),
                   ("batch_stride", C.c_int64), ("inputs_changed", C.c_int32)])


# kkt_debug_row_step: the forms (KKT_ROWSTEP_*), modes, kernel families it reports and its records
ROWSTEP_FORMS = {name: k for k, name in enumerate(("rows", "single", "shared", "interleaved"))}
ROWSTEP_LIN, ROWSTEP_CHEB = 0, 1
ROWSTEP_FAMILIES = ("pc_rows", "pc_row_step", "pc_rows_shared", "pc_rows_shared_g", "pc_rows_il")
ROWSTEP_MAX_TERMS = 8


class RowStepOp(C.Structure):
    _fields_ = ([("mode", C.c_int32), ("nterms", C.c_int32)]
                + [(n, C.c_int32 * ROWSTEP_MAX_TERMS) for n in ("term_q", "term_i", "term_j",
                                                                "term_x")]
                + [(n, C.c_int32) for n in ("y", "y2", "yin", "z", "mx", "b", "pkm1", "pk")]
                + [(n, C.c_double) for n in ("ca", "cy", "cz", "malpha", "c1", "c2", "c3",
                                             "post1", "post2")])


class RowStep(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("form", "q", "i", "j", "nops", "pc_xcd", "nvec", "pad_")]
                + [("ops", C.POINTER(RowStepOp)), ("vecs", c_f64p), ("rowmask", c_u8p),
                   ("dinv", c_f64p), ("il_x", c_f64p), ("il_pkm1", c_f64p), ("il_y", c_f64p)]
                + [(n, C.c_int32) for n in ("family", "width", "launched", "inputs_changed", "R",
                                            "uniform_w", "sorted", "nslices")])


# kkt_debug_tile_levels: one level and the whole launch
class TileLevel(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("q", "i", "j", "n_upd", "uq", "ui", "uj", "pad_")]
                + [(n, C.c_double) for n in ("ca", "cy", "p1_scale", "post1", "post2")]
                + [(n, c_f64p) for n in ("dinv", "coef", "einv", "bin", "out", "bout")])


class TileLevels(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("nlevels", "its", "cycles", "own_cap")]
                + [("levels", C.POINTER(TileLevel)), ("own_ptr", c_i32p), ("own_rows", c_i32p)]
                + [(n, C.c_int32) for n in ("inputs_changed", "tiles", "threads", "row_slots",
                                            "depth", "W", "nk_pad", "cache", "rings", "ew",
                                            "n_coarse", "nrows")])


# kkt_anderson_*: the mixer's depth limit, what a step reports, the debug operations and record
ANDERSON_MAX_DEPTH = 8
ANDERSON_OPS = {name: k for k, name in enumerate(("push", "gram", "mix", "read"))}


class AndersonInfo(C.Structure):
    _fields_ = [("columns", C.c_int32), ("dropped", C.c_int32),
                ("gamma", C.c_double * ANDERSON_MAX_DEPTH),
                ("G", C.c_double * (ANDERSON_MAX_DEPTH * ANDERSON_MAX_DEPTH)),
                ("r", C.c_double * ANDERSON_MAX_DEPTH)] + \
               [(n, C.c_double) for n in ("push_ms", "gram_ms", "mix_ms")]


class AndersonOp(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("op", "c", "alias", "which", "slot", "inputs_changed")]
                + [("n", C.c_int64), ("slack", C.c_int64), ("beta", C.c_double),
                   ("gamma", C.c_double * ANDERSON_MAX_DEPTH)]
                + [(n, c_f64p) for n in ("f", "dF", "dX", "f_prev", "out", "out2", "G", "r")]
                + [("ring", C.c_int32 * 4)])


PC_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, c_f64p, c_f64p, c_f64p, c_f64p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, c_f64p, C.c_int, C.c_int)
SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, c_f64p, C.c_int64, C.c_int,
                          c_f64p, C.c_int64, C.c_int)

# name -> (restype, argtypes); every symbol include/kkt.h declares
SIGNATURES = {
    "kkt_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "kkt_destroy": (C.c_int, [C.c_void_p]),
    "kkt_last_error": (C.c_char_p, [C.c_void_p]),
    "kkt_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "kkt_set_tile_coordinates": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, c_f64p]),
    "kkt_set_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                 C.c_int, C.c_int, C.c_int]),
    "kkt_set_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "kkt_set_shard_families": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "kkt_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)]),
    "kkt_add_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                C.c_int64, c_i32p, c_i32p, c_f64p, C.c_int64]),
    "kkt_add_block_structure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                          C.c_int64, c_i32p, c_i32p]),
    "kkt_update_block_values": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_f64p]),
    "kkt_set_bc": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, c_i32p, C.c_double]),
    "kkt_set_const_nullspace": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "kkt_finalize": (C.c_int, [C.c_void_p]),
    "kkt_set_pc_schur": (C.c_int, [C.c_void_p, C.POINTER(PcDesc)]),
    "kkt_set_pc_stokes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(PcStokesDesc)]),
    "kkt_set_pc_callback": (C.c_int, [C.c_void_p, PC_CALLBACK, C.c_void_p]),
    "kkt_set_pc_identity": (C.c_int, [C.c_void_p]),
    "kkt_set_krylov": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                 C.c_double, C.c_double, C.c_int]),
    "kkt_apply": (C.c_int, [C.c_void_p, c_f64p, c_f64p]),
    "kkt_pc_apply": (C.c_int, [C.c_void_p, c_f64p, c_f64p]),
    "kkt_solve": (C.c_int, [C.c_void_p, c_f64p, c_f64p, C.POINTER(C.c_int),
                            C.POINTER(C.c_int), c_f64p, c_f64p, C.c_int,
                            C.POINTER(C.c_int)]),
    "kkt_local_size": (C.c_int64, [C.c_void_p]),
    "kkt_vec_alloc": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "kkt_vec_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kkt_vec_upload": (C.c_int, [C.c_void_p, C.c_void_p, c_f64p]),
    "kkt_vec_download": (C.c_int, [C.c_void_p, C.c_void_p, c_f64p]),
    "kkt_apply_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "kkt_pc_apply_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "kkt_solve_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), c_f64p, c_f64p, C.c_int,
                                   C.POINTER(C.c_int)]),
    "kkt_sync": (C.c_int, [C.c_void_p]),
    "kkt_set_relinearisation": (C.c_int, [C.c_void_p, C.POINTER(RelinDesc)]),
    "kkt_relinearise_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(RelinRecipe)]),
    "kkt_picard_state": (C.c_int, [C.c_void_p, C.c_int, c_f64p, c_f64p, c_f64p, c_f64p]),
    "kkt_picard_iterate": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4),
    "kkt_picard_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "kkt_picard_residual_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_f64p]),
    "kkt_picard_update_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kkt_debug_relin_array": (C.c_int, [C.c_void_p, C.c_int, c_f64p, C.c_int64]),
    "kkt_set_reaction_relinearisation": (C.c_int, [C.c_void_p, C.POINTER(ReactionDesc)]),
    "kkt_reaction_relinearise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.POINTER(RelinRecipe)]),
    "kkt_reaction_state": (C.c_int, [C.c_void_p, C.c_int, c_f64p, c_f64p]),
    "kkt_reaction_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "kkt_reaction_iterate": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 2),
    "kkt_reaction_residual_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_f64p]),
    "kkt_reaction_update_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kkt_debug_reaction_array": (C.c_int, [C.c_void_p, C.c_int, c_f64p, C.c_int64]),
    "kkt_anderson_set": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "kkt_anderson_step": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AndersonInfo)]),
    "kkt_anderson_reset": (C.c_int, [C.c_void_p]),
    "kkt_debug_anderson_op": (C.c_int, [C.c_void_p, C.POINTER(AndersonOp)]),
    "kkt_debug_block_values": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_f64p,
                                         C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "kkt_time_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_float)]),
    "kkt_time_pc_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_float)]),
    "kkt_time_pc_sweeps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "kkt_get_stage_times": (C.c_int, [C.c_void_p, C.POINTER(StageTimes)]),
    "kkt_time_pc_stages": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(PcStageTimes)]),
    "kkt_coarse_setup_stats": (C.c_int, [C.c_void_p, C.POINTER(CoarseStats)]),
    "kkt_spectrum_stats_get": (C.c_int, [C.c_void_p, C.POINTER(SpectrumStats)]),
    "kkt_debug_coarse_matrices": (C.c_int, [C.c_void_p, c_f64p, C.c_int64]),
    "kkt_debug_coarse_inverses": (C.c_int, [C.c_void_p, c_f64p, C.c_int64]),
    "kkt_debug_dense_inverse": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_f64p, c_f64p, c_i32p]),
    "kkt_debug_coarse_correction": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, c_f64p, c_f64p,
                                              c_f64p, c_f64p, c_f64p, c_f64p, c_i32p]),
    "kkt_debug_krylov_op": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, c_f64p, c_f64p,
                                      c_f64p, C.c_double, C.c_double, c_f64p, c_f64p, c_f64p]),
    "kkt_debug_block_op": (C.c_int, [C.c_void_p, C.POINTER(BlockOp)]),
    "kkt_debug_spectrum_op": (C.c_int, [C.c_void_p, C.POINTER(SpectrumOp)]),
    "kkt_debug_row_step": (C.c_int, [C.c_void_p, C.POINTER(RowStep)]),
    "kkt_debug_tile_levels": (C.c_int, [C.c_void_p, C.POINTER(TileLevels)]),
    "kkt_debug_set_steplock": (C.c_int, [C.c_void_p, C.POINTER(StepLock)]),
    "kkt_debug_apply_forms": (C.c_int, [C.c_void_p, c_i32p, C.c_int]),
    "kkt_debug_pc_forms": (C.c_int, [C.c_void_p, c_i32p, C.c_int]),
    "kkt_debug_pc_solves": (C.c_int, [C.c_void_p, c_f64p, C.c_int]),
    "kkt_debug_pc_matrices": (C.c_int, [C.c_void_p, c_f64p, C.c_int]),
    "kkt_debug_pc_alias": (C.c_int, [C.c_void_p, c_i32p, C.c_int]),
    "kkt_debug_mass_tile_values": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             c_f64p, c_i32p, c_f64p]),
    "kkt_get_info": (C.c_int, [C.c_void_p, C.POINTER(Info)]),
    "kkt_comm_unique_id": (C.c_int, [C.c_void_p]),
    "kkt_comm_init_rccl": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kkt_comm_init_callbacks": (C.c_int, [C.c_void_p, ALLREDUCE_FN, SENDRECV_FN,
                                          C.c_void_p]),
    "kkt_comm_barrier": (C.c_int, [C.c_void_p]),
    "kkt_comm_max": (C.c_int, [C.c_void_p, c_f64p]),
}

_lib = None


def load():
    """The loaded library with typed entry points.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C control_amd/csrc` "
            "(hipcc --offload-arch=gfx950).  control_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(c_f64p)


def i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(c_i32p)
