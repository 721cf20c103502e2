"""The Python mirror of include/molnextr_hip.h, once: the ABI version, the structs (ctypes) and records (numpy dtypes), every
flag and limit constant, the prototype of every entry point as ONE table (PROTOTYPES), and the loader that applies it.

Nothing here knows an engine: engine.py, engine_tables.py and engine_lab.py (the three files `class Engine` is written in) and
graphs.py import from here, and this module imports nothing of the package. It is importable without the library having been
built (tests/test_binding_mirror_host.py reads the table against the header that way). PyTorch is plumbing: it owns device
memory and the HIP stream; every tensor crosses the C ABI as a raw device pointer (_ptr, _stream). There is NO CPU fallback: if
the library is missing, load_library raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmolnextr_hip.so")
_lib = None

ABI_VERSION = 7

# Encoder operand modes (include/molnextr_hip.h MNX_DTYPE_*). "fp16x3" — split fp16 operands, three MFMA terms per
# product, fp32-class results — is the default: it is the fastest mode whose results stay a factor of four inside north_star's
# tolerance (raw logits within 2.5e-4 of the reference's over EVERY step of 181 539 checked beyond the fixtures, features within 3e-5).
# "fp16x3m" (opt-in) is fp16x3 with the layers of FP16X3M_TWO_TERM (qkv, fc1, fc2 of Swin stage 3: 60 % of the encoder's GEMM time)
# on TWO terms — the activation's lo plane dropped, the weight's kept: +8-11 % throughput. On the committed fixtures (12863
# teacher-forced steps, both checkpoints) every token / atom / bond is the reference's, log-probs within 1.8e-4, raw logits of
# steps 0..3 within 4.997e-4 — the round-5 review's 5e-4 gate met to the letter; on 384 further images against the oracle
# (tools/extended_parity.py, 77 790 steps, still 0 flips, every row exact) the raw logits reach 7.2e-4 / 8.7e-4 (hostile
# checkpoint), and on 384 more images of the hostile checkpoint 1.2e-3 — BEYOND north_star's 1e-3 in 2 of 12 batches (tokens
# still exact: 0 flips in 141 939 steps). A throughput mode for the caller who accepts that (profiles/r06_extended_parity_*.json,
# r06_two_term_tables_gpu.json; tests/test_gpu_pixels.py). Both modes run the same weights and kernels (Engine.set_op_terms).
DTYPES = {"bf16": 0, "fp16": 1, "fp32": 2, "bf16x3": 3, "fp16x3": 4, "fp16x3m": 5}
DEFAULT_DTYPE = "fp16x3"
SPLIT_CLASSES = {"qkv": 1, "attn": 2, "proj": 4, "fc1": 8, "fc2": 16, "merge": 32}
# FP16X3M's table for Swin-B's four stages, as set_op_terms arguments. The library installs it from include/molnextr_hip.h
# MNX_FP16X3M_TWO_TERM_BY_STAGE / _FIRST_BLOCK_BY_STAGE (tests/test_abi.py checks that these two say the same).
FP16X3M_BLOCKS = {}                                       # {stage: (first_block, last_block)}
FP16X3M_TWO_TERM = ("qkv.s2", "fc1.s2", "fc2.s2")       # tags: "cls" or "cls.sN", N 0-based


def two_term_masks(two_term, n_stages):
    """Per-stage MNX_OP_* masks of set_op_terms tags ("cls" or "cls.sN")."""
    masks = [0] * n_stages
    for tag in two_term:
        cls, _, st = tag.partition(".s")
        for i in ([int(st)] if st else range(n_stages)):
            masks[i] |= SPLIT_CLASSES[cls]
    return masks


class MnxConfig(C.Structure):
    _fields_ = [("img_size", C.c_int32), ("patch", C.c_int32), ("embed_dim", C.c_int32), ("n_stages", C.c_int32),
                ("depths", C.c_int32 * 4), ("heads", C.c_int32 * 4), ("window", C.c_int32),
                ("dec_layers", C.c_int32), ("dec_dim", C.c_int32), ("dec_heads", C.c_int32), ("dec_ff", C.c_int32),
                ("vocab", C.c_int32), ("sym_offset", C.c_int32), ("coord_bins", C.c_int32), ("pe_len", C.c_int32),
                ("max_len", C.c_int32), ("max_batch", C.c_int32), ("max_atoms", C.c_int32),
                ("compute_dtype", C.c_int32), ("dec_slots", C.c_int32)]


class MnxWeightDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class MnxPage(C.Structure):
    """include/molnextr_hip.h mnx_page: one page of a mnx_preprocess_batch arena."""
    _fields_ = [("offset", C.c_uint64), ("height", C.c_int32), ("width", C.c_int32)]


class MnxMol(C.Structure):
    """include/molnextr_hip.h mnx_mol: one molecule of mnx_graph_pack (40 bytes)."""
    _fields_ = [("atom0", C.c_uint32), ("n_atoms", C.c_uint32), ("bond0", C.c_uint32), ("n_bonds", C.c_uint32),
                ("text0", C.c_uint32), ("smiles_len", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("overall_score", C.c_double)]


class MnxAtom(C.Structure):
    """include/molnextr_hip.h mnx_atom (24 bytes)."""
    _fields_ = [("sym0", C.c_uint32), ("sym_len", C.c_uint16), ("index", C.c_uint16), ("x_bin", C.c_uint16),
                ("y_bin", C.c_uint16), ("score", C.c_double)]


class MnxBond(C.Structure):
    """include/molnextr_hip.h mnx_bond (16 bytes)."""
    _fields_ = [("i", C.c_uint16), ("j", C.c_uint16), ("type", C.c_uint8), ("rev", C.c_uint8), ("score", C.c_double)]


class MnxMolfile(C.Structure):
    """include/molnextr_hip.h mnx_molfile: one molecule of mnx_molfile_pack (16 bytes)."""
    _fields_ = [("text0", C.c_uint32), ("len", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class MnxSmiles(C.Structure):
    """include/molnextr_hip.h mnx_smiles: one molecule of mnx_smiles_pack (16 bytes)."""
    _fields_ = [("text0", C.c_uint32), ("len", C.c_uint32), ("flags", C.c_uint32), ("n_rings", C.c_uint32)]


# the same three records as numpy structured dtypes (C layout: align=True), what Engine.graph_pack returns
MOL_DTYPE = np.dtype([("atom0", "<u4"), ("n_atoms", "<u4"), ("bond0", "<u4"), ("n_bonds", "<u4"), ("text0", "<u4"),
                      ("smiles_len", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("overall_score", "<f8")], align=True)
ATOM_DTYPE = np.dtype([("sym0", "<u4"), ("sym_len", "<u2"), ("index", "<u2"), ("x_bin", "<u2"), ("y_bin", "<u2"),
                       ("score", "<f8")], align=True)
BOND_DTYPE = np.dtype([("i", "<u2"), ("j", "<u2"), ("type", "u1"), ("rev", "u1"), ("score", "<f8")], align=True)
MOL_TRUNCATED = 1                       # mnx_mol.flags bit 0: more atoms than kmax, the tables hold the first kmax
# mnx_mol.flags of mnx_expand_pack's output (MNX_MOL_EXPAND*): a label was replaced by its fragment; a pseudo-atom other than a
# parsed '*' remains; the molecule was refused (records beyond the tables, bonds not sorted by i, more than 2047 atoms): no records
MOL_EXPANDED, MOL_LABEL_LEFT, MOL_EXPAND_REFUSED = 2, 4, 8
# mnx_mol.flags of mnx_normalize_pack's output: an atom became aromatic; a bracket atom lost its brackets; the molecule was refused
# (records beyond the tables, more than 999 atoms or bonds): no records. The bits of its `atom_notes`: the H count, made aromatic
# by the call, brackets removed, the symbol copied uninterpreted
MOL_AROMATIZED, MOL_UNBRACKETED, MOL_NORMALIZE_REFUSED = 16, 32, 64
# mnx_mol.flags of mnx_kekulize_pack's output: a system was rewritten; a system stayed aromatic; the molecule was refused. Its
# atom_notes: NOTE_H_MASK, NOTE_COPIED and the three bits below; KEKULE_DEFAULT_STEPS is what max_steps = 0 stands for
MOL_KEKULIZED, MOL_KEKULE_LEFT, MOL_KEKULIZE_REFUSED = 128, 256, 512
NOTE_KEKULIZED, NOTE_KEKULE_LEFT, NOTE_KEKULE_LIMIT = 16, 32, 128
KEKULE_DEFAULT_STEPS = 16384
NOTE_H_MASK, NOTE_AROMATIZED, NOTE_UNBRACKETED, NOTE_COPIED = 15, 16, 32, 64
# mnx_mol.flags of mnx_formula_pack's output: a condensed-formula label was replaced by the structure the search found; a candidate
# label stayed; the search of a label passed the step limit; the molecule was refused (as MOL_EXPAND_REFUSED): no records.
# FORMULA_DEFAULT_STEPS is what max_steps = 0 stands for
MOL_FORMULA_EXPANDED, MOL_FORMULA_LEFT, MOL_FORMULA_LIMIT, MOL_FORMULA_REFUSED = 1 << 10, 1 << 11, 1 << 16, 1 << 17
FORMULA_DEFAULT_STEPS = 4096
# mnx_mol.flags of mnx_main_pack's output: the molecule had more than one component and atoms were dropped; another component had
# as many atoms as the kept one (the choice rests on the atom numbering, as the reference's); the molecule was refused (records
# beyond the tables, a bond to no atom of the molecule, more than 2047 atoms): no records
MOL_MAIN_KEPT, MOL_MAIN_TIE, MOL_MAIN_REFUSED = 1 << 18, 1 << 19, 1 << 20
MOLFILE_DTYPE = np.dtype([("text0", "<u4"), ("len", "<u4"), ("flags", "<u4"), ("reserved", "<u4")], align=True)
# mnx_molfile.flags (MNX_MOLFILE_*): no molfile (len 0) for more than 999 atoms / bonds or records beyond the tables passed;
# the molecule holds a pseudo-atom (R-group, abbreviation, unparsable symbol); a copy of MOL_TRUNCATED
MOLFILE_TOO_LARGE, MOLFILE_BEYOND_TABLES, MOLFILE_PSEUDO_ATOM, MOLFILE_TRUNCATED = 1, 2, 4, 8
SMILES_DTYPE = np.dtype([("text0", "<u4"), ("len", "<u4"), ("flags", "<u4"), ("n_rings", "<u4")], align=True)
# mnx_smiles.flags (MNX_SMILES_*): the first four as the molfile's; the same atom pair in two bond records; more than 99 ring
# closure numbers in use; wedge bonds written as plain single bonds; a bond of an unknown class written as '~'
(SMILES_TOO_LARGE, SMILES_BEYOND_TABLES, SMILES_PSEUDO_ATOM, SMILES_TRUNCATED, SMILES_DUPLICATE_BOND, SMILES_RING_NUMBERS,
 SMILES_WEDGES_DROPPED, SMILES_UNKNOWN_BOND) = 1, 2, 4, 8, 16, 32, 64, 128
# mnx_smiles_pack_stereo only: at least one '@' / '@@' was written; a marked carbon with a wedge seen from it got no mark. There
# SMILES_WEDGES_DROPPED means a wedge bond neither end of which received a mark.
SMILES_STEREO, SMILES_STEREO_UNRESOLVED = 256, 512
# mnx_smiles_pack_marks with SMILES_MARK_DOUBLE_BOND only: at least one '/' or '\' was written; a candidate double bond got no
# marks; a double bond without marks of its own stands between two directed bonds (a reader would take a configuration from there
# that the drawing did not give: fall back to the string without double-bond marks for that molecule).
SMILES_EZ, SMILES_EZ_UNRESOLVED, SMILES_EZ_IMPLIED = 1024, 2048, 4096
SMILES_MARK_TETRAHEDRAL, SMILES_MARK_DOUBLE_BOND = 1, 2     # the `marks` of mnx_smiles_pack_marks
# mnx_smiles_pack_canonical only: a tie between atoms of one rank was broken by the drawing; in one of them the atom index alone
# decided (two tied atoms on one bin): only then can the bytes depend on the numbering of the drawing
SMILES_CANON_TIE, SMILES_CANON_TIE_INDEX = 8192, 16384
# mnx_smiles_pack_symmetric only: a candidate centre or double bond wrote no mark because two of its substituents share a symmetry
# class; the per-atom bits of its `atom_marks` (ATOM_MARKS_NONE for every atom of a molecule that got no string)
SMILES_SYM_DROPPED = 32768
ATOM_MARK_CW, ATOM_MARK_CCW, ATOM_MARK_SYM, ATOM_EZ, ATOM_EZ_SYM = 1, 2, 4, 8, 16
ATOM_MARKS_NONE = 0xFF
SMILES_REFUSED = SMILES_TOO_LARGE | SMILES_BEYOND_TABLES | SMILES_DUPLICATE_BOND | SMILES_RING_NUMBERS    # no SMILES: len 0
SMILES_NO_POSITION = 0xFFFF             # `order` of an atom whose molecule got no SMILES
# mnx_read, one string of mnx_smiles_read (16 bytes), and its flags (MNX_READ_*): a rule of the grammar breaks at err_pos; more
# than 4096 bytes, 999 atoms or 999 bonds; '/' '\' or '@' were read and dropped (no refusal); offsets beyond the bytes passed
READ_DTYPE = np.dtype([("flags", "<u4"), ("err_pos", "<u4"), ("n_rings", "<u4"), ("reserved", "<u4")], align=True)
READ_SYNTAX, READ_TOO_LARGE, READ_STEREO_DROPPED, READ_BEYOND = 1, 2, 4, 8
READ_REFUSED = READ_SYNTAX | READ_TOO_LARGE | READ_BEYOND      # the empty molecule stands in its place
# mnx_molread, one file of mnx_molfile_read (16 bytes), and its flags (MNX_MOLREAD_*): a rule breaks at line err_line (SYNTAX; QUERY
# for a query bond type); more than 262144 bytes or 8192 lines; offsets beyond the bytes passed — the refusals —; and the notes: a
# bond of either / unknown stereo read as plain, an H count from the default-valence table, a coordinate outside the bins, a line or
# field that was skipped, an atom that is a label
MOLREAD_DTYPE = np.dtype([("flags", "<u4"), ("err_line", "<u4"), ("n_marked", "<u4"), ("reserved", "<u4")], align=True)
MOLREAD_SYNTAX, MOLREAD_TOO_LARGE, MOLREAD_BEYOND, MOLREAD_QUERY = 1, 2, 8, 16
MOLREAD_STEREO_EITHER, MOLREAD_H_DEFAULT, MOLREAD_CLAMPED, MOLREAD_IGNORED, MOLREAD_LABEL = 32, 64, 128, 256, 512
MOLREAD_REFUSED = MOLREAD_SYNTAX | MOLREAD_TOO_LARGE | MOLREAD_BEYOND | MOLREAD_QUERY      # the empty molecule stands in its place
# mnx_fp, one molecule of mnx_fingerprint_pack (16 bytes; its FP_WORDS words of bits stand in a table of their own), and its flags
# (MNX_FP_*): bits 0-3 as mnx_smiles'; the same atom pair in two bond records, a bond from an atom to itself or to no atom of the
# molecule; a directed bond begins more than max_steps paths. FP_DEFAULT_STEPS is what max_steps = 0 stands for, FP_MAX_STEPS the
# most a caller may pass, FP_MAX_BONDS the longest path (what max_bonds = 0 stands for)
FP_DTYPE = np.dtype([("flags", "<u4"), ("n_bits", "<u4"), ("max_paths", "<u4"), ("reserved", "<u4")], align=True)
FP_TOO_LARGE, FP_BEYOND_TABLES, FP_PSEUDO_ATOM, FP_TRUNCATED, FP_BAD_BOND, FP_LIMIT = 1, 2, 4, 8, 16, 1 << 16
FP_REFUSED = FP_TOO_LARGE | FP_BEYOND_TABLES | FP_BAD_BOND      # no fingerprint: every word 0 (as with FP_LIMIT)
FP_WORDS, FP_MAX_BONDS, FP_DEFAULT_STEPS, FP_MAX_STEPS = 64, 7, 4096, 1 << 20
# mnx_match, one pair of mnx_substructure_match (16 bytes; its map of MATCH_MAX_QUERY target atoms stands in a table of its own), and
# its flags (MNX_MATCH_*): bits 0-4 the target's admission with the FP_* values, bits 8-12 the query's (<< MATCH_QUERY_SHIFT); the
# query has more than MATCH_MAX_QUERY atoms or MATCH_MAX_QUERY_BONDS bonds, or none; a root's search passed max_steps and fewer than
# max_matches embeddings were found (the count is a lower bound); a pair names a molecule outside a table. MATCH_DEFAULT_STEPS is what
# max_steps = 0 stands for, MATCH_MAX_STEPS the most a caller may pass, MATCH_NO_ATOM a map entry beyond the query or without a match
MATCH_DTYPE = np.dtype([("flags", "<u4"), ("n_matches", "<u4"), ("steps", "<u4"), ("reserved", "<u4")], align=True)
MATCH_QUERY_TOO_LARGE, MATCH_QUERY_EMPTY, MATCH_LIMIT, MATCH_BAD_PAIR, MATCH_QUERY_SHIFT = 32, 64, 1 << 16, 1 << 17, 8
MATCH_REFUSED = FP_REFUSED | FP_REFUSED << MATCH_QUERY_SHIFT | MATCH_QUERY_TOO_LARGE | MATCH_QUERY_EMPTY | MATCH_BAD_PAIR   # no search
MATCH_MAX_QUERY, MATCH_MAX_QUERY_BONDS, MATCH_DEFAULT_STEPS, MATCH_MAX_STEPS, MATCH_NO_ATOM = 64, 128, 65536, 1 << 20, 0xFFFF
# mnx_tanimoto_search (MNX_NEAREST_*): the most neighbours, queries and library rows of one call; the index behind a query's last
# hit; the flag that keeps library row q from query q; and the call's geometry — the queries a workgroup holds at once, the library
# rows of a slab, the partial lists of a query at the most — from which the tests take their shapes
NEAREST_MAX_K, NEAREST_MAX_QUERIES, NEAREST_MAX_ROWS, NEAREST_NONE, NEAREST_SKIP_SELF = 64, 4096, 1 << 24, 0xFFFFFFFF, 1
NEAREST_QUERY_TILE, NEAREST_SLAB_ROWS, NEAREST_MAX_LISTS = 32, 256, 512


PREP_MAX_PAGES = 4096                   # include/molnextr_hip.h MNX_PREP_MAX_PAGES: pages per mnx_preprocess_batch call
IMAGE_FORMATS = {"fp32": 0, "gray8": 1}  # MNX_IMG_*: what the transform hands to the encoder
MNX_ERR_RANGE = -6      # include/molnextr_hip.h: the encoder produced non-finite features (fp16 operand range)
RANGE_FALLBACK = {"fp16x3": "bf16x3", "fp16x3m": "bf16x3", "fp16": "bf16"}    # the same operand structure with the fp32 exponent range


class MnxError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def range_fallback_dtype(err, dtype):
    """The operand mode to retry in when `err` says that an activation left the fp16 range of `dtype` (None: not that case).
    The reference handles any checkpoint in fp32; a drop-in must not die on one whose activations exceed 65504: the split
    bf16 mode keeps three-term products with the fp32 exponent range (logits within 1e-3)."""
    if isinstance(err, MnxError) and err.code == MNX_ERR_RANGE:
        return RANGE_FALLBACK.get(dtype)
    return None


# -- the prototypes: every declaration of include/molnextr_hip.h as ctypes argument types, the engine handle first -----------------
# The runs that repeat are written once (tests/test_binding_mirror_host.py holds every list against the header's parameters):
_vp, _i32, _u32, _i64, _f32, _f64p = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float, C.POINTER(C.c_double)
_TABLES_IN = [_vp, _i32, _vp, _u32, _vp, _u32, _vp, _u32]   # the input side of a packed table: mols, n, atoms, na, bonds, nb, text, nt
_ARENAS = [_vp, _u32, _vp, _u32, _vp, _u32]                 # atoms_out, atom_cap, bonds_out, bond_cap, text_out, text_cap
_TABLES_OUT = [_vp] + _ARENAS                               # the output tables: mols_out in front of the arenas
_TEXT_OUT = [_vp, _u32, _vp]                                # a text writer's out, out_cap, totals
_BYTES_IN = [_vp, _u32, _vp, _i32]                          # a reader's bytes, n_bytes, offsets, n
_WRITER = [_vp] + _TABLES_IN + [_vp, _vp] + _TEXT_OUT       # molfile_pack: scale, files; smiles_pack: recs, order — then the text
_PASS = [_vp] + _TABLES_IN + _TABLES_OUT + [_vp, _vp]       # tables to tables: the per-atom output (origin / atom_notes), totals
_DENSE = [_vp, _vp, _vp, _vp, _vp, _i32]                    # predict's tokens, lengths, n_atoms, atom_idx, edges, kmax
_SCORES = [_vp, _vp, _vp, _vp]                              # token_logp, edge_scores, atom_scores, overall_score

_STATUS_CALLS = {       # everything that returns an mnx_status
    # engine.hip: the model path
    "mnx_create": [C.POINTER(MnxConfig), C.POINTER(MnxWeightDesc), _i32, _i32, C.POINTER(_vp)],
    "mnx_encode": [_vp, _vp, _i32, _vp, _vp],
    "mnx_encode_gray8": [_vp, _vp, _i32, _vp, _vp],
    "mnx_set_encoder_tap": [_vp, _i32, _vp],
    "mnx_set_split_terms": [_vp, _i32],
    "mnx_set_op_terms": [_vp, _i32, _i32, _i32, _i32],
    "mnx_encoder_status": [_vp, C.POINTER(_i32), _vp],
    "mnx_decode_greedy": [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mnx_decode_forced": [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mnx_decode_guided": [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mnx_decode_beam": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "mnx_edges": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "mnx_preprocess": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "mnx_preprocess_batch": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp],
    "mnx_set_token_classes": [_vp, C.c_char_p] + [_i32] * 7,
    "mnx_atom_scan": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "mnx_confidence": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "mnx_predict": [_vp, _vp, _i32, _i32, _i32, _i32] + _DENSE + [_vp],
    "mnx_predict_confidence": [_vp, _vp, _i32, _i32, _i32] + _DENSE + _SCORES + [_vp],
    "mnx_predict_gray8": [_vp, _vp, _i32, _i32, _i32] + _DENSE + _SCORES + [_vp],
    "mnx_predict_guided": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32] + _DENSE + _SCORES + [_vp],
    "mnx_predict_beam": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp],
    # engine_tables.hip: the packed-table layer
    "mnx_set_vocab_text": [_vp, C.c_char_p, _vp, _i32],
    "mnx_set_symbol_tables": [_vp, C.c_char_p, _vp, _vp, _i32],
    "mnx_set_fragments": [_vp] + _TABLES_IN + [_vp, _i32],
    "mnx_graph_pack": [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp] + _TABLES_OUT + [_vp, _vp],
    "mnx_molfile_pack": _WRITER + [_vp],
    "mnx_smiles_pack": _WRITER + [_vp],
    "mnx_smiles_pack_stereo": _WRITER + [_vp],
    "mnx_smiles_pack_marks": _WRITER + [_u32, _vp],                                                  # marks in front of stream
    "mnx_smiles_pack_canonical": [_vp] + _TABLES_IN + [_vp] * 4 + _TEXT_OUT + [_u32, _vp],           # recs, order, rank, sym_class
    "mnx_smiles_pack_symmetric": [_vp] + _TABLES_IN + [_vp] * 5 + _TEXT_OUT + [_u32, _vp],           # ... and atom_marks
    "mnx_expand_pack": _PASS + [_vp],
    "mnx_main_pack": _PASS + [_vp],                         # expand's arguments exactly
    "mnx_normalize_pack": _PASS + [_vp],                    # atom_notes in the place of origin
    "mnx_formula_pack": _PASS + [_u32, _vp],                # expand's arguments, max_steps in front of stream
    "mnx_kekulize_pack": _PASS + [_u32, _vp],               # normalize's arguments, max_steps in front of stream
    "mnx_fingerprint_pack": [_vp] + _TABLES_IN + [_vp, _vp, _u32, _u32, _vp],                        # recs, bits, max_bonds, max_steps
    "mnx_substructure_match": [_vp] + _TABLES_IN + _TABLES_IN + [_vp, _i32, _vp, _vp, _u32, _u32, _vp],   # both sides, pairs, n_pairs, recs, maps, max_matches, max_steps
    "mnx_tanimoto": [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    # queries, nq, library, nl, k, min_similarity, flags, the five outputs, work, work_bytes
    "mnx_tanimoto_search": [_vp, _vp, _i32, _vp, _u32, _u32, C.c_double, _u32] + [_vp] * 6 + [C.c_size_t, _vp],
    "mnx_smiles_read": [_vp] + _BYTES_IN + [_vp, _vp] + _ARENAS + [_vp, _vp],                        # mols, recs, the arenas, totals
    "mnx_molfile_read": [_vp] + _BYTES_IN + [_vp, _i32, _vp, _vp] + _ARENAS + [_vp, _vp],            # scale, fit in front of them
    # engine_lab.hip: the test and measurement aids
    "mnx_edge_probs": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "mnx_gemm16": [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "mnx_gemm16_split": [_vp, _i32, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp],
    "mnx_window_attn": [_vp, _vp, _i64, _vp, _vp, _i64] + [_i32] * 7 + [_vp],
    "mnx_kv_block": [_vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "mnx_beam_scripted": [_vp, _vp] + [_i32] * 6 + [_vp, _vp, _vp, C.POINTER(_i32)] + [_vp] * 6,
    "mnx_decode_beam_forced": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    "mnx_patch_embed": [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "mnx_layernorm16": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _f32, _i32, _vp, _vp],
    "mnx_merge_ln16": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f32, _i32, _vp],
    "mnx_cast16": [_vp, _vp, _vp, _i64, _i64, _f32, _vp],
    "mnx_sgemm_tn": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "mnx_dec_linear": [_vp, _i32, _i32] + [_vp] * 6 + [_i32, _i32, _vp, _vp] + [_i32] * 4 + [_vp, _vp],
    "mnx_profile_enable": [_vp, _i32],
    "mnx_profile_read": [_vp, _i32, _f64p, _f64p, C.POINTER(_i64)],
    "mnx_probe_decode_attn": [_vp, _i32, _i32, _i32, _f64p, _f64p, _vp],
    "mnx_gemm_clock": [_vp, _i32, _f64p],
    "mnx_probe_mfma": [_vp, _i32, _f64p, _f64p, _vp],
}
PROTOTYPES = {"mnx_abi_version": (C.c_int, []), "mnx_destroy": (None, [_vp]), "mnx_last_error": (C.c_char_p, [_vp]),
              "mnx_workspace_bytes": (C.c_size_t, [_vp]), "mnx_tanimoto_search_work_bytes": (C.c_size_t, [_i32, _u32, _u32]), **{name: (C.c_int, args) for name, args in _STATUS_CALLS.items()}}
SYMBOLS = tuple(PROTOTYPES)


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """Loads libmolnextr_hip.so and declares the prototype of every symbol of include/molnextr_hip.h (PROTOTYPES)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C molnextr_amd/csrc`). molnextr_amd has no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.mnx_abi_version() != ABI_VERSION:
        raise ImportError(f"libmolnextr_hip.so ABI {lib.mnx_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
