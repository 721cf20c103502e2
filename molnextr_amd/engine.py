"""ctypes binding of libmolnextr_hip.so (include/molnextr_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the HIP stream; every tensor crosses the C ABI as a raw
device pointer. There is NO CPU fallback: if the library is missing or no MI355X is present, construction
raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import weights as W

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmolnextr_hip.so")
_lib = None

ABI_VERSION = 7
SYMBOLS = ("mnx_abi_version", "mnx_create", "mnx_destroy", "mnx_last_error", "mnx_workspace_bytes", "mnx_encode",
           "mnx_set_encoder_tap", "mnx_decode_greedy", "mnx_edges", "mnx_gemm16", "mnx_profile_enable",
           "mnx_profile_read", "mnx_set_token_classes", "mnx_predict", "mnx_atom_scan", "mnx_decode_beam", "mnx_preprocess",
           "mnx_probe_decode_attn", "mnx_predict_beam", "mnx_set_split_terms", "mnx_encoder_status",
           "mnx_gemm16_split", "mnx_decode_forced", "mnx_gemm_clock", "mnx_probe_mfma", "mnx_set_op_terms",
           "mnx_predict_confidence", "mnx_confidence", "mnx_window_attn", "mnx_kv_block", "mnx_preprocess_batch",
           "mnx_encode_gray8", "mnx_predict_gray8", "mnx_decode_guided", "mnx_predict_guided", "mnx_patch_embed",
           "mnx_layernorm16", "mnx_merge_ln16", "mnx_cast16", "mnx_sgemm_tn", "mnx_set_vocab_text", "mnx_graph_pack",
           "mnx_set_symbol_tables", "mnx_molfile_pack", "mnx_smiles_pack", "mnx_smiles_pack_stereo",
           "mnx_smiles_pack_marks", "mnx_smiles_pack_canonical", "mnx_smiles_pack_symmetric", "mnx_set_fragments", "mnx_expand_pack", "mnx_smiles_read",
           "mnx_beam_scripted", "mnx_edge_probs", "mnx_normalize_pack", "mnx_kekulize_pack", "mnx_formula_pack",
           "mnx_decode_beam_forced", "mnx_main_pack", "mnx_fingerprint_pack", "mnx_tanimoto", "mnx_molfile_read",
           "mnx_substructure_match")

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


def vocab_text(tok):
    """mnx_set_vocab_text arguments of a tokenizer: (bytes, uint32 offsets [n + 1], n) — the UTF-8 names of ids 0 .. n - 1."""
    names = [tok.itos[i].encode("utf-8") for i in range(tok.offset)]
    offsets = np.zeros(len(names) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(b) for b in names])
    return b"".join(names), offsets, len(names)


def symbol_tables():
    """mnx_set_symbol_tables arguments from vocab/abbreviations.json (chem.RGROUP_SYMBOLS / ABBREVIATIONS): (bytes, uint32
    offsets [n + 1], uint8 kinds [n], n) — the UTF-8 names sorted bytewise, kind 1 R-group, 2 abbreviation. A name in both
    tables is an R-group: the reference tests that table first (chemical.py:888-895)."""
    from .chem import ABBREVIATIONS, RGROUP_SYMBOLS
    kind = {s.encode("utf-8"): 2 for s in ABBREVIATIONS}
    kind.update({s.encode("utf-8"): 1 for s in RGROUP_SYMBOLS})
    names = sorted(kind)
    long = [b for b in names if not 1 <= len(b) <= 16]
    if long or len(names) > 512:
        raise ValueError(f"symbol tables: {len(names)} names (at most 512), outside 1..16 bytes: {long}")
    offsets = np.zeros(len(names) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(b) for b in names])
    return b"".join(names), offsets, np.array([kind[b] for b in names], dtype=np.uint8), len(names)


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


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """Loads libmolnextr_hip.so and declares the prototypes of every symbol of include/molnextr_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C molnextr_amd/csrc`). molnextr_amd has no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.mnx_abi_version.restype = C.c_int
    lib.mnx_create.restype = C.c_int
    lib.mnx_create.argtypes = [C.POINTER(MnxConfig), C.POINTER(MnxWeightDesc), i32, i32, C.POINTER(vp)]
    lib.mnx_destroy.restype = None
    lib.mnx_destroy.argtypes = [vp]
    lib.mnx_last_error.restype = C.c_char_p
    lib.mnx_last_error.argtypes = [vp]
    lib.mnx_workspace_bytes.restype = C.c_size_t
    lib.mnx_workspace_bytes.argtypes = [vp]
    lib.mnx_encode.restype = C.c_int
    lib.mnx_encode.argtypes = [vp, vp, i32, vp, vp]
    lib.mnx_set_encoder_tap.restype = C.c_int
    lib.mnx_set_encoder_tap.argtypes = [vp, i32, vp]
    lib.mnx_set_split_terms.restype = C.c_int
    lib.mnx_set_split_terms.argtypes = [vp, i32]
    lib.mnx_set_op_terms.restype = C.c_int
    lib.mnx_set_op_terms.argtypes = [vp, i32, i32, i32, i32]
    lib.mnx_encoder_status.restype = C.c_int
    lib.mnx_encoder_status.argtypes = [vp, C.POINTER(i32), vp]
    lib.mnx_decode_greedy.restype = C.c_int
    lib.mnx_decode_greedy.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mnx_decode_forced.restype = C.c_int
    lib.mnx_decode_forced.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mnx_edges.restype = C.c_int
    lib.mnx_edges.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.mnx_gemm16.restype = C.c_int
    lib.mnx_gemm16.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mnx_gemm16_split.restype = C.c_int
    lib.mnx_gemm16_split.argtypes = [vp, i32, vp, C.c_int64, vp, C.c_int64, C.c_float, vp, C.c_int64, vp, i32, i32, i32, i32, vp]
    lib.mnx_window_attn.restype = C.c_int
    lib.mnx_window_attn.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.mnx_edge_probs.restype = C.c_int
    lib.mnx_edge_probs.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.mnx_kv_block.restype = C.c_int
    lib.mnx_kv_block.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.mnx_beam_scripted.restype = C.c_int
    lib.mnx_beam_scripted.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_int32), vp, vp, vp, vp,
                                      vp, vp]
    lib.mnx_decode_beam_forced.restype = C.c_int
    lib.mnx_decode_beam_forced.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.mnx_patch_embed.restype = C.c_int
    lib.mnx_patch_embed.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mnx_layernorm16.restype = C.c_int
    lib.mnx_layernorm16.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp, i32, i32, C.c_float, i32, vp, vp]
    lib.mnx_merge_ln16.restype = C.c_int
    lib.mnx_merge_ln16.argtypes = [vp, vp, vp, vp, vp, C.c_int64, i32, i32, i32, i32, C.c_float, i32, vp]
    lib.mnx_cast16.restype = C.c_int
    lib.mnx_cast16.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_float, vp]
    lib.mnx_sgemm_tn.restype = C.c_int
    lib.mnx_sgemm_tn.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.mnx_profile_enable.restype = C.c_int
    lib.mnx_profile_enable.argtypes = [vp, i32]
    lib.mnx_profile_read.restype = C.c_int
    lib.mnx_profile_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.mnx_probe_decode_attn.restype = C.c_int
    lib.mnx_probe_decode_attn.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.mnx_gemm_clock.restype = C.c_int
    lib.mnx_gemm_clock.argtypes = [vp, i32, C.POINTER(C.c_double)]
    lib.mnx_probe_mfma.restype = C.c_int
    lib.mnx_probe_mfma.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.mnx_set_token_classes.restype = C.c_int
    lib.mnx_set_token_classes.argtypes = [vp, C.c_char_p, i32, i32, i32, i32, i32, i32, i32]
    lib.mnx_set_vocab_text.restype = C.c_int
    lib.mnx_set_vocab_text.argtypes = [vp, C.c_char_p, vp, i32]
    lib.mnx_graph_pack.restype = C.c_int
    lib.mnx_graph_pack.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp,
                                   C.c_uint32, vp, vp]
    lib.mnx_set_symbol_tables.restype = C.c_int
    lib.mnx_set_symbol_tables.argtypes = [vp, C.c_char_p, vp, vp, i32]
    lib.mnx_molfile_pack.restype = C.c_int
    lib.mnx_molfile_pack.argtypes = [vp, vp, i32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp]
    lib.mnx_smiles_pack.restype = C.c_int
    lib.mnx_smiles_pack.argtypes = [vp, vp, i32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp]
    lib.mnx_smiles_pack_stereo.restype = C.c_int
    lib.mnx_smiles_pack_stereo.argtypes = list(lib.mnx_smiles_pack.argtypes)
    lib.mnx_smiles_pack_marks.restype = C.c_int
    lib.mnx_smiles_pack_marks.argtypes = lib.mnx_smiles_pack.argtypes[:-1] + [C.c_uint32, vp]
    lib.mnx_smiles_pack_canonical.restype = C.c_int
    lib.mnx_smiles_pack_canonical.argtypes = lib.mnx_smiles_pack.argtypes[:11] + [vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp]
    lib.mnx_smiles_pack_symmetric.restype = C.c_int
    lib.mnx_smiles_pack_symmetric.argtypes = lib.mnx_smiles_pack.argtypes[:11] + [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp]
    lib.mnx_set_fragments.restype = C.c_int
    lib.mnx_set_fragments.argtypes = [vp, vp, i32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, i32]
    lib.mnx_expand_pack.restype = C.c_int
    lib.mnx_expand_pack.argtypes = [vp, vp, i32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32,
                                    vp, C.c_uint32, vp, vp, vp]
    lib.mnx_normalize_pack.restype = C.c_int
    lib.mnx_normalize_pack.argtypes = lib.mnx_expand_pack.argtypes      # atom_notes in the place of origin
    lib.mnx_kekulize_pack.restype = C.c_int                             # normalize's arguments, max_steps in front of stream
    lib.mnx_kekulize_pack.argtypes = lib.mnx_expand_pack.argtypes[:-1] + [C.c_uint32, lib.mnx_expand_pack.argtypes[-1]]
    lib.mnx_formula_pack.restype = C.c_int                              # expand's arguments, max_steps in front of stream
    lib.mnx_formula_pack.argtypes = lib.mnx_kekulize_pack.argtypes
    lib.mnx_main_pack.restype = C.c_int
    lib.mnx_main_pack.argtypes = lib.mnx_expand_pack.argtypes           # expand's arguments exactly
    lib.mnx_fingerprint_pack.restype = C.c_int                          # the writers' input side, recs, bits, max_bonds, max_steps
    lib.mnx_fingerprint_pack.argtypes = lib.mnx_smiles_pack.argtypes[:9] + [vp, vp, C.c_uint32, C.c_uint32, vp]
    lib.mnx_substructure_match.restype = C.c_int                        # the input side twice, pairs, n_pairs, recs, maps, max_matches, max_steps
    lib.mnx_substructure_match.argtypes = (lib.mnx_smiles_pack.argtypes[:9] + lib.mnx_smiles_pack.argtypes[1:9] +
                                           [vp, i32, vp, vp, C.c_uint32, C.c_uint32, vp])
    lib.mnx_tanimoto.restype = C.c_int
    lib.mnx_tanimoto.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.mnx_smiles_read.restype = C.c_int
    lib.mnx_smiles_read.argtypes = [vp, vp, C.c_uint32, vp, i32, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    lib.mnx_molfile_read.restype = C.c_int
    lib.mnx_molfile_read.argtypes = [vp, vp, C.c_uint32, vp, i32, vp, i32, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    lib.mnx_atom_scan.restype = C.c_int
    lib.mnx_atom_scan.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.mnx_preprocess.restype = C.c_int
    lib.mnx_preprocess.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.mnx_preprocess_batch.restype = C.c_int
    lib.mnx_preprocess_batch.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mnx_encode_gray8.restype = C.c_int
    lib.mnx_encode_gray8.argtypes = [vp, vp, i32, vp, vp]
    lib.mnx_predict_gray8.restype = C.c_int
    lib.mnx_predict_gray8.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.mnx_decode_guided.restype = C.c_int
    lib.mnx_decode_guided.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mnx_predict_guided.restype = C.c_int
    lib.mnx_predict_guided.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.mnx_decode_beam.restype = C.c_int
    lib.mnx_decode_beam.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.mnx_predict.restype = C.c_int
    lib.mnx_predict.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.mnx_predict_confidence.restype = C.c_int
    lib.mnx_predict_confidence.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.mnx_confidence.restype = C.c_int
    lib.mnx_confidence.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.mnx_predict_beam.restype = C.c_int
    lib.mnx_predict_beam.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    if lib.mnx_abi_version() != ABI_VERSION:
        raise ImportError(f"libmolnextr_hip.so ABI {lib.mnx_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check_labels(labels, n: int, free_run=False) -> torch.Tensor:
    """Labels of guided decoding as a contiguous int32 [n, L] tensor (on the device it came from): L >= 2, and an '<eos>'
    (id 2) in every row that free_run does not exempt. A row without one would decode past its label, which the reference
    answers with IndexError and the library with free-running (include/molnextr_hip.h); asking for that takes free_run:
    True for every row, or one bool per row (the rows of a job that were cut at max_len, say)."""
    lab = torch.as_tensor(labels)
    if lab.dim() != 2 or lab.shape[0] != n or lab.shape[1] < 2:
        raise ValueError(f"labels must be [n = {n}, L >= 2], got {tuple(lab.shape)}")
    lab = lab.to(dtype=torch.int32).contiguous()
    exempt = torch.as_tensor(free_run, dtype=torch.bool).reshape(-1)
    if exempt.numel() not in (1, n):
        raise ValueError(f"free_run must be a bool or {n} bools (one per label row), got {exempt.numel()}")
    bad = (~(lab == 2).any(dim=1).cpu() & ~exempt.expand(n)).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"label rows {bad[:8]} hold no '<eos>' (free_run exempts rows that are meant to run on freely)")
    return lab


def check_beam_script(parent, token, n_best: int, vocab: int, eos: int = 2):
    """The script of Engine.decode_beam_forced as two contiguous host int32 [max_len, B, beam] tensors. ValueError for a
    shape or an element out of range and for what no top-K could have chosen (include/molnextr_hip.h): '<eos>' at step 0, a
    hypothesis that has finished as a parent, the same (parent, token) twice for one image at one step. Images are followed
    as the search will run them (an image leaves once its top hypothesis has finished at some step and n_best are stored);
    entries of an image that has left are only range-checked."""
    par = torch.as_tensor(parent).cpu()
    tok = torch.as_tensor(token).cpu()
    if par.dim() != 3 or par.shape != tok.shape or par.is_floating_point() or tok.is_floating_point():
        raise ValueError(f"script parent / token must be int [max_len, B, beam], got {tuple(par.shape)} and {tuple(tok.shape)}")
    max_len, B, K = par.shape
    if not 1 <= n_best <= K:
        raise ValueError(f"n_best must be 1..beam = {K}, got {n_best}")
    for name, a, hi in (("parent", par, K), ("token", tok, vocab)):
        bad = ((a < 0) | (a >= hi)).nonzero()
        if len(bad):
            raise ValueError(f"script {name}{bad[0].tolist()} = {int(a[tuple(bad[0])])} is outside 0..{hi - 1}")
    p, v = par.tolist(), tok.tolist()
    for b in range(B):
        finished, top, stored = [False] * K, False, 0
        for t in range(max_len):
            if t == 0 and eos in v[t][b]:
                raise ValueError(f"script: image {b} emits '<eos>' at step 0, where the head bans it")
            if any(finished[j] for j in p[t][b]):
                raise ValueError(f"script: step {t} image {b} descends from a finished hypothesis")
            if len(set(zip(p[t][b], v[t][b]))) < K:
                raise ValueError(f"script: step {t} image {b} makes the same (parent, token) choice twice")
            finished = [x == eos or t + 1 == max_len for x in v[t][b]]
            top, stored = top or finished[0], stored + sum(finished)
            if top and stored >= n_best:
                break
    return par.to(torch.int32).contiguous(), tok.to(torch.int32).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Engine:
    """One engine per GPU. Holds the packed weights and all workspace for `max_batch` images."""

    ROWS_PER_DECODE = 32      # rows per call of decode_greedy / decode_forced / decode_beam, and per reference batch of beam search
    MAX_REF_BATCH = 512       # rows per reference batch of greedy `predict` (include/molnextr_hip.h mnx_predict)

    def __init__(self, encoder_state: Dict[str, torch.Tensor], decoder_state: Dict[str, torch.Tensor],
                 device: int = 0, max_batch: int = 32, enc: W.EncoderDims = W.SWIN_B, dec: W.DecoderDims = W.DEC,
                 dtype: str = DEFAULT_DTYPE, max_len: int = 480, max_atoms: int = 160, dec_slots: int = 2048,
                 image_format: str = "fp32"):
        """image_format: what `preprocess` returns — "fp32" [n,3,S,S] normalised (the per-image mnx_preprocess path) or
        "gray8" [n,S,S] gray bytes (preprocess_batch: one mnx_preprocess_batch per PREP_MAX_PAGES pages, a twelfth of the
        bytes). `encode` / `predict` take either and give bit-identical results; the choice is this object's, the library
        handle has no format state."""
        if image_format not in IMAGE_FORMATS:
            raise ValueError(f"image_format must be one of {sorted(IMAGE_FORMATS)}, got {image_format!r}")
        self.image_format = image_format
        self._stage = None            # pinned staging of preprocess_batch: kept, grown geometrically
        self._stage_free = None       # event: the last H2D copy out of _stage has completed
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise MnxError("no HIP device visible: molnextr_amd needs an MI355X (gfx950); there is no CPU fallback")
        encoder_state = W.strip_module_prefix(encoder_state)
        decoder_state = W.strip_module_prefix(decoder_state)
        W.validate_state(encoder_state, W.encoder_spec(enc), "encoder")
        W.validate_state(decoder_state, W.decoder_spec(dec), "decoder")
        ref_idx = W.relative_position_index(enc.window)
        for k, v in encoder_state.items():
            if k.endswith("relative_position_index") and not torch.equal(v.cpu().long(), ref_idx):
                raise ValueError(f"{k} differs from the (dy+11)*23+(dx+11) formula the kernels implement")
        self.enc, self.dec, self.device = enc, dec, device
        self.max_batch, self.max_len, self.max_atoms = max_batch, max_len, max_atoms
        self.dec_slots = dec_slots or 2048
        cfg = MnxConfig()
        cfg.img_size, cfg.patch, cfg.embed_dim, cfg.n_stages = enc.img_size, enc.patch, enc.embed_dim, len(enc.depths)
        for i, (d, h) in enumerate(zip(enc.depths, enc.heads)):
            cfg.depths[i], cfg.heads[i] = d, h
        cfg.window = enc.window
        cfg.dec_layers, cfg.dec_dim, cfg.dec_heads, cfg.dec_ff = dec.layers, dec.d_model, dec.heads, dec.d_ff
        cfg.vocab, cfg.sym_offset, cfg.coord_bins, cfg.pe_len = dec.vocab, dec.vocab - 128, 64, dec.pe_len
        cfg.max_len, cfg.max_batch, cfg.max_atoms = max_len, max_batch, max_atoms
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
        cfg.compute_dtype = DTYPES[dtype]
        cfg.dec_slots = dec_slots
        self.dtype = dtype
        keep, descs = [], []
        for state in (encoder_state, decoder_state):
            for k, v in state.items():
                if not v.dtype.is_floating_point:
                    continue
                a = np.ascontiguousarray(v.detach().cpu().float().numpy())
                keep.append(a)
                d = MnxWeightDesc()
                d.name = k.encode()
                d.data = a.ctypes.data
                d.ndim = a.ndim
                for i, s in enumerate(a.shape):
                    d.shape[i] = s
                descs.append(d)
        arr = (MnxWeightDesc * len(descs))(*descs)
        handle = C.c_void_p()
        rc = self.lib.mnx_create(C.byref(cfg), arr, len(descs), device, C.byref(handle))
        if rc != 0:
            raise MnxError(f"mnx_create failed ({rc}): {self.lib.mnx_last_error(None).decode()}")
        self.h = handle
        self._set_token_classes()
        self._set_vocab_text()
        self._set_symbol_tables()
        self._set_fragments()
        self.n_feat = enc.num_features
        g = enc.img_size // enc.patch >> (len(enc.depths) - 1)
        self.n_mem = g * g

    @staticmethod
    def token_class_flags(tok) -> bytes:
        """mnx_set_token_classes flags of every symbol id of `tok`: bit0 is_symbol, bit1 is_atom, bits 2-4 the length of a
        symbol's name in characters - 1 (the span of an atom's confidence: '<unk>' is one id of five characters)."""
        def flag(i):
            if not tok.is_symbol(i):
                return 0
            return 1 | (2 if tok.is_atom(i) else 0) | (min(len(tok.itos[i]), 8) - 1) << 2
        return bytes(flag(i) for i in range(tok.offset))

    def _set_token_classes(self):
        """Hands the vocabulary's token classes to the on-device atom-position scan and confidences (mnx_predict)."""
        from .tokenizer import CharTokenizer
        tok = CharTokenizer(64)
        n = tok.offset
        flags = self.token_class_flags(tok)
        ids = [tok.stoi[c] for c in "[]ClBr"]
        self._check(self.lib.mnx_set_token_classes(self.h, flags, n, *ids), "mnx_set_token_classes")

    def _set_vocab_text(self):
        """Hands the names of the vocabulary's symbol ids to the library: what graph_pack spells the SMILES with."""
        from .tokenizer import CharTokenizer
        text, offsets, n = vocab_text(CharTokenizer(64))
        self._check(self.lib.mnx_set_vocab_text(self.h, text, offsets.ctypes.data, n), "mnx_set_vocab_text")

    def _set_symbol_tables(self):
        """Hands the R-group and abbreviation names to the library: what molfile_pack tests an atom's symbol against."""
        text, offsets, kinds, n = symbol_tables()
        self._check(self.lib.mnx_set_symbol_tables(self.h, text, offsets.ctypes.data, kinds.ctypes.data, n),
                    "mnx_set_symbol_tables")
        self._have_symbol_tables = True

    _have_symbol_tables = False

    def _set_fragments(self):
        """Hands the fragment library (vocab/fragments.json) to the library: what expand_pack replaces a label by. The table is
        parallel to the names of _set_symbol_tables: a handle that was given no names takes no fragments."""
        if not self._have_symbol_tables:
            return
        from .fragments import fragment_tables
        self.set_fragments(*fragment_tables())

    def set_fragments(self, mols, atoms, bonds, text, frag_of_name):
        """mnx_set_fragments: packed tables of fragments (one MOL_DTYPE record each) and the int32 table parallel to the names of
        symbol_tables(). Construction sets fragments.fragment_tables(); a caller with a library of its own replaces it here."""
        mols, atoms, bonds = (np.ascontiguousarray(a) for a in (mols, atoms, bonds))
        fo = np.ascontiguousarray(frag_of_name, dtype=np.int32)
        text = bytes(text)
        self._check(self.lib.mnx_set_fragments(self.h, mols.ctypes.data if len(mols) else None, len(mols),
                                               atoms.ctypes.data if len(atoms) else None, len(atoms),
                                               bonds.ctypes.data if len(bonds) else None, len(bonds), text if text else None,
                                               len(text), fo.ctypes.data if len(fo) else None, len(fo)), "mnx_set_fragments")

    def close(self):
        if getattr(self, "h", None):
            self.lib.mnx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise MnxError(f"{what} failed ({rc}): {self.lib.mnx_last_error(self.h).decode()}", code=int(rc))

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.mnx_workspace_bytes(self.h))

    # -- Encoder.forward -------------------------------------------------------------------------
    def _is_gray(self, images: torch.Tensor) -> bool:
        """Which of the two image forms `images` is: uint8 [n,S,S] gray bytes (True) or fp32 [n,3,S,S] normalised (False)."""
        S = self.enc.img_size
        assert images.is_cuda and images.is_contiguous()
        if images.dtype == torch.uint8:
            assert tuple(images.shape[1:]) == (S, S), images.shape
            return True
        assert images.dtype == torch.float32 and tuple(images.shape[1:]) == (3, S, S), (images.dtype, images.shape)
        return False

    def encode(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [B,3,S,S] normalised images (mnx_encode) or uint8 [B,S,S] gray bytes (mnx_encode_gray8) -> features."""
        gray = self._is_gray(images)
        B = images.shape[0]
        if out is None:
            out = torch.empty(B, self.n_mem, self.n_feat, device=images.device, dtype=torch.float32)
        if gray:
            self._check(self.lib.mnx_encode_gray8(self.h, _ptr(images), B, _ptr(out), _stream()), "mnx_encode_gray8")
        else:
            self._check(self.lib.mnx_encode(self.h, _ptr(images), B, _ptr(out), _stream()), "mnx_encode")
        return out

    def set_tap(self, item: int, dst: Optional[torch.Tensor]):
        self._check(self.lib.mnx_set_encoder_tap(self.h, item, _ptr(dst)), "mnx_set_encoder_tap")

    def set_split_terms(self, three_term_classes=None):
        """Split modes only (test aid): the op classes (names of SPLIT_CLASSES) evaluated with their full term count (three,
        or two for the classes of set_op_terms); the others run hi.hi alone, as the plain 16-bit mode would. None = all
        classes (the default)."""
        mask = 63 if three_term_classes is None else sum(SPLIT_CLASSES[c] for c in three_term_classes)
        self._check(self.lib.mnx_set_split_terms(self.h, mask), "mnx_set_split_terms")

    def set_op_terms(self, two_term=None, blocks=None):
        """fp16x3 / fp16x3m engines: the Linear op classes that run on TWO product terms (ah.wh + ah.wl), as tags "cls" (every
        stage) or "cls.sN" (encoder stage N, 0-based) with cls a name of SPLIT_CLASSES other than 'attn' — the syntax of
        tools/study_split_terms.py --two. blocks: {stage: (first_block, last_block)} restricts a stage's table to those Swin
        blocks (default: all of them). None = the mode's own table as the engine was created with it (fp16x3: none, fp16x3m:
        the header's, on the encoder's last stages); blocks must then be None."""
        if two_term is None:
            assert blocks is None, "blocks go with an explicit table"
            self._check(self.lib.mnx_set_op_terms(self.h, -1, -1, 0, 0), "mnx_set_op_terms")
            return
        for i, m in enumerate(two_term_masks(two_term, len(self.enc.depths))):
            lo, hi = (blocks or {}).get(i, (0, 1 << 30))
            self._check(self.lib.mnx_set_op_terms(self.h, i, m, lo, hi), "mnx_set_op_terms")

    def encoder_nonfinite(self) -> bool:
        """Synchronises and reports (then clears) whether an encode since the last call produced non-finite features
        (fp16 operand range exceeded)."""
        flag = C.c_int32(0)
        self._check(self.lib.mnx_encoder_status(self.h, C.byref(flag), _stream()), "mnx_encoder_status")
        return bool(flag.value)

    # -- TransformerDecoderAR.decode (greedy) ----------------------------------------------------
    def decode_greedy(self, features: torch.Tensor, chunk_id: Optional[torch.Tensor] = None,
                      max_len: Optional[int] = None, stop_on_eos: bool = True, want_hidden: bool = True,
                      want_logp: bool = True, trace_logits: bool = False) -> dict:
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B = features.shape[0]
        max_len = self.max_len if max_len is None else max_len
        dev = features.device
        tokens = torch.empty(B, max_len, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, dtype=torch.int32, device=dev)
        logp = torch.empty(B, max_len, dtype=torch.float32, device=dev) if want_logp else None
        hidden = torch.empty(B, max_len, self.dec.d_model, dtype=torch.float32, device=dev) if want_hidden else None
        trace = torch.empty(max_len, B, self.dec.vocab, dtype=torch.float32, device=dev) if trace_logits else None
        if chunk_id is not None:
            chunk_id = chunk_id.to(device=dev, dtype=torch.int32).contiguous()
        rc = self.lib.mnx_decode_greedy(self.h, _ptr(features), B, _ptr(chunk_id), max_len, int(stop_on_eos),
                                        _ptr(tokens), _ptr(lengths), _ptr(logp), _ptr(hidden), _ptr(trace),
                                        _stream())
        self._check(rc, "mnx_decode_greedy")
        return {"tokens": tokens, "lengths": lengths, "token_logp": logp, "hidden": hidden, "logits": trace}

    def decode_guided(self, features: torch.Tensor, labels, chunk_id: Optional[torch.Tensor] = None,
                      max_len: Optional[int] = None, want_hidden: bool = True, want_logp: bool = True,
                      trace_logits: bool = False, free_run=False) -> dict:
        """Label-guided greedy decode of up to ROWS_PER_DECODE rows (mnx_decode_guided; the reference's
        TransformerDecoderAR.decode(labels=...)): labels [B,L] int, '<sos>' first, forced ids, '<mask>' (4) where the model
        fills in, '<eos>', '<pad>'. Returns decode_greedy's dict: 'tokens' are the merged ids, 'token_logp' the own picks'.
        A row without '<eos>' raises ValueError unless free_run exempts it (check_labels: a bool, or one per row)."""
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B = features.shape[0]
        max_len = self.max_len if max_len is None else max_len
        dev = features.device
        lab = check_labels(labels, B, free_run).to(dev)
        tokens = torch.empty(B, max_len, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, dtype=torch.int32, device=dev)
        logp = torch.empty(B, max_len, dtype=torch.float32, device=dev) if want_logp else None
        hidden = torch.empty(B, max_len, self.dec.d_model, dtype=torch.float32, device=dev) if want_hidden else None
        trace = torch.empty(max_len, B, self.dec.vocab, dtype=torch.float32, device=dev) if trace_logits else None
        if chunk_id is not None:
            chunk_id = chunk_id.to(device=dev, dtype=torch.int32).contiguous()
        rc = self.lib.mnx_decode_guided(self.h, _ptr(features), B, _ptr(chunk_id), max_len, _ptr(lab), lab.shape[1],
                                        _ptr(tokens), _ptr(lengths), _ptr(logp), _ptr(hidden), _ptr(trace), _stream())
        self._check(rc, "mnx_decode_guided")
        return {"tokens": tokens, "lengths": lengths, "token_logp": logp, "hidden": hidden, "logits": trace}

    def decode_forced(self, features: torch.Tensor, forced_ids: torch.Tensor, max_len: Optional[int] = None,
                      trace_logits: bool = False) -> dict:
        """Teacher-forced greedy decode (test aid, mnx_decode_forced): rows advance with forced_ids [B,max_len] (each
        ending with EOS or filling max_len). Returns the engine's own argmax at every step given that history
        ('argmax'), the masked log-prob of the forced id ('forced_logp'), 'lengths' and optionally 'logits'."""
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B = features.shape[0]
        max_len = self.max_len if max_len is None else max_len
        dev = features.device
        forced = forced_ids.to(device=dev, dtype=torch.int32).contiguous()
        assert tuple(forced.shape) == (B, max_len), forced.shape
        argmax = torch.zeros(B, max_len, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, dtype=torch.int32, device=dev)
        logp = torch.zeros(B, max_len, dtype=torch.float32, device=dev)
        trace = torch.empty(max_len, B, self.dec.vocab, dtype=torch.float32, device=dev) if trace_logits else None
        rc = self.lib.mnx_decode_forced(self.h, _ptr(features), B, None, max_len, _ptr(forced), _ptr(argmax), _ptr(lengths),
                                        _ptr(logp), _ptr(trace), _stream())
        self._check(rc, "mnx_decode_forced")
        return {"argmax": argmax, "lengths": lengths, "forced_logp": logp, "logits": trace}

    # -- CropWhite + Resize + ToGray + Normalize on device ---------------------------------------------
    def preprocess(self, images, pad: int = 50, pad_to_square: bool = False, return_crops: bool = False):
        """List of HWC uint8 RGB pages (numpy arrays or tensors, any sizes) -> [n,3,S,S] fp32 on the device.
        pad_to_square: PadToSquare after CropWhite (the reference's transform for real/acs.csv and real/UOB.csv).
        return_crops: also return the CropWhite parameters [n,4] (crop_top, crop_bottom, crop_left, crop_right).
        An engine built with image_format="gray8" forwards to preprocess_batch(out="gray8"): uint8 [n,S,S]."""
        if self.image_format == "gray8":
            return self.preprocess_batch(images, pad=pad, pad_to_square=pad_to_square, return_crops=return_crops, out="gray8")
        dev = torch.device("cuda", self.device)
        S = self.enc.img_size
        out = torch.empty(len(images), 3, S, S, dtype=torch.float32, device=dev)
        crops = torch.zeros(len(images), 4, dtype=torch.int32, device=dev) if return_crops else None
        keep = []
        for i, im in enumerate(images):
            if torch.is_tensor(im) and im.is_cuda:
                t = im if im.dim() == 3 else im[..., None].expand(-1, -1, 3)
                t = t[..., :3].to(dtype=torch.uint8).contiguous()
            else:
                a = np.asarray(im)
                if a.ndim == 2:
                    a = np.repeat(a[..., None], 3, axis=2)
                a = np.ascontiguousarray(a[..., :3], dtype=np.uint8)
                # page -> pinned staging -> device: the H2D copy is then truly asynchronous on this stream (a pageable
                # source makes it synchronous) and can overlap the engine working on another stream
                pin = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
                pin.numpy()[...] = a
                t = pin.to(dev, non_blocking=True)
                keep.append(pin)
            keep.append(t)
            self._check(self.lib.mnx_preprocess(self.h, _ptr(t), t.shape[0], t.shape[1], pad, int(pad_to_square),
                                                _ptr(crops[i]) if return_crops else None, _ptr(out[i]), _stream()),
                        "mnx_preprocess")
        torch.cuda.current_stream().synchronize()      # the uploaded pages must outlive the kernels
        return (out, crops) if return_crops else out

    def _staging(self, nbytes: int) -> torch.Tensor:
        """The pinned staging buffer of preprocess_batch with room for nbytes, free to be overwritten: ONE buffer per
        engine, grown geometrically; a refill waits for the event behind the previous copy out of it (not for the device)."""
        if self._stage_free is not None:
            self._stage_free.synchronize()
        if self._stage is None or self._stage.numel() < nbytes:
            self._stage = torch.empty(max(nbytes, 2 * (self._stage.numel() if self._stage is not None else 0), 1 << 20),
                                      dtype=torch.uint8, pin_memory=True)
        return self._stage

    def preprocess_batch(self, images, pad: int = 50, pad_to_square: bool = False, return_crops: bool = False,
                         out: str = "gray8"):
        """`preprocess` for the whole list at once (mnx_preprocess_batch): the pages are packed into one pinned staging
        buffer behind their table, ONE H2D copy carries both, pages that already live on the device are copied into the
        arena there, and every PREP_MAX_PAGES pages (or STAGE_MAX_BYTES of them) take one library call of three launches. out: "gray8" -> uint8 [n,S,S]
        (the input of encode / predict at a twelfth of the bytes), "fp32" -> [n,3,S,S] as `preprocess` writes it.
        One call at a time per engine (the staging buffer and the library's box scratch are the engine's)."""
        if out not in IMAGE_FORMATS:
            raise ValueError(f"out must be one of {sorted(IMAGE_FORMATS)}, got {out!r}")
        dev = torch.device("cuda", self.device)
        S, n = self.enc.img_size, len(images)
        res = (torch.empty(n, S, S, dtype=torch.uint8, device=dev) if out == "gray8"
               else torch.empty(n, 3, S, S, dtype=torch.float32, device=dev))
        crops = torch.zeros(n, 4, dtype=torch.int32, device=dev) if return_crops else None
        if n == 0:
            return (res, crops) if return_crops else res
        # a call's pages are cut into chunks of at most PREP_MAX_PAGES pages and STAGE_MAX_BYTES bytes (one page at least):
        # one staging fill, one H2D copy and one library call each
        sizes = []
        for i, im in enumerate(images):
            shp = im.shape if hasattr(im, "shape") else np.shape(im)
            h, w = int(shp[0]), int(shp[1])
            if h < 1 or w < 1 or h > 16384 or w > 16384:
                raise ValueError(f"page {i}: {h} x {w} is outside 1..16384")
            sizes.append((3 * h * w + 15) & ~15)
        keep, p0 = [], 0
        while p0 < n:
            p1, nbytes = p0 + 1, sizes[p0]
            while p1 < n and p1 - p0 < PREP_MAX_PAGES and nbytes + sizes[p1] <= self.STAGE_MAX_BYTES:
                nbytes += sizes[p1]
                p1 += 1
            keep.append(self._preprocess_chunk(images[p0:p1], pad, pad_to_square, crops[p0:p1] if return_crops else None,
                                               res[p0:p1], IMAGE_FORMATS[out]))
            p0 = p1
        torch.cuda.current_stream().synchronize()      # the arenas (`keep`) must outlive the kernels
        return (res, crops) if return_crops else res

    STAGE_MAX_BYTES = 1 << 30     # pinned staging (and device arena) per mnx_preprocess_batch call of preprocess_batch

    def _preprocess_chunk(self, images, pad, pad_to_square, crops, res, fmt):
        """One mnx_preprocess_batch call of preprocess_batch; returns the device buffer the enqueued kernels read."""
        dev, n = res.device, len(images)
        # layout: [page table: n x 16 bytes][pages, each at a multiple of 16]; host pages are written into the staging
        # buffer, device pages only reserve their place in the arena
        pages, host, on_dev, off = (MnxPage * n)(), [], [], 0
        for i, im in enumerate(images):
            if torch.is_tensor(im) and im.is_cuda:
                t = im if im.dim() == 3 else im[..., None].expand(-1, -1, 3)
                t = t[..., :3].to(dtype=torch.uint8).contiguous()
                on_dev.append((i, t))
                h, w = t.shape[0], t.shape[1]
            else:
                a = np.asarray(im)
                if a.ndim == 2:
                    a = a[..., None]
                host.append((i, a))
                h, w = a.shape[0], a.shape[1]
            pages[i].offset, pages[i].height, pages[i].width = off, h, w
            off += (3 * h * w + 15) & ~15
        table = 16 * n
        # everything up to the end of the last host page crosses the bus: the table alone when every page is on the device
        end = table + max([pages[i].offset + 3 * pages[i].height * pages[i].width for i, _ in host], default=0)
        stage = self._staging(end)
        flat = stage.numpy()
        flat[:table] = np.frombuffer(pages, dtype=np.uint8)
        for i, a in host:
            h, w, o = pages[i].height, pages[i].width, table + pages[i].offset
            flat[o:o + 3 * h * w].reshape(h, w, 3)[...] = a[..., :3]      # one channel broadcasts to three
        # the device side is allocated per call (the caching allocator recycles it); the copy is asynchronous on this stream
        # and can overlap the engine working on another one
        buf = torch.empty(table + off, dtype=torch.uint8, device=dev)
        buf[:end].copy_(stage[:end], non_blocking=True)
        self._stage_free = torch.cuda.Event()
        self._stage_free.record()
        arena = buf[table:]
        for i, t in on_dev:
            o = pages[i].offset
            arena[o:o + t.numel()].copy_(t.reshape(-1), non_blocking=True)
        tallest = max(pages[i].height for i in range(n))
        rc = self.lib.mnx_preprocess_batch(self.h, _ptr(arena), _ptr(buf), n, tallest, pad, int(pad_to_square), _ptr(crops),
                                           _ptr(res), fmt, _stream())
        self._check(rc, "mnx_preprocess_batch")
        return buf

    # -- TransformerDecoderAR.decode, beam_size > 1 --------------------------------------------------
    def decode_beam(self, features: torch.Tensor, beam: int = 5, n_best: int = 1, max_len: Optional[int] = None,
                    want_hidden: bool = True) -> dict:
        """Beam search over one reference batch (<= 32 images). Returns tokens [B,n_best,max_len], lengths
        [B,n_best], scores [B,n_best] (average log-prob, hypotheses by descending score) and hidden
        [B,n_best,max_len,256]."""
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B = features.shape[0]
        max_len = self.max_len if max_len is None else max_len
        dev = features.device
        tokens = torch.zeros(B, n_best, max_len, dtype=torch.int32, device=dev)
        lengths = torch.zeros(B, n_best, dtype=torch.int32, device=dev)
        scores = torch.zeros(B, n_best, dtype=torch.float32, device=dev)
        hidden = torch.zeros(B, n_best, max_len, self.dec.d_model, dtype=torch.float32, device=dev) if want_hidden else None
        rc = self.lib.mnx_decode_beam(self.h, _ptr(features), B, beam, n_best, max_len, _ptr(tokens), _ptr(lengths),
                                      _ptr(scores), _ptr(hidden), _stream())
        self._check(rc, "mnx_decode_beam")
        return {"tokens": tokens, "lengths": lengths, "scores": scores, "hidden": hidden}

    def decode_beam_forced(self, features: torch.Tensor, parent, token, n_best: int = 1, want_hidden: bool = True,
                           trace_logits: bool = True, fill: float = float("nan")) -> dict:
        """Beam search whose choices are read from a script while the real decoder runs (test aid, mnx_decode_beam_forced):
        parent / token int [max_len, B, beam] — new hypothesis j of original image b at step t descends from hypothesis parent
        and emits id token (check_beam_script: what a script may not do raises ValueError). Returns decode_beam's dict and,
        with trace_logits, 'logits' [max_len, B*beam, V]: the raw logits of slot b * beam + j at step t, `fill` where the
        slot was not alive."""
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        par, tok = check_beam_script(parent, token, n_best, self.dec.vocab)
        max_len, B, beam = par.shape
        if features.shape[0] != B:
            raise ValueError(f"the script is for {B} images, features for {features.shape[0]}")
        dev = features.device
        tokens = torch.zeros(B, n_best, max_len, dtype=torch.int32, device=dev)
        lengths = torch.zeros(B, n_best, dtype=torch.int32, device=dev)
        scores = torch.zeros(B, n_best, dtype=torch.float32, device=dev)
        hidden = torch.zeros(B, n_best, max_len, self.dec.d_model, dtype=torch.float32, device=dev) if want_hidden else None
        trace = torch.full((max_len, B * beam, self.dec.vocab), fill, dtype=torch.float32, device=dev) if trace_logits else None
        rc = self.lib.mnx_decode_beam_forced(self.h, _ptr(features), B, beam, n_best, max_len, _ptr(par), _ptr(tok), par.numel(),
                                             _ptr(tokens), _ptr(lengths), _ptr(scores), _ptr(hidden), _ptr(trace), _stream())
        self._check(rc, "mnx_decode_beam_forced")
        return {"tokens": tokens, "lengths": lengths, "scores": scores, "hidden": hidden, "logits": trace}

    def beam_scripted(self, table: torch.Tensor, n_best: int = 1, eos: int = 2, trace: bool = True,
                      fill: int = -7) -> dict:
        """The beam-search strategy kernels on scripted log-probs (test aid, mnx_beam_scripted): table fp32
        [max_len, B, beam, V] on the device, row (t, b, j) = what hypothesis j of original image b sees at step t; the eos
        column of step 0 is banned, nothing else is applied. Returns tokens [B,n_best,max_len], lengths, scores as
        decode_beam does, 'steps_run', and with trace=True the per-step 'parent', 'token', 'score' [max_len,B,beam], 'alive'
        [max_len,B] and 'n_active' [max_len]: rows of images not alive at the start of a step keep `fill`."""
        assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 4
        max_len, B, beam, V = table.shape
        dev = table.device
        out = {"tokens": torch.zeros(B, n_best, max_len, dtype=torch.int32, device=dev),
               "lengths": torch.zeros(B, n_best, dtype=torch.int32, device=dev),
               "scores": torch.zeros(B, n_best, dtype=torch.float32, device=dev)}
        tr = {}
        if trace:
            tr = {"parent": torch.full((max_len, B, beam), fill, dtype=torch.int32, device=dev),
                  "token": torch.full((max_len, B, beam), fill, dtype=torch.int32, device=dev),
                  "score": torch.full((max_len, B, beam), float(fill), dtype=torch.float32, device=dev),
                  "alive": torch.full((max_len, B), fill, dtype=torch.int32, device=dev),
                  "n_active": torch.full((max_len,), fill, dtype=torch.int32, device=dev)}
        steps = C.c_int32(-1)
        rc = self.lib.mnx_beam_scripted(self.h, _ptr(table), B, beam, n_best, max_len, V, eos, _ptr(out["tokens"]),
                                        _ptr(out["lengths"]), _ptr(out["scores"]), C.byref(steps), _ptr(tr.get("parent")),
                                        _ptr(tr.get("token")), _ptr(tr.get("score")), _ptr(tr.get("alive")),
                                        _ptr(tr.get("n_active")), _stream())
        self._check(rc, "mnx_beam_scripted")
        out.update(tr)
        out["steps_run"] = steps.value
        return out

    # -- GraphPredictor + get_edge_prediction ----------------------------------------------------
    def edges(self, hidden: torch.Tensor, atom_idx: torch.Tensor, n_atoms: torch.Tensor, want_scores: bool = False):
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous()
        B, max_len, _ = hidden.shape
        atom_idx = atom_idx.to(device=hidden.device, dtype=torch.int32).contiguous()
        n_atoms = n_atoms.to(device=hidden.device, dtype=torch.int32).contiguous()
        kmax = atom_idx.shape[1]
        edges = torch.zeros(B, kmax, kmax, dtype=torch.uint8, device=hidden.device)
        scores = torch.zeros(B, kmax, kmax, dtype=torch.float64, device=hidden.device) if want_scores else None
        rc = self.lib.mnx_edges(self.h, _ptr(hidden), _ptr(atom_idx), _ptr(n_atoms), B, kmax, max_len, _ptr(edges),
                                _ptr(scores), _stream())
        self._check(rc, "mnx_edges")
        return edges, scores

    def edge_probs(self, hidden: torch.Tensor, atom_idx: torch.Tensor, n_atoms: torch.Tensor, want_scores: bool = True):
        """edges() plus the seven class probabilities of every pair as the pair kernel left them (test aid,
        mnx_edge_probs): -> edges, scores, probs fp32 [B,kmax,kmax,8]; slot 7 and pairs beyond n_atoms[b] are undefined."""
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous()
        B, max_len, _ = hidden.shape
        atom_idx = atom_idx.to(device=hidden.device, dtype=torch.int32).contiguous()
        n_atoms = n_atoms.to(device=hidden.device, dtype=torch.int32).contiguous()
        kmax = atom_idx.shape[1]
        edges = torch.zeros(B, kmax, kmax, dtype=torch.uint8, device=hidden.device)
        scores = torch.zeros(B, kmax, kmax, dtype=torch.float64, device=hidden.device) if want_scores else None
        probs = torch.zeros(B, kmax, kmax, 8, dtype=torch.float32, device=hidden.device)
        rc = self.lib.mnx_edge_probs(self.h, _ptr(hidden), _ptr(atom_idx), _ptr(n_atoms), B, kmax, max_len, _ptr(edges),
                                     _ptr(scores), _ptr(probs), _stream())
        self._check(rc, "mnx_edge_probs")
        return edges, scores, probs

    # -- whole path, continuous batching ----------------------------------------------------------
    @property
    def max_ref_batch(self) -> int:
        """The largest `ref_batch` greedy `predict` accepts on this engine: min(MAX_REF_BATCH, max_batch, dec_slots)."""
        return min(self.MAX_REF_BATCH, self.max_batch, self.dec_slots, self.dec.pe_len)

    def predict(self, images: torch.Tensor, ref_batch: int = 32, max_len: Optional[int] = None,
                stop_on_eos: bool = True, beam: int = 1, confidence: bool = False, labels=None,
                free_run=False) -> dict:
        """Encoder + decode + atom positions + bond head for all images: greedy with continuous batching (mnx_predict),
        or beam search reference batch by reference batch with the encoder running ahead (mnx_predict_beam; adds
        'scores', the average log-prob of the returned hypothesis). Images are decoded as consecutive reference batches of
        `ref_batch` rows, each numbered as one batch of the reference (its positional-encoding row quirk): greedy takes
        1 <= ref_batch <= max_ref_batch (up to MAX_REF_BATCH = 512 rows), beam search up to ROWS_PER_DECODE = 32; beyond
        that MnxError (MNX_ERR_CAPACITY) names the bound. confidence=True (greedy, stop_on_eos only):
        mnx_predict_confidence, which adds 'token_logp' [n,max_len] fp32, 'edge_scores' [n,kmax,kmax], 'atom_scores'
        [n,kmax] and 'overall_score' [n] fp64. images: fp32 [n,3,S,S] normalised, or uint8 [n,S,S] gray bytes
        (mnx_predict_gray8: greedy with stop_on_eos only; beam search stays on fp32 images) — the same results bit for bit.
        labels [n,L] (see decode_guided): label-guided decoding of every image along its row (mnx_predict_guided; greedy with
        stop_on_eos only, either image format, with or without confidences). A row without '<eos>' raises ValueError unless
        free_run exempts it (check_labels: a bool, or one per row); an exempt row runs on freely beyond its label."""
        gray = self._is_gray(images)
        if labels is not None:
            if beam > 1 or not stop_on_eos:
                raise ValueError("labels go with greedy decoding and stop_on_eos=True (beam search with labels is not built)")
            labels = check_labels(labels, images.shape[0], free_run).to(images.device)
        if gray and beam > 1:
            raise ValueError("beam search takes fp32 images: the library has no gray-byte beam entry point (mnx_predict_beam "
                             "reads [n,3,S,S] fp32); use preprocess_batch(out='fp32') or image_format='fp32'")
        if gray and not stop_on_eos:
            raise ValueError("gray-byte input runs the reference's decode (stop_on_eos=True); fixed-length decoding is a bench "
                             "aid of the fp32 entry point")
        n = images.shape[0]
        max_len = self.max_len if max_len is None else max_len
        dev, k = images.device, self.max_atoms
        tokens = torch.zeros(n, max_len, dtype=torch.int32, device=dev)
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        n_atoms = torch.empty(n, dtype=torch.int32, device=dev)
        atom_idx = torch.zeros(n, k, dtype=torch.int32, device=dev)
        edges = torch.zeros(n, k, k, dtype=torch.uint8, device=dev)
        if confidence:
            if beam > 1:
                raise NotImplementedError("beam search does not track token scores (neither does the reference's)")
            if not stop_on_eos:
                raise ValueError("confidences are computed for the reference's decode (stop_on_eos=True)")
            logp = torch.zeros(n, max_len, dtype=torch.float32, device=dev)
            edge_scores = torch.zeros(n, k, k, dtype=torch.float64, device=dev)
            atom_scores = torch.zeros(n, k, dtype=torch.float64, device=dev)
            overall = torch.zeros(n, dtype=torch.float64, device=dev)
            if labels is not None:
                fn = "mnx_predict_guided"
                rc = self.lib.mnx_predict_guided(self.h, _ptr(images), int(gray), n, ref_batch, max_len, _ptr(labels),
                                                 labels.shape[1], _ptr(tokens), _ptr(lengths), _ptr(n_atoms), _ptr(atom_idx),
                                                 _ptr(edges), k, _ptr(logp), _ptr(edge_scores), _ptr(atom_scores),
                                                 _ptr(overall), _stream())
            else:
                fn = "mnx_predict_gray8" if gray else "mnx_predict_confidence"
                rc = getattr(self.lib, fn)(self.h, _ptr(images), n, ref_batch, max_len, _ptr(tokens), _ptr(lengths),
                                           _ptr(n_atoms), _ptr(atom_idx), _ptr(edges), k, _ptr(logp), _ptr(edge_scores),
                                           _ptr(atom_scores), _ptr(overall), _stream())
            self._check(rc, fn)
            return {"tokens": tokens, "lengths": lengths, "n_atoms": n_atoms, "atom_idx": atom_idx, "edges": edges,
                    "token_logp": logp, "edge_scores": edge_scores, "atom_scores": atom_scores, "overall_score": overall}
        if beam > 1:
            scores = torch.zeros(n, dtype=torch.float32, device=dev)
            rc = self.lib.mnx_predict_beam(self.h, _ptr(images), n, ref_batch, beam, max_len, _ptr(tokens), _ptr(lengths),
                                           _ptr(scores), _ptr(n_atoms), _ptr(atom_idx), _ptr(edges), k, _stream())
            self._check(rc, "mnx_predict_beam")
            return {"tokens": tokens, "lengths": lengths, "n_atoms": n_atoms, "atom_idx": atom_idx, "edges": edges,
                    "scores": scores}
        if labels is not None:
            rc = self.lib.mnx_predict_guided(self.h, _ptr(images), int(gray), n, ref_batch, max_len, _ptr(labels),
                                             labels.shape[1], _ptr(tokens), _ptr(lengths), _ptr(n_atoms), _ptr(atom_idx),
                                             _ptr(edges), k, None, None, None, None, _stream())
            self._check(rc, "mnx_predict_guided")
            return {"tokens": tokens, "lengths": lengths, "n_atoms": n_atoms, "atom_idx": atom_idx, "edges": edges}
        if gray:
            rc = self.lib.mnx_predict_gray8(self.h, _ptr(images), n, ref_batch, max_len, _ptr(tokens), _ptr(lengths),
                                            _ptr(n_atoms), _ptr(atom_idx), _ptr(edges), k, None, None, None, None, _stream())
            self._check(rc, "mnx_predict_gray8")
            return {"tokens": tokens, "lengths": lengths, "n_atoms": n_atoms, "atom_idx": atom_idx, "edges": edges}
        rc = self.lib.mnx_predict(self.h, _ptr(images), n, ref_batch, max_len, int(stop_on_eos), _ptr(tokens), _ptr(lengths),
                                  _ptr(n_atoms), _ptr(atom_idx), _ptr(edges), k, _stream())
        self._check(rc, "mnx_predict")
        return {"tokens": tokens, "lengths": lengths, "n_atoms": n_atoms, "atom_idx": atom_idx, "edges": edges}

    # modest first capacities of graph_pack per image (a drug-like molecule has 20-40 heavy atoms, about as many bonds and a
    # SMILES of well under 200 bytes); `totals` sizes the one repeat when a job needs more
    PACK_GUESS = (48, 56, 192)

    def graph_pack(self, out: dict, caps=None, keep_device: bool = False) -> dict:
        """predict's result dict (device tensors) -> the molecules as numpy structured arrays (mnx_graph_pack): {'mols'
        [n] MOL_DTYPE, 'atoms' ATOM_DTYPE, 'bonds' BOND_DTYPE, 'text' bytes, 'totals' uint32 [4]}. With 'atom_scores',
        'edge_scores' and 'overall_score' in `out` the records carry the confidences, otherwise zeros. One D2H copy per table
        (plus the 16 bytes of totals); starts from PACK_GUESS per image (or caps = (atom_cap, bond_cap, text_cap)) and
        repeats at most once with the sizes `totals` reports. keep_device: also 'device' = the four tables as the uint8 device
        tensors they were written to, for molfile_pack and smiles_pack."""
        tokens, lengths = out["tokens"], out["lengths"]
        n, T = tokens.shape
        kmax = out["atom_idx"].shape[1]
        dev = tokens.device
        scored = out.get("edge_scores") is not None
        sc = [out["atom_scores"], out["edge_scores"], out["overall_score"]] if scored else [None, None, None]
        head = [_ptr(tokens), _ptr(lengths), n, T, _ptr(out["atom_idx"]), _ptr(out["n_atoms"]), _ptr(out["edges"]), kmax,
                _ptr(sc[0]), _ptr(sc[1]), _ptr(sc[2])]
        return self._sized_tables("mnx_graph_pack", n, caps if caps is not None else tuple(n * g for g in self.PACK_GUESS),
                                  lambda mols, arenas, totals: self.lib.mnx_graph_pack(self.h, *head, mols, *arenas, totals, _stream()),
                                  dev, keep_device)

    def _sized_tables(self, fn: str, n: int, caps, call, dev, keep_device: bool, side=None) -> dict:
        """One table writer over n molecules at capacities caps = (atom_cap, bond_cap, text_cap) and at most once more with
        the sizes `totals` reports: {'mols' [n] MOL_DTYPE, 'atoms' ATOM_DTYPE, 'bonds' BOND_DTYPE, 'text' bytes, 'totals'
        uint32 [4]}, keep_device: plus 'device' = the four tables as the uint8 device tensors they were written to.
        call(mols, arenas, totals) makes the library call lib.<fn> for one set of arenas and returns its code: mols and
        totals are pointers, arenas = [atoms, atom_cap, bonds, bond_cap, text, text_cap] as the three writers take them. side: the
        torch dtype of an output per atom (expand_pack's `origin`, the `atom_notes`), allocated at every attempt's atom capacity:
        call takes its pointer as a fourth argument, and 'side' is the last attempt's, one element per atom, on the device."""
        mols = torch.empty(n * MOL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        caps = tuple(int(c) for c in caps)
        for attempt in range(2):
            atoms = torch.empty(max(caps[0], 1) * ATOM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            bonds = torch.empty(max(caps[1], 1) * BOND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            text = torch.empty(max(caps[2], 1), dtype=torch.uint8, device=dev)
            arenas = [_ptr(atoms), caps[0], _ptr(bonds), caps[1], _ptr(text), caps[2]]
            per_atom = [] if side is None else [torch.empty(max(caps[0], 1), dtype=side, device=dev)]
            self._check(call(_ptr(mols), arenas, _ptr(totals), *map(_ptr, per_atom)), fn)
            tot = totals.cpu().numpy().view(np.uint32)
            if not tot[3]:
                break
            if attempt:
                raise MnxError(f"{fn}: capacities {caps} too small after sizing them from totals {tot.tolist()}")
            caps = (int(tot[0]), int(tot[1]), int(tot[2]))
        na, nb, nt = int(tot[0]), int(tot[1]), int(tot[2])
        rec = {"mols": mols.cpu().numpy().view(MOL_DTYPE),
               "atoms": atoms[:na * ATOM_DTYPE.itemsize].cpu().numpy().view(ATOM_DTYPE),
               "bonds": bonds[:nb * BOND_DTYPE.itemsize].cpu().numpy().view(BOND_DTYPE),
               "text": text[:nt].cpu().numpy().tobytes(), "totals": tot.copy()}
        if keep_device:
            rec["device"] = (mols, atoms, bonds, text)
        if per_atom:
            rec["side"] = per_atom[0][:na]
        return rec

    def _packed_tables(self, rec: dict):
        """graph_pack's records -> (the four tables as device tensors: those graph_pack(keep_device=True) left, or an upload;
        the leading arguments mols, n, atoms, na, bonds, nb, text, nt of a writer, None for an empty table)"""
        dev = torch.device("cuda", self.device)

        def up(a):
            raw = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
            return torch.frombuffer(bytearray(raw) or bytearray(8), dtype=torch.uint8).to(dev)

        tables = rec.get("device") or tuple(up(rec[k]) for k in ("mols", "atoms", "bonds", "text"))
        args = [_ptr(tables[0]), len(rec["mols"])]
        for t, k in zip(tables[1:], (len(rec["atoms"]), len(rec["bonds"]), len(rec["text"]))):
            args += [_ptr(t) if k else None, k]
        return tables, args

    def _sized_text(self, fn: str, head, cap: int, tail=()) -> bytes:
        """One text writer, lib.<fn>(h, *head, out, out_cap, totals, *tail, stream), at capacity `cap` and at most once more with
        the size `totals` reports: the bytes it wrote."""
        dev = torch.device("cuda", self.device)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        for attempt in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            self._check(getattr(self.lib, fn)(self.h, *head, _ptr(out), cap, _ptr(totals), *tail, _stream()), fn)
            tot = totals.cpu().numpy().view(np.uint32)
            if not tot[1]:
                break
            if attempt:
                raise MnxError(f"{fn}: capacity {cap} too small after sizing it from totals {tot.tolist()}")
            cap = int(tot[0])
        return out[:int(tot[0])].cpu().numpy().tobytes()

    MOLFILE_GUESS = 4096      # first capacity of molfile_pack per molecule (30 atoms and 30 bonds take about 2.6 KB)

    def molfile_pack(self, rec: dict, scale=None, cap: Optional[int] = None):
        """graph_pack's records -> (files [n] MOLFILE_DTYPE, bytes): the V2000 molfile of molecule b is
        bytes[files[b]['text0'] : +files[b]['len']] (mnx_molfile_pack; len 0 and a flag for a molecule that gets none).
        scale: int [n, 2] = (Sx, Sy) per molecule in units of 1e-4, None = 100000 each (include/molnextr_hip.h). The records
        go back to the device as they are (or stay there: graph_pack(keep_device=True)); starts from MOLFILE_GUESS bytes per
        molecule (or cap) and repeats at most once with the size `totals` reports."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        sc = None
        if scale is not None:
            sc = torch.as_tensor(np.ascontiguousarray(scale, dtype=np.int32).reshape(n, 2)).to(dev)
        files = torch.empty(n * MOLFILE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        data = self._sized_text("mnx_molfile_pack", args + [_ptr(sc), _ptr(files)], int(cap) if cap is not None else n * self.MOLFILE_GUESS)
        return files.cpu().numpy().view(MOLFILE_DTYPE), data

    SMILES_GUESS = 256        # first capacity of smiles_pack per molecule (a drug-like SMILES is well under 200 bytes)

    def smiles_pack(self, rec: dict, cap: Optional[int] = None, stereo: bool = False, double_bonds: bool = False,
                    canonical: bool = False, symmetry: bool = False):
        """graph_pack's records -> (recs [n] SMILES_DTYPE, order uint16 [atoms], bytes): the graph SMILES of molecule b is
        bytes[recs[b]['text0'] : +recs[b]['len']] (mnx_smiles_pack: valid, not canonical, no stereo, pseudo-atoms as '*'; len 0
        and a flag of SMILES_REFUSED for a molecule that gets none), order[atom0 + k] the position of its atom k in that
        string (SMILES_NO_POSITION without one). The records go back to the device as they are (or stay there:
        graph_pack(keep_device=True)); starts from SMILES_GUESS bytes per molecule (or cap) and repeats at most once with the
        size `totals` reports. stereo: mnx_smiles_pack_stereo — the same string with '@' / '@@' at the marked carbons that a
        wedge begins at (the rule: include/molnextr_hip.h), flags with SMILES_STEREO / SMILES_STEREO_UNRESOLVED. double_bonds:
        mnx_smiles_pack_marks — '/' and '\\' at the double bonds off every cycle that the coordinate bins resolve (the rule: the
        same header), with or without stereo's marks; flags with SMILES_EZ / SMILES_EZ_UNRESOLVED / SMILES_EZ_IMPLIED. Without
        it the calls are the ones made before it existed. canonical: mnx_smiles_pack_canonical — the same writer on canonical
        atom ranks, with the marks that stereo and double_bonds select; returns (recs, order, bytes, rank uint16 [atoms],
        sym_class uint16 [atoms]): the bytes do not depend on the numbering of a drawing's atoms (flags with SMILES_CANON_TIE /
        SMILES_CANON_TIE_INDEX; SMILES_NO_POSITION in rank and sym_class where the molecule was not read). This project's own
        ranking, NOT RDKit's canonical SMILES; the known limit stands in the header. symmetry (canonical only, else ValueError):
        mnx_smiles_pack_symmetric — a candidate centre or double bond with two substituents of one symmetry class, both on bonds
        off every cycle, writes no mark (flags with SMILES_SYM_DROPPED; off for a molecule with a pseudo-atom: expand first);
        returns a sixth value, atom_marks uint8 [atoms]: the ATOM_* bits per atom, ATOM_MARKS_NONE where `order` holds
        SMILES_NO_POSITION. The ranks ignore stereo and a pair on ring bonds is never dropped: the limits stand in the header."""
        if symmetry and not canonical:
            raise ValueError("smiles_pack: symmetry=True needs canonical=True")
        dev = torch.device("cuda", self.device)
        n, na = len(rec["mols"]), len(rec["atoms"])
        tables, args = self._packed_tables(rec)
        recs = torch.empty(n * SMILES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        order = torch.full((max(na, 1),), -1, dtype=torch.int16, device=dev)     # every entry SMILES_NO_POSITION
        if canonical:
            rank, sym_class = torch.full_like(order, -1), torch.full_like(order, -1)
            marks = (SMILES_MARK_TETRAHEDRAL if stereo else 0) | (SMILES_MARK_DOUBLE_BOND if double_bonds else 0)
            if symmetry:
                atom_marks = torch.zeros(max(na, 1), dtype=torch.uint8, device=dev)
                data = self._sized_text("mnx_smiles_pack_symmetric",
                                        args + [_ptr(recs), _ptr(order), _ptr(rank), _ptr(sym_class), _ptr(atom_marks)],
                                        int(cap) if cap is not None else n * self.SMILES_GUESS, (marks,))
                return (recs.cpu().numpy().view(SMILES_DTYPE), order[:na].cpu().numpy().view(np.uint16), data,
                        rank[:na].cpu().numpy().view(np.uint16), sym_class[:na].cpu().numpy().view(np.uint16),
                        atom_marks[:na].cpu().numpy())
            data = self._sized_text("mnx_smiles_pack_canonical", args + [_ptr(recs), _ptr(order), _ptr(rank), _ptr(sym_class)],
                                    int(cap) if cap is not None else n * self.SMILES_GUESS, (marks,))
            return (recs.cpu().numpy().view(SMILES_DTYPE), order[:na].cpu().numpy().view(np.uint16), data,
                    rank[:na].cpu().numpy().view(np.uint16), sym_class[:na].cpu().numpy().view(np.uint16))
        fn, tail = ("mnx_smiles_pack_stereo" if stereo else "mnx_smiles_pack"), ()
        if double_bonds:
            fn, tail = "mnx_smiles_pack_marks", (SMILES_MARK_DOUBLE_BOND | (SMILES_MARK_TETRAHEDRAL if stereo else 0),)
        data = self._sized_text(fn, args + [_ptr(recs), _ptr(order)], int(cap) if cap is not None else n * self.SMILES_GUESS, tail)
        return recs.cpu().numpy().view(SMILES_DTYPE), order[:na].cpu().numpy().view(np.uint16), data

    # margin, side, key of _tables_pass for the three frames of a pass: one that grows a molecule (room for a label of about ten
    # atoms), one that selects atoms (nothing grows), one that respells them (a new symbol is rarely longer than the old one)
    GROWS, SELECTS, RESPELLS = ((12, 12, 16), torch.int16, "origin"), ((0, 0, 0), torch.int16, "origin"), ((0, 0, 2), torch.uint8, "atom_notes")

    def _tables_pass(self, fn: str, rec: dict, caps, keep_device: bool, margin, side, key: str, tail=()) -> dict:
        """The five passes from tables to tables: lib.<fn>(h, tables, mols_out, arenas, per_atom, totals, *tail, stream) from the
        input's sizes plus margin = (atoms, bonds, text bytes) per molecule, or caps. side, key: the per-atom output's torch dtype
        and its key in the result — int16 -> 'origin' as uint16 [atoms], uint8 -> 'atom_notes'."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        if caps is None:
            caps = tuple(len(rec[k]) + m * n for k, m in zip(("atoms", "bonds", "text"), margin))
        out = self._sized_tables(fn, n, caps,
                                 lambda mols, arenas, totals, per_atom: getattr(self.lib, fn)(self.h, *args, mols, *arenas, per_atom, totals, *tail, _stream()),
                                 dev, keep_device, side=side)
        per_atom = out.pop("side").cpu().numpy()
        out[key] = per_atom.view(np.uint16) if side == torch.int16 else per_atom
        return out

    def expand_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records -> the same molecules with every abbreviation label that has a fragment replaced by the
        fragment's atoms and bonds (mnx_expand_pack; the rule: include/molnextr_hip.h): a dict with graph_pack's keys — 'mols',
        'atoms', 'bonds', 'text', 'totals' — plus 'origin' uint16 [atoms], the input index of the atom every output atom came
        from. molfile_pack and smiles_pack take it as it is. 'text' is the atoms' symbols behind one another, no token SMILES;
        the atoms of a fragment share the label's coordinates; mols['flags'] carries MOL_EXPANDED / MOL_LABEL_LEFT /
        MOL_EXPAND_REFUSED. Starts from the input's sizes plus a margin (or caps = (atom_cap, bond_cap, text_cap)) and repeats
        at most once with the sizes `totals` reports. keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_expand_pack", rec, caps, keep_device, *self.GROWS)

    def formula_pack(self, rec: dict, caps=None, keep_device: bool = False, max_steps: int = 0) -> dict:
        """graph_pack's records (or smiles_read's) -> the same molecules with every condensed-formula label ('CH2CH3', 'N(CH3)2',
        'COOCH3', 'CH2Ph': a symbol without a parse that is in neither name table, 2 to 20 bytes) that the valence search finds a
        structure for replaced by its atoms and bonds (mnx_formula_pack; the rule: include/molnextr_hip.h — this library's own
        repair of the reference's search, no toolkit has parsed the result). A group token inside a label ('Ph' in 'CH2Ph') is
        written as '[Ph]': run expand_pack behind this call. A dict with expand_pack's keys — 'mols', 'atoms', 'bonds', 'text',
        'totals', 'origin' —; mols['flags'] carries MOL_FORMULA_EXPANDED / MOL_FORMULA_LEFT / MOL_FORMULA_LIMIT /
        MOL_FORMULA_REFUSED. max_steps: the placements one label's search may try (0: FORMULA_DEFAULT_STEPS). Sizes itself as
        expand_pack does; keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_formula_pack", rec, caps, keep_device, *self.GROWS, (int(max_steps),))

    def main_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> of every molecule the connected component with the most
        atoms, among equals the one with the lowest atom, every other atom and its bonds dropped (mnx_main_pack; the rule: the
        reference's _keep_main_molecule, include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds',
        'text', 'totals' — plus 'origin' uint16 [atoms], the input index of every kept atom. 'text' is the kept atoms' symbols
        behind one another, as expand_pack's; mols['flags'] carries MOL_MAIN_KEPT / MOL_MAIN_TIE / MOL_MAIN_REFUSED. Run it
        behind expand_pack, so that a label counts with the atoms it stands for, and in front of kekulize_pack. Sized from the
        input — nothing grows — or caps = (atom_cap, bond_cap, text_cap), then once more with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_main_pack", rec, caps, keep_device, *self.SELECTS)

    def normalize_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> the same molecules with one normal spelling per atom
        (mnx_normalize_pack; the rule: include/molnextr_hip.h — this library's own, NOT a toolkit's aromaticity model): rings of 5
        and 6 atoms that the rule finds aromatic get lower-case atoms and class-4 bonds, a bracket atom that says no more than a
        reader infers loses its brackets, everything else is respelled as the writers spell it. A dict with graph_pack's keys —
        'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'atom_notes' uint8 [atoms]: NOTE_H_MASK the atom's H count,
        NOTE_AROMATIZED / NOTE_UNBRACKETED / NOTE_COPIED. Atom and bond counts and order are the input's; mols['flags'] carries
        MOL_AROMATIZED / MOL_UNBRACKETED / MOL_NORMALIZE_REFUSED. Starts from the input's sizes (a new symbol is rarely longer
        than the old one; or caps = (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_normalize_pack", rec, caps, keep_device, *self.RESPELLS)

    def kekulize_pack(self, rec: dict, caps=None, keep_device: bool = False, max_steps: int = 0) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> the same molecules with every aromatic system that has a
        Kekule structure written as one (mnx_kekulize_pack; the rule: include/molnextr_hip.h): lower-case atoms on type-4 bonds
        become upper-case atoms on double and single bonds, H counts kept; a system without a matching, a blocked one and one
        whose search passes max_steps pairings (0: KEKULE_DEFAULT_STEPS) stay as they came. A Kekule structure is a perfect
        matching; the choice among several is this library's own search order, NOT RDKit's Kekulize. A dict with graph_pack's
        keys — 'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'atom_notes' uint8 [atoms]: NOTE_H_MASK the H count of an
        aromatic atom, NOTE_KEKULIZED / NOTE_KEKULE_LEFT (with NOTE_KEKULE_LIMIT) / NOTE_COPIED. Atom and bond counts and order
        are the input's; mols['flags'] carries MOL_KEKULIZED / MOL_KEKULE_LEFT / MOL_KEKULIZE_REFUSED. Run it behind expand_pack
        and in front of normalize_pack. Sizes itself as normalize_pack does; keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_kekulize_pack", rec, caps, keep_device, *self.RESPELLS, (int(max_steps),))

    def fingerprint_pack(self, rec: dict, max_bonds: int = 0, max_steps: int = 0, keep_device: bool = False) -> dict:
        """graph_pack's records (or any pass's, or smiles_read's) -> {'fp' [n] FP_DTYPE, 'bits' uint32 [n, FP_WORDS]}: of every
        molecule the 2048 bits of its paths of up to max_bonds bonds (mnx_fingerprint_pack; the rule: include/molnextr_hip.h —
        this library's own, after the idea of Daylight's and RDKit's path fingerprints, NOT RDKit's bits). max_bonds 1 .. 7 (0:
        FP_MAX_BONDS); max_steps: the paths one directed bond may begin (0: FP_DEFAULT_STEPS; FP_MAX_STEPS at the most), beyond
        which the molecule gets FP_LIMIT. A molecule with a bit of FP_REFUSED or FP_LIMIT has every word 0; fp['n_bits'] counts
        the bits, fp['max_paths'] is the largest number of paths from one directed bond. Run it behind kekulize_pack and
        normalize_pack, so that an aromatic and a Kekule spelling give the same bits. One launch, nothing to size. keep_device:
        'bits' stays a device tensor (int32 [n, FP_WORDS], the same words), for tanimoto."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        recs = torch.empty(n * FP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        bits = torch.empty((n, FP_WORDS), dtype=torch.int32, device=dev)
        self._check(self.lib.mnx_fingerprint_pack(self.h, *args, _ptr(recs), _ptr(bits), int(max_bonds), int(max_steps), _stream()),
                    "mnx_fingerprint_pack")
        return {"fp": recs.cpu().numpy().view(FP_DTYPE), "bits": bits if keep_device else bits.cpu().numpy().view(np.uint32)}

    def tanimoto(self, a, b) -> dict:
        """Two tables of fingerprints [n, FP_WORDS] (fingerprint_pack's 'bits': numpy uint32 or the device tensors), row i of a
        against row i of b -> {'both' uint32 [n], 'either' uint32 [n], 'similarity' float64 [n]}: the bits both rows hold, the
        bits either holds, and their quotient — 0.0 where neither holds a bit: an empty side is a mismatch (mnx_tanimoto)."""
        dev = torch.device("cuda", self.device)

        def rows(x):
            if not isinstance(x, torch.Tensor):
                x = torch.from_numpy(np.array(x, dtype=np.uint32).view(np.int32))      # a copy: the caller's rows may be read-only
            x = x.to(dev).contiguous()
            if x.dim() != 2 or x.shape[1] != FP_WORDS or x.dtype != torch.int32:
                raise ValueError(f"tanimoto needs [n, {FP_WORDS}] words of 32 bits, not {tuple(x.shape)} {x.dtype}")
            return x

        a, b = rows(a), rows(b)
        if a.shape != b.shape:
            raise ValueError(f"tanimoto compares row with row: {tuple(a.shape)} against {tuple(b.shape)}")
        n = a.shape[0]
        both, either = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        similarity = torch.empty(n, dtype=torch.float64, device=dev)
        self._check(self.lib.mnx_tanimoto(self.h, _ptr(a), _ptr(b), n, _ptr(both), _ptr(either), _ptr(similarity), _stream()), "mnx_tanimoto")
        return {"both": both.cpu().numpy().view(np.uint32), "either": either.cpu().numpy().view(np.uint32),
                "similarity": similarity.cpu().numpy()}

    def substructure_match(self, query_rec: dict, target_rec: dict, pairs=None, max_matches: int = 1, max_steps: int = 0,
                           keep_device: bool = False) -> dict:
        """Two sets of records (graph_pack's, any pass's, a reader's; host arrays or keep_device=True outputs, and they may be the
        same dict) -> {'match' [n_pairs] MATCH_DTYPE, 'map' uint16 [n_pairs, MATCH_MAX_QUERY]}: per pair (query index, target
        index) whether the query molecule embeds in the target molecule (mnx_substructure_match; the rule: include/molnextr_hip.h
        — this library's own, NOT RDKit's HasSubstructMatch and not SMARTS). pairs: int [n_pairs, 2]; None pairs one query with
        every target, or item with item where the counts are equal. match['n_matches'] counts the embeddings up to max_matches
        (0: 1), match['steps'] is the longest search of one root, map[p][a] the target atom under query atom a in the first
        embedding (MATCH_NO_ATOM beyond the query or without a match). max_steps: the candidates one root's search may examine
        (0: MATCH_DEFAULT_STEPS; MATCH_MAX_STEPS at the most), beyond which the pair gets MATCH_LIMIT unless max_matches
        embeddings were found. A pair with a bit of MATCH_REFUSED was not searched. Run both sides through kekulize_pack and
        normalize_pack first, so that an aromatic query finds a Kekule drawing. One launch, nothing to size. keep_device: 'map'
        stays a device tensor (int16 [n_pairs, MATCH_MAX_QUERY], the same words)."""
        dev = torch.device("cuda", self.device)
        nq, nt = len(query_rec["mols"]), len(target_rec["mols"])
        if pairs is None:
            if nq != 1 and nq != nt:
                raise ValueError(f"substructure_match pairs one query with every target or item with item: {nq} queries against {nt} targets")
            pairs = np.stack([np.zeros(nt, np.int64) if nq == 1 else np.arange(nt), np.arange(nt)], axis=1)
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        if len(pairs) and (pairs.min() < 0 or pairs.max() > 0xFFFFFFFF):
            raise ValueError("substructure_match: a pair index outside 0 .. 2^32 - 1")
        n = len(pairs)
        q_tables, q_args = self._packed_tables(query_rec)
        t_tables, t_args = self._packed_tables(target_rec)
        d_pairs = torch.from_numpy(pairs.astype(np.uint32).view(np.int32)).to(dev)
        recs = torch.empty(n * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        maps = torch.empty((n, MATCH_MAX_QUERY), dtype=torch.int16, device=dev)
        self._check(self.lib.mnx_substructure_match(self.h, *q_args, *t_args, _ptr(d_pairs), n, _ptr(recs), _ptr(maps), int(max_matches),
                                                    int(max_steps), _stream()), "mnx_substructure_match")
        return {"match": recs.cpu().numpy().view(MATCH_DTYPE), "map": maps if keep_device else maps.cpu().numpy().view(np.uint16)}

    def smiles_read(self, strings, caps=None, keep_device: bool = False) -> dict:
        """SMILES strings (str or bytes) -> the molecules as packed tables, read on the device (mnx_smiles_read; the rule:
        include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'read' [n]
        READ_DTYPE (flags READ_*, err_pos, n_rings). molfile_pack, smiles_pack(... canonical=True) and expand_pack take it as it
        is. A refused string (READ_REFUSED) is the empty molecule. Starts from PACK_GUESS atoms and bonds per string, one per byte
        at the most (or caps = (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        dev = torch.device("cuda", self.device)
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in strings]
        n = len(raw)
        if n < 1:
            raise ValueError("smiles_read needs at least one string")
        lens = np.fromiter((len(x) for x in raw), dtype=np.int64, count=n)
        if int(lens.sum()) > 0xFFFFFFFF:
            raise ValueError("smiles_read: more than 2^32 - 1 bytes in one call")
        offsets = np.zeros(n + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum(lens)
        arena = b"".join(raw)
        d_bytes = torch.frombuffer(bytearray(arena) or bytearray(8), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int32)).to(dev)
        recs = torch.empty(n * READ_DTYPE.itemsize, dtype=torch.uint8, device=dev)      # per string: one for both attempts
        if caps is None:        # an atom takes a byte at least, a string has about as many bonds as atoms, and its text is itself
            caps = (min(len(arena), n * self.PACK_GUESS[0]), min(len(arena), n * self.PACK_GUESS[1]), len(arena))
        out = self._sized_tables("mnx_smiles_read", n, caps,
                                 lambda mols, arenas, totals: self.lib.mnx_smiles_read(
                                     self.h, _ptr(d_bytes), len(arena), _ptr(d_off), n, mols, _ptr(recs), *arenas, totals, _stream()),
                                 dev, keep_device)
        out["read"] = recs.cpu().numpy().view(READ_DTYPE)
        return out

    def molfile_read(self, files, scale=None, fit: bool = False, caps=None, keep_device: bool = False) -> dict:
        """V2000 molfiles (bytes or str, one molecule each; model.split_sdf cuts an SDF) -> the molecules as packed tables with
        their coordinate bins and wedge classes, read on the device (mnx_molfile_read; the rule — this library's own, NOT a
        toolkit's valence model: include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds', 'text',
        'totals' — plus 'read' [n] MOLREAD_DTYPE (flags MOLREAD_*, err_line, n_marked). Every pass and writer takes it as it is;
        smiles_pack(stereo=True, double_bonds=True) finds the marks a SMILES cannot bring. A refused file (MOLREAD_REFUSED) is the
        empty molecule. scale: int [n, 2] = (Sx, Sy) per file in units of 1e-4, None = 100000 each — molfile_pack's argument, and
        with the scale a file was written at the bins come back exactly; fit=True (no scale then): one uniform scale per file that
        fits its atoms into the bins, for files drawn elsewhere. Starts from one atom and one bond per 48 bytes (or caps =
        (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports. keep_device: also 'device', as
        graph_pack."""
        dev = torch.device("cuda", self.device)
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in files]
        n = len(raw)
        if n < 1:
            raise ValueError("molfile_read needs at least one file")
        if fit and scale is not None:
            raise ValueError("molfile_read: fit=True takes no scale")
        lens = np.fromiter((len(x) for x in raw), dtype=np.int64, count=n)
        if int(lens.sum()) > 0xFFFFFFFF:
            raise ValueError("molfile_read: more than 2^32 - 1 bytes in one call")
        offsets = np.zeros(n + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum(lens)
        arena = b"".join(raw)
        d_bytes = torch.frombuffer(bytearray(arena) or bytearray(8), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int32)).to(dev)
        sc = None
        if scale is not None:
            sc = torch.as_tensor(np.ascontiguousarray(scale, dtype=np.int32).reshape(n, 2)).to(dev)
        recs = torch.empty(n * MOLREAD_DTYPE.itemsize, dtype=torch.uint8, device=dev)   # per file: one for both attempts
        if caps is None:        # an atom line has 31 bytes at least, a bond line 12 in the writer's files; a symbol is short
            caps = (len(arena) // 48 + n, len(arena) // 48 + n, len(arena) // 16 + n)
        out = self._sized_tables("mnx_molfile_read", n, caps,
                                 lambda mols, arenas, totals: self.lib.mnx_molfile_read(
                                     self.h, _ptr(d_bytes), len(arena), _ptr(d_off), n, _ptr(sc), int(bool(fit)), mols, _ptr(recs), *arenas,
                                     totals, _stream()),
                                 dev, keep_device)
        out["read"] = recs.cpu().numpy().view(MOLREAD_DTYPE)
        return out

    def atom_scan(self, tokens: torch.Tensor, lengths: torch.Tensor, kmax: Optional[int] = None):
        """On-device CharTokenizer.sequence_to_smiles 'indices' for [n,T] int32 id sequences."""
        n, T = tokens.shape
        kmax = kmax or self.max_atoms
        idx = torch.zeros(n, kmax, dtype=torch.int32, device=tokens.device)
        cnt = torch.zeros(n, dtype=torch.int32, device=tokens.device)
        self._check(self.lib.mnx_atom_scan(self.h, _ptr(tokens), _ptr(lengths), n, T, kmax, _ptr(idx), _ptr(cnt),
                                           _stream()), "mnx_atom_scan")
        return idx, cnt

    def confidence(self, tokens: torch.Tensor, lengths: torch.Tensor, token_logp: torch.Tensor, atom_idx: torch.Tensor,
                   n_atoms: torch.Tensor, edge_scores: torch.Tensor):
        """On-device confidences (mnx_confidence) of [n,T] id sequences with their log-probs, atom positions [n,kmax] and
        fp64 edge scores [n,kmax,kmax]: (atom_scores [n,kmax], overall_score [n]), both fp64."""
        n, T = tokens.shape
        kmax = atom_idx.shape[1]
        dev = tokens.device
        tokens = tokens.to(dtype=torch.int32).contiguous()
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
        token_logp = token_logp.to(device=dev, dtype=torch.float32).contiguous()
        atom_idx = atom_idx.to(device=dev, dtype=torch.int32).contiguous()
        n_atoms = n_atoms.to(device=dev, dtype=torch.int32).contiguous()
        edge_scores = edge_scores.to(device=dev, dtype=torch.float64).contiguous()
        assert tuple(token_logp.shape) == (n, T) and tuple(edge_scores.shape) == (n, kmax, kmax)
        atom_scores = torch.zeros(n, kmax, dtype=torch.float64, device=dev)
        overall = torch.zeros(n, dtype=torch.float64, device=dev)
        self._check(self.lib.mnx_confidence(self.h, _ptr(tokens), _ptr(lengths), _ptr(token_logp), n, T, _ptr(atom_idx),
                                            _ptr(n_atoms), _ptr(edge_scores), kmax, _ptr(atom_scores), _ptr(overall),
                                            _stream()), "mnx_confidence")
        return atom_scores, overall

    def profile(self, enable):
        """True / n: bracket the GEMMs of every n-th encode call with HIP events (at most 16 calls); False: off."""
        self._check(self.lib.mnx_profile_enable(self.h, int(enable)), "mnx_profile_enable")

    # "gemm" = encoder GEMMs of the stages with C < 512 + the patch-merging reductions, "gemm_s34" = the block Linears
    # with C >= 512 (Swin-B stages 3 and 4: the MFMA-bound shapes); the GEMM family is the sum of the two
    PROFILE_KINDS = {"gemm": 0, "layernorm": 1, "window_attn": 2, "patch_embed": 3, "gemm_s34": 4}

    def profile_read(self, kind: str = "gemm", reset: bool = True):
        """(ms, work, launches) accumulated by HIP events for one kernel class since the last reset; work = FLOP for
        'gemm', algorithmic HBM bytes for the others."""
        ms, wk, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.mnx_profile_read(self.h, self.PROFILE_KINDS[kind], C.byref(ms), C.byref(wk), C.byref(n)),
                    "mnx_profile_read")
        if reset:
            self._check(self.lib.mnx_profile_read(self.h, -1, None, None, None), "mnx_profile_read")
        return ms.value, wk.value, n.value

    def profile_read_all(self):
        out = {k: self.profile_read(k, reset=False) for k in self.PROFILE_KINDS}
        self._check(self.lib.mnx_profile_read(self.h, -1, None, None, None), "mnx_profile_read")
        return out

    def probe_decode_attn(self, rows: int, t: int, iters: int = 20):
        """Isolated timing of the two per-row decode attention kernels: (self_ms, cross_ms) per launch."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.mnx_probe_decode_attn(self.h, rows, t, iters, C.byref(a), C.byref(b), _stream()),
                    "mnx_probe_decode_attn")
        return a.value, b.value

    def gemm_clock(self, reset: bool = True) -> float:
        """Shader clock (MHz) averaged over the persistent split-operand GEMM launches since the last reset (0.0: none ran)."""
        mhz = C.c_double()
        self._check(self.lib.mnx_gemm_clock(self.h, int(reset), C.byref(mhz)), "mnx_gemm_clock")
        return mhz.value

    def probe_mfma(self, ms: int = 30):
        """(TFLOP/s, MHz) of a register-only fp16 MFMA loop on random operands on every CU: what the matrix pipes sustain
        under this device's power budget."""
        tf, mhz = C.c_double(), C.c_double()
        self._check(self.lib.mnx_probe_mfma(self.h, ms, C.byref(tf), C.byref(mhz), _stream()), "mnx_probe_mfma")
        return tf.value, mhz.value

    def gemm16_split(self, epi: int, A2: torch.Tensor, W2: torch.Tensor, Cout: torch.Tensor,
                     bias: Optional[torch.Tensor], oscale: float = 1.0, terms: int = 3):
        """Split-mode GEMM on caller buffers: A2 [2,M,K] (terms = 2: [1,M,K] will do, the lo plane is not read) and W2 [2,N,K]
        hold the hi / lo planes (16-bit); Cout is [2,M,N] 16-bit (epi 0, 1; with epi | 0x400 [1,M,N]: hi plane only) or
        [M,N] fp32 (epi 2: bias + residual in place, 3: bias). epi | 0x200: the 128x128 kernel whatever the dispatch."""
        _, M, K = A2.shape
        N = W2.shape[1]
        c_lo = M * N if Cout.dim() == 3 and Cout.shape[0] == 2 else 0
        self._check(self.lib.mnx_gemm16_split(self.h, epi, _ptr(A2), M * K, _ptr(W2), N * K, float(oscale), _ptr(Cout), c_lo,
                                              _ptr(bias), M, N, K, terms, _stream()), "mnx_gemm16_split")
        return Cout

    def window_attn(self, qkv: torch.Tensor, table: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, heads: int,
                    shift: int, terms: int = 3, qkv_lo: int = 0, out_lo: int = 0):
        """The encoder's window attention on caller buffers (test aid, mnx_window_attn): qkv [B*H*W, 3C] -> out [B*H*W, C]
        in the engine's operand type, table fp32 [529, heads]. Split modes: qkv / out start with the hi planes, qkv_lo /
        out_lo are the element offsets of the lo planes from them; terms 3, 1 or 3 | 0x100 (the non-persistent kernel).
        Plain modes: terms = 1."""
        assert qkv.is_cuda and out.is_cuda and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()
        self._check(self.lib.mnx_window_attn(self.h, _ptr(qkv), qkv_lo, _ptr(table), _ptr(out), out_lo, B, H, W, heads * 32,
                                             heads, shift, terms, _stream()), "mnx_window_attn")
        return out

    KV_WHICH = {"self_k": 0, "self_v": 1, "mem_k": 2, "mem_v": 3}

    def kv_block(self, which: str, layer: int, owner: int, head: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One raw block of the decoder's K / V cache (test aid, mnx_kv_block) as uint8 bytes on the device: which is a key
        of KV_WHICH, owner the slot (self) or memory block (memory); after decode_greedy / decode_forced row b used slot b and
        memory block b. The block holds nk = kvq_rows(max_len) (self) or kvq_rows(144) (memory) rows of 100 bytes:
        [nk][32] int16 hi | [nk][32] uint8 lo | [nk] float32 scale (csrc/kvq.h)."""
        nk = ((self.max_len if which.startswith("self") else self.n_mem) + 3) & ~3
        if out is None:
            out = torch.empty(nk * 100, dtype=torch.uint8, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.uint8 and out.numel() >= nk * 100
        self._check(self.lib.mnx_kv_block(self.h, self.KV_WHICH[which], layer, owner, head, _ptr(out), _stream()),
                    "mnx_kv_block")
        return out

    # -- the encoder's non-GEMM kernels and the fp32 SGEMM on caller buffers (test aids) -----------------------------------
    # Thin: every argument goes to the library as given, which validates it (tests/test_gpu_encoder_ops.py).
    def patch_embed(self, img: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor,
                    beta: torch.Tensor, x: torch.Tensor, B: int, S: int, C_: int):
        """mnx_patch_embed: img fp32 [B,3,S,S] or uint8 [B,S,S] (gray bytes), w_t fp32 [48, C] -> x fp32 [B, (S/4)^2, C]"""
        fmt = IMAGE_FORMATS["gray8" if img.dtype == torch.uint8 else "fp32"]
        self._check(self.lib.mnx_patch_embed(self.h, _ptr(img), fmt, _ptr(w_t), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(x),
                                             B, S, C_, _stream()), "mnx_patch_embed")
        return x

    def layernorm16(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y16: Optional[torch.Tensor],
                    y32: Optional[torch.Tensor], M: int, C_: int, eps: float = 1e-5, y_lo: int = 0, planes: int = 2,
                    flag: Optional[torch.Tensor] = None):
        """mnx_layernorm16: x fp32 [M, C] -> y16 [M, C] in the engine's operand type (split modes: the hi plane, the lo plane
        y_lo elements behind it; planes = 1: hi only) and / or y32 fp32 [M, C]; flag: device int32, set on a non-finite row."""
        self._check(self.lib.mnx_layernorm16(self.h, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y16), y_lo, _ptr(y32), M, C_,
                                             float(eps), planes, _ptr(flag), _stream()), "mnx_layernorm16")

    def merge_ln16(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y16: torch.Tensor, B: int, H: int,
                   W_: int, C_: int, eps: float = 1e-5, y_lo: int = 0, planes: int = 2):
        """mnx_merge_ln16: x fp32 [B,H,W,C] -> y16 [B * H/2 * W/2, 4C], the patch-merging gather + LayerNorm(4C)"""
        self._check(self.lib.mnx_merge_ln16(self.h, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y16), y_lo, B, H, W_, C_,
                                            float(eps), planes, _stream()), "mnx_merge_ln16")

    def cast16(self, x: torch.Tensor, y16: torch.Tensor, n: int, y_lo: int = 0, scale: float = 1.0):
        """mnx_cast16: x fp32 [n] -> y16 [n] in the engine's operand type; split modes: hi / lo planes of scale * x"""
        self._check(self.lib.mnx_cast16(self.h, _ptr(x), _ptr(y16), y_lo, n, float(scale), _stream()), "mnx_cast16")

    def sgemm_tn(self, A: torch.Tensor, Wt: torch.Tensor, bias: Optional[torch.Tensor], Cout: torch.Tensor, M: int, N: int,
                 K: int, perm_S: int = 0):
        """mnx_sgemm_tn: Cout[M,N] = A[M,K] . Wt[N,K]^T + bias in fp32; perm_S > 0: the [M/S][N/256][8][S][32] layout"""
        self._check(self.lib.mnx_sgemm_tn(self.h, _ptr(A), _ptr(Wt), _ptr(bias), _ptr(Cout), M, N, K, perm_S, _stream()),
                    "mnx_sgemm_tn")

    def gemm16(self, epi: int, A: torch.Tensor, Wt: torch.Tensor, Cout: torch.Tensor, bias: Optional[torch.Tensor]):
        M, K = A.shape
        N = Wt.shape[0]
        self._check(self.lib.mnx_gemm16(self.h, epi, _ptr(A), _ptr(Wt), _ptr(Cout), _ptr(bias), M, N, K, _stream()),
                    "mnx_gemm16")
        return Cout
