"""`class Engine` over libmolnextr_hip.so (include/molnextr_hip.h): construction, the setters and the model path — encode, the
decodes, preprocess, predict, the bond head, the atom scan, the confidences. The class is written in three files, as the C host
side is (csrc/engine.hip, engine_tables.hip, engine_lab.hip): the packed-table layer is its base TableCalls (engine_tables.py),
the test and measurement aids its base LabCalls (engine_lab.py). The header's mirror — structs, dtypes, constants, prototypes,
the loader — is abi.py; every name this module used to define is still importable from here.

PyTorch is plumbing here: it owns device memory and the HIP stream; every tensor crosses the C ABI as a raw
device pointer. There is NO CPU fallback: if the library is missing or no MI355X is present, construction
raises.
"""
from __future__ import annotations

import ctypes as C
import os  # noqa: F401  (a name of this module's old surface)
from typing import Dict, Optional

import numpy as np
import torch

from . import weights as W
from .abi import (  # noqa: F401  (what this file uses, and the old import path of the whole mirror: new code imports from .abi)
    ABI_VERSION, ATOM_DTYPE, ATOM_EZ, ATOM_EZ_SYM, ATOM_MARKS_NONE, ATOM_MARK_CCW, ATOM_MARK_CW,
    ATOM_MARK_SYM, BOND_DTYPE, DEFAULT_DTYPE, DTYPES, FORMULA_DEFAULT_STEPS, FP16X3M_BLOCKS, FP16X3M_TWO_TERM,
    FP_BAD_BOND, FP_BEYOND_TABLES, FP_DEFAULT_STEPS, FP_DTYPE, FP_LIMIT, FP_MAX_BONDS, FP_MAX_STEPS,
    FP_PSEUDO_ATOM, FP_REFUSED, FP_TOO_LARGE, FP_TRUNCATED, FP_WORDS, IMAGE_FORMATS, KEKULE_DEFAULT_STEPS,
    MATCH_BAD_PAIR, MATCH_DEFAULT_STEPS, MATCH_DTYPE, MATCH_LIMIT, MATCH_MAX_QUERY, MATCH_MAX_QUERY_BONDS,
    MATCH_MAX_STEPS, MATCH_NO_ATOM, MATCH_QUERY_EMPTY, MATCH_QUERY_SHIFT, MATCH_QUERY_TOO_LARGE, MATCH_REFUSED,
    MNX_ERR_RANGE, MOLFILE_BEYOND_TABLES, MOLFILE_DTYPE, MOLFILE_PSEUDO_ATOM, MOLFILE_TOO_LARGE,
    MOLFILE_TRUNCATED, MOLREAD_BEYOND, MOLREAD_CLAMPED, MOLREAD_DTYPE, MOLREAD_H_DEFAULT, MOLREAD_IGNORED,
    MOLREAD_LABEL, MOLREAD_QUERY, MOLREAD_REFUSED, MOLREAD_STEREO_EITHER, MOLREAD_SYNTAX, MOLREAD_TOO_LARGE,
    MOL_AROMATIZED, MOL_DTYPE, MOL_EXPANDED, MOL_EXPAND_REFUSED, MOL_FORMULA_EXPANDED, MOL_FORMULA_LEFT,
    MOL_FORMULA_LIMIT, MOL_FORMULA_REFUSED, MOL_KEKULE_LEFT, MOL_KEKULIZED, MOL_KEKULIZE_REFUSED, MOL_LABEL_LEFT,
    MOL_MAIN_KEPT, MOL_MAIN_REFUSED, MOL_MAIN_TIE, MOL_NORMALIZE_REFUSED, MOL_TRUNCATED, MOL_UNBRACKETED,
    MnxAtom, MnxBond, MnxConfig, MnxError, MnxMol, MnxMolfile, MnxPage, MnxSmiles, MnxWeightDesc,
    NOTE_AROMATIZED, NOTE_COPIED, NOTE_H_MASK, NOTE_KEKULE_LEFT, NOTE_KEKULE_LIMIT, NOTE_KEKULIZED,
    NOTE_UNBRACKETED, PREP_MAX_PAGES, PROTOTYPES, RANGE_FALLBACK, READ_BEYOND, READ_DTYPE, READ_REFUSED,
    READ_STEREO_DROPPED, READ_SYNTAX, READ_TOO_LARGE, SMILES_BEYOND_TABLES, SMILES_CANON_TIE,
    SMILES_CANON_TIE_INDEX, SMILES_DTYPE, SMILES_DUPLICATE_BOND, SMILES_EZ, SMILES_EZ_IMPLIED,
    SMILES_EZ_UNRESOLVED, SMILES_MARK_DOUBLE_BOND, SMILES_MARK_TETRAHEDRAL, SMILES_NO_POSITION, SMILES_PSEUDO_ATOM,
    SMILES_REFUSED, SMILES_RING_NUMBERS, SMILES_STEREO, SMILES_STEREO_UNRESOLVED, SMILES_SYM_DROPPED,
    SMILES_TOO_LARGE, SMILES_TRUNCATED, SMILES_UNKNOWN_BOND, SMILES_WEDGES_DROPPED, SPLIT_CLASSES, SYMBOLS,
    _ptr, _stream, library_path, load_library, range_fallback_dtype, two_term_masks)
from .engine_lab import LabCalls, check_beam_script  # noqa: F401  (check_beam_script: the old import path)
from .engine_tables import TableCalls


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


class Engine(TableCalls, LabCalls):
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
