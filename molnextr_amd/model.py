"""Model facade: mirrors the reference's `molnextr` class and `Decoder.decode` on top of the HIP engine.

  decode_batch(...)        <-> Decoder.decode                       reference MolNexTR/components.py:443-492
  molnextr.predict_images  <-> molnextr.predict_images              reference MolNexTR/model.py:97-146
  molnextr.predict_image / predict_image_files / predict_final_results   reference MolNexTR/model.py:148-196

Same method names, argument meaning and output dict keys. Everything between "normalised image batch" and "token
ids / hidden states / bond matrix" runs in libmolnextr_hip.so; tokens are turned into symbols / coordinates /
atom positions on the host (tokenizer.py), as in the reference. No CPU fallback exists for the device part.
"""
from __future__ import annotations

import argparse
import re  # noqa: F401  (a name of this module's old surface)
from typing import List, Optional

import numpy as np
import torch

from . import weights as W
from .abi import (DEFAULT_DTYPE, FP_LIMIT, FP_REFUSED, FP_WORDS, MATCH_BAD_PAIR, MATCH_LIMIT, MATCH_REFUSED,  # noqa: F401
                  MOL_FORMULA_LEFT, MOL_TRUNCATED, NOTE_H_MASK, SMILES_NO_POSITION, SMILES_REFUSED, MnxError, range_fallback_dtype)
from .chain import BY_NAME, PASSES, passes_on, run_chain  # noqa: F401
from .engine import Engine
from .graphs import (_same_graph_tables, canonical_molfiles, canonical_smiles, formula_candidate,  # noqa: F401
                     molfile_fingerprints, nearest_smiles, packed_predictions, page_scale, same_graph, smiles_fingerprints,
                     smiles_library, smiles_substructure, split_sdf, tanimoto, unpack_graphs)
from .preprocess import load_image_rgb, transform_image, transform_image_gray
from .tokenizer import coords_labels, get_tokenizer

BOND_TYPES = ["", "single", "double", "triple", "aromatic", "solid wedge", "dashed wedge"]  # reference model.py:30
ROWS = Engine.ROWS_PER_DECODE
MAX_REF_BATCH = Engine.MAX_REF_BATCH      # rows of one reference batch on the continuous-batching greedy path (predict_pipeline)


def decode_batch(engine: Engine, features: torch.Tensor, tokenizer=None, ref_batch_size: Optional[int] = None,
                 compute_confidence: bool = False, max_len: Optional[int] = None, beam_size: int = 1,
                 n_best: int = 1) -> List[dict]:
    """Decoder.decode for formats ['chartok_coords', 'edges'] (reference components.py:443-492).

    features [B,144,1024] on the GPU. `ref_batch_size`: rows are numbered as if the reference had decoded them in
    consecutive batches of this size (its positional encoding is indexed by the row inside the batch and finished
    rows are compacted away, so results depend on the batch composition); None = one batch of B (B <= 32) or
    batches of 32. Returns one dict per image: {'chartok_coords': {smiles, symbols, coords, indices[, atom_scores]},
    'edges': [[...]] [, 'edge_scores', 'overall_score']}.

    beam_size > 1 (reference signature components.py:443; its own beam branch cannot run): the
    best hypothesis of each image is detokenised, as the reference does with `pred[0]` (components.py:453-455), and
    the bond head runs on the decoder outputs along that hypothesis; `beam_scores` lists the n_best average
    log-probs. Token confidences are not tracked by beam search (nor by the reference's BeamSearch).
    """
    tok = (tokenizer or get_tokenizer())["chartok_coords"]
    B = features.shape[0]
    rbs = ref_batch_size or ROWS
    if rbs > ROWS:
        raise ValueError(f"decode_batch decodes reference batches of at most {ROWS} rows per engine call; use predict_pipeline "
                         f"(greedy, up to {MAX_REF_BATCH} rows per reference batch) for ref_batch_size={rbs}")
    group = (ROWS // rbs) * rbs          # rows per engine call: whole reference batches only
    if beam_size > 1:
        if compute_confidence:
            raise NotImplementedError("beam search does not track token scores (neither does the reference's)")
        group = rbs                      # one reference batch per beam call
    preds: List[dict] = []
    for g0 in range(0, B, group):
        feats = features[g0:g0 + group].contiguous()
        n = feats.shape[0]
        beam_scores = None
        if beam_size > 1:
            bo = engine.decode_beam(feats, beam=beam_size, n_best=n_best, max_len=max_len)
            out = {"lengths": bo["lengths"][:, 0].contiguous(), "tokens": bo["tokens"][:, 0].contiguous(),
                   "hidden": bo["hidden"][:, 0].contiguous()}
            beam_scores = bo["scores"].cpu().numpy()
        else:
            chunk = torch.arange(n, dtype=torch.int32) // rbs
            out = engine.decode_greedy(feats, chunk_id=chunk, max_len=max_len, want_logp=True)
        lens = out["lengths"].cpu().numpy()
        toks = out["tokens"].cpu().numpy()
        logp = out["token_logp"].cpu().numpy() if compute_confidence else None
        rows = [tok.sequence_to_smiles(toks[b, :lens[b]].tolist()) for b in range(n)]
        kmax = engine.max_atoms
        n_atoms = np.array([len(r["indices"]) for r in rows], dtype=np.int32)
        if n_atoms.max(initial=0) > kmax:
            raise RuntimeError(f"{int(n_atoms.max())} atoms exceed the engine capacity max_atoms={kmax}")
        atom_idx = np.zeros((n, kmax), dtype=np.int32)
        for b, r in enumerate(rows):
            atom_idx[b, :n_atoms[b]] = r["indices"]
        edges, scores = engine.edges(out["hidden"], torch.from_numpy(atom_idx), torch.from_numpy(n_atoms),
                                     want_scores=compute_confidence)
        edges = edges.cpu().numpy()
        scores = scores.cpu().numpy() if scores is not None else None
        for b, r in enumerate(rows):
            k = int(n_atoms[b])
            pred = {"chartok_coords": r, "edges": edges[b, :k, :k].astype(int).tolist()}
            if beam_scores is not None:
                pred["beam_scores"] = beam_scores[b].tolist()
            if compute_confidence:   # reference components.py:456-469, 485-491
                ts = np.exp(logp[b, :lens[b]].astype(np.float64))
                idx = np.array(r["indices"]) - 3
                r["atom_scores"] = [float(np.prod(ts[i - len(s) + 1:i + 1]) ** (1 / len(s)))
                                    for s, i in zip(r["symbols"], idx)]
                avg = float(np.exp(np.mean(logp[b, :lens[b]].astype(np.float64))))
                es = scores[b, :k, :k]
                pred["edge_scores"] = es.tolist()
                pred["overall_score"] = avg * float(np.sqrt(np.prod(es)))
            preds.append(pred)
    return preds


def predict_pipeline(engine: Engine, images: torch.Tensor, tokenizer=None, ref_batch_size: int = 16,
                     max_len: Optional[int] = None, beam_size: int = 1, compute_confidence: bool = False,
                     labels=None, free_run=False, packed: bool = False, molfile: bool = False,
                     molfile_scale=None, smiles: bool = False, stereo: bool = False, double_bonds: bool = False,
                     canonical: bool = False, expand: bool = False, symmetry: bool = False, normalize: bool = False,
                     kekulize: bool = False, formula: bool = False, keep_main: bool = False) -> List[dict]:
    """Encoder + Decoder.decode for MANY images through the engine's continuous-batching path (mnx_predict):
    same per-image dicts as `decode_batch`, identical results (the on-device atom scan equals
    sequence_to_smiles' indices), much higher throughput. compute_confidence=True: mnx_predict_confidence, the same
    pipeline with the confidences computed on the device when a reference batch retires; the dicts gain the keys of
    decode_batch(compute_confidence=True) ('atom_scores' in 'chartok_coords', 'edge_scores', 'overall_score').
    beam_size > 1: mnx_predict_beam (best hypothesis per image, 'beam_scores' = [its average log-prob]); no confidences.
    ref_batch_size: rows per reference batch (the positional-encoding numbering unit), up to MAX_REF_BATCH = 512 for greedy
    decoding (and the engine's max_batch / dec_slots: Engine.max_ref_batch), up to 32 with beam_size > 1.
    labels: int [n, L] — label-guided decoding along row i for image i (mnx_predict_guided; Engine.decode_guided describes the
    rows; a row without '<eos>' raises ValueError unless free_run — a bool, or one per row — exempts it); greedy only.
    packed: the molecules are put together on the device (mnx_graph_pack) and only their records cross to the host
    (unpack_graphs: 'bonds' instead of the dense 'edges' / 'edge_scores'); greedy only, beam search keeps the dense path.
    The packed path does not run the host tokenizer, so it does not re-verify the device atom scan as the dense path's
    assertion does: 'indices' are the scan's atom_idx, and a molecule beyond max_atoms raises RuntimeError.
    molfile (packed only): every dict gains 'molfile', the molecule as a V2000 molfile written on the device from the packed
    tables (mnx_molfile_pack; a str, None for a molecule that gets none); molfile_scale: int [n, 2] = (Sx, Sy) per image in
    units of 1e-4, None = 100000 each — the reference's factor 10 on a square page.
    smiles (packed only): every dict gains 'graph_smiles', a SMILES of the predicted graph written on the device from the packed
    tables (mnx_smiles_pack: valid, not canonical, no stereo, abbreviations and R-groups as '*'; a str, None for a molecule
    that gets none), and 'graph_smiles_order', the position of every atom in that string (None without one).
    stereo (smiles only): the graph SMILES carry '@' / '@@' at the marked carbons that a wedge begins at, decided by the wedges and
    the coordinate bins (mnx_smiles_pack_stereo: this library's own rule, include/molnextr_hip.h; no '/' '\\').
    double_bonds (smiles only): the graph SMILES carry '/' and '\\' at the double bonds off every cycle whose substituents the
    coordinate bins put on either side (mnx_smiles_pack_marks: this library's own rule, the same header), with stereo's marks or
    without; a double bond on a cycle is never marked and no symmetry check is made.
    canonical (smiles only): the graph SMILES are written on canonical atom ranks (mnx_smiles_pack_canonical, with the marks that
    stereo and double_bonds select), so two numberings of one drawing give the same bytes, and every dict gains 'canonical_rank'
    and 'symmetry_class', a list per atom (None for a molecule that was not ranked). This library's own ranking: it is NOT
    RDKit's canonical SMILES, no toolkit has parsed it, and the header states the known limit (a few graphs whose string still
    depends on the drawing).
    symmetry (smiles and canonical only, else ValueError): mnx_smiles_pack_symmetric instead — a candidate centre or double bond
    with two substituents of one symmetry class, both on bonds off every cycle, writes no mark, so an isopropyl carbon drawn with
    a wedge and its mirror image get one string. Every dict gains 'stereo_atoms', the ATOM_* bits of abi.py per atom (per
    EXPANDED atom with expand), None for a molecule that got no string. The rule is off for a molecule with a pseudo-atom
    (expand first), the ranks ignore stereo (a pseudo-asymmetric centre is dropped), a pair on ring bonds is never dropped, and
    no toolkit has parsed the result: the limits stand in the header.
    expand (packed only): abbreviation labels that have a fragment in vocab/fragments.json ('Ph', 'OMe', 'Boc', ...) are replaced
    by the fragment's atoms and bonds on the device before anything is written (mnx_expand_pack; the rule: the header), so
    'molfile' and 'graph_smiles' describe the expanded molecule instead of writing 'R' / '*' for the label. Every dict gains
    'expanded' = {'symbols', 'coords', 'bonds' [(i, j, type, rev[, score])], 'origin' (per expanded atom, the index of the
    predicted atom it came from), 'flags' (MOL_EXPANDED / MOL_LABEL_LEFT of abi.py)}; 'graph_smiles_order', 'canonical_rank'
    and 'symmetry_class' then have one entry per EXPANDED atom, in the order of expanded['symbols']. The predicted atoms and
    bonds ('chartok_coords', 'bonds') are what they are without it. From a table only (a condensed formula is `formula`'s, below), the atoms
    of a fragment share the label's coordinates, and no toolkit has parsed the result.
    normalize (packed only; behind expand when both are set): the molecule is given one normal spelling per atom on the device
    before anything is written (mnx_normalize_pack; the rule: the header) — rings of 5 and 6 atoms that the rule finds aromatic get
    lower-case atoms and class-4 bonds, a bracket atom that says no more than a reader infers loses its brackets —, so a Kekule
    drawing and an aromatic one, [CH] and C, N and [nH] get one canonical string. 'molfile' and 'graph_smiles' then describe the
    normalised molecule, and every dict gains 'normalized' = {'symbols', 'bonds' [(i, j, type, rev[, score])], 'hydrogens' (per
    atom: written for a bracket atom, inferred otherwise), 'notes' (the NOTE_* bits of abi.py per atom), 'flags'
    (MOL_AROMATIZED / MOL_UNBRACKETED)}, atom for atom in the order of the expanded (or predicted) atoms. This library's own
    rule: NOT RDKit's aromaticity model, no toolkit has checked it, rings of other sizes stay as drawn.
    kekulize (packed only; behind expand and in front of normalize): every aromatic system that has a Kekule structure is written
    as one on the device before anything else runs on the molecule (mnx_kekulize_pack; the rule: the header) — lower-case atoms on
    class-4 bonds become upper-case atoms on double and single bonds, so 'molfile' carries no bond type 4 for them. Every dict
    gains 'kekulized' = {'symbols', 'bonds', 'hydrogens' (per aromatic atom), 'notes' (NOTE_KEKULIZED / NOTE_KEKULE_LEFT /
    NOTE_KEKULE_LIMIT / NOTE_COPIED of abi.py per atom), 'flags' (MOL_KEKULIZED / MOL_KEKULE_LEFT)}, the molecule as it left
    that pass. A Kekule structure is a perfect matching; the choice among several is this library's own search order, NOT RDKit's
    Kekulize, and a system without a matching or on a class-4 bond to an upper-case atom stays aromatic.
    formula (packed only; in front of expand): condensed-formula labels that are in neither name table ('CH2CH3', 'N(CH3)2',
    'COOCH3', 'CH2Ph') are replaced on the device by the atoms and bonds a valence-guided search finds for them
    (mnx_formula_pack; the rule: the header — this library's own repair of the reference's search, no toolkit has parsed the
    result), before expand replaces the table's labels and the group tokens a formula holds ('[Ph]'). Every dict gains 'formula'
    = {'symbols', 'coords', 'bonds', 'origin', 'flags' (MOL_FORMULA_EXPANDED / MOL_FORMULA_LEFT / MOL_FORMULA_LIMIT of
    abi.py), 'replaced' (the predicted atoms whose label was replaced), 'left' (the predicted atoms that were candidates and
    stayed)}, the molecule as it left that pass; expanded['origin'] still names the PREDICTED atom. Without expand the per-atom
    lists of the writers have one entry per atom of formula['symbols'].
    keep_main (packed only; behind expand and in front of kekulize): of every molecule the connected component with the most atoms
    stays — among equals the one with the lowest atom — and every other atom and its bonds are dropped on the device before
    anything else runs on the molecule (mnx_main_pack; the rule is the reference's _keep_main_molecule: salts, counter-ions and
    stray atoms go; behind expand, so that a label counts with the atoms it stands for). 'molfile' and 'graph_smiles' then
    describe the main molecule, and every dict gains 'main' = {'symbols', 'coords', 'bonds', 'origin' (per kept atom, its index
    in the molecule the pass received: expanded['symbols'] with expand, else formula['symbols'] with formula, else the predicted
    atoms), 'flags' (MOL_MAIN_KEPT / MOL_MAIN_TIE of abi.py)}; the per-atom lists of the writers have one entry per atom of
    main['symbols']. The predicted atoms and bonds ('chartok_coords', 'bonds') are what they are without it.
    The order of the five passes — formula, expand, keep_main, kekulize, normalize — stands in chain.PASSES.
    predict_fingerprints is this call with the path fingerprint of every molecule in its dict."""
    return _pipeline(engine, images, tokenizer, ref_batch_size, max_len, beam_size, compute_confidence, labels, free_run, packed,
                     molfile, molfile_scale, smiles, stereo, double_bonds, canonical, expand, symmetry, normalize, kekulize, formula,
                     keep_main, fingerprint=False)


def predict_fingerprints(engine: Engine, images: torch.Tensor, tokenizer=None, **options) -> List[dict]:
    """predict_pipeline(engine, images, tokenizer, packed=True, **options) with one more sink behind the last pass, beside the
    writers: every dict gains 'fingerprint', the 2048 bits of the molecule's paths of up to 7 bonds as 256 bytes (64
    little-endian words of mnx_fingerprint_pack; the rule: include/molnextr_hip.h — this library's own, after the idea of
    Daylight's and RDKit's path fingerprints, NOT RDKit's bits), None for a molecule that is refused (FP_REFUSED) or passes the
    step limit (FP_LIMIT). options: predict_pipeline's keywords (packed is set here: the paths are walked in the packed tables);
    kekulize=True and normalize=True make an aromatic and a Kekule drawing give the same bits. Engine.tanimoto compares two. A
    function of its own because predict_pipeline's parameter list is closed."""
    if not options.setdefault("packed", True):
        raise ValueError("predict_fingerprints needs packed=True: the paths are walked in the packed tables")
    return _pipeline(engine, images, tokenizer, fingerprint=True, **options)


def predict_substructures(engine: Engine, images: torch.Tensor, queries, tokenizer=None, **options) -> List[dict]:
    """predict_pipeline(engine, images, tokenizer, packed=True, **options) with one more sink behind the last pass, beside the
    writers and the fingerprint: every dict gains 'substructure', per query SMILES of `queries` {'matched': True, False, or None
    when the pair was refused or its search broken off without a match; 'atoms': the predicted atoms (of the molecule behind the
    passes) under the query's atoms, in the query's atom order; 'coords': their page coordinates} — does this prediction hold that
    scaffold, and where on the page (mnx_substructure_match; the rule: include/molnextr_hip.h — this library's own, NOT RDKit's
    HasSubstructMatch and not SMARTS). The queries are read on the device and pass through the same passes as the predictions;
    kekulize=True and normalize=True make an aromatic query find a Kekule drawing. options: predict_pipeline's keywords, and
    fingerprint=True for predict_fingerprints' key. A function of its own because predict_pipeline's parameter list is closed."""
    if not options.setdefault("packed", True):
        raise ValueError("predict_substructures needs packed=True: the search runs in the packed tables")
    return _pipeline(engine, images, tokenizer, substructure=list(queries), **options)


def predict_nearest(engine: Engine, images: torch.Tensor, library, k: int = 1, min_similarity: float = 0.0, tokenizer=None,
                    **options) -> List[dict]:
    """predict_pipeline(engine, images, tokenizer, packed=True, **options) with one more sink behind the last pass, beside the
    writers, the fingerprint and the substructure search: every dict gains 'nearest', the k compounds of `library` nearest to the
    prediction by the Tanimoto similarity of this library's path fingerprints — [{'index', 'smiles', 'similarity'}], the first k
    by similarity, among equals the lower index, of those the ones at or above min_similarity; [] for a molecule that is refused
    or passes the step limit (mnx_fingerprint_pack, mnx_tanimoto_search; the rule: include/molnextr_hip.h — NOT RDKit's
    fingerprint, k <= NEAREST_MAX_K). library: a list of SMILES, read on the device and sent through the same passes as the
    predictions, or graphs.smiles_library's dict, made once with those passes. options: predict_pipeline's keywords, fingerprint=True
    for predict_fingerprints' key and substructure=[...] for predict_substructures'. A function of its own because
    predict_pipeline's parameter list is closed."""
    if not options.setdefault("packed", True):
        raise ValueError("predict_nearest needs packed=True: the fingerprints are made from the packed tables")
    return _pipeline(engine, images, tokenizer, nearest=(library, int(k), float(min_similarity)), **options)


def _pipeline(engine, images, tokenizer=None, ref_batch_size=16, max_len=None, beam_size=1, compute_confidence=False, labels=None,
              free_run=False, packed=False, molfile=False, molfile_scale=None, smiles=False, stereo=False, double_bonds=False,
              canonical=False, expand=False, symmetry=False, normalize=False, kekulize=False, formula=False, keep_main=False,
              fingerprint=False, substructure=None, nearest=None) -> List[dict]:
    """The body of predict_pipeline (its arguments, its defaults), of predict_fingerprints (fingerprint=True), of
    predict_substructures (substructure: the query SMILES) and of predict_nearest (nearest: (library, k, min_similarity))."""
    tok =(tokenizer or get_tokenizer())["chartok_coords"]
    why = {**{p.name: p.packed_why for p in PASSES}, "molfile": "the molfiles are written from the packed tables",
           "smiles": "the graph SMILES are written from the packed tables"}
    for name, given in (("formula", formula), ("keep_main", keep_main), ("normalize", normalize), ("kekulize", kekulize),
                        ("expand", expand), ("molfile", molfile), ("smiles", smiles)):      # the order they are reported in
        if given and not packed:
            raise ValueError(f"{name}=True needs packed=True: {why[name]}")
    if stereo and not smiles:
        raise ValueError("stereo=True needs smiles=True: the marks are written into the graph SMILES")
    if double_bonds and not smiles:
        raise ValueError("double_bonds=True needs smiles=True: the marks are written into the graph SMILES")
    if canonical and not smiles:
        raise ValueError("canonical=True needs smiles=True: the ranks order the graph SMILES")
    if symmetry and not (smiles and canonical):
        raise ValueError("symmetry=True needs smiles=True and canonical=True: the rule reads the symmetry classes of the ranks")
    if packed and beam_size > 1:
        raise NotImplementedError("packed results are built for greedy decoding (beam search keeps the dense path)")
    if labels is not None and beam_size > 1:
        raise NotImplementedError("label-guided decoding is greedy (beam search with labels is not built)")
    if compute_confidence and beam_size > 1:
        raise NotImplementedError("beam search does not track token scores (neither does the reference's)")
    if beam_size > 1 and ref_batch_size > ROWS:
        raise ValueError(f"beam search takes reference batches of at most {ROWS} rows; got ref_batch_size={ref_batch_size} "
                         f"(greedy decoding takes up to {MAX_REF_BATCH})")
    conf = {"confidence": True} if compute_confidence else {}
    if labels is not None:
        conf.update(labels=labels, free_run=free_run)
    out = engine.predict(images, ref_batch=ref_batch_size, max_len=max_len, beam=beam_size, **conf)
    if packed:
        on = passes_on(formula, expand, keep_main, kekulize, normalize)
        return packed_predictions(engine, out, tok, on, compute_confidence, molfile, molfile_scale, smiles, stereo, double_bonds,
                                  canonical, symmetry, fingerprint, substructure, nearest)
    scores = out["scores"].cpu().numpy() if beam_size > 1 else None
    lens = out["lengths"].cpu().numpy()
    toks = out["tokens"].cpu().numpy()
    n_atoms = out["n_atoms"].cpu().numpy()
    edges = out["edges"].cpu().numpy()
    if compute_confidence:
        k_hi = int(n_atoms.max(initial=0))          # only the atoms of this call cross to the host (fp64 [n,160,160]: 205 KB each)
        edge_scores = out["edge_scores"][:, :k_hi, :k_hi].cpu().numpy()
        atom_scores = out["atom_scores"][:, :k_hi].cpu().numpy()
        overall = out["overall_score"].cpu().numpy()
    preds = []
    for b in range(len(lens)):
        r = tok.sequence_to_smiles(toks[b, :lens[b]].tolist())
        k = int(n_atoms[b])
        assert k == len(r["indices"]), "device atom scan disagrees with the host tokenizer"
        preds.append({"chartok_coords": r, "edges": edges[b, :k, :k].astype(int).tolist()})
        if scores is not None:
            preds[-1]["beam_scores"] = [float(scores[b])]
        if compute_confidence:
            r["atom_scores"] = atom_scores[b, :k].tolist()
            preds[-1]["edge_scores"] = edge_scores[b, :k, :k].tolist()
            preds[-1]["overall_score"] = float(overall[b])
    return preds


class _RestartCall(Exception):
    """Private: the facade's engine was rebuilt in the range-fallback mode after part of a call had been computed."""


class molnextr:
    """Main interface (reference MolNexTR/model.py:33-196).

    model_path: a checkpoint in the reference's format ({'encoder','decoder','args'}, `.pth`) or our `.safetensors`;
    the literal 'synthetic' opts into the deterministic hash-generated checkpoint (tests / bench only: its predictions
    are meaningless as chemistry). There is no default: like the reference, the model cannot run without weights.
    device: torch.device('cuda', i) — an MI355X is required.
    dtype: encoder operand mode. 'fp16x3' (the default, abi.DEFAULT_DTYPE: split fp16 operands, three MFMA terms per product:
    features equal the reference's to fp32 rounding level, logits within 2.5e-4), 'fp16x3m' (opt-in: the Linear layers of
    abi.FP16X3M_TWO_TERM on two terms, +8-11 % throughput; every token / atom / bond still the reference's on everything
    measured, raw logits within 5e-4 on the fixtures, 7.2e-4 on further images and up to 1.2e-3 on a hostile checkpoint — at and
    beyond north_star's 1e-3),
    'bf16x3' (three terms with the fp32 exponent range), 'fp32' (exact-fp32 MFMA, slowest), 'bf16' / 'fp16' (fastest; argmax
    decisions near a tie can differ).
    image_format: what the transform hands to the encoder — "fp32" (the default: normalised [n,3,S,S], one mnx_preprocess per
    page) or "gray8" (the gray byte per pixel, [n,S,S]: all pages of a group in one mnx_preprocess_batch, a twelfth of the
    staged bytes; every output bit for bit the same).
    packed_results: True = the molecules are put together on the device (mnx_graph_pack) and cross to the host as packed atom /
    bond / text records instead of the dense token, bond and score matrices; the output dicts are the same.
    graph_molfile: True (opt-in; implies the packed path) = when RDKit is absent 'predicted_molfile' is the V2000 molfile that
    the device writes from the packed tables (mnx_molfile_pack: this library's own writer, not RDKit's), with the reference's
    page ratio in x (chemical.py:935-937); 'predicted_smiles' stays None — a canonical SMILES needs RDKit.
    graph_smiles: True (opt-in; implies the packed path) = when RDKit is absent 'predicted_smiles' is the SMILES that the device
    writes from the predicted graph (mnx_smiles_pack). That SMILES is valid but not canonical: two drawings of one molecule
    can give two different strings, so compare them only after a toolkit has canonicalised both. It carries no stereo (no
    '@', '/' or '\\' unless graph_stereo / graph_double_bonds ask for them: wedge bonds are written as plain single bonds), and
    an abbreviation or R-group stays a '*' atom
    instead of being expanded. A molecule the writer refuses (more than 99 ring closures open at once, say) keeps None. The
    default stays None; with RDKit present chem.py's path is unchanged.
    graph_stereo: True (opt-in; needs graph_smiles) = that SMILES carries '@' / '@@' at the marked carbons that a wedge begins at
    (mnx_smiles_pack_stereo: this library's own rule after OpenSMILES, not RDKit's; not canonical).
    graph_double_bonds: True (opt-in; needs graph_smiles) = that SMILES carries '/' and '\\' at the double bonds off every cycle
    that the coordinates resolve (mnx_smiles_pack_marks: this library's own rule after OpenSMILES, not RDKit's; no toolkit has
    parsed it here; double bonds on a cycle and symmetry are not handled).
    graph_canonical: True (opt-in; needs graph_smiles; combines with graph_stereo / graph_double_bonds) = that SMILES is written
    on canonical atom ranks (mnx_smiles_pack_canonical), so it does not depend on the order in which the decoder emitted the
    atoms of a drawing, and every output dict gains 'canonical_rank' and 'symmetry_class', a list per atom (None for a
    molecule that was not ranked). This library's own ranking: NOT RDKit's canonical SMILES (no toolkit has parsed it, and it
    never compares with a toolkit's string); the known limit of include/molnextr_hip.h applies — a few graphs whose string
    still depends on the drawing.
    graph_symmetry: True (opt-in, default False; needs graph_smiles and graph_canonical) = the marks of that SMILES pass the
    symmetry rule of mnx_smiles_pack_symmetric (a centre or double bond with two substituents of one symmetry class, both on
    bonds off every cycle, writes no mark), and every output dict gains 'stereo_atoms', the ATOM_* bits per atom (None for a
    molecule that got no string). Off for a molecule with a pseudo-atom (combine with graph_expand); the ranks ignore stereo, a
    pair on ring bonds is never dropped, and no toolkit has parsed the result: the limits stand in include/molnextr_hip.h.
    graph_normalize: True (opt-in, default False; needs graph_smiles or graph_molfile; behind graph_expand) = the molecule gets one
    normal spelling per atom before it is written (mnx_normalize_pack: aromatic rings of 5 and 6 atoms perceived from a Kekule
    drawing, brackets dropped where a reader infers them), and every output dict gains 'hydrogens', the H count per atom (in the
    order of expanded['symbols'] with graph_expand, of atom_sets without), and 'normalized' (symbols, bonds, notes, flags). This
    library's own rule, NOT RDKit's aromaticity model; no toolkit has checked it.
    graph_kekulize: True (opt-in, default False; needs graph_smiles or graph_molfile; behind graph_expand, in front of
    graph_normalize) = every aromatic system that has a Kekule structure is written as one before the molecule is written
    (mnx_kekulize_pack), so the molfile of an aromatic prediction carries bond types 1 and 2 in the place of the query type 4,
    and every output dict gains 'kekulized' (symbols, bonds, hydrogens, notes, flags). A Kekule structure is a perfect
    matching; the choice among several is this library's own search order, NOT RDKit's Kekulize, and a system without a
    matching stays aromatic (flags & MOL_KEKULE_LEFT).
    graph_formula: True (opt-in, default False; needs graph_smiles or graph_molfile; in front of graph_expand) = a condensed-formula
    label that is in neither name table ('CH2CH3', 'N(CH3)2', 'COOCH3', 'CH2Ph') is replaced by the atoms and bonds a
    valence-guided search finds for it before anything is written (mnx_formula_pack), and every output dict gains 'formula'
    (symbols, coords, bonds, origin, flags, and 'replaced' / 'left': the predicted atoms whose label was replaced / stayed). This
    library's own repair of the reference's search: no toolkit has parsed the result, rings, charges, explicit bonds and
    two-ended labels stay labels; combine with graph_expand for the group tokens a formula holds ('Ph' in 'CH2Ph').
    graph_keep_main: True (opt-in, default False; needs graph_smiles or graph_molfile; behind graph_expand, in front of
    graph_kekulize) = only the connected component with the most atoms is written, among equals the one with the lowest atom
    (mnx_main_pack: the reference's _keep_main_molecule — salts, counter-ions and stray atoms are dropped), and every output
    dict gains 'main_atoms', the kept atoms' indices in the molecule the pass received (expanded['symbols'] with graph_expand,
    atom_sets without), and 'main' (symbols, coords, bonds, origin, flags). The per-atom lists then follow main['symbols'].
    graph_fingerprint: an attribute, set behind the constructor, whose parameter list is closed (`m.graph_fingerprint = True`;
    opt-in, default False; the results are put together on the device as with packed_results) = every output dict gains
    'fingerprint', 256 bytes: the 2048 bits of the paths of up to 7 bonds of the molecule behind the graph_* passes
    (mnx_fingerprint_pack through predict_fingerprints: this library's own rule, NOT RDKit's bits), None for a molecule that is
    refused or passes the step limit. molnextr.tanimoto compares SMILES strings by the same fingerprint.
    graph_substructure: an attribute like graph_fingerprint (`m.graph_substructure = ["c1ccccc1", "C(=O)O"]`; default None) = a
    list of query SMILES; every output dict gains 'substructure', per query {'matched', 'atoms', 'coords'}: whether the molecule
    behind the graph_* passes holds the query, under which of its atoms and where on the page (mnx_substructure_match through
    predict_substructures: this library's own rule, NOT RDKit's HasSubstructMatch and not SMARTS). molnextr.has_substructure asks
    the same of SMILES strings.
    graph_nearest: an attribute like graph_fingerprint (`m.graph_nearest = ["CCO", "c1ccccc1"]`, or model.smiles_library's dict made
    once with the graph_* passes that are on; default None) = a library of known compounds; every output dict gains 'nearest',
    the graph_nearest_k (an attribute, default 1, at most 64) compounds nearest to the molecule behind the graph_* passes as
    [{'index', 'smiles', 'similarity'}], [] for a molecule without a fingerprint (mnx_tanimoto_search through predict_nearest: this
    library's own fingerprint, NOT RDKit's). molnextr.nearest asks the same of SMILES strings."""

    image_format = "fp32"
    packed_results = False
    graph_molfile = False
    graph_smiles = False
    graph_stereo = False
    graph_double_bonds = False
    graph_canonical = False
    graph_symmetry = False
    graph_expand = False
    graph_normalize = False
    graph_kekulize = False
    graph_formula = False
    graph_keep_main = False
    graph_fingerprint = False
    graph_substructure = None
    graph_nearest = None
    graph_nearest_k = 1

    def __init__(self, model_path, device=None, max_batch: int = 32, dtype: str = DEFAULT_DTYPE,
                 device_preprocess: bool = True, image_format: str = "fp32", packed_results: bool = False,
                 graph_molfile: bool = False, graph_smiles: bool = False, graph_stereo: bool = False,
                 graph_double_bonds: bool = False, graph_canonical: bool = False, graph_expand: bool = False,
                 graph_symmetry: bool = False, graph_normalize: bool = False, graph_kekulize: bool = False,
                 graph_formula: bool = False, graph_keep_main: bool = False):
        if model_path is None:
            raise ValueError("molnextr(model_path): a checkpoint path is required (pass 'synthetic' explicitly for the "
                             "deterministic test checkpoint)")
        if model_path == "synthetic":
            states = W.synthetic_checkpoint(0)
        else:
            from .checkpoint import load_checkpoint      # .pth in the reference format or our .safetensors; strict
            states = load_checkpoint(model_path)
        args = self._get_args(states.get("args"))
        if device is None:
            device = torch.device("cuda", 0)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("molnextr_amd runs the model on an MI355X only (no CPU path); pass device='cuda:N'")
        self.device = device
        self.args = args
        self.tokenizer = get_tokenizer(args)
        self._states, self._max_batch = states, max_batch      # kept for the operand-range fallback (_with_fallback)
        if image_format not in ("fp32", "gray8"):
            raise ValueError(f"image_format must be 'fp32' or 'gray8', got {image_format!r}")
        self.image_format = image_format
        self.packed_results = bool(packed_results)
        self.graph_molfile = bool(graph_molfile)
        self.graph_smiles = bool(graph_smiles)
        self.graph_stereo = bool(graph_stereo)
        if self.graph_stereo and not self.graph_smiles:
            raise ValueError("graph_stereo=True needs graph_smiles=True: the marks are written into the graph SMILES")
        self.graph_double_bonds = bool(graph_double_bonds)
        if self.graph_double_bonds and not self.graph_smiles:
            raise ValueError("graph_double_bonds=True needs graph_smiles=True: the marks are written into the graph SMILES")
        self.graph_canonical = bool(graph_canonical)
        if self.graph_canonical and not self.graph_smiles:
            raise ValueError("graph_canonical=True needs graph_smiles=True: the ranks order the graph SMILES")
        self.graph_symmetry = bool(graph_symmetry)
        if self.graph_symmetry and not (self.graph_smiles and self.graph_canonical):
            raise ValueError("graph_symmetry=True needs graph_smiles=True and graph_canonical=True: the rule reads the symmetry classes")
        for name, given in (("expand", graph_expand), ("normalize", graph_normalize), ("kekulize", graph_kekulize),
                            ("formula", graph_formula), ("keep_main", graph_keep_main)):       # the order they are reported in
            setattr(self, "graph_" + name, bool(given))
            if given and not (self.graph_smiles or self.graph_molfile):
                raise ValueError(f"graph_{name}=True needs graph_smiles=True or graph_molfile=True: {BY_NAME[name].written} is what they write")
        self.engine = Engine(states["encoder"], states["decoder"], device=device.index or 0, max_batch=max_batch,
                             dtype=dtype, image_format=image_format)
        self.input_size = args.input_size
        self.device_preprocess = device_preprocess
        self.group_images = 1024          # images per engine call of the throughput path (whole reference batches)

    def canonical_smiles(self, smiles_list, expand: bool = False, normalize: bool = False, kekulize: bool = False,
                         formula: bool = False, keep_main: bool = False) -> List[dict]:
        """The canonical graph SMILES of the caller's own strings, for comparison with 'predicted_smiles' of graph_canonical=True
        (model.canonical_smiles: read on the device, optionally expanded and normalised, written without marks)."""
        given = {"expand": expand, "normalize": normalize, "kekulize": kekulize, "formula": formula, "keep_main": keep_main}
        return canonical_smiles(self.engine, smiles_list, **{name: True for name, v in given.items() if v})

    def canonical_molfiles(self, molfiles, **options) -> List[dict]:
        """The canonical graph SMILES of the caller's own V2000 molfiles, with the stereo marks their wedges and coordinates
        resolve when stereo / double_bonds are given (model.canonical_molfiles, whose options these are)."""
        return canonical_molfiles(self.engine, molfiles, **options)

    def tanimoto(self, smiles_a, smiles_b, **passes) -> List[float]:
        """The similarity of two lists of SMILES, item by item, by this library's path fingerprint (model.tanimoto; passes:
        smiles_fingerprints' options). NOT RDKit's fingerprint."""
        return tanimoto(self.engine, smiles_a, smiles_b, **passes)

    def nearest(self, smiles_list, library, k: int = 1, **passes) -> List[list]:
        """Per string of smiles_list its k nearest strings of `library` (a list of SMILES, or model.smiles_library's dict) as
        [{'index', 'smiles', 'similarity'}] (model.nearest_smiles; passes: its options). NOT RDKit's fingerprint."""
        return nearest_smiles(self.engine, smiles_list, library, k=k, **passes)

    def has_substructure(self, smiles_list, query, **passes) -> List:
        """Per string of smiles_list whether it holds the query SMILES: True, False, or None where a string was not read or the
        search gave no answer (model.smiles_substructure; passes: its options). NOT RDKit's HasSubstructMatch."""
        return [item["matched"] for item in smiles_substructure(self.engine, [query], smiles_list, **passes)]

    _groups_done = 0          # groups of the running predict_images call that have produced predictions

    def _with_fallback(self, job):
        """job(engine) -> result. When the engine reports that an activation left the fp16 range of its operand mode
        (MNX_ERR_RANGE: possible with fp16x3 / fp16 on checkpoints with very large activations), the engine is rebuilt ONCE
        in the corresponding bf16 mode (fp32 exponent range) with a warning and the job runs again; the instance keeps the
        new engine. The reference runs such a checkpoint without complaint, so the drop-in must too."""
        try:
            return job(self.engine)
        except MnxError as e:
            to = range_fallback_dtype(e, self.engine.dtype)
            if to is None:
                raise
            import warnings
            warnings.warn(f"molnextr_amd: an encoder activation left the fp16 range of operand mode '{self.engine.dtype}' "
                          f"({e}); rebuilding the engine with dtype='{to}' and repeating the batch", RuntimeWarning)
            self._rebuild_engine(dtype=to)  # joins the helper of group g + 1: it may still be inside mnx_preprocess on this handle
            if self._groups_done:
                # earlier groups of this predict_images call were computed in the fp16 mode: one call, one operand mode —
                # the call starts again from its first image (predict_images catches this)
                raise _RestartCall()
            return job(self.engine)

    def _rebuild_engine(self, max_batch=None, dtype=None):
        """Replaces the engine by one with this max_batch / operand mode (the others kept). The prefetch helper works on
        the current engine, so it is joined before that engine is closed."""
        dev, dtype = self.engine.device, dtype or self.engine.dtype
        if max_batch is not None:
            self._max_batch = max_batch
        self._join_prefetch()
        self.engine.close()
        self.engine = Engine(self._states["encoder"], self._states["decoder"], device=dev, max_batch=self._max_batch,
                             dtype=dtype, image_format=self.image_format)

    @staticmethod
    def _get_args(args_states=None):
        """Inference defaults of the reference (model.py:50-81) overridden by the checkpoint's saved args."""
        a = argparse.Namespace(encoder="swin_base", decoder="transformer", enc_pos_emb=False, dec_num_layers=6,
                               dec_hidden_size=256, dec_attn_heads=8, continuous_coords=False,
                               compute_confidence=False, input_size=384, vocab_file=None, coord_bins=64, sep_xy=True,
                               formats=["chartok_coords", "edges"])
        for k, v in (args_states or {}).items():
            setattr(a, k, v)
        if a.encoder != "swin_base" or a.input_size != 384 or a.continuous_coords:
            raise NotImplementedError("engine is built for the swin_base / 384 / discrete-coordinate configuration")
        return a

    def _transform(self, images: List, engine=None) -> torch.Tensor:
        """CropWhite + Resize + ToGray + Normalize (reference model.py:104): on the device (mnx_preprocess), or with the
        bit-identical host restatement when `device_preprocess` is off. The result is a torch tensor of integer-exact
        arithmetic: it does not depend on the engine's operand mode and outlives the engine that made it."""
        if self.device_preprocess:
            return (engine or self.engine).preprocess(images)      # the engine carries the image format
        host = transform_image_gray if self.image_format == "gray8" else transform_image
        return torch.from_numpy(np.stack([host(im, self.input_size) for im in images])).to(self.device)

    _prefetch_thread = None       # the helper thread of the running _prefetched generator, if one is in flight

    def _join_prefetch(self):
        """Waits for the prefetch helper (if any). Called before the engine it works on is closed (_with_fallback)."""
        t = self._prefetch_thread
        if t is not None:
            t.join()

    def _side_context(self):
        """The context the prefetch helper runs in: this device, a side stream (a seam for the CPU tests)."""
        import contextlib
        stack = contextlib.ExitStack()
        stack.enter_context(torch.cuda.device(self.device))
        stack.enter_context(torch.cuda.stream(torch.cuda.Stream(device=self.device)))
        return stack

    def _prefetched(self, groups: List[List]):
        """Yields the transformed tensor of every group; group g+1 is uploaded (pinned staging -> H2D) and transformed on a
        side stream by a helper thread while the caller runs the engine on group g (reference main.py gets the same
        overlap from DataLoader workers + pin_memory). `mnx_preprocess` is the one entry point that may run beside
        another call on the same handle (include/molnextr_hip.h) — ONE such call: at most one helper exists at a time, it
        works on the engine that was current when it was started, and whoever replaces that engine joins the helper first
        (_with_fallback -> _join_prefetch); closing the generator (a call that is abandoned and restarted) joins it too."""
        if len(groups) <= 1 or not self.device_preprocess:
            for g in groups:
                yield self._transform(g)
            return
        import threading

        def work(g, box, engine):
            try:
                with self._side_context():
                    box.append(self._transform(g, engine))      # Engine.preprocess synchronises the side stream before returning
            except BaseException as e:  # noqa: BLE001 - re-raised in the caller's thread
                box.append(e)

        def start(g):
            box: list = []
            t = threading.Thread(target=work, args=(g, box, self.engine), daemon=True)
            self._prefetch_thread = t
            t.start()
            return t, box

        t, box = start(groups[0])
        try:
            for gi in range(len(groups)):
                t.join()
                item = box.pop()
                if isinstance(item, BaseException):
                    raise item
                if gi + 1 < len(groups):
                    t, box = start(groups[gi + 1])
                yield item
        finally:
            t.join()
            self._prefetch_thread = None

    def predict_images(self, input_images: List, return_atoms_bonds=False, return_confidence=False, batch_size=16):
        if len(input_images) == 0:
            return []                                      # reference model.py:101-102: empty loop, empty list
        try:
            self._groups_done = 0
            preds = self._predict_all(input_images, return_confidence, batch_size)
        except _RestartCall:                               # the engine was rebuilt in the bf16 split mode after some groups
            self._groups_done = 0
            preds = self._predict_all(input_images, return_confidence, batch_size)
        finally:
            self._groups_done = 0
        return self._assemble(preds, input_images, return_atoms_bonds, return_confidence)

    def predict_coords(self, input_images: List, smiles_list: List[str], return_confidence=False, batch_size=16):
        """Coordinate prediction for KNOWN structures (the reference's main.py --predict_coords): image i is decoded along
        smiles_list[i] tokenised with mask_ratio=1 (dataset.py:459-464) and cut to max_len ids (dataset.py:473), so the model
        fills in every atom's x and y and the bond head reads the hidden states of that guided pass. Returns predict_images'
        dicts with 'atom_sets' and 'bond_sets' always present. Greedy only; both image formats; the same grouping, prefetch
        and range fallback as predict_images. A label that the cut shortened has lost its '<eos>': that row alone is passed on
        as free-running (it ends at max_len); every other row goes through the engine's refusal of labels without '<eos>'."""
        if len(input_images) != len(smiles_list):
            raise ValueError(f"input_images and smiles_list must have the same length; got {len(input_images)} and {len(smiles_list)}")
        if len(input_images) == 0:
            return []
        tok = self.tokenizer["chartok_coords"]
        max_len = self.engine.max_len
        labels, cut = coords_labels(tok, smiles_list, max_len)
        try:
            self._groups_done = 0
            preds = self._predict_all(input_images, return_confidence, batch_size, labels, cut)
        except _RestartCall:
            self._groups_done = 0
            preds = self._predict_all(input_images, return_confidence, batch_size, labels, cut)
        finally:
            self._groups_done = 0
        return self._assemble(preds, input_images, True, return_confidence)

    def _predict_all(self, input_images: List, return_confidence: bool, batch_size: int, labels=None, cut=None) -> List[dict]:
        """The engine part of predict_images: one prediction dict per image, every group in ONE operand mode.
        labels [n, L], cut [n] (coords_labels): label-guided (predict_coords); each group takes its rows."""
        preds: List[dict] = []
        batch_size = min(batch_size, len(input_images))     # a batch larger than the job is the whole job: same numbering
        if batch_size < 1 or batch_size > MAX_REF_BATCH:
            # results depend on the row inside the reference batch (positional-encoding quirk), so a silently
            # different batch size would silently change tokens
            raise ValueError(f"batch_size must be 1..{MAX_REF_BATCH} (one reference batch is decoded as one unit); got {batch_size}")
        if batch_size > self.engine.max_batch:
            # a reference batch is encoded in one launch group: grow the engine once (the encoder is bitwise batch-invariant,
            # so results do not depend on max_batch)
            self._rebuild_engine(max_batch=-(-batch_size // ROWS) * ROWS)
        # throughput path: many images per engine call, reference batches of `batch_size` kept as numbering units;
        # the group is a whole number of reference batches so that batch boundaries do not drift between groups
        group = (self.group_images // batch_size) * batch_size
        groups = [input_images[i:i + group] for i in range(0, len(input_images), group)]
        conf = {"compute_confidence": True} if return_confidence else {}
        if (self.packed_results or self.graph_molfile or self.graph_smiles or self.graph_fingerprint or self.graph_substructure is not None
                or self.graph_nearest is not None):
            conf["packed"] = True
        if self.graph_smiles:
            conf["smiles"] = True
            conf["stereo"] = self.graph_stereo
            if self.graph_double_bonds:
                conf["double_bonds"] = True
            if self.graph_canonical:
                conf["canonical"] = True
            if self.graph_symmetry:
                conf["symmetry"] = True
        conf.update({row.name: True for row in PASSES if getattr(self, "graph_" + row.name)})      # a flag travels only when it is on
        if self.graph_nearest is not None:                    # a list is read and fingerprinted once per call, not once per group
            library = self.graph_nearest if isinstance(self.graph_nearest, dict) else smiles_library(
                self.engine, self.graph_nearest, **{row.name: True for row in PASSES if row.name in conf})
            conf["nearest"] = (library, int(self.graph_nearest_k), 0.0)
        gen = self._prefetched(groups)
        try:
            for x in gen:
                if self.graph_molfile:
                    pages = input_images[len(preds):len(preds) + x.shape[0]]
                    conf.update(molfile=True, molfile_scale=[page_scale(im) for im in pages])
                if labels is not None:
                    rows = slice(len(preds), len(preds) + x.shape[0])
                    conf.update(labels=labels[rows], free_run=cut[rows])
                if self.graph_substructure is not None:       # predict_fingerprints' key travels as an option of this route
                    job = lambda eng: predict_substructures(eng, x, list(self.graph_substructure), self.tokenizer, ref_batch_size=batch_size,  # noqa: E731
                                                            **({"fingerprint": True} if self.graph_fingerprint else {}), **conf)
                elif "nearest" in conf and not self.graph_fingerprint:    # on either route above predict_nearest's key travels in conf
                    rest = {key: v for key, v in conf.items() if key != "nearest"}
                    job = lambda eng: predict_nearest(eng, x, *conf["nearest"], self.tokenizer, ref_batch_size=batch_size, **rest)  # noqa: E731
                else:
                    job = lambda eng: (predict_fingerprints if self.graph_fingerprint else predict_pipeline)(  # noqa: E731
                        eng, x, self.tokenizer, ref_batch_size=batch_size, **conf)
                preds += self._with_fallback(job)
                self._groups_done += 1
        finally:
            if hasattr(gen, "close"):
                gen.close()         # a call abandoned by _RestartCall leaves no helper thread behind
        return preds

    def _assemble(self, preds: List[dict], input_images: List, return_atoms_bonds: bool, return_confidence: bool):
        """Output dicts of predict_images (reference model.py:111-196) from the per-image predictions."""
        from .chem import convert_graph_to_smiles, have_rdkit
        packed = bool(preds) and "bonds" in preds[0]          # predictions of predict_pipeline(packed=True): bond records
        if not packed:
            edges = [p["edges"] for p in preds]
        elif have_rdkit():                                    # chem.py reads edges[i][j] for i < j only: the upper triangle
            edges = []
            for p in preds:
                k = len(p["chartok_coords"]["symbols"])
                e = [[0] * k for _ in range(k)]
                for b in p["bonds"]:
                    e[b[0]][b[1]] = b[2]
                edges.append(e)
        else:
            edges = [None] * len(preds)
        smiles_list, molblock_list, _ = convert_graph_to_smiles(
            [p["chartok_coords"]["coords"] for p in preds], [p["chartok_coords"]["symbols"] for p in preds],
            edges, images=input_images)
        outputs = []
        for smiles, molfile, pred in zip(smiles_list, molblock_list, preds):
            if molfile is None:                               # no RDKit: the device's own molfile, when it was asked for
                molfile = pred.get("molfile")
            if smiles is None and not have_rdkit():           # no RDKit: the device's graph SMILES, when it was asked for
                smiles = pred.get("graph_smiles")
            d = {"predicted_smiles": smiles, "predicted_molfile": molfile}
            if "canonical_rank" in pred:                      # graph_canonical: per atom, in the order of atom_sets
                d["canonical_rank"], d["symmetry_class"] = pred["canonical_rank"], pred["symmetry_class"]
            if "stereo_atoms" in pred:                        # graph_symmetry: per atom, as the ranks
                d["stereo_atoms"] = pred["stereo_atoms"]
            for row in PASSES:                                # graph_<name>: the molecule as it left that pass; the ranks follow
                if row.key in pred:                           # the atoms of the last one that adds or drops any, not atom_sets
                    d[row.key] = pred[row.key]
            if "normalized" in pred:                          # graph_normalize: per atom of the molecule that was written
                d["hydrogens"] = pred["normalized"]["hydrogens"]
            if "main" in pred:                                # graph_keep_main: where the main molecule's atoms came from
                d["main_atoms"] = pred["main"]["origin"]
            if "fingerprint" in pred:                         # graph_fingerprint: 256 bytes, None when refused or limited
                d["fingerprint"] = pred["fingerprint"]
            if "substructure" in pred:                        # graph_substructure: per query matched / atoms / coords
                d["substructure"] = pred["substructure"]
            if "nearest" in pred:                             # graph_nearest: the nearest known compounds, index / smiles / similarity
                d["nearest"] = pred["nearest"]
            if return_atoms_bonds:
                c = pred["chartok_coords"]
                atoms = []
                for i, (sym, xy) in enumerate(zip(c["symbols"], c["coords"])):
                    a = {"atom_number": f"{i}", "atom_symbol": sym, "coords": (round(xy[0], 3), round(xy[1], 3))}
                    if return_confidence:
                        a["confidence"] = c["atom_scores"][i]
                    atoms.append(a)
                d["atom_sets"] = atoms
                if packed:                                    # one record per bond already, in the pair loop's order
                    d["bond_sets"] = [
                        {"atom_number": f"{b[0]}", "bond_type": BOND_TYPES[b[2]], "endpoints": (b[0], b[1]),
                         **({"confidence": b[4]} if return_confidence else {})} for b in pred["bonds"]]
                    outputs.append(d)
                    continue
                bonds = []
                k = len(c["symbols"])
                for i in range(k - 1):
                    for j in range(i + 1, k):
                        t = pred["edges"][i][j]
                        if t != 0:
                            bd = {"atom_number": f"{i}", "bond_type": BOND_TYPES[t], "endpoints": (i, j)}
                            if return_confidence:
                                bd["confidence"] = pred["edge_scores"][i][j]
                            bonds.append(bd)
                d["bond_sets"] = bonds
            outputs.append(d)
        return outputs

    def predict_image(self, image, return_atoms_bonds=False, return_confidence=False):
        return self.predict_images([image], return_atoms_bonds, return_confidence)[0]

    def predict_image_files(self, image_files: List, return_atoms_bonds=False, return_confidence=False):
        return self.predict_images([load_image_rgb(p) for p in image_files], return_atoms_bonds, return_confidence)

    def predict_final_results(self, image_file: str, return_atoms_bonds=False, return_confidence=False):
        return self.predict_image_files([image_file], return_atoms_bonds, return_confidence)[0]
