"""Evaluation harness around the device path: the reference's `inference()` / `valid_fn()` driver
(reference main.py:259-303, 429-532) and the prediction CSV that `evaluate.py` consumes (reference evaluate.py:157-218,
MolNexTR/utils.py:145-163).

What is mirrored:
  * sharding: `DistributedSampler(dataset, shuffle=False)` (main.py:440-441) — rank r takes indices r, r+W, r+2W, ...
    of the list padded (by wrapping around) to a multiple of W; per-rank batches of `batch_size * 2` (main.py:445).
    These batches ARE part of the parity contract (the decoder's positional encoding depends on the row inside the
    batch), so the harness hands exactly them to the engine as reference batches;
  * gather: fixed-size records through one all-gather (molnextr_amd/shard.py) instead of `all_gather_object`
    (main.py:295-301); padded duplicates overwrite themselves, as in the reference;
  * output: `prediction_<file>.csv` with image_id, SMILES, node_coords, node_symbols, edges (+ graph_SMILES /
    post_SMILES when RDKit is importable), lists serialised like `format_df` (3-decimal floats, no spaces), and
    `eval_scores_<file>.json`.
Scores: with RDKit the reference's canonicalised exact-match family; without it (this image) only a raw string match
is reported and labelled as such.

    python -m molnextr_amd.evaluate --data_path data --test_file real/acs.csv --save_path out --batch_size 4 \\
           [--load_path ckpt.pth] (under torchrun for several GPUs)
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import shard
from .tokenizer import coords_labels, get_tokenizer


def sampler_indices(n: int, rank: int, world: int) -> List[int]:
    """torch DistributedSampler(shuffle=False, drop_last=False): pad by wrapping around, then stride by world."""
    if n == 0:
        return []
    per = -(-n // world)
    total = per * world
    idx = list(range(n))
    pad = total - n
    if pad:
        idx += (idx * (-(-pad // n)))[:pad]
    return idx[rank:total:world]


def reference_batches(indices: Sequence[int], batch_size: int) -> List[List[int]]:
    """DataLoader(batch_size=batch_size * 2, drop_last=False) over the rank's indices (main.py:443-451)."""
    step = batch_size * 2
    return [list(indices[i:i + step]) for i in range(0, len(indices), step)]


def round_floats(o):
    if isinstance(o, float):
        return round(o, 3)
    if isinstance(o, dict):
        return {k: round_floats(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [round_floats(x) for x in o]
    return o


def dumps_field(obj) -> Optional[str]:
    """One cell of node_coords / node_symbols / edges, as `format_df` writes it (utils.py:155-163)."""
    if obj is None:
        return None
    return json.dumps(round_floats(obj)).replace(" ", "")


PAD_TO_SQUARE_FILES = ("real/acs.csv", "real/UOB.csv")     # reference dataset.py:163-164


class PeerFailed(RuntimeError):
    """Raised by run_inference on the ranks that were fine when ANOTHER rank failed with an error that has no fallback
    (capacity, I/O, a HIP error): every rank leaves together instead of waiting in the gather for a peer that is gone."""


class RangeFallback(RuntimeError):
    """Raised by run_inference on EVERY rank when any rank's encoder left the fp16 range of the operand mode: the caller
    rebuilds its engine in the fallback mode (abi.RANGE_FALLBACK) and repeats the whole evaluation."""


MAX_BATCH_SIZE = 256      # --batch_size: per-rank reference batches of 2 x 256 = 512 rows (Engine.MAX_REF_BATCH)


def run_inference(engine, load_image: Callable[[int], np.ndarray], n_items: int, batch_size: int, rank: int = 0,
                  world: int = 1, tokenizer=None, group: int = 512, pad_to_square: bool = False,
                  smiles: Optional[Sequence[str]] = None, keep_records: Optional[dict] = None) -> Dict[int, dict]:
    """valid_fn for this rank's shard, then the gather: returns {dataset index: prediction dict} on every rank
    (the reference keeps it on all ranks too, main.py:295-301). `engine`: molnextr_amd.engine.Engine.
    pad_to_square: the PadToSquare step `get_transforms` inserts for the test files in PAD_TO_SQUARE_FILES.
    smiles: the known structure of every item (main.py --predict_coords): item i is decoded along
    smiles_to_sequence(smiles[i], mask_ratio=1) cut to max_len ids (dataset.py:459-464,473), label-guided. Only a row
    that the cut shortened, and so lost its '<eos>', is passed on as free-running; every other row goes through the
    engine's refusal of labels without '<eos>'.
    keep_records: a dict that receives 'records', the gathered dense records int32 [n_items, shard.record_words(kmax)] in
    dataset order (graph_match_scores re-uploads them)."""
    tok = (tokenizer or get_tokenizer())["chartok_coords"]
    ref_batch = batch_size * 2
    cap = getattr(engine, "MAX_REF_BATCH", engine.ROWS_PER_DECODE)     # rows of one reference batch on the greedy path
    if ref_batch > cap:
        raise ValueError(f"per-rank batches of {ref_batch} exceed the engine's reference-batch capacity "
                         f"({cap}); use --batch_size <= {cap // 2}")
    mine = sampler_indices(n_items, rank, world)
    kmax = engine.max_atoms
    recs = []
    step = max(group // ref_batch, 1) * ref_batch          # whole reference batches per engine call
    dev = getattr(engine, "torch_device", None) or torch.device("cuda", engine.device)
    # An activation beyond the fp16 range of the operand mode ends THIS rank's shard with MNX_ERR_RANGE. Every rank must then
    # repeat its shard in the fallback mode — one predictions table must not mix operand modes, and a rank that restarts
    # alone would leave its peers waiting in the gather —, so the ranks agree on "somebody saw a range error" (one scalar
    # all-reduce MAX) BEFORE the gather and raise together.
    # ANY other failure of one rank (capacity, a missing image file, a HIP error) must not leave its peers in that collective
    # either: the ranks exchange a status code — 0 ok, 1 range error, 2 fatal — and the fatal rank re-raises its own error
    # after the exchange, the others raise PeerFailed.
    from .abi import MnxError, range_fallback_dtype
    range_err, fatal = None, None
    try:
        for g0 in range(0, len(mine), step):
            ids = mine[g0:g0 + step]
            x = engine.preprocess([load_image(i) for i in ids], pad_to_square=pad_to_square)
            guide = {}
            if smiles is not None:
                lab, cut = coords_labels(tok, [smiles[i] for i in ids], engine.max_len)
                guide = {"labels": lab, "free_run": cut}      # a label cut at max_len has no '<eos>': its row ends at max_len
            out = engine.predict(x, ref_batch=ref_batch, **guide)
            recs.append(shard.pack_records_device(out["tokens"], out["lengths"], out["atom_idx"], out["n_atoms"],
                                                  out["edges"]))
    except MnxError as err:
        if range_fallback_dtype(err, getattr(engine, "dtype", None)) is None:
            fatal = err
        else:
            range_err = err
    except BaseException as err:  # noqa: BLE001 - re-raised below, after the peers have been told
        fatal = err
    mine_status = 2 if fatal is not None else (1 if range_err is not None else 0)
    status = shard.max_over_ranks(mine_status, dev) if world > 1 else mine_status
    if fatal is not None:
        raise fatal
    if status == 2:
        raise PeerFailed("another rank failed during inference; this rank leaves before the gather")
    if status == 1:
        raise RangeFallback(str(range_err) if range_err is not None else "another rank's encoder left the fp16 operand range")
    rec = torch.cat(recs) if recs else torch.zeros(0, shard.record_words(kmax), dtype=torch.int32, device=dev)
    index = torch.tensor(mine, dtype=torch.int32, device=dev).view(-1, 1)
    rec = torch.cat([index, rec], dim=1).contiguous()      # the dataset index travels with its record
    if world > 1:
        rec = shard.gather_records(rec)
    rec = rec.cpu().numpy()
    preds: Dict[int, dict] = {}
    rows = shard.unpack_records(torch.from_numpy(np.ascontiguousarray(rec[:, 1:])), kmax)
    for r, row in enumerate(rows):
        preds[int(rec[r, 0])] = {"chartok_coords": tok.sequence_to_smiles(row["tokens"]), "edges": row["edges"]}
    if keep_records is not None:
        dense = np.zeros((n_items, rec.shape[1] - 1), dtype=np.int32)
        dense[rec[:, 0]] = rec[:, 1:]                       # padded duplicates overwrite themselves
        keep_records["records"] = dense
    return preds


def predictions_table(image_ids: Sequence, preds: Dict[int, dict]) -> Dict[str, list]:
    """Columns of the reference's pred_df (main.py:466-487), already serialised with `format_df`."""
    from .chem import convert_graph_to_smiles, have_rdkit
    rows = [preds[i] for i in range(len(image_ids))]
    coords = [p["chartok_coords"]["coords"] for p in rows]
    symbols = [p["chartok_coords"]["symbols"] for p in rows]
    edges = [p["edges"] for p in rows]
    table = {"image_id": list(image_ids), "SMILES": [p["chartok_coords"]["smiles"] for p in rows],
             "node_coords": [dumps_field(c) for c in coords], "node_symbols": [dumps_field(s) for s in symbols],
             "edges": [dumps_field(e) for e in edges]}
    if have_rdkit():
        table["graph_SMILES"] = convert_graph_to_smiles(coords, symbols, edges)[0]
    return table


def smiles_scores(gold: Sequence[str], pred: Sequence[str]) -> Dict[str, float]:
    """evaluate.py's SmilesEvaluator needs RDKit canonicalisation; without RDKit only the raw string match exists."""
    from .chem import have_rdkit
    gold, pred = list(gold), list(pred)
    out = {"raw_string_match": float(np.mean([g == p for g, p in zip(gold, pred)])) if gold else 0.0}
    if have_rdkit():  # pragma: no cover - rdkit is absent in the build image
        from rdkit import Chem

        def canon(s, chiral):
            try:
                m = Chem.MolFromSmiles(s)
                return Chem.MolToSmiles(m, isomericSmiles=chiral) if m is not None else ""
            except Exception:  # noqa: BLE001
                return ""
        g1 = [canon(s, True) or "<empty>" for s in gold]
        out["canon_smiles"] = float(np.mean([a == canon(b, True) for a, b in zip(g1, pred)]))
        g0 = [canon(s, False) or "<empty>" for s in gold]
        out["graph"] = float(np.mean([a == canon(b, False) for a, b in zip(g0, pred)]))
    return out


def write_predictions(save_path: str, file_name: str, table: Dict[str, list], scores: Optional[dict] = None,
                      tag: str = "best") -> str:
    import pandas as pd
    os.makedirs(save_path, exist_ok=True)
    base = os.path.basename(file_name)
    out_csv = os.path.join(save_path, f"prediction_{base}")
    pd.DataFrame(table).to_csv(out_csv, index=False)
    if scores is not None:
        with open(os.path.join(save_path, f"eval_scores_{os.path.splitext(base)[0]}_{tag}.json"), "w") as f:
            json.dump(scores, f)
    return out_csv


def graph_match_scores(engine, records: np.ndarray, gold: Sequence[str], chunk: int = 512, normalize: bool = False,
                       kekulize: bool = False, formula: bool = False, keep_main: bool = False) -> Dict[str, float]:
    """--graph_match: the share of items whose prediction and gold string are the same graph as THIS library's canonical SMILES
    sees it (marks 0: no stereo), on the device. records: the gathered dense records in dataset order (shard.pack_records
    layout), re-uploaded in chunks -> graph_pack -> mnx_smiles_pack_canonical; gold -> mnx_smiles_read -> the same writer. A
    refused side is a mismatch. NOT the reference's RDKit `graph` score: nothing normalises [CH] against C, nothing kekulises,
    stereo is dropped, and the canonical ranks keep the limit DESIGN 4.15 states.
    normalize (--graph_normalize): adds graph_match_normalized, the same comparison with BOTH sides passed through
    mnx_normalize_pack first (this library's own aromaticity and bracket rule), so that a gold string in Kekule form
    or with [CH] spelled out equals an aromatic prediction of the same graph. graph_match_device is what it is without the
    flag. Still NOT the reference's RDKit `graph` score: the rule is not RDKit's model, nothing kekulises, rings of other sizes
    than 5 and 6 stay as drawn, stereo is dropped.
    kekulize (--graph_kekulize): adds graph_match_kekulized — BOTH sides pass through mnx_kekulize_pack, then
    mnx_normalize_pack, and are ranked then, so that an aromatic prediction equals a gold string in aromatic,
    Kekule or half-aromatic form, and an aromatic azulene equals its Kekule string although normalize finds no ring of 7. The
    other scores stay as they are. Still NOT the reference's RDKit `graph` score: the matching is this library's own search
    order and not RDKit's Kekulize, the aromaticity rule is not RDKit's model, stereo is dropped, and no toolkit has checked either.
    formula (--graph_formula): adds graph_match_formula — BOTH sides pass through mnx_formula_pack and then mnx_expand_pack and
    are ranked then, so that a predicted label 'CH2CH3' or 'COOCH3' equals a gold string that draws the group out,
    and a gold [Et] equals a predicted 'C2H5'. The other scores stay as they are. NOT the reference's RDKit `graph` score: the
    structure of a formula is this library's own repaired search, not the reference's RDKit bookkeeping, nothing normalises or
    kekulises here, stereo is dropped, and no toolkit has parsed the result.
    keep_main (--graph_keep_main): adds graph_match_main — the prediction goes graph_pack -> mnx_main_pack -> the canonical
    writer, so only its connected component with the most atoms (among equals the one with the lowest atom) is compared; the
    gold side is left as read, as in the reference, whose --keep_main trims predictions only. The other scores stay as they
    are. Only the component rule is the reference's (_keep_main_molecule): the comparison is still this
    project's canonical string and NOT the reference's RDKit `graph` score."""
    from .chain import run_chain
    from .abi import READ_REFUSED, SMILES_REFUSED
    gold = _gold_strings(gold, records)
    # the scores a flag adds: its name, the passes in front of the writer (chain.run_chain orders them), whether the gold side too
    extra = [row for row, given in ((("graph_match_normalized", ("normalize",), True), normalize),
                                    (("graph_match_kekulized", ("kekulize", "normalize"), True), kekulize),
                                    (("graph_match_formula", ("formula", "expand"), True), formula),
                                    (("graph_match_main", ("keep_main",), False), keep_main)) if given]
    equal = dict.fromkeys(["graph_match_device"] + [row[0] for row in extra], 0)
    unreadable = refused = 0

    def texts(rec, passes=()):
        recs, _, data, _, _ = engine.smiles_pack(run_chain(engine, rec, passes, keep_last=True)[1], canonical=True)
        return [None if int(r["flags"]) & SMILES_REFUSED else data[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in recs]

    def score(name, pred, want, read):
        equal[name] += sum(not int(r["flags"]) & READ_REFUSED and p is not None and w is not None and p == w
                           for p, w, r in zip(pred, want, read["read"]))

    for packed, read in _both_sides(engine, records, gold, chunk):
        pred, want = texts(packed), texts(read)
        unreadable += sum(bool(int(r["flags"]) & READ_REFUSED) for r in read["read"])
        refused += sum(p is None for p in pred)
        score("graph_match_device", pred, want, read)
        for name, passes, both in extra:
            score(name, texts(packed, passes), texts(read, passes) if both else want, read)
    return {"graph_match_device": equal.pop("graph_match_device") / len(gold) if gold else 0.0, "gold_unreadable": int(unreadable),
            "pred_refused": int(refused), **{name: e / len(gold) if gold else 0.0 for name, e in equal.items()}}


def _gold_strings(gold, records) -> List[str]:
    """the gold column as strings, an empty cell as the empty string; one per record"""
    gold = ["" if g is None or (isinstance(g, float) and np.isnan(g)) else str(g) for g in gold]
    assert len(gold) == len(records)
    return gold


def _both_sides(engine, records: np.ndarray, gold: Sequence[str], chunk: int):
    """Per chunk of the gathered dense records (shard.pack_records layout) and their gold strings: (the predictions through
    graph_pack, the strings through mnx_smiles_read), both with their tables on the device — what the scores of --graph_match
    compare."""
    from .shard import MAX_LEN
    kmax = engine.max_atoms
    dev = torch.device("cuda", engine.device)
    for c0 in range(0, len(gold), chunk):
        rows = torch.from_numpy(np.ascontiguousarray(records[c0:c0 + chunk])).to(dev)
        n = rows.shape[0]
        e32 = rows[:, 2 + MAX_LEN + kmax:].contiguous()
        out = {"lengths": rows[:, 0].contiguous(), "n_atoms": rows[:, 1].contiguous(), "tokens": rows[:, 2:2 + MAX_LEN].contiguous(),
               "atom_idx": rows[:, 2 + MAX_LEN:2 + MAX_LEN + kmax].contiguous(),
               "edges": e32.view(torch.uint8)[:, :kmax * kmax].reshape(n, kmax, kmax).contiguous()}
        yield engine.graph_pack(out, keep_device=True), engine.smiles_read(gold[c0:c0 + chunk], keep_device=True)


def graph_tanimoto_scores(engine, records: np.ndarray, gold: Sequence[str], chunk: int = 512, max_bonds: int = 0) -> Dict[str, float]:
    """--graph_tanimoto: the one graded score beside graph_match_scores' yes-or-no ones, on the same records and gold column (a
    function of its own: graph_match_scores' parameter list is closed). graph_tanimoto is the mean Tanimoto similarity of
    prediction against gold by this library's path fingerprint (mnx_fingerprint_pack, mnx_tanimoto: paths of up to max_bonds
    bonds, --graph_tanimoto_bonds, 0 = 7). BOTH sides pass through mnx_kekulize_pack and mnx_normalize_pack first, so
    that aromatic and Kekule spellings agree; a refused, unreadable or limited side scores 0. tanimoto_limited counts the sides
    that passed the step limit (FP_LIMIT). This is NOT the reference's RDKit `tanimoto` score: the reference only names the
    metric and the path length; the bits are this library's own and no toolkit has seen them."""
    from .chain import run_chain
    from .abi import FP_LIMIT
    gold = _gold_strings(gold, records)
    limited, similar = 0, []                                   # per item, summed once at the end: no chunk size changes a bit
    for sides in _both_sides(engine, records, gold, chunk):
        fps = [engine.fingerprint_pack(run_chain(engine, rec, ("kekulize", "normalize"), keep_last=True)[1], max_bonds=max_bonds,
                                       keep_device=True) for rec in sides]
        limited += sum(int(((fp["fp"]["flags"] & FP_LIMIT) != 0).sum()) for fp in fps)
        # a refused or limited side holds no bit and an unreadable gold string is the empty molecule: each scores 0 by itself
        similar += engine.tanimoto(fps[0]["bits"], fps[1]["bits"])["similarity"].tolist()
    return {"graph_tanimoto": math.fsum(similar) / len(gold) if gold else 0.0, "tanimoto_limited": int(limited)}


def graph_isomorphic_scores(engine, records: np.ndarray, gold: Sequence[str], chunk: int = 512, max_steps: int = 0) -> Dict[str, float]:
    """--graph_isomorphic: graph_match_kekulized's question asked of the graphs instead of a string, on the same records and gold
    column (a function of its own: graph_match_scores' parameter list is closed). BOTH sides pass through mnx_kekulize_pack and
    mnx_normalize_pack; graph_match_isomorphic is the share of items whose prediction and gold have equal atom and bond counts
    and embed in each other (model.same_graph's rule on the tables: mnx_substructure_match in both directions). It
    depends on no canonical ranking, so a correct prediction that the ranks' KNOWN LIMIT gives another string than its gold counts
    here. isomorphic_skipped counts the items that were not compared — a side of more than 64 atoms, a refused side, a search
    broken off at max_steps (0: MATCH_DEFAULT_STEPS) without a match —; they count as mismatches. An unreadable gold string is the
    empty molecule and a mismatch. This is NOT the reference's RDKit `graph` score: atoms and bonds are compared by this library's
    own rule (H counts and stereo are not compared), and no toolkit has checked it."""
    from .chain import run_chain
    from .graphs import _same_graph_tables
    gold = _gold_strings(gold, records)
    same = skipped = 0
    for sides in _both_sides(engine, records, gold, chunk):
        pred, want = (run_chain(engine, rec, ("kekulize", "normalize"), keep_last=True)[1] for rec in sides)
        yes, unknown = _same_graph_tables(engine, pred, want, max_steps)
        same += sum(yes)
        skipped += sum(unknown)
    return {"graph_match_isomorphic": same / len(gold) if gold else 0.0, "isomorphic_skipped": int(skipped)}


def build_parser() -> argparse.ArgumentParser:
    from .abi import DTYPES
    ap = argparse.ArgumentParser(description="MolNexTR test-set inference on MI355X (reference main.py --do_test)")
    ap.add_argument("--data_path", default=".")
    ap.add_argument("--test_file", required=True, help="CSV with file_path (and SMILES / image_id) columns")
    ap.add_argument("--save_path", default="predict_output")
    ap.add_argument("--load_path", required=True,
                    help="checkpoint: reference .pth or .safetensors; 'synthetic' = deterministic test weights")
    ap.add_argument("--batch_size", type=int, default=4,
                    help=f"per-GPU batch size, 1..{MAX_BATCH_SIZE} (main.py's default 256); inference uses twice that")
    ap.add_argument("--dtype", default=None, choices=sorted(DTYPES),
                    help="encoder operand mode; default abi.DEFAULT_DTYPE = fp16x3 (every token / atom / bond as the reference's fp32 path; "
                         "fp16x3m = qkv / fc1 / fc2 of Swin stage 3 on two product terms: faster, tokens exact on everything measured, raw logits up to "
                         "1.2e-3 off on a hostile checkpoint)")
    ap.add_argument("--fp16", action="store_true",
                    help="the reference's flag (main.py:40, exps/eval.sh: fp16 autocast): without --dtype it selects the one-plane "
                         "fp16 operand mode, which stays closer to the fp32 result than the reference's autocast path does "
                         "(tests/test_gpu_pixels.py, tests/golden/pixels_autocast_fp16.json)")
    ap.add_argument("--image_format", default="fp32", choices=["fp32", "gray8"],
                    help="what the transform hands to the encoder: fp32 = normalised [n,3,S,S], one mnx_preprocess per page; gray8 = "
                         "the gray byte per pixel, all pages of a group in one mnx_preprocess_batch (same predictions bit for bit)")
    ap.add_argument("--predict_coords", action="store_true",
                    help="the reference's main.py --predict_coords: the test file's SMILES column is the known structure of every "
                         "image; decoding is guided along it and only the atom coordinates are predicted. Writes image_id, SMILES "
                         "(the input string), node_coords (main.py:534-535)")
    ap.add_argument("--graph_match", action="store_true",
                    help="opt-in: add graph_match_device, gold_unreadable and pred_refused to the scores. Predictions (graph_pack) and "
                         "the SMILES column (mnx_smiles_read) are both written as this library's canonical SMILES without stereo marks "
                         "on the device and compared as strings; a refused side counts as a mismatch. This is NOT the reference's RDKit "
                         "`graph` score: no normalisation of [CH] against C, no kekulisation, no stereo, and the canonical ranks have "
                         "the known limit of DESIGN 4.15; no toolkit has parsed either string")
    ap.add_argument("--graph_normalize", action="store_true",
                    help="opt-in, with --graph_match: add graph_match_normalized, the same comparison with both sides passed through "
                         "mnx_normalize_pack first (aromatic rings of 5 and 6 atoms perceived from Kekule drawings, [CH] against C, N "
                         "against [nH]: this library's own rule, DESIGN 4.19). graph_match_device stays as it is. Still NOT the "
                         "reference's RDKit `graph` score: the rule is not RDKit's aromaticity model and no toolkit has checked it")
    ap.add_argument("--graph_kekulize", action="store_true",
                    help="opt-in, with --graph_match: add graph_match_kekulized, the same comparison with both sides passed through "
                         "mnx_kekulize_pack and then mnx_normalize_pack first, so that aromatic, Kekule and half-aromatic forms of one "
                         "molecule compare equal, rings of 7 included (DESIGN 4.20). The other scores stay as they are. Still NOT the "
                         "reference's RDKit `graph` score: the choice among Kekule structures is this library's own search order, not "
                         "RDKit's Kekulize, the aromaticity rule is not RDKit's model, and no toolkit has checked either")
    ap.add_argument("--graph_formula", action="store_true",
                    help="opt-in, with --graph_match: add graph_match_formula, the same comparison with both sides passed through "
                         "mnx_formula_pack and then mnx_expand_pack first, so that a condensed-formula label ('CH2CH3', 'COOCH3') "
                         "equals the group drawn out (DESIGN 4.22). The other scores stay as they are. It is NOT the reference's "
                         "`graph` score: the structure of a formula is this library's own repaired valence search, not the "
                         "reference's RDKit bookkeeping, and no toolkit has parsed the result")
    ap.add_argument("--graph_keep_main", action="store_true",
                    help="opt-in, with --graph_match: add graph_match_main, the same comparison with the PREDICTION passed through "
                         "mnx_main_pack first, so that only its connected component with the most atoms is compared (DESIGN 4.24); "
                         "the gold side is left as read, as the reference's --keep_main trims predictions only. The other scores "
                         "stay as they are. Only the component rule is the reference's: the comparison is this project's canonical "
                         "string, NOT the reference's RDKit `graph` score")
    ap.add_argument("--graph_tanimoto", action="store_true",
                    help="opt-in, with --graph_match: add graph_tanimoto, the mean Tanimoto similarity of prediction against gold by "
                         "this library's own path fingerprint (mnx_fingerprint_pack; both sides through mnx_kekulize_pack and "
                         "mnx_normalize_pack first; DESIGN 4.26), and tanimoto_limited, the sides that passed the step limit. A "
                         "refused, unreadable or limited side scores 0. The other scores stay as they are. NOT the reference's RDKit "
                         "`tanimoto` score: the bits are not RDKit's and no toolkit has seen them")
    ap.add_argument("--graph_isomorphic", action="store_true",
                    help="opt-in, with --graph_match: add graph_match_isomorphic, the share of predictions that are the same graph as "
                         "their gold string by a subgraph search in both directions (mnx_substructure_match; both sides through "
                         "mnx_kekulize_pack and mnx_normalize_pack first; DESIGN 4.30) — it depends on no canonical ranking —, and "
                         "isomorphic_skipped, the items not compared (over 64 atoms, refused or limited; mismatches). The other scores "
                         "stay as they are. NOT the reference's RDKit `graph` score: this library's own atom and bond match")
    ap.add_argument("--graph_tanimoto_bonds", type=int, default=0, metavar="N",
                    help="with --graph_tanimoto: the longest path in bonds, 1..7; 0 (default) = 7, the reference's maxPath")
    return ap


def main(argv=None):
    import pandas as pd
    import torch.distributed as dist
    from . import weights as W
    from .abi import DEFAULT_DTYPE
    from .engine import Engine
    from .preprocess import load_image_rgb
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.batch_size <= MAX_BATCH_SIZE:
        ap.error(f"--batch_size must be 1..{MAX_BATCH_SIZE} (reference batches of 2 x batch_size <= {2 * MAX_BATCH_SIZE} rows)")
    for flag in ("graph_normalize", "graph_kekulize", "graph_formula", "graph_keep_main", "graph_tanimoto", "graph_isomorphic"):
        if getattr(args, flag) and not args.graph_match:
            ap.error(f"--{flag} adds a score to --graph_match")
    if args.graph_tanimoto_bonds and not args.graph_tanimoto:
        ap.error("--graph_tanimoto_bonds sets the path length of --graph_tanimoto")
    if not 0 <= args.graph_tanimoto_bonds <= 7:
        ap.error("--graph_tanimoto_bonds must be 1..7, or 0 for 7")
    dtype = args.dtype or ("fp16" if args.fp16 else DEFAULT_DTYPE)
    max_batch = max(64, 2 * args.batch_size)          # one reference batch is encoded in one launch group
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    from .checkpoint import load_checkpoint               # strict validation, no optimizer state, safetensors-aware
    states = W.synthetic_checkpoint(0) if args.load_path == "synthetic" else load_checkpoint(args.load_path)
    engine = Engine(states["encoder"], states["decoder"], device=local, max_batch=max_batch, dtype=dtype,
                    image_format=args.image_format)
    df = pd.read_csv(os.path.join(args.data_path, args.test_file))
    paths = [os.path.join(args.data_path, p) for p in df["file_path"]]
    if args.predict_coords and "SMILES" not in df.columns:
        ap.error("--predict_coords needs a SMILES column in --test_file")
    known = ["" if pd.isna(s) else str(s) for s in df["SMILES"]] if args.predict_coords else None      # an empty cell: no atoms
    if args.graph_match and (args.predict_coords or "SMILES" not in df.columns):
        ap.error("--graph_match compares predictions with the SMILES column of --test_file (and not under --predict_coords)")
    kept = {} if args.graph_match else None
    def infer(e):
        return run_inference(e, lambda i: load_image_rgb(paths[i]), len(df), args.batch_size, rank, world,
                             pad_to_square=args.test_file in PAD_TO_SQUARE_FILES, smiles=known, keep_records=kept)
    try:
        preds = infer(engine)
    except RangeFallback as err:
        # the reference evaluates any checkpoint; an activation beyond the fp16 range must not end the run. All ranks arrive
        # here together (run_inference agrees on the flag before its gather): one table, one operand mode.
        from .abi import RANGE_FALLBACK
        to = RANGE_FALLBACK.get(dtype)
        if to is None:
            raise
        print(f"[rank {rank}] {err}: repeating the evaluation with --dtype {to} on every rank", file=sys.stderr, flush=True)
        engine.close()
        engine = Engine(states["encoder"], states["decoder"], device=local, max_batch=max_batch, dtype=to,
                        image_format=args.image_format)
        preds = infer(engine)
    if rank == 0:
        if "image_id" not in df.columns:    # main.py:461-462
            df["image_id"] = [p.split("/")[-1].split(".")[0] for p in df["file_path"]]
        table = predictions_table(df["image_id"], preds)
        if args.predict_coords:      # main.py:534-535: the known structure and where its atoms are
            table = {"image_id": table["image_id"], "SMILES": known, "node_coords": table["node_coords"]}
            scores = None            # the SMILES column is the input here: there is no predicted string to score
        else:
            scores = smiles_scores(df["SMILES"], table["SMILES"]) if "SMILES" in df.columns else None
            if args.graph_match:
                scores.update(graph_match_scores(engine, kept["records"], list(df["SMILES"]), normalize=args.graph_normalize,
                                                 kekulize=args.graph_kekulize, **({"formula": True} if args.graph_formula else {}),
                                                 **({"keep_main": True} if args.graph_keep_main else {})))
                if args.graph_tanimoto:
                    scores.update(graph_tanimoto_scores(engine, kept["records"], list(df["SMILES"]), max_bonds=args.graph_tanimoto_bonds))
                if args.graph_isomorphic:
                    scores.update(graph_isomorphic_scores(engine, kept["records"], list(df["SMILES"])))
        print(write_predictions(args.save_path, args.test_file, table, scores), json.dumps(scores))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
