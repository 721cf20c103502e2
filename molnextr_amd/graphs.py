"""The caller-facing functions of the packed-table layer: predictions out of the packed records (unpack_graphs,
packed_predictions), and a caller's own SMILES and molfiles through the readers, the chain of passes (chain.py) and a writer or
sink — canonical_smiles, canonical_molfiles, the fingerprints, tanimoto, the nearest-row search (smiles_library, nearest_smiles),
the substructure search, same_graph. Each takes an
Engine and calls its table methods (engine_tables.TableCalls); the flags come from abi.py. The model path — decode_batch,
predict_pipeline and the reference's facade — is model.py, from where every name here is still importable.
"""
from __future__ import annotations

import re
from typing import TYPE_CHECKING, List

import numpy as np

from .abi import (FP_LIMIT, FP_REFUSED, FP_WORDS, MATCH_BAD_PAIR, MATCH_LIMIT, MATCH_REFUSED, MOL_FORMULA_LEFT, MOL_TRUNCATED,
                  MOLREAD_REFUSED, NOTE_H_MASK, READ_REFUSED, SMILES_NO_POSITION, SMILES_REFUSED)
from .chain import PASSES, named_passes, passes_on, run_chain

if TYPE_CHECKING:
    from .engine import Engine


def unpack_graphs(mols, atoms, bonds, text, coord_bins: int = 64, with_scores: bool = False, rank=None,
                  sym_class=None) -> List[dict]:
    """The records of mnx_graph_pack (Engine.graph_pack's 'mols', 'atoms', 'bonds' structured arrays and 'text' bytes) as the
    per-image dicts of predict_pipeline. Pure host code: every field is copied, the only arithmetic is the reference's own
    coordinate division bin / (coord_bins - 1). 'chartok_coords' = {smiles, symbols, coords, indices[, atom_scores]};
    'bonds' = [(i, j, type, rev[, score])] in the reference's loop order (i < j ascending) stands where the dense path has
    'edges' (and 'edge_scores'); with_scores also carries 'overall_score'. rank, sym_class: the uint16 arrays of
    Engine.smiles_pack(canonical=True), one entry per atom record — every dict gains 'canonical_rank' and 'symmetry_class', a
    list per atom (None for a molecule whose atoms hold 0xFFFF: it was not ranked)."""
    text = bytes(text)
    den = coord_bins - 1
    a_sym0, a_len, a_idx = atoms["sym0"].tolist(), atoms["sym_len"].tolist(), atoms["index"].tolist()
    a_x, a_y = atoms["x_bin"].tolist(), atoms["y_bin"].tolist()
    b_i, b_j, b_t, b_r = bonds["i"].tolist(), bonds["j"].tolist(), bonds["type"].tolist(), bonds["rev"].tolist()
    if with_scores:
        a_sc, b_sc, overall = atoms["score"].tolist(), bonds["score"].tolist(), mols["overall_score"].tolist()
    preds = []
    for m, (a0, na, b0, nb, t0, tl) in enumerate(zip(mols["atom0"].tolist(), mols["n_atoms"].tolist(), mols["bond0"].tolist(),
                                                     mols["n_bonds"].tolist(), mols["text0"].tolist(),
                                                     mols["smiles_len"].tolist())):
        a1, b1 = a0 + na, b0 + nb
        r = {"smiles": text[t0:t0 + tl].decode("utf-8"),
             "symbols": [text[t0 + s:t0 + s + n].decode("utf-8") for s, n in zip(a_sym0[a0:a1], a_len[a0:a1])],
             "indices": a_idx[a0:a1],
             "coords": [[x / den, y / den] for x, y in zip(a_x[a0:a1], a_y[a0:a1])]}
        pred = {"chartok_coords": r}
        if with_scores:
            r["atom_scores"] = a_sc[a0:a1]
            pred["bonds"] = list(zip(b_i[b0:b1], b_j[b0:b1], b_t[b0:b1], b_r[b0:b1], b_sc[b0:b1]))
            pred["overall_score"] = overall[m]
        else:
            pred["bonds"] = list(zip(b_i[b0:b1], b_j[b0:b1], b_t[b0:b1], b_r[b0:b1]))
        for key, per_atom in (("canonical_rank", rank), ("symmetry_class", sym_class)):
            if per_atom is not None:
                v = per_atom[a0:a1].tolist()
                pred[key] = None if SMILES_NO_POSITION in v else v
        preds.append(pred)
    return preds


def _origin_stage(stage: dict, graphs: List[dict]) -> List[dict]:
    """Per molecule the dict of a pass that adds or drops atoms (formula, expand, keep_main): graphs = unpack_graphs(stage)."""
    mols, origin = stage["mols"], stage["origin"].tolist()
    return [{"symbols": g["chartok_coords"]["symbols"], "coords": g["chartok_coords"]["coords"], "bonds": g["bonds"],
             "origin": origin[a0:a0 + na], "flags": flags}
            for g, a0, na, flags in zip(graphs, mols["atom0"].tolist(), mols["n_atoms"].tolist(), mols["flags"].tolist())]


def _notes_stage(stage: dict, graphs: List[dict]) -> List[dict]:
    """Per molecule the dict of a pass that respells the atoms (kekulize, normalize): graphs = unpack_graphs(stage)."""
    mols, notes, hydrogens = stage["mols"], stage["atom_notes"].tolist(), (stage["atom_notes"] & NOTE_H_MASK).tolist()
    return [{"symbols": g["chartok_coords"]["symbols"], "bonds": g["bonds"], "hydrogens": hydrogens[a0:a0 + na],
             "notes": notes[a0:a0 + na], "flags": flags}
            for g, a0, na, flags in zip(graphs, mols["atom0"].tolist(), mols["n_atoms"].tolist(), mols["flags"].tolist())]


_STAGE_DICTS = {"origin": _origin_stage, "atom_notes": _notes_stage}


def packed_predictions(engine: Engine, out: dict, tok, on=(), compute_confidence: bool = False, molfile: bool = False,
                       molfile_scale=None, smiles: bool = False, stereo: bool = False, double_bonds: bool = False,
                       canonical: bool = False, symmetry: bool = False, fingerprint: bool = False, substructure=None,
                       nearest=None) -> List[dict]:
    """predict_pipeline(packed=True) behind Engine.predict: `out`, its result dict, through mnx_graph_pack, the passes named in
    `on` (chain.run_chain: their order, and which stage keeps its tables on the device), the canonical ranking, the two
    writers, the fingerprint, the substructure search (substructure: a list of query SMILES, or None) and the nearest-row search
    (nearest: (library, k, min_similarity) of model.predict_nearest, or None), to the per-image dicts that predict_pipeline
    describes. tok: the 'chartok_coords' tokenizer."""
    writer = molfile or smiles or fingerprint or substructure is not None or nearest is not None    # the sinks: they read the last record on the device
    drawn = engine.graph_pack(out, keep_device=writer or bool(on))       # what the predicted atoms and bonds are read from
    if (drawn["mols"]["flags"] & MOL_TRUNCATED).any():
        raise RuntimeError(f"a molecule has more atoms than the engine capacity max_atoms={engine.max_atoms}")
    stages, rec = run_chain(engine, drawn, on, keep_last=writer)         # rec: what the writers read
    ranked = engine.smiles_pack(rec, stereo=stereo, double_bonds=double_bonds, canonical=True,
                                **({"symmetry": True} if symmetry else {})) if canonical else None

    # The ranks are those of the tables the writer read. They are cut per molecule at the offsets of the last record that adds or
    # drops atoms, and travel with that record's dicts alone: a respelling pass keeps every count — except that it empties a
    # molecule it refuses, and the lists behind such a molecule are then cut at the wrong offsets, as they always were.
    counted = ([drawn] + [stages[row.name] for row in PASSES if row.name in stages and row.side == "origin"])[-1]

    def unpack(r):
        return unpack_graphs(r["mols"], r["atoms"], r["bonds"], r["text"], tok.maxx, compute_confidence,
                             **({"rank": ranked[3], "sym_class": ranked[4]} if canonical and r is counted else {}))

    preds = unpack(drawn)
    for row in PASSES:
        if row.name not in stages:
            continue
        graphs = unpack(stages[row.name])
        for p, g, d in zip(preds, graphs, _STAGE_DICTS[row.side](stages[row.name], graphs)):
            p[row.key] = d
            for key in ("canonical_rank", "symmetry_class"):
                if key in g:
                    p[key] = g[key]
    if "formula" in stages:
        for p in preds:
            before, found = p["chartok_coords"]["symbols"], p["formula"]
            after, left = found["symbols"], found["flags"] & MOL_FORMULA_LEFT
            found["replaced"] = [a for a, s in enumerate(before) if after[a] != s]
            found["left"] = [a for a, s in enumerate(before) if after[a] == s and left and formula_candidate(s)]
            if "expand" in stages:                                       # through the formula pass back to the predicted atom
                p["expanded"]["origin"] = [found["origin"][k] for k in p["expanded"]["origin"]]
    if molfile:
        files, data = engine.molfile_pack(rec, scale=molfile_scale)
        for p, f in zip(preds, files):
            t0, n = int(f["text0"]), int(f["len"])
            p["molfile"] = data[t0:t0 + n].decode("utf-8", errors="replace") if n else None
    if smiles:
        recs, order, data = ranked[:3] if canonical else \
            engine.smiles_pack(rec, stereo=stereo, **({"double_bonds": True} if double_bonds else {}))
        for p, r, m in zip(preds, recs, rec["mols"]):
            t0, n, a0, na = int(r["text0"]), int(r["len"]), int(m["atom0"]), int(m["n_atoms"])
            written = not int(r["flags"]) & SMILES_REFUSED               # an empty molecule is written as the empty string
            p["graph_smiles"] = data[t0:t0 + n].decode("ascii") if written else None
            p["graph_smiles_order"] = order[a0:a0 + na].tolist() if written else None
            if symmetry:
                p["stereo_atoms"] = ranked[5][a0:a0 + na].tolist() if written else None
    if fingerprint or nearest is not None:
        fp = engine.fingerprint_pack(rec, keep_device=nearest is not None)
        if fingerprint:
            for p, r, words in zip(preds, fp["fp"], fp["bits"].cpu().numpy().view(np.uint32) if nearest is not None else fp["bits"]):
                p["fingerprint"] = None if int(r["flags"]) & (FP_REFUSED | FP_LIMIT) else words.tobytes()
        if nearest is not None:
            library, k, min_similarity = nearest
            if not isinstance(library, dict):                            # a list of SMILES: through the passes the predictions took
                library = smiles_library(engine, library, **{name: True for name in on})
            answered = [not int(r["flags"]) & (FP_REFUSED | FP_LIMIT) for r in fp["fp"]]
            for p, found in zip(preds, _nearest_of(engine, fp["bits"], answered, library, k, min_similarity)):
                p["nearest"] = found
    if substructure is not None:
        for p, found in zip(preds, _substructures_of(engine, rec, list(substructure), on, tok.maxx)):
            p["substructure"] = found
    return preds


def _matched(flags: int, n_matches: int):
    """True: the query embeds; False: it does not; None: the pair was refused, or a search was broken off before one was found"""
    if flags & MATCH_REFUSED:
        return None
    return True if n_matches else None if flags & MATCH_LIMIT else False


def _substructures_of(engine: Engine, rec: dict, queries, on, coord_bins: int) -> List[list]:
    """Per molecule of rec (a record of the chain, its tables on the device) one item per query SMILES: {'matched' (_matched),
    'atoms': the molecule's atoms under the query's atoms in the query's atom order, None without a match, 'coords': their page
    coordinates, bin / (coord_bins - 1) as unpack_graphs computes them}. The queries are read on the device and pass through the
    passes of `on`, as the molecules did: one spelling on both sides. One launch for all pairs."""
    n, nq = len(rec["mols"]), len(queries)
    if not nq or not n:
        return [[] for _ in range(n)]
    q_rec = run_chain(engine, engine.smiles_read(queries, keep_device=True), on, keep_last=True)[1]
    pairs = np.stack([np.tile(np.arange(nq), n), np.repeat(np.arange(n), nq)], axis=1)
    res = engine.substructure_match(q_rec, rec, pairs)
    den = coord_bins - 1
    a_x, a_y = rec["atoms"]["x_bin"].tolist(), rec["atoms"]["y_bin"].tolist()
    out = []
    for t, a0 in enumerate(rec["mols"]["atom0"].tolist()):
        items = []
        for k in range(nq):
            r, images = res["match"][t * nq + k], res["map"][t * nq + k]
            matched = _matched(int(r["flags"]), int(r["n_matches"]))
            atoms = images[:int(q_rec["mols"]["n_atoms"][k])].tolist() if matched else None
            items.append({"matched": matched, "atoms": atoms,
                          "coords": [[a_x[a0 + a] / den, a_y[a0 + a] / den] for a in atoms] if matched else None})
        out.append(items)
    return out


_SMILES_ATOM = re.compile(r"Cl|Br|[BCNOPSFIbcnops*]|\[\d{0,3}(se|as|[bcnops]|\*|[A-Z][a-z]?)(@@?)?(H\d?)?(\++|-+|[+-]\d+)?(:\d+)?\]")


def formula_candidate(symbol: str) -> bool:
    """Whether mnx_formula_pack takes an atom's symbol for a condensed formula: in neither name table, 2 to 20 bytes without its
    brackets, and no atom of the SMILES grammar (the host's reading of the header's candidate rule, for reporting only)."""
    from .chem import classify_symbol
    inner = symbol[1:-1] if len(symbol) >= 2 and symbol[0] == "[" and symbol[-1] == "]" else symbol
    return classify_symbol(symbol) == "atom" and 2 <= len(inner.encode("utf-8")) <= 20 and _SMILES_ATOM.fullmatch(symbol) is None


def canonical_smiles(engine: Engine, smiles_list, expand: bool = False, normalize: bool = False, kekulize: bool = False,
                     formula: bool = False, keep_main: bool = False) -> List[dict]:
    """A caller's own SMILES in the form the device writes predictions in: mnx_smiles_read, optionally mnx_expand_pack ([Ph],
    [OMe], ... replaced by their atoms), then mnx_smiles_pack_canonical without marks. Per item {'smiles': the canonical string,
    None where the reader or the writer refused; 'read_flags' (abi.READ_*), 'err_pos' (of READ_SYNTAX), 'smiles_flags'
    (abi.SMILES_*)}. Equal strings mean equal graphs as this library sees them — no stereo, no kekulisation, no [CH] against
    C; it is NOT a toolkit's canonical SMILES and never compares with one. normalize: mnx_normalize_pack in front of the writer
    (behind the expansion): aromatic rings of 5 and 6 atoms perceived from a Kekule string, [CH] against C, N against [nH] — this
    library's own rule, not a toolkit's aromaticity model; the items gain 'normalize_flags' (abi.MOL_AROMATIZED / ...).
    kekulize: mnx_kekulize_pack behind the expansion and in front of normalize — an aromatic string is written as a Kekule
    structure first (a perfect matching in this library's own search order, not RDKit's Kekulize), so that with normalize an
    aromatic string, a Kekule string and a half-aromatic one of the same molecule get one string where the rule finds the rings,
    and without it azulene and its aromatic form do; the items gain 'kekulize_flags' (abi.MOL_KEKULIZED / ...).
    formula: mnx_formula_pack in front of the expansion — a condensed-formula atom such as [CH2CH3] or [N(CH3)2] is replaced by
    the atoms a valence search finds for it (this library's own rule; combine with expand for the group tokens a formula
    holds); the items gain 'formula_flags' (abi.MOL_FORMULA_EXPANDED / ...).
    keep_main: mnx_main_pack behind the expansion and in front of kekulize — only the connected component with the most atoms is
    written, among equals the one with the lowest atom (the reference's _keep_main_molecule: 'CCO.[Na+]' is written as 'CCO'
    is); the items gain 'main_flags' (abi.MOL_MAIN_KEPT / MOL_MAIN_TIE)."""
    smiles_list = list(smiles_list)
    if not smiles_list:
        return []
    on = passes_on(formula, expand, keep_main, kekulize, normalize)
    return _canonical_of_read(engine, engine.smiles_read(smiles_list, keep_device=True), on, READ_REFUSED, "err_pos")


def _canonical_of_read(engine: Engine, read: dict, on, refused: int, err_key: str, **marks) -> List[dict]:
    """The back half of canonical_smiles and canonical_molfiles: a reader's tables through the passes named in `on` and the
    canonical writer (marks: smiles_pack's stereo / double_bonds / symmetry), one item per molecule; refused: the reader's refusal
    bits, err_key: the field of read['read'] that says where it refused"""
    stages, rec = run_chain(engine, read, on, keep_last=True)
    written = engine.smiles_pack(rec, canonical=True, **marks)          # symmetry adds a sixth value
    recs, data = written[0], written[2]
    out = []
    for r, w in zip(read["read"], recs):
        ok = not (int(r["flags"]) & refused or int(w["flags"]) & SMILES_REFUSED)
        out.append({"smiles": data[int(w["text0"]):int(w["text0"]) + int(w["len"])].decode("utf-8", "replace") if ok else None,
                    "read_flags": int(r["flags"]), err_key: int(r[err_key]), "smiles_flags": int(w["flags"])})
    for row in PASSES:
        if row.name in stages and row.flags_key:
            for item, flags in zip(out, stages[row.name]["mols"]["flags"]):
                item[row.flags_key] = int(flags)
    return out


def split_sdf(data) -> List[bytes]:
    """The records of an SDF (bytes or str) as bytes, split at the lines "$$$$" (host only): each begins with its molfile, whose
    "M  END" line ends what mnx_molfile_read reads, so the data items behind it may stay. Nothing but line ends behind the last
    "$$$$" is no record."""
    data = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    out, start, at = [], 0, 0
    while at < len(data):
        nl = data.find(b"\n", at)
        end = len(data) if nl < 0 else nl + 1
        if data[at:end].rstrip(b"\r\n") == b"$$$$":
            out.append(data[start:at])
            start = end
        at = end
    if data[start:].strip(b"\r\n"):
        out.append(data[start:])
    return out


def canonical_molfiles(engine: Engine, molfiles, fit: bool = True, scale=None, stereo: bool = False, double_bonds: bool = False,
                       symmetry: bool = False, expand: bool = False, normalize: bool = False, kekulize: bool = False,
                       formula: bool = False, keep_main: bool = False) -> List[dict]:
    """A caller's own V2000 molfiles (bytes or str, one molecule each; split_sdf cuts an SDF) in the form the device writes
    predictions in: mnx_molfile_read, the passes named (canonical_smiles' options, in the chain's order), then
    mnx_smiles_pack_canonical — with stereo / double_bonds the '@' / '@@' and '/' '\\' that the file's wedges and coordinates
    resolve, which no SMILES brings into the chain; symmetry: mnx_smiles_pack_symmetric's rule. fit (the default): one uniform
    scale per file that fits its atoms into the coordinate bins; else scale = (Sx, Sy) per file, mnx_molfile_pack's argument (None
    with fit=False: 100000 each). Per item canonical_smiles' keys with 'err_line' (of MOLREAD_SYNTAX / MOLREAD_QUERY) in the
    place of 'err_pos'; 'read_flags' are abi.MOLREAD_*. This library's own reading and ranking, NOT a toolkit's."""
    molfiles = list(molfiles)
    if not molfiles:
        return []
    if scale is not None:
        fit = False
    on = passes_on(formula, expand, keep_main, kekulize, normalize)
    read = engine.molfile_read(molfiles, scale=scale, fit=fit, keep_device=True)
    return _canonical_of_read(engine, read, on, MOLREAD_REFUSED, "err_line", stereo=stereo, double_bonds=double_bonds, symmetry=symmetry)


def smiles_fingerprints(engine: Engine, smiles_list, max_bonds: int = 0, **passes) -> List[dict]:
    """The path fingerprints of a caller's own SMILES: mnx_smiles_read, the passes named (canonical_smiles' pass options, in the
    chain's order), then mnx_fingerprint_pack instead of a writer. Per item {'fingerprint': the 2048 bits of the molecule's paths
    of up to max_bonds bonds (0: 7) as 256 bytes — this library's own rule, NOT RDKit's bits —, None where the reader refused the
    string or the molecule is refused or limited; 'read_flags' (abi.READ_*), 'fingerprint_flags' (abi.FP_*)}."""
    smiles_list = list(smiles_list)
    if not smiles_list:
        return []
    on = named_passes("smiles_fingerprints", passes)
    return _fingerprints_of_read(engine, engine.smiles_read(smiles_list, keep_device=True), on, READ_REFUSED, max_bonds)


def _fingerprints_of_read(engine: Engine, read: dict, on, refused: int, max_bonds: int) -> List[dict]:
    """The back half of smiles_fingerprints and molfile_fingerprints: a reader's tables through the passes named in `on` and
    mnx_fingerprint_pack, one item per molecule; refused: the reader's refusal bits"""
    fp = engine.fingerprint_pack(run_chain(engine, read, on, keep_last=True)[1], max_bonds=max_bonds)
    return [{"fingerprint": None if int(r["flags"]) & refused or int(f["flags"]) & (FP_REFUSED | FP_LIMIT) else words.tobytes(),
             "read_flags": int(r["flags"]), "fingerprint_flags": int(f["flags"])} for r, f, words in zip(read["read"], fp["fp"], fp["bits"])]


def molfile_fingerprints(engine: Engine, molfiles, max_bonds: int = 0, **passes) -> List[dict]:
    """The path fingerprints of a caller's own V2000 molfiles: mnx_molfile_read, the passes named, then mnx_fingerprint_pack —
    smiles_fingerprints' items, 'read_flags' being abi.MOLREAD_*. The bits hold no coordinates, so no scale is asked for."""
    molfiles = list(molfiles)
    if not molfiles:
        return []
    on = named_passes("molfile_fingerprints", passes)
    return _fingerprints_of_read(engine, engine.molfile_read(molfiles, fit=True, keep_device=True), on, MOLREAD_REFUSED, max_bonds)


def tanimoto(engine: Engine, smiles_a, smiles_b, **passes) -> List[float]:
    """The Tanimoto similarity of the path fingerprints of two lists of SMILES, item by item (mnx_fingerprint_pack and
    mnx_tanimoto; passes: smiles_fingerprints' options — kekulize=True, normalize=True make aromatic and Kekule spellings agree).
    A string the reader refuses and a molecule that is refused or limited score 0.0, as two empty molecules do. This library's own
    fingerprint: NOT RDKit's, and not the reference's `tanimoto` score."""
    smiles_a, smiles_b = list(smiles_a), list(smiles_b)
    if len(smiles_a) != len(smiles_b):
        raise ValueError(f"tanimoto compares item with item: {len(smiles_a)} strings against {len(smiles_b)}")
    if not smiles_a:
        return []
    empty = bytes(4 * FP_WORDS)
    sides = [[x["fingerprint"] or empty for x in smiles_fingerprints(engine, side, **passes)] for side in (smiles_a, smiles_b)]
    a, b = (np.frombuffer(b"".join(side), np.uint32).reshape(-1, FP_WORDS) for side in sides)
    return engine.tanimoto(a, b)["similarity"].tolist()


def smiles_library(engine: Engine, smiles_list, max_bonds: int = 0, **passes) -> dict:
    """A caller's own list of known compounds, read and fingerprinted once, for any number of nearest_smiles and predict_nearest
    calls: mnx_smiles_read, the passes named (smiles_fingerprints' options), mnx_fingerprint_pack. {'bits': the fingerprints as a
    device tensor int32 [n, FP_WORDS], 'flags': per string abi.FP_* of its fingerprint with bit 31 set where the reader refused
    the string (either way every word is 0 then and the row scores 0.0 against everything), 'smiles': the strings}. Search it
    with the passes it was made with: kekulize=True, normalize=True on both sides make aromatic and Kekule spellings agree."""
    smiles_list = list(smiles_list)
    if not smiles_list:
        raise ValueError("smiles_library: an empty library has no nearest row")
    on = named_passes("smiles_library", passes)
    read = engine.smiles_read(smiles_list, keep_device=True)
    fp = engine.fingerprint_pack(run_chain(engine, read, on, keep_last=True)[1], max_bonds=max_bonds, keep_device=True)
    unread = (read["read"]["flags"] & READ_REFUSED) != 0
    return {"bits": fp["bits"], "flags": (fp["fp"]["flags"] | np.where(unread, np.uint32(1 << 31), np.uint32(0))).astype(np.uint32),
            "smiles": [s.decode("utf-8", "replace") if isinstance(s, bytes) else s for s in smiles_list]}


def _nearest_of(engine: Engine, bits, answered, library: dict, k: int, min_similarity: float) -> List[list]:
    """Per row of bits (fingerprints on the device) its hits in the library of smiles_library: [{'index', 'smiles',
    'similarity'}] in mnx_tanimoto_search's order; [] for a row that is not `answered` — it has no fingerprint. One search."""
    res = engine.tanimoto_search(bits, library["bits"], k=k, min_similarity=min_similarity)
    names = library["smiles"]
    return [[{"index": int(i), "smiles": names[int(i)], "similarity": float(s)} for i, s in zip(row[:n], sims[:n])] if ok else []
            for ok, n, row, sims in zip(answered, res["count"].tolist(), res["index"], res["similarity"])]


def nearest_smiles(engine: Engine, queries, library, k: int = 1, min_similarity: float = 0.0, **passes) -> List[list]:
    """Which known compound is nearest: per query SMILES the k nearest strings of `library` — a list of SMILES, or
    smiles_library's dict, made once — by the Tanimoto similarity of this library's path fingerprints (mnx_tanimoto_search: the
    first k by similarity, among equals the lower library index, of those the ones at or above min_similarity). Per query a list
    of {'index', 'smiles', 'similarity'}; [] for a query that was not read, was refused or passed the step limit. passes:
    smiles_fingerprints' pass options, applied to the queries and to a library given as a list. NOT RDKit's fingerprint, k <=
    NEAREST_MAX_K, and no count of all rows above a threshold."""
    queries = list(queries)
    if not queries:
        return []
    on = named_passes("nearest_smiles", passes)
    if not isinstance(library, dict):
        library = smiles_library(engine, library, **passes)
    read = engine.smiles_read(queries, keep_device=True)
    fp = engine.fingerprint_pack(run_chain(engine, read, on, keep_last=True)[1], keep_device=True)
    answered = [not (int(r["flags"]) & READ_REFUSED or int(f["flags"]) & (FP_REFUSED | FP_LIMIT)) for r, f in zip(read["read"], fp["fp"])]
    return _nearest_of(engine, fp["bits"], answered, library, k, min_similarity)


def _chained(engine: Engine, smiles_list, passes: dict, who: str):
    """a caller's strings read on the device and sent through the passes named: (the reader's record, the last record)"""
    on = named_passes(who, passes)
    read = engine.smiles_read(list(smiles_list), keep_device=True)
    return read, run_chain(engine, read, on, keep_last=True)[1]


def smiles_substructure(engine: Engine, queries, targets, pairs=None, max_matches: int = 1, **passes) -> List[dict]:
    """Substructure search on a caller's own SMILES: both lists through mnx_smiles_read and the passes named (canonical_smiles' pass
    options, in the chain's order; kekulize=True, normalize=True make aromatic and Kekule spellings agree), then
    mnx_substructure_match. pairs: [(query index, target index)]; None pairs one query with every target, or item with item where
    the lists are equally long (anything else: ValueError). Per pair {'matched': True, False, or None where a string was not read,
    the pair was refused or a search was broken off without a match; 'n_matches': the embeddings counted, max_matches at the most;
    'atoms': the target's atoms under the query's atoms in the query's atom order, None without a match; 'flags' (abi.MATCH_*)}.
    This library's own rule (include/molnextr_hip.h): NOT RDKit's HasSubstructMatch, not SMARTS — H counts and stereo are not
    compared."""
    queries, targets = list(queries), list(targets)
    if not queries or not targets:
        return []
    (q_read, q_rec), (t_read, t_rec) = (_chained(engine, side, passes, "smiles_substructure") for side in (queries, targets))
    res = engine.substructure_match(q_rec, t_rec, pairs, max_matches=max_matches)
    if pairs is None:
        pairs = [(0 if len(queries) == 1 else k, k) for k in range(len(targets))]
    out = []
    for (qi, ti), r, images in zip(pairs, res["match"], res["map"]):
        flags, n = int(r["flags"]), int(r["n_matches"])
        unread = flags & MATCH_BAD_PAIR == 0 and (int(q_read["read"]["flags"][qi]) | int(t_read["read"]["flags"][ti])) & READ_REFUSED
        matched = None if unread else _matched(flags, n)
        out.append({"matched": matched, "n_matches": n, "atoms": images[:int(q_rec["mols"]["n_atoms"][qi])].tolist() if matched else None,
                    "flags": flags})
    return out


def _same_graph_tables(engine: Engine, a_rec: dict, b_rec: dict, max_steps: int = 0):
    """Two records of equally many molecules, item by item: (same, skipped) — same[i]: the atom and bond counts are equal, a
    embeds in b and b embeds in a (mnx_substructure_match both ways: the rule is asymmetric at wildcards, at isotope 0 and at bonds
    of class ANY); skipped[i]: a direction was refused (a side of more than MATCH_MAX_QUERY atoms among them) or broken off without
    a match, so same[i] is False without the graphs having been compared"""
    ab, ba = (engine.substructure_match(x, y, max_steps=max_steps)["match"] for x, y in ((a_rec, b_rec), (b_rec, a_rec)))
    equal = (a_rec["mols"]["n_atoms"] == b_rec["mols"]["n_atoms"]) & (a_rec["mols"]["n_bonds"] == b_rec["mols"]["n_bonds"])
    found = (ab["n_matches"] > 0) & (ba["n_matches"] > 0)
    unknown = [_matched(int(x["flags"]), int(x["n_matches"])) is None or _matched(int(y["flags"]), int(y["n_matches"])) is None for x, y in zip(ab, ba)]
    return (equal & found).tolist(), (equal & ~found & np.array(unknown, bool)).tolist()


def same_graph(engine: Engine, smiles_a, smiles_b, **passes) -> List[bool]:
    """Are these the same graph, item by item — asked of the graphs, not of a string: both lists through mnx_smiles_read and the
    passes named (smiles_substructure's options), then item i is True when the atom and bond counts are equal, a embeds in b and b
    embeds in a (mnx_substructure_match in both directions). It depends on no canonical ranking, so the drawings that the ranks'
    known limit gives two canonical strings are one graph here. By this library's own atom and bond match: H counts and stereo are
    not compared, a molecule of more than 64 atoms is never the same as anything."""
    smiles_a, smiles_b = list(smiles_a), list(smiles_b)
    if len(smiles_a) != len(smiles_b):
        raise ValueError(f"same_graph compares item with item: {len(smiles_a)} strings against {len(smiles_b)}")
    if not smiles_a:
        return []
    return _same_graph_tables(engine, _chained(engine, smiles_a, passes, "same_graph")[1], _chained(engine, smiles_b, passes, "same_graph")[1])[0]


def page_scale(image) -> tuple:
    """(Sx, Sy) of mnx_molfile_pack for one input page [height, width, ...]: Sx = round(100000 * width / height), the reference's
    `ratio` times its factor 10 (chemical.py:935-937) in units of 1e-4, inside the call's range; Sy = 100000."""
    height, width = int(image.shape[0]), int(image.shape[1])
    return min(max((200000 * width + height) // (2 * height), 1), 10000000), 100000
