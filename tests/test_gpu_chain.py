"""GPU (-m gpu): the chain of passes over the packed tables as Python drives it (molnextr_amd/chain.py) against the same chain
written out here by hand — five plain `if` statements in the documented order, formula -> expand -> keep_main -> kekulize ->
normalize, calling Engine.*_pack, unpack_graphs, smiles_pack and molfile_pack — for all 32 subsets of the five flags: the packed
tail of predict_pipeline on one prediction of 8 synthetic images, canonical_smiles on eight strings that every pass changes one
of, and evaluate's graph_match_scores with every flag. Equality throughout, no tolerances."""
import itertools

import pytest
import torch

from molnextr_amd import weights as W
from molnextr_amd.engine import (MOL_AROMATIZED, MOL_EXPANDED, MOL_FORMULA_EXPANDED, MOL_FORMULA_LEFT, MOL_KEKULIZED, MOL_MAIN_KEPT,
                                 MOL_UNBRACKETED, NOTE_H_MASK, READ_REFUSED, SMILES_REFUSED)
from molnextr_amd.model import canonical_smiles, formula_candidate, packed_predictions, unpack_graphs
from molnextr_amd.tokenizer import get_tokenizer
from packed_tables import dev, eng  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ("formula", "expand", "keep_main", "kekulize", "normalize")
SUBSETS = [dict(zip(NAMES, bits)) for bits in itertools.product((False, True), repeat=5)]
E2E_FIRST_INDEX = 500          # the batch of the writers' end-to-end tests


def by_hand(eng, rec, formula, expand, keep_main, kekulize, normalize):
    """the chain in the documented order: (the record the writers read, the record of every pass that ran)"""
    stages = {}
    if formula:
        rec = stages["formula"] = eng.formula_pack(rec, keep_device=True)
    if expand:
        rec = stages["expand"] = eng.expand_pack(rec, keep_device=True)
    if keep_main:
        rec = stages["keep_main"] = eng.main_pack(rec, keep_device=True)
    if kekulize:
        rec = stages["kekulize"] = eng.kekulize_pack(rec, keep_device=True)
    if normalize:
        rec = stages["normalize"] = eng.normalize_pack(rec, keep_device=True)
    return rec, stages


def per_molecule(rec, per_atom):
    """an array per atom of the record (or the record's own, by its key) cut into the molecules' parts"""
    a = rec[per_atom] if isinstance(per_atom, str) else per_atom
    return [a[int(m["atom0"]):int(m["atom0"]) + int(m["n_atoms"])] for m in rec["mols"]]


@pytest.fixture(scope="module")
def predicted(eng, dev):
    return eng.predict(W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev), ref_batch=4)


def test_packed_predictions_equal_the_chain_by_hand_for_every_subset(eng, predicted):
    tok = get_tokenizer()["chartok_coords"]

    def graphs(r, **ranks):
        return unpack_graphs(r["mols"], r["atoms"], r["bonds"], r["text"], tok.maxx, False, **ranks)

    def with_origin(r):
        return [{"symbols": g["chartok_coords"]["symbols"], "coords": g["chartok_coords"]["coords"], "bonds": g["bonds"],
                 "origin": o.tolist(), "flags": int(m["flags"])} for g, o, m in zip(graphs(r), per_molecule(r, "origin"), r["mols"])]

    def with_notes(r):
        return [{"symbols": g["chartok_coords"]["symbols"], "bonds": g["bonds"], "hydrogens": (n & NOTE_H_MASK).tolist(),
                 "notes": n.tolist(), "flags": int(m["flags"])} for g, n, m in zip(graphs(r), per_molecule(r, "atom_notes"), r["mols"])]

    for on in SUBSETS:
        got = packed_predictions(eng, predicted, tok, [k for k in NAMES if on[k]], molfile=True, smiles=True, canonical=True, symmetry=True)
        drawn = eng.graph_pack(predicted, keep_device=True)
        rec, stages = by_hand(eng, drawn, **on)
        recs, order, data, rank, sym_class, marks = eng.smiles_pack(rec, canonical=True, symmetry=True)
        files, molfiles = eng.molfile_pack(rec)
        want = graphs(drawn)
        # the ranks are cut at the offsets of the last record that adds or drops atoms: a respelling pass keeps every count of a
        # molecule it does not refuse (one it refuses is emptied, and the lists behind it are cut where they always were)
        counted = stages.get("keep_main") or stages.get("expand") or stages.get("formula") or drawn
        ranked = graphs(counted, rank=rank, sym_class=sym_class)
        for b, p in enumerate(want):
            p["canonical_rank"], p["symmetry_class"] = ranked[b]["canonical_rank"], ranked[b]["symmetry_class"]
            written = not int(recs[b]["flags"]) & SMILES_REFUSED
            t0, n = int(recs[b]["text0"]), int(recs[b]["len"])
            p["graph_smiles"] = data[t0:t0 + n].decode("ascii") if written else None
            p["graph_smiles_order"] = per_molecule(rec, order)[b].tolist() if written else None
            p["stereo_atoms"] = per_molecule(rec, marks)[b].tolist() if written else None
            t0, n = int(files[b]["text0"]), int(files[b]["len"])
            p["molfile"] = molfiles[t0:t0 + n].decode("utf-8", errors="replace") if n else None
        if on["formula"]:
            for p, d in zip(want, with_origin(stages["formula"])):
                before, after = p["chartok_coords"]["symbols"], d["symbols"]
                d["replaced"] = [a for a, s in enumerate(before) if after[a] != s]
                d["left"] = [a for a, s in enumerate(before) if after[a] == s and d["flags"] & MOL_FORMULA_LEFT and formula_candidate(s)]
                p["formula"] = d
        if on["expand"]:
            for p, d in zip(want, with_origin(stages["expand"])):
                if on["formula"]:                                                  # back to the predicted atom
                    d["origin"] = [p["formula"]["origin"][k] for k in d["origin"]]
                p["expanded"] = d
        if on["keep_main"]:
            for p, d in zip(want, with_origin(stages["keep_main"])):               # the molecule the pass received: not composed
                p["main"] = d
        if on["kekulize"]:
            for p, d in zip(want, with_notes(stages["kekulize"])):
                p["kekulized"] = d
        if on["normalize"]:
            for p, d in zip(want, with_notes(stages["normalize"])):
                p["normalized"] = d
        assert got == want, on
    assert any(p["graph_smiles"] is not None for p in got)


STRINGS = ["CCO.[Na+]", "[Ph].CCCCC", "CC[CH2CH3]", "C1=CC=CC=C1", "c1ccccc1[OMe]", "[nH]1cccc1", "c1ccccc1", "C[CH](C)F"]
# the bits that say a pass changed a molecule, under the key canonical_smiles reports its flags by (expand's are not reported)
CHANGED = {"formula": ("formula_flags", MOL_FORMULA_EXPANDED), "expand": (None, MOL_EXPANDED), "keep_main": ("main_flags", MOL_MAIN_KEPT),
           "kekulize": ("kekulize_flags", MOL_KEKULIZED), "normalize": ("normalize_flags", MOL_AROMATIZED | MOL_UNBRACKETED)}


def test_canonical_smiles_equals_the_chain_by_hand_for_every_subset(eng):
    plain = canonical_smiles(eng, STRINGS)
    assert all(set(x) == {"smiles", "read_flags", "err_pos", "smiles_flags"} for x in plain)
    for on in SUBSETS:
        got = canonical_smiles(eng, STRINGS, **on)
        read = eng.smiles_read(STRINGS, keep_device=True)
        assert not (read["read"]["flags"] & READ_REFUSED).any()                    # no string is refused by the reader
        rec, stages = by_hand(eng, read, **on)
        recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
        want = []
        for b, (r, w) in enumerate(zip(read["read"], recs)):
            ok = not (int(r["flags"]) & READ_REFUSED or int(w["flags"]) & SMILES_REFUSED)
            item = {"smiles": data[int(w["text0"]):int(w["text0"]) + int(w["len"])].decode() if ok else None,
                    "read_flags": int(r["flags"]), "err_pos": int(r["err_pos"]), "smiles_flags": int(w["flags"])}
            for name, (key, _) in CHANGED.items():
                if on[name] and key:
                    item[key] = int(stages[name]["mols"]["flags"][b])
            want.append(item)
        assert got == want, on
        for name, (key, bits) in CHANGED.items():                                  # every pass that is on changes a string
            if on[name]:
                assert (stages[name]["mols"]["flags"] & bits).any(), (name, on)
                if key:
                    assert any(x[key] & bits for x in got), (name, on)
        if any(on.values()):
            assert [x["smiles"] for x in got] != [x["smiles"] for x in plain], on
    alone = {name: [x["smiles"] for x in canonical_smiles(eng, STRINGS, **{name: True})] for name in NAMES}
    assert len({tuple(v) for v in alone.values()}) == 5                            # and each changes them in its own way


def test_graph_match_scores_with_every_flag_equal_the_scores_by_hand(eng):
    """evaluate's --graph_match with all four flags on 8 synthetic pages in chunks of 4, against the same calls made here over
    all 8: the gold column is the predictions' own canonical strings — of the main molecule for the first half —, one string the
    reader refuses and one other molecule"""
    from molnextr_amd import evaluate as E
    from molnextr_amd.shard import MAX_LEN
    kept, n, kmax = {}, 8, eng.max_atoms
    E.run_inference(eng, lambda i: W.synthetic_page(i % 15), n, batch_size=4, keep_records=kept)
    r = torch.from_numpy(kept["records"]).to(torch.device("cuda", 0))
    edges = r[:, 2 + MAX_LEN + kmax:].contiguous().view(torch.uint8)[:, :kmax * kmax].reshape(n, kmax, kmax).contiguous()
    pack = eng.graph_pack({"lengths": r[:, 0].contiguous(), "n_atoms": r[:, 1].contiguous(), "tokens": r[:, 2:2 + MAX_LEN].contiguous(),
                           "atom_idx": r[:, 2 + MAX_LEN:2 + MAX_LEN + kmax].contiguous(), "edges": edges}, keep_device=True)

    def texts(rec):
        recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
        return [None if int(x["flags"]) & SMILES_REFUSED else data[int(x["text0"]):int(x["text0"]) + int(x["len"])] for x in recs]

    own, main = texts(pack), texts(eng.main_pack(pack, keep_device=True))
    gold = [(t or b"C").decode() for t in main[:4] + own[4:]]
    gold[6], gold[7] = "C(", "CCO"
    read = eng.smiles_read(gold, keep_device=True)
    readable = [not int(x["flags"]) & READ_REFUSED for x in read["read"]]
    assert readable == [True] * 6 + [False, True]

    def share(pred, want):
        return sum(ok and p is not None and w is not None and p == w for ok, p, w in zip(readable, pred, want)) / n

    def both(*passes):
        sides = []
        for rec in (pack, read):
            for name in passes:
                rec = getattr(eng, name)(rec, keep_device=True)
            sides.append(texts(rec))
        return share(*sides)

    want = {"graph_match_device": both(), "gold_unreadable": 1, "pred_refused": sum(t is None for t in own),
            "graph_match_normalized": both("normalize_pack"), "graph_match_kekulized": both("kekulize_pack", "normalize_pack"),
            "graph_match_formula": both("formula_pack", "expand_pack"), "graph_match_main": share(main, texts(read))}
    got = E.graph_match_scores(eng, kept["records"], gold, chunk=4, normalize=True, kekulize=True, formula=True, keep_main=True)
    assert got == want and list(got)[:3] == ["graph_match_device", "gold_unreadable", "pred_refused"]
    assert got["graph_match_main"] >= sum(t is not None for t in main[:4]) / n
    for flags in ({}, {"kekulize": True}, {"normalize": True, "keep_main": True}):
        some = E.graph_match_scores(eng, kept["records"], gold, chunk=4, **flags)
        names = {"normalize": "graph_match_normalized", "kekulize": "graph_match_kekulized", "keep_main": "graph_match_main"}
        assert some == {k: v for k, v in want.items() if k in list(want)[:3] + [names[f] for f in flags]}
