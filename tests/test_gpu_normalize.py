"""GPU (-m gpu): mnx_normalize_pack — one normal spelling per atom on the device — against the oracle of tests/normalize_ref.py,
records field by field and all four tables and `atom_notes` byte for byte (no tolerances): the hand table of the host test, random
molecules, the sizes at which the kernel's loops take another turn, the refusals, the capacity protocol, determinism, every argument
error, the chains read -> normalize -> canonical writer and expand -> normalize, one end-to-end run and evaluate's
--graph_normalize. The rule is the project's own (include/molnextr_hip.h): no toolkit has checked it."""
import functools
import json

import numpy as np
import pytest
import torch

import molfile_ref as M
import normalize_ref as N
import test_normalize_host as H
from molnextr_amd import evaluate as E
from molnextr_amd import weights as W
from molnextr_amd.engine import MOL_AROMATIZED, MOL_NORMALIZE_REFUSED, MOL_UNBRACKETED, NOTE_H_MASK, SMILES_REFUSED, Engine
from molnextr_amd.model import canonical_smiles, predict_pipeline
from molnextr_amd.shard import MAX_LEN, pack_records
from packed_tables import (FILL, Tables, _p, assert_refused, call_tables, clean, compare_tables, dev, eng, mol, path, same_mols,  # noqa: F401
                           same_results)

pytestmark = pytest.mark.gpu
TABLES = H.TABLES

run = functools.partial(call_tables, "mnx_normalize_pack")    # run(eng, t, caps, **over); the result's `side` is `atom_notes`


def check(eng, t, ref=None, **cut):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    ref = ref or N.pack(t.mols, t.atoms, t.bonds, t.text, tables=TABLES, n_atom_records=cut.get("na"), n_bond_records=cut.get("nb"),
                        n_text_bytes=cut.get("nt"))
    compare_tables(run(eng, t, ref["totals"], **cut), ref, "atom_notes")
    return ref


def hand_strings():
    return (sorted(H.AROMATIC) + sorted(set(H.AROMATIC.values())) + H.NOT_AROMATIC + sorted(H.BRACKETS) +
            ["[C@H]", "N[C@@H](C)O", "[C@@]1=CC=CC=C1", "c1ccc2C=CC=Cc2c1", "C:C", "[Ph]C", "*C", "S(=O)(=O)(O)O", ""])


def test_the_hand_table_one_by_one_and_as_one_batch(eng, dev):
    strings = hand_strings()
    for s in strings:
        check(eng, Tables(dev, arrays=H.tables_of([s])))                           # n = 1
    ref = check(eng, Tables(dev, arrays=H.tables_of(strings)))
    assert H.written(ref)[:len(H.AROMATIC)] == [H.AROMATIC[s] for s in sorted(H.AROMATIC)]
    assert all(int(f) & MOL_AROMATIZED for f in ref["mols"]["flags"][:len(H.AROMATIC)])


def test_scores_indices_and_the_truncated_bit_travel(eng, dev):
    mols, atoms, bonds, text = (x.copy() if isinstance(x, np.ndarray) else x for x in H.tables_of(hand_strings()))
    rng = np.random.default_rng(1)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"], atoms["x_bin"], atoms["y_bin"] = (rng.integers(0, 500, len(atoms)) for _ in range(3))
    mols["flags"] = rng.integers(0, 16, len(mols))                                 # bit 0 travels, the expansion's bits do not
    bonds["rev"] = rng.integers(0, 7, len(bonds))
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert set((ref["mols"]["flags"] & 15).tolist()) == {0, 1}


@pytest.fixture(scope="module")
def batch(dev):
    """1025 generated molecules of 1..40 atoms (one past the scan tile of 1024), 12 of them near-complete graphs of 30 atoms, and
    the oracle's tables"""
    t = Tables(dev, H.kekule_batch(np.random.default_rng(7), 1013, dense=12))
    return t, N.pack(t.mols, t.atoms, t.bonds, t.text, tables=TABLES)


def test_1025_generated_molecules_and_two_runs_with_identical_bytes(eng, batch):
    t, ref = batch
    flags = ref["mols"]["flags"]
    assert (flags & MOL_AROMATIZED).astype(bool).sum() > 100 and (flags & MOL_UNBRACKETED).astype(bool).sum() > 100
    assert (ref["atom_notes"] & 64).any() and not (flags & MOL_NORMALIZE_REFUSED).any()
    check(eng, t, ref)
    same_results(run(eng, t, ref["totals"]), run(eng, t, ref["totals"]))


def acene(rings, first=0):
    """a chain of `rings` fused six-rings in Kekule form on atoms first .. first + 4 * rings + 1: top row t0 .. t2k, bottom row
    b0 .. b2k, a rung at every even position; double bonds on the first rung and on (t1 t2), (b1 b2), (t3 t4), ..."""
    w = 2 * rings + 1
    top, bottom = [first + k for k in range(w)], [first + w + k for k in range(w)]
    bonds = []
    for row in (top, bottom):
        bonds += [(row[k], row[k + 1], 2 if k % 2 else 1, 2 if k % 2 else 1) for k in range(w - 1)]
    bonds += [(top[k], bottom[k], 2 if k == 0 else 1, 2 if k == 0 else 1) for k in range(0, w, 2)]
    return [b"C"] * (2 * w), bonds


def with_tail(rings, n_atoms, ring_first=False):
    """an acene and a path that bring the molecule to n_atoms atoms: the path bonded to the acene's first atom, or (ring_first =
    False and no bond between them) the path in front, so that the rings lie on the highest atom indices"""
    n_ring = 4 * rings + 2
    if ring_first:
        syms, bonds = acene(rings)
        bonds += [(0, n_ring, 1, 1)] + path(n_atoms - n_ring, first=n_ring) if n_atoms > n_ring else []
        return mol(syms + [b"C"] * (n_atoms - n_ring), sorted(bonds))
    syms, bonds = acene(rings, first=n_atoms - n_ring)
    return mol([b"C"] * (n_atoms - n_ring) + syms, sorted(path(n_atoms - n_ring) + bonds))


def test_molecules_of_1_256_257_and_999_atoms(eng, dev):
    molecules = [mol([b"C"]), mol([b"[nH]"]),
                 with_tail(63, 256, ring_first=True), with_tail(63, 257, ring_first=True),     # 254 ring atoms and a tail of 2 or 3
                 with_tail(2, 999), mol([b"C"] * 999, path(999)),                              # 999 atoms and 999 / 998 bonds
                 mol(*acene(199)), with_tail(64, 258)]                                         # 798 atoms on 996 bonds
    t = Tables(dev, molecules)
    ref = check(eng, t)
    assert [int(f) for f in ref["mols"]["flags"]] == [0, 0, 16, 16, 16, 0, 16, 16]
    assert ref["mols"]["n_atoms"].tolist() == [1, 1, 256, 257, 999, 999, 798, 258] and ref["mols"]["n_bonds"].tolist()[4] == 999
    assert [int((ref["atom_notes"][int(m["atom0"]):int(m["atom0"]) + int(m["n_atoms"])] & 16).astype(bool).sum()) for m in ref["mols"]] == \
        [0, 0, 254, 254, 10, 0, 798, 258]
    for m in molecules[2:]:
        check(eng, Tables(dev, [m]))


def test_refusals(eng, dev):
    ok = mol([b"C", b"[CH3]"], path(2))
    ring = H.tables_of(["C1=CC=CC=C1"])
    molecules = [ok, mol([b"C"] * 1000, path(1000)), ok, mol([b"C"] * 500, path(500) + [(0, k, 1, 1) for k in range(2, 500)] + [(1, k, 1, 1) for k in (3, 4, 5)]),
                 mol([b"C", b"C"], [(0, 2, 1, 1)]), mol([b"C", b"C"], [(2, 1, 1, 1)]), ok]
    assert [len(m[2]) for m in molecules][3] == 1000
    t = Tables(dev, molecules)
    ref = check(eng, t)
    assert [int(f) & MOL_NORMALIZE_REFUSED for f in ref["mols"]["flags"]] == [0, 64, 0, 64, 64, 64, 0]
    assert ref["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 0, 0, 2] and ref["text"] == b"CCCCCC"
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        want = check(eng, t, **cut)
        assert int(want["mols"]["flags"][-1]) & MOL_NORMALIZE_REFUSED and want["mols"]["n_atoms"].tolist()[:3] == [2, 0, 2]
    mols, atoms, bonds, text = M.build_tables([ok, ok])                            # a symbol behind the text
    atoms["sym0"][3] = 60000
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert ref["mols"]["flags"].tolist() == [MOL_UNBRACKETED, MOL_NORMALIZE_REFUSED]
    mols, atoms, bonds, text = (x.copy() if isinstance(x, np.ndarray) else x for x in ring)
    mols["atom0"][0] = 1 << 31                                                     # a record that points far beyond the tables
    assert check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))["mols"]["flags"].tolist() == [MOL_NORMALIZE_REFUSED]


def test_the_empty_molecule_and_pseudo_atoms_only(eng, dev):
    ref = check(eng, Tables(dev, [mol([]), mol([b"[Ph]", b"[R1]", b"<unk>", b"", b"*"], path(5)), mol([]), mol([b"[R1]"])]))
    assert ref["mols"]["flags"].tolist() == [0, 0, 0, 0] and ref["atom_notes"].tolist() == [64] * 6
    check(eng, Tables(dev, [mol([])]))


def test_a_bond_of_type_0_or_7_at_a_ring_atom_excludes_it(eng, dev):
    molecules = []
    for ty in (0, 7, 4, 9, 255):
        syms, bonds = acene(1)
        molecules.append(mol(syms + [b"[CH3]"], sorted(bonds + [(2, 6, ty, ty)])))
    syms, bonds = acene(1)
    molecules.append(mol(syms, sorted(bonds + [(2, 2, 1, 1)])))                    # a bond from an atom to itself
    molecules.append(mol(syms, sorted(bonds + [(1, 2, 1, 1)])))                    # the same pair in two records: no candidates
    molecules.append(mol(syms + [b"[CH3]"], sorted(bonds + [(2, 6, 5, 6)])))       # a wedge is a single bond
    ref = check(eng, Tables(dev, molecules))
    assert ref["mols"]["flags"].tolist() == [0, 0, 0, 0, 0, 0, 0, MOL_AROMATIZED | MOL_UNBRACKETED]
    assert ref["atom_notes"][:7].tolist() == [1, 1, 64, 1, 1, 1, 64 | 3]


def test_capacities_exact_and_one_short(eng, batch):
    """each capacity one record or byte short, separately: nothing is written beyond it, what lies in front of it is right, and
    mols_out and totals are complete"""
    t, ref = batch
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8),
             np.frombuffer(ref["text"], np.uint8), ref["atom_notes"])
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, t, caps)                                                      # run() checks the FILL bytes behind every capacity
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same_mols(a.mols, ref["mols"])
        for got, want in zip((a.atoms, a.bonds, a.text, a.side), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None, atom_notes=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]                           # the sizing call
    same_mols(a.mols, ref["mols"])
    a = run(eng, t, full, atom_notes=None)                                         # the notes are optional
    assert a.rc == 0 and a.totals.tolist() == full + [0] and np.all(a.side == FILL) and a.text.tobytes() == ref["text"]


def test_engine_normalize_pack_sizes_itself(eng, batch):
    t, ref = batch
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}
    for caps in (None, (1, 1, 1)):
        out = eng.normalize_pack(rec, caps=caps)
        same_mols(out["mols"], ref["mols"])
        assert out["atoms"].tobytes() == clean(ref["atoms"]) and out["bonds"].tobytes() == clean(ref["bonds"]) and out["text"] == ref["text"]
        assert out["atom_notes"].tolist() == ref["atom_notes"].tolist() and out["totals"].tolist() == list(ref["totals"]) + [0]


def test_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, [mol([b"C", b"[CH3]"], path(2))])

    def refused(expect, **over):
        assert_refused(run(eng, t, (64, 64, 64), **over), "mnx_normalize_pack: " + expect)

    for name in ("mols", "atoms", "bonds", "text", "mols_out", "atoms_out", "bonds_out", "text_out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, the output tables too, totals 4-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2), ("mols_out", 0), ("atoms_out", 1), ("bonds_out", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, totals=_p(t.d[0], 2))
    odd = torch.zeros(80, dtype=torch.uint8, device=dev)
    assert run(eng, t, (64, 64, 64), atom_notes=_p(odd, 1)).rc == 0                # a byte array needs no alignment
    assert odd.cpu().tolist()[:4] == [0, 3, 3 | 32, 0]
    assert run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None).rc == 0      # a table of capacity 0 may be null

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        assert run(bare, t, (64, 64, 64)).rc == -1
        assert bare.lib.mnx_last_error(bare.h) == b"mnx_normalize_pack: call mnx_set_symbol_tables first"
        Engine._set_symbol_tables(bare)                                            # no fragments are needed
        check(bare, t)
    finally:
        bare.close()


def canonical_of(eng, rec):
    recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
    return [None if int(r["flags"]) & SMILES_REFUSED else data[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in recs]


def test_chain_read_normalize_canonical(eng):
    """every Kekule / aromatic pair and every bracket pair of the hand table: EQUAL canonical bytes behind normalize, different
    ones without it"""
    pairs = sorted(H.AROMATIC.items()) + sorted(H.SAME_GRAPH.items()) + sorted((a, b) for a, b in H.BRACKETS.items() if a != b)
    left, right = [a for a, _ in pairs], [b for _, b in pairs]
    read = eng.smiles_read(left + right, keep_device=True)
    assert not read["read"]["flags"].any()
    plain = canonical_of(eng, read)
    normal = canonical_of(eng, eng.normalize_pack(read, keep_device=True))
    n = len(pairs)
    for k, (a, b) in enumerate(pairs):
        assert normal[k] == normal[n + k] and normal[k], (a, b, normal[k], normal[n + k])
        assert plain[k] != plain[n + k], (a, b, plain[k])
        assert normal[n + k] == plain[n + k]                                       # the normal spelling is a fixed point
    # the same through the caller's entry point
    theirs = canonical_smiles(eng, ["C1=CC=CC=C1", "c1ccccc1", "C[CH](C)F", "C("], normalize=True)
    assert theirs[0]["smiles"] == theirs[1]["smiles"] == "c1ccccc1" and theirs[2]["smiles"] == canonical_smiles(eng, ["CC(C)F"])[0]["smiles"]
    assert [x["normalize_flags"] for x in theirs] == [MOL_AROMATIZED, 0, MOL_UNBRACKETED, 0] and theirs[3]["smiles"] is None
    assert "normalize_flags" not in canonical_smiles(eng, ["C"])[0]
    # unchanged rows stay unchanged on the device too
    same = H.NOT_AROMATIC + [a for a, b in H.BRACKETS.items() if a == b]
    read = eng.smiles_read(same, keep_device=True)
    assert canonical_of(eng, read) == canonical_of(eng, eng.normalize_pack(read, keep_device=True))


def test_chain_expand_normalize(eng):
    """[Ph]C and Cc1ccccc1 compare equal behind the expansion already; behind normalize the Kekule toluene equals them too"""
    read = eng.smiles_read(["[Ph]C", "Cc1ccccc1", "CC1=CC=CC=C1", "[Ph][CH3]"], keep_device=True)
    grown = eng.expand_pack(read, keep_device=True)
    before = canonical_of(eng, grown)
    assert before[0] == before[1] and before[2] != before[0] and before[3] != before[0]
    after = canonical_of(eng, eng.normalize_pack(grown, keep_device=True))
    assert after[0] == after[1] == after[2] == after[3] == before[0]
    theirs = canonical_smiles(eng, ["[Ph]C", "CC1=CC=CC=C1"], expand=True, normalize=True)
    assert theirs[0]["smiles"] == theirs[1]["smiles"] == before[0].decode()


def test_end_to_end_predict_normalize_write(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: predict_pipeline(normalize=True, ...) against the oracles applied to the same run's un-normalised tables;
    without the switch the dicts are what they were; then the facade's graph_normalize"""
    import canon_ref as K
    import expand_ref as X
    from molnextr_amd.model import molnextr, unpack_graphs
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    grown = X.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tables=TABLES)
    for source, switches in ((rec, {}), (grown, {"expand": True})):
        ref = N.pack(source["mols"], source["atoms"], source["bonds"], source["text"], tables=TABLES)
        smi = K.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], 0, TABLES)
        mf = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=TABLES)
        plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True, **switches)
        normal = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True, normalize=True, **switches)
        after = unpack_graphs(ref["mols"], ref["atoms"], ref["bonds"], ref["text"])
        for b, (p, g) in enumerate(zip(plain, normal)):
            assert "normalized" not in p and set(g) == set(p) | {"normalized"}
            assert p["chartok_coords"] == g["chartok_coords"] and p["bonds"] == g["bonds"] and p.get("expanded") == g.get("expanded")
            r, m, f = smi["recs"][b], ref["mols"][b], mf["files"][b]
            a0, na = int(m["atom0"]), int(m["n_atoms"])
            written = not int(r["flags"]) & 0x33                                   # SMILES_REFUSED
            assert g["graph_smiles"] == (smi["out"][r["text0"]:r["text0"] + r["len"]].decode() if written else None)
            assert g["molfile"] == (mf["out"][f["text0"]:f["text0"] + f["len"]].decode() if f["len"] else None)
            notes = ref["atom_notes"][a0:a0 + na]
            assert g["normalized"] == {"symbols": after[b]["chartok_coords"]["symbols"], "bonds": after[b]["bonds"],
                                       "hydrogens": (notes & NOTE_H_MASK).tolist(), "notes": notes.tolist(), "flags": int(m["flags"])}
    with pytest.raises(ValueError, match="normalize=True needs packed=True"):
        predict_pipeline(eng, imgs[:1], normalize=True)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_normalize=True needs graph_smiles=True or graph_molfile=True"):
        molnextr("synthetic", dev, graph_normalize=True)
    pages = [W.synthetic_page(c) for c in range(4)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_canonical=True, graph_normalize=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True, canonical=True,
                                normalize=True)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert [o["hydrogens"] for o in got] == [p["normalized"]["hydrogens"] for p in want]
        m.graph_normalize = False                                                  # the default
        assert all("hydrogens" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()


TOLUENE = ("Ccccccc", [(0, 1, 1)] + [(k, k + 1, 4) for k in range(1, 6)] + [(1, 6, 4)])       # a prediction in aromatic form
ETHANOL = ("CCO", [(0, 1, 1), (1, 2, 1)])


def records_of(eng, molecules):
    """dense records (shard.pack_records) of hand-made predictions [(SMILES of the atoms, bonds (i, j, type))]"""
    from molnextr_amd.tokenizer import get_tokenizer
    tok = get_tokenizer()["chartok_coords"]
    kmax, n = eng.max_atoms, len(molecules)
    tokens, lengths = np.zeros((n, MAX_LEN), np.int32), np.zeros(n, np.int32)
    atom_idx, n_atoms, edges = np.zeros((n, kmax), np.int32), np.zeros(n, np.int32), np.zeros((n, kmax, kmax), np.uint8)
    for b, (smiles, bonds) in enumerate(molecules):
        k = len(bonds and {a for e in bonds for a in e[:2]}) or 1
        labels, indices = tok.smiles_to_sequence(smiles, coords=[[0.1 * a, 0.5] for a in range(k)], atom_only=True)
        assert len(indices) == k
        tokens[b, :len(labels)], lengths[b], atom_idx[b, :k], n_atoms[b] = labels, len(labels), indices, k
        for i, j, ty in bonds:
            edges[b, i, j] = edges[b, j, i] = ty
    return pack_records(tokens, lengths, atom_idx, n_atoms, edges, kmax)


def test_graph_match_normalized_counts_a_kekule_gold_row(eng):
    """evaluate's score function, as --graph_match --graph_normalize calls it, on three hand-made predictions: an aromatic toluene
    against a Kekule gold string (only the normalised score counts it), ethanol against ethanol (both), ethanol against
    ethylamine (neither)"""
    records = np.asarray(records_of(eng, [TOLUENE, ETHANOL, ETHANOL]))
    gold = ["CC1=CC=CC=C1", "OCC", "NCC"]
    assert E.graph_match_scores(eng, records, gold) == {"graph_match_device": 1 / 3, "gold_unreadable": 0, "pred_refused": 0}
    assert E.graph_match_scores(eng, records, gold, normalize=True) == {"graph_match_device": 1 / 3, "gold_unreadable": 0, "pred_refused": 0,
                                                                        "graph_match_normalized": 2 / 3}
    assert E.graph_match_scores(eng, records, ["Cc1ccccc1", "[CH3][CH2][OH]", "C("], chunk=2, normalize=True) == {
        "graph_match_device": 1 / 3, "gold_unreadable": 1, "pred_refused": 0, "graph_match_normalized": 2 / 3}


def test_evaluate_graph_normalize_on_a_three_row_file(eng, synth_ckpt, tmp_path, monkeypatch):
    """evaluate --graph_match --graph_normalize on a three-row file, through main(): pages in, scores file out. The synthetic
    checkpoint predicts near-complete graphs in which the rule finds no ring, so the records that the two graph scores read are
    put in the place of the checkpoint's once its inference has run: an aromatic toluene and two ethanols, against the gold
    column Kekule toluene, ethanol, ethylamine. graph_match_normalized counts the Kekule row, graph_match_device misses it."""
    import pandas as pd
    from PIL import Image
    hand = np.asarray(records_of(eng, [TOLUENE, ETHANOL, ETHANOL]))
    for k in range(3):
        Image.fromarray(W.synthetic_page(k)).save(tmp_path / f"p{k}.png")
    pd.DataFrame({"file_path": [f"p{k}.png" for k in range(3)], "SMILES": ["CC1=CC=CC=C1", "OCC", "NCC"]}).to_csv(tmp_path / "t.csv", index=False)
    real, seen = E.run_inference, []

    def run_inference(engine, *args, keep_records=None, **more):
        preds = real(engine, *args, keep_records=keep_records, **more)
        assert keep_records["records"].shape == hand.shape and keep_records["records"].dtype == hand.dtype
        keep_records["records"] = hand
        seen.append(len(preds))
        return preds

    monkeypatch.setattr(E, "run_inference", run_inference)
    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    argv = ["--data_path", str(tmp_path), "--test_file", "t.csv", "--save_path", str(tmp_path / "out"), "--load_path", "synthetic",
            "--batch_size", "2", "--graph_match"]
    E.main(argv + ["--graph_normalize"])
    with open(tmp_path / "out" / "eval_scores_t_best.json") as f:
        scores = json.load(f)
    assert seen == [3] and scores["graph_match_device"] == 1 / 3 and scores["graph_match_normalized"] == 2 / 3, scores
    assert scores["gold_unreadable"] == 0 and scores["pred_refused"] == 0 and "raw_string_match" in scores
    assert E.build_parser().parse_args(argv).graph_normalize is False              # opt-in
    with pytest.raises(SystemExit):
        E.main(argv[:-1] + ["--graph_normalize"])                                  # the flag adds to --graph_match
