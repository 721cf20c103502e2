"""GPU (-m gpu): mnx_kekulize_pack — Kekule structures for the aromatic systems of the packed tables, on the device — against the
oracle of tests/kekulize_ref.py, all four tables and `atom_notes` word for word (no tolerances), and against check_kekule(), which
judges the device's own output without knowing the search: the hand table of the host test, the generated set in batches of 1 and
33, the empty molecule, 999 atoms, the round trip through mnx_normalize_pack, the fixed point, the step limit, two systems in one
molecule, the capacity protocol, every refusal, determinism, molfiles without bond type 4, the facade and evaluate's
--graph_kekulize. The choice among valid matchings is the project's own order (include/molnextr_hip.h): not RDKit's Kekulize."""
import json

import numpy as np
import pytest
import torch

import kekulize_ref as Q
import molfile_ref as M
import normalize_ref as N
import packed_tables
import test_kekulize_host as K
import test_normalize_host as H
from molnextr_amd import evaluate as E
from molnextr_amd import weights as W
from molnextr_amd.engine import (MOL_KEKULE_LEFT, MOL_KEKULIZE_REFUSED, MOL_KEKULIZED, NOTE_KEKULE_LEFT, NOTE_KEKULE_LIMIT, NOTE_KEKULIZED,
                                 Engine)
from molnextr_amd.model import canonical_smiles, page_scale, predict_pipeline
from packed_tables import (FILL, Tables, _p, assert_refused, call_tables, clean, compare_tables, dev, eng, mol, path, same_mols,  # noqa: F401
                           same_results)
from test_gpu_normalize import ETHANOL, records_of

pytestmark = pytest.mark.gpu
TABLES = H.TABLES


def run(eng, t, caps, max_steps=0, **over):
    """one call at the capacities caps; the result's `side` is `atom_notes`"""
    return call_tables("mnx_kekulize_pack", eng, t, caps, step_cap=max_steps, **over)


def normalize(eng, t, caps, **over):
    return call_tables("mnx_normalize_pack", eng, t, caps, **over)


def as_rec(got):
    """a TablesResult at exact capacities as the dict check_kekule and Tables take"""
    return {"mols": got.mols, "atoms": got.atoms.view(packed_tables.ATOM_DTYPE), "bonds": got.bonds.view(packed_tables.BOND_DTYPE),
            "text": got.text.tobytes(), "atom_notes": got.side}


def check(eng, t, ref=None, max_steps=0, **cut):
    """the device's tables equal the oracle's at the exact capacities, word for word, and check_kekule accepts the DEVICE's output
    (a wrong oracle and a wrong kernel that agree are still caught); returns the oracle's"""
    ref = ref or Q.pack(t.mols, t.atoms, t.bonds, t.text, tables=TABLES, max_steps=max_steps, n_atom_records=cut.get("na"),
                        n_bond_records=cut.get("nb"), n_text_bytes=cut.get("nt"))
    got = run(eng, t, ref["totals"], max_steps, **cut)
    compare_tables(got, ref, "atom_notes")
    if not cut:
        bad = Q.check_kekule({"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}, as_rec(got), TABLES)
        assert not bad, bad[:5]
    return ref


def hand_strings():
    return sorted(K.HAND) + K.LEFT + K.UNTOUCHED


def test_the_hand_table_in_one_batch(eng, dev):
    strings = hand_strings()
    ref = check(eng, Tables(dev, arrays=H.tables_of(strings)))
    assert H.written(ref)[:len(K.HAND)] == [K.HAND[s] for s in sorted(K.HAND)]
    flags = ref["mols"]["flags"].tolist()
    assert all(f & MOL_KEKULIZED for f in flags[:len(K.HAND)]) and flags[len(K.HAND):] == [MOL_KEKULE_LEFT] * len(K.LEFT) + [0] * len(K.UNTOUCHED)


def test_scores_indices_and_the_truncated_bit_travel(eng, dev):
    mols, atoms, bonds, text = (x.copy() if isinstance(x, np.ndarray) else x for x in H.tables_of(hand_strings()))
    rng = np.random.default_rng(1)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"], atoms["x_bin"], atoms["y_bin"] = (rng.integers(0, 500, len(atoms)) for _ in range(3))
    mols["flags"] = rng.integers(0, 128, len(mols))                                # bit 0 travels, the other passes' bits do not
    bonds["rev"] = rng.integers(0, 7, len(bonds))
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert set((ref["mols"]["flags"] & 127).tolist()) == {0, 1}


@pytest.fixture(scope="module")
def generated(dev):
    """the aromatic generated set of the host test, eight random molecules of every symbol class and bond type in front of it (two
    records of one pair, type-4 records to upper-case atoms), and the oracle's tables"""
    arrays = K.generated_tables()
    rng = np.random.default_rng(3)
    wild = [packed_tables.random_molecule(rng, int(rng.integers(2, 40)), int(rng.integers(1, 60)), [b"c", b"c", b"c", b"n", b"[nH]", b"C", b"s", b"[Ph]"])
            for _ in range(8)]
    molecules = wild + [(s, xy, [b[:4] for b in bonds]) for s, xy, bonds in K.generated()]
    t = Tables(dev, molecules)
    assert t.n == 8 + len(arrays[0])
    return t, Q.pack(t.mols, t.atoms, t.bonds, t.text, tables=TABLES), molecules


def test_the_generated_set_in_one_batch_and_two_runs_with_identical_bytes(eng, generated):
    t, ref, _ = generated
    flags = ref["mols"]["flags"]
    assert (flags & MOL_KEKULIZED).astype(bool).sum() > 80 and (flags & MOL_KEKULE_LEFT).any() and not (flags & MOL_KEKULIZE_REFUSED).any()
    assert any(s["result"] == Q.BLOCKED for m in ref["systems"][:8] for s in m)
    check(eng, t, ref)
    same_results(run(eng, t, ref["totals"]), run(eng, t, ref["totals"]))


def test_the_generated_set_in_batches_of_1_and_33(eng, dev, generated):
    _, _, molecules = generated
    for size in (33, 1):
        for first in range(0, len(molecules) if size == 33 else 24, size):
            check(eng, Tables(dev, molecules[first:first + size]))


def test_the_empty_molecule_and_999_atoms(eng, dev):
    ref = check(eng, Tables(dev, [mol([])]))
    assert ref["mols"]["flags"].tolist() == [0] and ref["totals"] == (0, 0, 0)
    big = K.aromatic_acene(199, extra=201)
    ref = check(eng, Tables(dev, [mol([]), big, mol([b"[Ph]", b"[R1]", b"<unk>", b"", b"*"], path(5)), mol([b"c"])]))
    assert ref["mols"]["flags"].tolist() == [0, MOL_KEKULIZED, 0, MOL_KEKULE_LEFT] and ref["mols"]["n_atoms"].tolist() == [0, 999, 5, 1]
    assert (ref["atom_notes"][:999] & NOTE_KEKULIZED).astype(bool).sum() == 798
    # 999 atoms AND 999 bonds, the rings on the highest atom indices: 201 atoms with three bonds among them, then an acene of 199 rings
    syms, _, bonds = K.aromatic_acene(199)
    tail = 999 - len(syms)
    full = mol([b"C"] * tail + syms, sorted(path(4) + [(i + tail, j + tail, ty, rv) for i, j, ty, rv in bonds]))
    assert len(full[0]) == 999 and len(full[2]) == 999
    assert check(eng, Tables(dev, [full]))["mols"]["flags"].tolist() == [MOL_KEKULIZED]


def test_round_trip_and_fixed_point_on_the_device(eng, dev):
    """mnx_normalize_pack(mnx_kekulize_pack(mnx_normalize_pack(K))) equals mnx_normalize_pack(K) on the generated set — all four
    tables but for mols['flags'], which say what a call changed —, and a second mnx_kekulize_pack changes no table"""
    t = Tables(dev, arrays=K.generated_tables())                                   # normalize_ref(K) of the kept molecules
    caps = (len(t.atoms), len(t.bonds), len(t.text))
    once = normalize(eng, t, caps)
    assert once.rc == 0 and once.totals.tolist() == list(caps) + [0] and once.text.tobytes() == t.text
    kek = run(eng, Tables(dev, arrays=(once.mols, once.atoms.view(packed_tables.ATOM_DTYPE), once.bonds.view(packed_tables.BOND_DTYPE), once.text.tobytes())),
              (caps[0], caps[1], caps[2] + 4 * t.n))
    assert kek.rc == 0 and not kek.totals[3] and (kek.mols["flags"] & MOL_KEKULIZED).astype(bool).sum() > 0.9 * t.n
    sizes = tuple(int(x) for x in kek.totals[:3])
    kt = Tables(dev, arrays=(kek.mols, kek.atoms.view(packed_tables.ATOM_DTYPE)[:sizes[0]], kek.bonds.view(packed_tables.BOND_DTYPE)[:sizes[1]],
                             kek.text.tobytes()[:sizes[2]]))
    back = normalize(eng, kt, caps)
    assert back.rc == 0 and back.totals.tolist() == list(caps) + [0]
    for name in once.mols.dtype.names:
        if name != "flags":
            assert back.mols[name].tolist() == once.mols[name].tolist(), name
    assert back.atoms.tobytes() == once.atoms.tobytes() and back.bonds.tobytes() == once.bonds.tobytes() and back.text.tobytes() == once.text.tobytes()
    again = run(eng, kt, sizes)
    assert again.rc == 0 and again.totals.tolist() == list(sizes) + [0] and not (again.mols["flags"] & MOL_KEKULIZED).any()
    assert again.atoms.tobytes() == kt.atoms.tobytes() and again.bonds.tobytes() == clean(kt.bonds) and again.text.tobytes() == kt.text


def test_the_step_limit(eng, dev):
    """naphthalene needs five pairings, the pyridone two: at max_steps = 2 the first is left with the LIMIT note and copied bytes,
    the second is written; 0 is the default"""
    t = Tables(dev, arrays=H.tables_of(["c1ccc2ccccc2c1", "O=c1cccc[nH]1"]))
    cut = check(eng, t, max_steps=2)
    limit = NOTE_KEKULE_LEFT | NOTE_KEKULE_LIMIT
    assert cut["atom_notes"].tolist() == [limit | 1] * 3 + [limit] + [limit | 1] * 4 + [limit, limit | 1] + [64, 16] + [NOTE_KEKULIZED | 1] * 5
    assert cut["mols"]["flags"].tolist() == [MOL_KEKULE_LEFT, MOL_KEKULIZED]
    assert cut["bonds"]["type"][:11].tolist() == [4] * 11 and cut["text"][:10] == b"c" * 10      # copied
    assert H.written(check(eng, t)) == H.written(check(eng, t, max_steps=5)) == ["C1=CC=C2C=CC=CC2=C1", "O=C1C=CC=CN1"]
    assert check(eng, t, max_steps=4)["mols"]["flags"].tolist() == [MOL_KEKULE_LEFT, MOL_KEKULIZED]
    assert check(eng, t, max_steps=1)["mols"]["flags"].tolist() == [MOL_KEKULE_LEFT, MOL_KEKULE_LEFT]


def test_systems_of_one_molecule_are_handled_on_their_own(eng, dev):
    ref = check(eng, Tables(dev, arrays=H.tables_of([K.TRIANGULENE + ".c1ccccc1", "c1cccc1-c1ccccc1", "c1ccccc1." + K.TRIANGULENE])))
    assert ref["mols"]["flags"].tolist() == [MOL_KEKULIZED | MOL_KEKULE_LEFT] * 3
    assert H.written(ref) == [K.TRIANGULENE + ".C1=CC=CC=C1", "c1cccc1C1=CC=CC=C1", "C1=CC=CC=C1." + K.TRIANGULENE]


def test_capacities(eng, generated):
    """the text capacity one byte short, each record capacity one short, zero capacities: nothing is written beyond a capacity (the
    harness checks FILL and guard bytes behind every output), what lies in front of it is right, mols_out and totals are complete"""
    t, ref, _ = generated
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8),
             np.frombuffer(ref["text"], np.uint8), ref["atom_notes"])
    for k in (2, 0, 1):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, t, caps)
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same_mols(a.mols, ref["mols"])
        for got, want in zip((a.atoms, a.bonds, a.text, a.side), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None, atom_notes=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]                           # the sizing call
    same_mols(a.mols, ref["mols"])
    a = run(eng, t, full, atom_notes=None)                                         # the notes are optional
    assert a.rc == 0 and a.totals.tolist() == full + [0] and np.all(a.side == FILL) and a.text.tobytes() == ref["text"]


def test_engine_kekulize_pack_sizes_itself(eng, generated):
    t, ref, _ = generated
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}
    for caps in (None, (1, 1, 1)):
        out = eng.kekulize_pack(rec, caps=caps)
        same_mols(out["mols"], ref["mols"])
        assert out["atoms"].tobytes() == clean(ref["atoms"]) and out["bonds"].tobytes() == clean(ref["bonds"]) and out["text"] == ref["text"]
        assert out["atom_notes"].tolist() == ref["atom_notes"].tolist() and out["totals"].tolist() == list(ref["totals"]) + [0]
    limited = eng.kekulize_pack({k: v for k, v in zip(("mols", "atoms", "bonds", "text"), H.tables_of(["c1ccc2ccccc2c1"]))}, max_steps=2)
    assert limited["mols"]["flags"].tolist() == [MOL_KEKULE_LEFT] and (limited["atom_notes"] & NOTE_KEKULE_LIMIT).all()


def test_refused_molecules_leave_their_neighbours_alone(eng, dev):
    ok = mol([b"c", b"c"], [(0, 1, 4, 4)])
    molecules = [ok, mol([b"c"] * 1000, path(1000, 4)), ok, mol([b"c", b"c"], [(0, 2, 4, 4)]), mol([b"c", b"c"], [(2, 1, 4, 4)]), ok]
    t = Tables(dev, molecules)
    ref = check(eng, t)
    assert ref["mols"]["flags"].tolist() == [128, 512, 128, 512, 512, 128]
    assert ref["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 0, 2] and ref["text"] == b"C" * 6 and ref["bonds"]["type"].tolist() == [2, 2, 2]
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        want = check(eng, t, **cut)
        assert int(want["mols"]["flags"][-1]) == MOL_KEKULIZE_REFUSED and want["mols"]["n_atoms"].tolist()[:3] == [2, 0, 2]
    mols, atoms, bonds, text = M.build_tables([ok, ok])                            # a symbol behind the text
    atoms["sym0"][3] = 60000
    assert check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))["mols"]["flags"].tolist() == [MOL_KEKULIZED, MOL_KEKULIZE_REFUSED]
    mols, atoms, bonds, text = M.build_tables([ok])
    mols["atom0"][0] = 1 << 31                                                     # a record that points far beyond the tables
    assert check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))["mols"]["flags"].tolist() == [MOL_KEKULIZE_REFUSED]


def test_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, [mol([b"c", b"c"], [(0, 1, 4, 4)])])

    def refused(expect, **over):
        assert_refused(run(eng, t, (64, 64, 64), **over), "mnx_kekulize_pack: " + expect)

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
    assert odd.cpu().tolist()[:4] == [0, 16 | 2, 16 | 2, 0]
    assert run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None).rc == 0      # a table of capacity 0 may be null

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        assert run(bare, t, (64, 64, 64)).rc == -1
        assert bare.lib.mnx_last_error(bare.h) == b"mnx_kekulize_pack: call mnx_set_symbol_tables first"
        Engine._set_symbol_tables(bare)                                            # no fragments are needed
        check(bare, t)
    finally:
        bare.close()


def test_molfiles_of_the_hand_table_carry_no_bond_type_4(eng, dev):
    """mnx_molfile_pack on the kekulised tables of the hand table against molfile_ref on the oracle's tables; no bond line of
    type 4 in a molecule whose systems all succeeded, and such lines before the pass"""
    strings = sorted(K.HAND)
    arrays = H.tables_of(strings)
    ref = Q.pack(*arrays, tables=TABLES)
    out = eng.kekulize_pack(dict(zip(("mols", "atoms", "bonds", "text"), arrays)), keep_device=True)
    files, data = eng.molfile_pack(out)
    want = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=TABLES)
    assert data == want["out"] and files["len"].tolist() == want["files"]["len"].tolist()

    def aromatic_bond_lines(text, m):
        lines = text.split("\n")
        na, nb = int(m["n_atoms"]), int(m["n_bonds"])
        return sum(line[6:9] == "  4" for line in lines[4 + na:4 + na + nb])

    plain_files, plain = eng.molfile_pack(dict(zip(("mols", "atoms", "bonds", "text"), arrays)))
    for f, g, m in zip(files, plain_files, ref["mols"]):
        after = data[int(f["text0"]):int(f["text0"]) + int(f["len"])].decode()
        assert aromatic_bond_lines(plain[int(g["text0"]):int(g["text0"]) + int(g["len"])].decode(), m) > 0
        if not int(m["flags"]) & MOL_KEKULE_LEFT:
            assert aromatic_bond_lines(after, m) == 0 and "  2  0" in after


def test_the_callers_entry_points(eng):
    theirs = canonical_smiles(eng, ["c1ccccc1", "C1=CC=CC=C1", "c1ccc2C=CC=Cc2c1", "c1ccc2ccccc2c1", "C("], kekulize=True, normalize=True)
    assert theirs[0]["smiles"] == theirs[1]["smiles"] == "c1ccccc1" and theirs[2]["smiles"] == theirs[3]["smiles"] and theirs[4]["smiles"] is None
    assert [x["kekulize_flags"] for x in theirs] == [MOL_KEKULIZED, 0, MOL_KEKULIZED, MOL_KEKULIZED, 0]
    half = canonical_smiles(eng, ["c1ccc2C=CC=Cc2c1", "c1ccc2ccccc2c1"], normalize=True)
    assert half[0]["smiles"] != half[1]["smiles"] and "kekulize_flags" not in half[0]           # what the pass is for
    azulene = canonical_smiles(eng, ["c1ccc2cccc2cc1", "C1=CC=C2C=CC=C2C=C1"], kekulize=True)
    assert azulene[0]["smiles"] == azulene[1]["smiles"] and "c" not in azulene[0]["smiles"]


def test_end_to_end_predict_kekulize_write(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: predict_pipeline(kekulize=True, ...) against the oracles applied to the same run's tables, in front of
    normalize when both are set; without the switch the dicts are what they were; then the facade's graph_kekulize"""
    import canon_ref as C
    from molnextr_amd.model import molnextr, unpack_graphs
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    kek = Q.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tables=TABLES)
    for normal in (False, True):
        ref = N.pack(kek["mols"], kek["atoms"], kek["bonds"], kek["text"], tables=TABLES) if normal else kek
        smi = C.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], 0, TABLES)
        mf = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=TABLES)
        switches = {"normalize": True} if normal else {}
        plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True, **switches)
        got = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True, kekulize=True, **switches)
        after = unpack_graphs(kek["mols"], kek["atoms"], kek["bonds"], kek["text"])
        for b, (p, g) in enumerate(zip(plain, got)):
            assert "kekulized" not in p and set(g) == set(p) | {"kekulized"}
            assert p["chartok_coords"] == g["chartok_coords"] and p["bonds"] == g["bonds"]
            r, m, f = smi["recs"][b], kek["mols"][b], mf["files"][b]
            a0, na = int(m["atom0"]), int(m["n_atoms"])
            written = not int(r["flags"]) & 0x33                                   # SMILES_REFUSED
            assert g["graph_smiles"] == (smi["out"][r["text0"]:r["text0"] + r["len"]].decode() if written else None)
            assert g["molfile"] == (mf["out"][f["text0"]:f["text0"] + f["len"]].decode() if f["len"] else None)
            notes = kek["atom_notes"][a0:a0 + na]
            assert g["kekulized"] == {"symbols": after[b]["chartok_coords"]["symbols"], "bonds": after[b]["bonds"],
                                      "hydrogens": (notes & 15).tolist(), "notes": notes.tolist(), "flags": int(m["flags"])}
    with pytest.raises(ValueError, match="kekulize=True needs packed=True"):
        predict_pipeline(eng, imgs[:1], kekulize=True)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_kekulize=True needs graph_smiles=True or graph_molfile=True"):
        molnextr("synthetic", dev, graph_kekulize=True)
    pages = [W.synthetic_page(c) for c in range(4)]
    m = molnextr("synthetic", dev, max_batch=4, graph_molfile=True, graph_kekulize=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, molfile=True, kekulize=True,
                                molfile_scale=[page_scale(p) for p in pages])
        assert [o["kekulized"] for o in got] == [p["kekulized"] for p in want]
        from molnextr_amd.chem import have_rdkit
        if not have_rdkit():
            assert [o["predicted_molfile"] for o in got] == [p["molfile"] for p in want]
        m.graph_kekulize = False                                                   # the default
        assert all("kekulized" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()


AZULENE = ("cccccccccc", [(k, k + 1, 4) for k in range(9)] + [(3, 7, 4), (0, 9, 4)])          # a prediction in aromatic form
NAPHTHALENE = ("cccccccccc", [(k, k + 1, 4) for k in range(9)] + [(3, 8, 4), (0, 9, 4)])


def test_graph_match_kekulized_counts_an_azulene_pair(eng):
    """evaluate's score function, as --graph_match --graph_kekulize calls it, on hand-made predictions: an aromatic azulene
    against its Kekule gold string (only the kekulised score counts it: normalize finds no ring of 7), an aromatic naphthalene
    against a Kekule gold string (the normalised and the kekulised score), ethanol against ethanol (all), against ethylamine (none)"""
    records = np.asarray(records_of(eng, [AZULENE, NAPHTHALENE, ETHANOL, ETHANOL]))
    gold = ["C1=CC=C2C=CC=C2C=C1", "C1=CC=C2C=CC=CC2=C1", "OCC", "NCC"]
    base = {"graph_match_device": 1 / 4, "gold_unreadable": 0, "pred_refused": 0}
    assert E.graph_match_scores(eng, records, gold) == base
    assert E.graph_match_scores(eng, records, gold, normalize=True) == {**base, "graph_match_normalized": 2 / 4}
    assert E.graph_match_scores(eng, records, gold, kekulize=True) == {**base, "graph_match_kekulized": 3 / 4}
    assert E.graph_match_scores(eng, records, gold, chunk=3, normalize=True, kekulize=True) == {
        **base, "graph_match_normalized": 2 / 4, "graph_match_kekulized": 3 / 4}


def test_evaluate_graph_kekulize_on_a_four_row_file(eng, synth_ckpt, tmp_path, monkeypatch):
    """evaluate --graph_match --graph_kekulize through main(): pages in, scores file out. The synthetic checkpoint predicts
    near-complete graphs without a ring the rule would touch, so the records that the graph scores read are put in the place of
    the checkpoint's once its inference has run, as the normalize test does"""
    import pandas as pd
    from PIL import Image
    hand = np.asarray(records_of(eng, [AZULENE, NAPHTHALENE, ETHANOL, ETHANOL]))
    for k in range(4):
        Image.fromarray(W.synthetic_page(k)).save(tmp_path / f"p{k}.png")
    pd.DataFrame({"file_path": [f"p{k}.png" for k in range(4)],
                  "SMILES": ["C1=CC=C2C=CC=C2C=C1", "C1=CC=C2C=CC=CC2=C1", "OCC", "NCC"]}).to_csv(tmp_path / "t.csv", index=False)
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
    E.main(argv + ["--graph_normalize", "--graph_kekulize"])
    with open(tmp_path / "out" / "eval_scores_t_best.json") as f:
        scores = json.load(f)
    assert seen == [4] and scores["graph_match_device"] == 1 / 4 and scores["graph_match_normalized"] == 2 / 4, scores
    assert scores["graph_match_kekulized"] == 3 / 4 and scores["gold_unreadable"] == 0 and scores["pred_refused"] == 0
    assert E.build_parser().parse_args(argv).graph_kekulize is False               # opt-in
    with pytest.raises(SystemExit):
        E.main(argv[:-1] + ["--graph_kekulize"])                                   # the flag adds to --graph_match
