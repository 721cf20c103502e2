"""GPU (-m gpu): mnx_main_pack — of every packed molecule the connected component with the most atoms, the rest dropped on the
device — against the oracle of tests/main_ref.py, byte for byte at exact capacities (no tolerances), guard bytes included: the
hand-made cases of the host test, the shapes at which the label propagation, the scans over the atoms and the tiles of the bond
scan take another turn, the refusals, the capacity protocol, determinism, the argument errors, the documented place in the chain
of passes, and one end-to-end run."""
import functools

import numpy as np
import pytest

import main_ref as X
import molfile_ref as M
import packed_tables
import test_main_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import MOL_MAIN_KEPT, MOL_MAIN_REFUSED, MOL_MAIN_TIE, READ_REFUSED, SMILES_REFUSED, Engine
from packed_tables import (POOL, UTF2, Tables, _p, assert_refused, call_tables, clean, compare_tables, dev, eng, mol,  # noqa: F401
                           random_molecule, same_mols, same_results)

pytestmark = pytest.mark.gpu

packed_tables.TABLE_ARGS["mnx_main_pack"] = packed_tables.TABLE_ARGS["mnx_expand_pack"]      # expand's argument list, exactly
run = functools.partial(call_tables, "mnx_main_pack")          # run(eng, t, caps, **over); the result's `side` is `origin`

E2E_FIRST_INDEX = 500          # the batch of the writers' end-to-end tests


def check(eng, t, ref=None):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    ref = ref or X.pack(t.mols, t.atoms, t.bonds, t.text)
    compare_tables(run(eng, t, ref["totals"]), ref, "origin")
    return ref


def two_strands():
    """17 atoms, the even ones a path and the odd ones a path: the kept atoms straddle every boundary between the 8 neighbouring
    atoms a thread scans, the last atom is one past two threads' worth; symbols of 0, 1, 2, 6 and 17 bytes among them"""
    lengths = [b"", b"[NH3+]", UTF2, b"[3,5-[CF3]2C6H3]", b"C"]
    assert all(s in POOL for s in lengths)
    syms = [lengths[(k * 3 + k // 5) % 5] for k in range(17)]
    return mol(syms, [(k, k + 2, 1 + k % 3, 1 + k % 2) for k in range(15)])


def test_hand_made_molecules_one_by_one_and_together(eng, dev):
    molecules = H.MOLECULES + [two_strands()]
    for m in molecules:
        check(eng, Tables(dev, [m]))                                               # n = 1
    ref = check(eng, Tables(dev, molecules))
    assert ref["mols"]["flags"].tolist() == [c[2][3] for c in H.CASES] + [MOL_MAIN_KEPT]
    assert ref["mols"]["n_atoms"].tolist() == [c[2][0] for c in H.CASES] + [9]
    a0 = int(ref["mols"]["atom0"][-1])
    assert ref["origin"][a0:].tolist() == list(range(0, 17, 2))
    lens = ref["atoms"]["sym_len"][a0:].tolist()
    assert len(set(lens)) >= 4 and ref["atoms"]["sym0"][a0:].tolist() == np.cumsum([0] + lens[:-1]).tolist()


def test_scores_indices_and_the_truncated_bit_travel(eng, dev):
    mols, atoms, bonds, text = M.build_tables(H.MOLECULES + [two_strands()])
    rng = np.random.default_rng(1)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"] = rng.integers(0, 500, len(atoms))
    mols["flags"] = rng.integers(0, 2, len(mols)) | 2 | 16 | 1 << 10 | 1 << 20       # bits of other passes are not copied
    check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))


def strand(order, ty=1):
    """a path through the atoms in `order`"""
    return [(int(a), int(b), ty, ty) for a, b in zip(order[:-1], order[1:])]


@pytest.mark.parametrize("numbering", ["ascending", "descending", "permuted", "interleaved"])
def test_2047_atoms_converge(eng, dev, numbering):
    """the largest molecule, as the shapes on which a propagation that stops early, or needs a round per atom, shows: a path of
    2046 atoms numbered three ways beside one isolated atom, and two interleaved paths of 1024 and 1023 atoms"""
    n = 2047
    if numbering == "interleaved":
        bonds, kept = strand(range(0, n, 2)) + strand(range(1, n, 2)), 1024
    else:
        order = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": np.random.default_rng(2047).permutation(n)}[numbering]
        bonds, kept = strand(order[:-1]), 2046                                     # order[-1] is the isolated atom
    ref = check(eng, Tables(dev, [mol([b"C"] * n, bonds)]))
    assert ref["mols"]["flags"].tolist() == [MOL_MAIN_KEPT] and ref["mols"]["n_atoms"].tolist() == [kept]
    assert ref["mols"]["n_bonds"].tolist() == [kept - 1]


def test_bond_records_beyond_two_tiles_of_the_bond_scan(eng, dev):
    """700 bond records, more than two tiles of 256: kept and dropped records alternate, so every tile hands a carry on; pairs
    repeat, which is legal"""
    kept, dropped = [(0, 1), (1, 2), (2, 0), (1, 0)], [(3, 4), (4, 3), (5, 5)]
    bonds = [(*(kept[k // 2 % 4] if k % 2 == 0 else dropped[k // 2 % 3]), 1 + k % 6, k % 7) for k in range(700)]
    mols, atoms, bonds, text = M.build_tables([mol([b"C", b"N", b"O", b"Cl", b"Br", b"I"], bonds), mol([b"C", b"N"], [(0, 1, 1, 1)])])
    bonds["score"] = np.random.default_rng(3).random(len(bonds))
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert ref["mols"]["n_bonds"].tolist() == [350, 1] and ref["mols"]["flags"].tolist() == [MOL_MAIN_KEPT, 0]
    assert ref["bonds"]["score"][:350].tolist() == bonds["score"][:700:2].tolist()


def test_refusals_leave_the_other_molecules_alone(eng, dev):
    ok = mol([b"C", b"[NH3+]", b"O"], [(1, 2, 1, 1)])
    t = Tables(dev, [ok, mol([b"C"] * 2048, strand(range(2048))), ok, mol([b"C", b"N"], [(0, 2, 1, 1)]),
                     mol([b"C", b"N"], [(2, 0, 1, 1)]), mol([b"C"] * 2047, strand(range(2047))), ok])
    ref = check(eng, t)
    assert [int(f) for f in ref["mols"]["flags"]] == [MOL_MAIN_KEPT, MOL_MAIN_REFUSED, MOL_MAIN_KEPT, MOL_MAIN_REFUSED, MOL_MAIN_REFUSED,
                                                      0, MOL_MAIN_KEPT]
    assert ref["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 0, 2047, 2]
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        want = X.pack(t.mols, t.atoms, t.bonds, t.text, n_atom_records=cut.get("na"), n_bond_records=cut.get("nb"), n_text_bytes=cut.get("nt"))
        assert int(want["mols"]["flags"][-1]) == MOL_MAIN_REFUSED and want["mols"]["n_atoms"].tolist()[:-1] == [2, 0, 2, 0, 0, 2047]
        compare_tables(run(eng, t, want["totals"], **cut), want, "origin")
    mols, atoms, bonds, text = M.build_tables([ok, ok])
    atoms["sym0"][3] = 60000                                                       # a symbol beyond the text
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert ref["mols"]["flags"].tolist() == [MOL_MAIN_KEPT, MOL_MAIN_REFUSED]


@pytest.fixture(scope="module")
def batch(dev):
    """64 random molecules of 0 to 40 atoms of every symbol class with about half as many bonds as atoms, and the oracle's result"""
    rng = np.random.default_rng(64)
    molecules = []
    for _ in range(64):
        na = int(rng.integers(0, 41))
        molecules.append(random_molecule(rng, na, na // 2 + int(rng.integers(0, 3))))
    t = Tables(dev, molecules)
    return t, X.pack(t.mols, t.atoms, t.bonds, t.text)


def test_64_random_molecules_and_two_runs_with_identical_bytes(eng, batch):
    t, ref = batch
    flags = ref["mols"]["flags"]
    assert ((flags & MOL_MAIN_KEPT) != 0).sum() >= 32 and ((flags & MOL_MAIN_TIE) != 0).sum() >= 4
    check(eng, t, ref)
    same_results(run(eng, t, ref["totals"]), run(eng, t, ref["totals"]))


def test_capacities_exact_and_one_short(eng, batch):
    """each capacity one record or byte short, separately: nothing is written at or beyond it (origin follows atom_cap), what lies
    in front of it is right, mols_out and totals are complete, and a second call at totals equals the oracle"""
    t, ref = batch
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8),
             np.frombuffer(ref["text"], np.uint8), ref["origin"].view(np.uint8))
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, t, caps)                                                      # run() checks the FILL bytes behind every capacity
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same_mols(a.mols, ref["mols"])
        for got, want in zip((a.atoms, a.bonds, a.text, a.side), exact):
            assert np.array_equal(got, want[:len(got)])
        compare_tables(run(eng, t, a.totals.tolist()[:3]), ref, "origin")
    a = run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None, origin=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]                           # the sizing call
    same_mols(a.mols, ref["mols"])
    a = run(eng, t, full, origin=None)                                             # origin may be null
    assert a.rc == 0 and a.totals.tolist() == full + [0] and a.atoms.tobytes() == clean(ref["atoms"])


def test_engine_main_pack_sizes_itself(eng, batch):
    t, ref = batch
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}
    for caps in (None, (1, 1, 1)):
        out = eng.main_pack(rec, caps=caps)
        same_mols(out["mols"], ref["mols"])
        assert out["atoms"].tobytes() == clean(ref["atoms"]) and out["bonds"].tobytes() == clean(ref["bonds"]) and out["text"] == ref["text"]
        assert out["origin"].tolist() == ref["origin"].tolist() and out["totals"].tolist() == list(ref["totals"]) + [0]


def test_main_pack_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, H.MOLECULES)
    ref = X.pack(t.mols, t.atoms, t.bonds, t.text)

    def refused(expect, **over):
        assert_refused(run(eng, t, (64, 64, 64), **over), "mnx_main_pack: " + expect)

    for name in ("mols", "atoms", "bonds", "text", "mols_out", "atoms_out", "bonds_out", "text_out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, the output tables too, totals 4-byte, origin 2-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2), ("mols_out", 0), ("atoms_out", 1), ("bonds_out", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, atoms_out=_p(t.d[1], 1))                                      # an odd pointer
    refused(aligned, totals=_p(t.d[0], 2))
    refused(aligned, origin=_p(t.d[0], 1))

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        compare_tables(run(eng, t, ref["totals"], h=bare.h), ref, "origin")       # it needs neither symbol tables nor fragments
        refused("null pointer", mols=None)
        a = run(eng, t, (64, 64, 64), h=bare.h, n=0)                               # the error text is the called handle's
        assert_refused(a, "mnx_main_pack: 1 <= n <= 65536 required")
        assert eng.lib.mnx_last_error(eng.h).decode() == "mnx_main_pack: null pointer"
    finally:
        bare.close()


def canonical(eng, rec):
    recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
    assert not (recs["flags"] & SMILES_REFUSED).any()
    return [data[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in recs]


def test_the_place_in_the_chain(eng):
    """read -> main -> canonical writer: the salt is gone; and the documented order: a label counts one atom in front of
    mnx_expand_pack and the atoms it stands for behind it"""
    rec = eng.smiles_read(["CCO.[Na+]", "CCO", "[Ph].CCCCC"], keep_device=True)
    assert not (rec["read"]["flags"] & READ_REFUSED).any() and rec["mols"]["n_atoms"].tolist() == [4, 3, 6]
    main = eng.main_pack(rec, keep_device=True)
    assert main["mols"]["flags"].tolist() == [MOL_MAIN_KEPT, 0, MOL_MAIN_KEPT] and main["mols"]["n_atoms"].tolist() == [3, 3, 5]
    first = canonical(eng, eng.expand_pack(main, keep_device=True))
    assert first[0] == first[1] and len(first[0]) > 0
    grown = eng.expand_pack(rec, keep_device=True)
    assert grown["mols"]["n_atoms"].tolist() == [4, 3, 11]
    behind = eng.main_pack(grown, keep_device=True)
    assert behind["mols"]["n_atoms"].tolist() == [3, 3, 6] and behind["origin"][6:].tolist() == [0, 6, 7, 8, 9, 10]
    second = canonical(eng, behind)
    chain, ring = canonical(eng, eng.expand_pack(eng.smiles_read(["CCCCC", "[Ph]"], keep_device=True), keep_device=True))
    assert first[2] == chain and second[2] == ring and chain != ring and second[:2] == first[:2]


def test_end_to_end_predict_keep_main_write(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: predict_pipeline(packed=True, smiles=True, keep_main=True) against the passes applied by hand to the
    tables of the same prediction; without keep_main the dicts are what they were; canonical_smiles; then the facade's
    graph_keep_main"""
    from molnextr_amd.model import canonical_smiles, molnextr, predict_pipeline, unpack_graphs
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4), keep_device=True)
    ref = X.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"])
    main = eng.main_pack(rec, keep_device=True)
    same_mols(main["mols"], ref["mols"])
    assert main["atoms"].tobytes() == clean(ref["atoms"]) and main["bonds"].tobytes() == clean(ref["bonds"]) and main["text"] == ref["text"]
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True)
    kept = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, keep_main=True)
    before = unpack_graphs(rec["mols"], rec["atoms"], rec["bonds"], rec["text"])
    after = unpack_graphs(main["mols"], main["atoms"], main["bonds"], main["text"])
    texts = []
    for side in (rec, main):
        recs, order, data = eng.smiles_pack(side)
        texts.append((recs, order, data))
    for b, (p, g) in enumerate(zip(plain, kept)):
        assert "main" not in p and set(g) == set(p) | {"main"}
        assert p["chartok_coords"] == g["chartok_coords"] == before[b]["chartok_coords"] and p["bonds"] == g["bonds"] == before[b]["bonds"]
        for got, (recs, order, data), m in ((p, texts[0], rec["mols"][b]), (g, texts[1], main["mols"][b])):
            r, a0, na = recs[b], int(m["atom0"]), int(m["n_atoms"])
            written = not int(r["flags"]) & SMILES_REFUSED
            assert got["graph_smiles"] == (data[int(r["text0"]):int(r["text0"]) + int(r["len"])].decode() if written else None)
            assert got["graph_smiles_order"] == (order[a0:a0 + na].tolist() if written else None)
        m = main["mols"][b]
        a0, na = int(m["atom0"]), int(m["n_atoms"])
        assert g["main"] == {"symbols": after[b]["chartok_coords"]["symbols"], "coords": after[b]["chartok_coords"]["coords"],
                             "bonds": after[b]["bonds"], "origin": main["origin"][a0:a0 + na].tolist(), "flags": int(m["flags"])}
        if g["graph_smiles"] is not None:
            assert "." not in g["graph_smiles"]
    with pytest.raises(ValueError, match="keep_main=True needs packed=True"):
        predict_pipeline(eng, imgs[:1], keep_main=True)

    got = canonical_smiles(eng, ["CCO.[Na+]", "CCO", "[Ph].CCCCC"], expand=True, keep_main=True)
    assert got[0]["smiles"] == got[1]["smiles"] and [x["main_flags"] & MOL_MAIN_KEPT for x in got] == [MOL_MAIN_KEPT, 0, MOL_MAIN_KEPT]
    assert got[2]["smiles"] == canonical_smiles(eng, ["[Ph]"], expand=True)[0]["smiles"]
    assert all("main_flags" not in x for x in canonical_smiles(eng, ["CCO.[Na+]"]))

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_keep_main=True needs graph_smiles=True or graph_molfile=True"):
        molnextr("synthetic", dev, graph_keep_main=True)
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_keep_main=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True, keep_main=True)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert [o["main_atoms"] for o in got] == [p["main"]["origin"] for p in want] and [o["main"] for o in got] == [p["main"] for p in want]
        m.graph_keep_main = False                                                  # the default: every atom is written
        assert all("main_atoms" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()


def test_evaluate_graph_match_main(eng):
    """evaluate's --graph_match --graph_keep_main on 8 synthetic pages: the gold column is the canonical string of every
    prediction's main molecule, read back as a caller's own SMILES — graph_match_main is the share the writer accepts, whatever
    stray atoms a prediction holds, and the other scores are what they are without the flag"""
    import torch
    from molnextr_amd import evaluate as E
    from molnextr_amd.shard import MAX_LEN
    kept, n, kmax = {}, 8, eng.max_atoms
    E.run_inference(eng, lambda i: W.synthetic_page(i % 15), n, batch_size=4, keep_records=kept)
    r = torch.from_numpy(kept["records"]).to(torch.device("cuda", 0))
    edges = r[:, 2 + MAX_LEN + kmax:].contiguous().view(torch.uint8)[:, :kmax * kmax].reshape(n, kmax, kmax).contiguous()
    pack = eng.graph_pack({"lengths": r[:, 0].contiguous(), "n_atoms": r[:, 1].contiguous(), "tokens": r[:, 2:2 + MAX_LEN].contiguous(),
                           "atom_idx": r[:, 2 + MAX_LEN:2 + MAX_LEN + kmax].contiguous(), "edges": edges}, keep_device=True)
    recs, _, data, _, _ = eng.smiles_pack(eng.main_pack(pack, keep_device=True), canonical=True)
    own = [None if int(x["flags"]) & SMILES_REFUSED else data[int(x["text0"]):int(x["text0"]) + int(x["len"])].decode() for x in recs]
    written = sum(t is not None for t in own)
    gold = [t if t is not None else "C" for t in own]
    plain = E.graph_match_scores(eng, kept["records"], gold, chunk=4)
    scores = E.graph_match_scores(eng, kept["records"], gold, chunk=4, keep_main=True)
    assert set(plain) == {"graph_match_device", "gold_unreadable", "pred_refused"} and {k: scores[k] for k in plain} == plain
    assert scores["graph_match_main"] == written / n >= plain["graph_match_device"] and scores["gold_unreadable"] == 0, (scores, written)
    assert E.build_parser().parse_args(["--test_file", "t.csv", "--load_path", "synthetic", "--graph_match", "--graph_keep_main"]).graph_keep_main
