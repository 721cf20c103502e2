"""GPU (-m gpu): mnx_formula_pack — condensed-formula labels replaced on the device by the structure a valence search finds —
against the oracle of tests/formula_ref.py, records field by field and tables byte for byte (no tolerances): the smallest shapes at
which the kernel's scans, batches and loops take another turn (one label, labels at both ends, two labels, a table label next to
one, no label, a refused molecule, 257 molecules, more candidates than one batch of search lanes), the capacity protocol, the
argument errors, determinism, the step limit, the label-versus-table-name pairs of the host test through the device chain, and
Engine.formula_pack, predict_pipeline(formula=True) and canonical_smiles(formula=True)."""
import numpy as np
import pytest

import expand_ref as X
import formula_ref as F
import molfile_ref as M
import test_formula_host as FH
import test_normalize_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import (FORMULA_DEFAULT_STEPS, MOL_FORMULA_EXPANDED, MOL_FORMULA_LEFT, MOL_FORMULA_LIMIT, MOL_FORMULA_REFUSED,
                                 Engine)
from packed_tables import Tables, _p, assert_refused, call_tables, clean, compare_tables, dev, eng, mol, path, same_mols, same_results  # noqa: F401

pytestmark = pytest.mark.gpu

TABLES, FRAGS = FH.TABLES, FH.FRAGS
SEARCH_LANES = 32               # labels one workgroup searches side by side (formula.hip FM_LANES)


def run(eng, t, caps, max_steps=0, **over):
    return call_tables("mnx_formula_pack", eng, t, caps, step_cap=max_steps, **over)


def oracle(t, **kw):
    return F.pack(t.mols, t.atoms, t.bonds, t.text, frags=FRAGS, tables=TABLES, **kw)


def check(eng, t, ref=None, max_steps=0):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    ref = ref or oracle(t, max_steps=max_steps)
    compare_tables(run(eng, t, ref["totals"], max_steps), ref, "origin")
    return ref


MANY = [b"[CH2CH3]", b"[OCH2Ph]", b"C", b"[N(CH3)2]", b"[C6H5]"] * 14                  # 56 candidates: two batches, the second partial
MANY_BONDS = [(5 * g + 2, 5 * g + k, 1, 1) if k > 2 else (5 * g + k, 5 * g + 2, 1, 1) for g in range(14) for k in (0, 1, 3, 4)]
SMALL = [
    mol([b"[CH2CH3]"]),                                                                # one molecule of one label, no bond: no structure
    mol([b"C", b"[CH2CH3]"], path(2)),                                                 # one bond
    mol([b"[COOCH3]", b"C", b"N", b"[Si(CH3)3]"], path(4)),                            # labels at index 0 and at the last index
    mol([b"[CH2Ph]", b"[NHCOCH3]"], path(2)),                                          # two labels bonded to each other
    mol([b"C", b"[OMe]", b"[SO2CH3]", b"[R1]", b"CH2I"], [(0, 1, 1, 1), (0, 2, 1, 1), (0, 3, 1, 1), (0, 4, 5, 6)]),     # next to table labels; a wedge
    mol([b"C", b"N", b"O", b"[nH]", b"[Ph]"], path(5)),                                # no candidate
    mol([]),                                                                           # no atom
    mol([b"C", b"[CH2CH3]", b"N"], [(1, 2, 1, 1), (0, 1, 1, 1)]),                      # refused: bond records not sorted by i
    mol([b"C", b"[CHCH3]", b"[C(CH3)2]", b"N"], [(0, 1, 2, 2), (0, 2, 1, 1), (2, 3, 2, 2)]),   # a double bond onto a label; a two-ended label stays
    mol([b"c", b"[CH2CH3]", b"C", b"[CH2CH3]"], [(0, 1, 4, 4), (2, 3, 7, 7)]),         # a class-4 bond and a type that is no order: both stay
    mol([b"C", b"[C6H5]", b"[CH=CH2]", b"[PO3H2]", b"[" + b"C" * 21 + b"]", b"[C33H68]"], [(0, k, 1, 1) for k in range(1, 6)]),
]


def test_small_molecules_one_by_one_and_together(eng, dev):
    for m in SMALL:
        check(eng, Tables(dev, [m]))                                                   # n = 1
    ref = check(eng, Tables(dev, SMALL))
    flags = ref["mols"]["flags"].tolist()
    assert flags == [MOL_FORMULA_LEFT, MOL_FORMULA_EXPANDED, MOL_FORMULA_EXPANDED, MOL_FORMULA_EXPANDED, MOL_FORMULA_EXPANDED, 0, 0,
                     MOL_FORMULA_REFUSED, MOL_FORMULA_EXPANDED | MOL_FORMULA_LEFT, MOL_FORMULA_LEFT, MOL_FORMULA_LEFT]
    assert ref["mols"]["n_atoms"].tolist()[:5] == [1, 3, 4 + 3 + 3, 2 + 1 + 3, 5 + 3 + 1]


def test_scores_indices_and_the_truncated_bit_travel(eng, dev):
    mols, atoms, bonds, text = M.build_tables(SMALL)
    rng = np.random.default_rng(1)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"] = rng.integers(0, 500, len(atoms))
    mols["flags"] = rng.integers(0, 2, len(mols))
    check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))


def random_batch(rng, n):
    pool = [b"C", b"N", b"O", b"c", b"[Ph]", b"[OMe]", b"[R1]", b"[Xx]", b"Cl"] + [b"[%s]" % s.encode() for s in FH.CORPUS]
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 9))
        syms = [pool[i] for i in rng.integers(0, len(pool), k)]
        bonds = sorted({(int(rng.integers(0, j)), j) for j in range(1, k)})            # a tree: every atom on an earlier one
        out.append(mol(syms, [(i, j, ty, ty) for (i, j), ty in zip(bonds, rng.choice([1, 1, 1, 2, 3, 4, 5], len(bonds)))]))
    return out


@pytest.fixture(scope="module")
def batch(dev):
    """257 random small molecules with labels of the corpus (one past a block of 256 in the scan over the molecules)"""
    t = Tables(dev, random_batch(np.random.default_rng(11), 257))
    return t, oracle(t)


def test_257_random_molecules_and_two_runs_with_identical_bytes(eng, batch):
    t, ref = batch
    flags = ref["mols"]["flags"]
    assert (flags & MOL_FORMULA_EXPANDED).astype(bool).sum() > 100 and (flags & MOL_FORMULA_LEFT).any()
    check(eng, t, ref)
    same_results(run(eng, t, ref["totals"]), run(eng, t, ref["totals"]))


def test_more_candidates_than_one_batch_of_lanes_and_large_molecules(eng, dev):
    assert sum(s[:1] == b"[" for s in MANY) > SEARCH_LANES
    rng = np.random.default_rng(3)
    pool = [b"C", b"N", b"[CH2CH3]", b"[OCH3]", b"[COOC2H5]", b"[R1]", b"c", b"[NHCH3]"]
    big = [pool[k] for k in rng.integers(0, len(pool), 257)]                           # more than one pass of a 256-thread workgroup
    most = [b"C", b"[CH2Cl]"] * 1023 + [b"C"]                                          # 2047 atoms, 1023 labels: the most that is taken
    comb = sorted([(k, k + 1, 1, 1) for k in range(0, 2046, 2)] + [(k, k + 2, 1, 1) for k in range(0, 2045, 2)])
    t = Tables(dev, [mol(MANY, sorted(MANY_BONDS)), mol(big, sorted(path(257) + [(0, 256, 1, 1)])), mol(most, comb),
                     mol([b"C"] * 2048, path(2048)), mol([b"C", b"[CH2CH3]"], [(0, 2, 1, 1)]), mol([b"C", b"[CH2CH3]"], path(2))])
    ref = check(eng, t)
    assert [int(f) & MOL_FORMULA_REFUSED for f in ref["mols"]["flags"]] == [0, 0, 0, MOL_FORMULA_REFUSED, MOL_FORMULA_REFUSED, 0]
    assert ref["mols"]["n_atoms"].tolist()[2:] == [2047 + 1023, 0, 0, 3] and ref["mols"]["n_atoms"][0] == 70 + 14 * (1 + 2 + 2)
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        want = F.pack(t.mols, t.atoms, t.bonds, t.text, frags=FRAGS, tables=TABLES, n_atom_records=cut.get("na"),
                      n_bond_records=cut.get("nb"), n_text_bytes=cut.get("nt"))
        assert int(want["mols"]["flags"][-1]) & MOL_FORMULA_REFUSED
        a = run(eng, t, want["totals"], **cut)
        assert a.rc == 0 and a.totals.tolist() == list(want["totals"]) + [0]
        same_mols(a.mols, want["mols"])
        assert a.atoms.tobytes() == clean(want["atoms"]) and a.bonds.tobytes() == clean(want["bonds"]) and a.text.tobytes() == want["text"]


def test_capacities_exact_and_one_short(eng, batch):
    """each capacity one record or byte short, separately: nothing is written beyond it, what lies in front of it is right, and
    mols_out and totals are complete"""
    t, ref = batch
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8),
             np.frombuffer(ref["text"], np.uint8), ref["origin"].view(np.uint8))
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, t, caps)                                                          # run() checks the FILL bytes behind every capacity
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same_mols(a.mols, ref["mols"])
        for got, want in zip((a.atoms, a.bonds, a.text, a.side), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None, origin=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]                               # the sizing call
    same_mols(a.mols, ref["mols"])


def test_the_step_limit(eng, dev):
    t = Tables(dev, [mol([b"C", b"[CH2CH3]", b"[CH2F]", b"[NHCH3]"], [(0, 1, 1, 1), (0, 2, 1, 1), (0, 3, 1, 1)])])      # 4, 3 and 4 placements
    assert FORMULA_DEFAULT_STEPS == F.DEFAULT_STEPS
    for limit, flags in ((1, MOL_FORMULA_LEFT | MOL_FORMULA_LIMIT), (3, MOL_FORMULA_EXPANDED | MOL_FORMULA_LEFT | MOL_FORMULA_LIMIT),
                         (4, MOL_FORMULA_EXPANDED), (0, MOL_FORMULA_EXPANDED), (FORMULA_DEFAULT_STEPS, MOL_FORMULA_EXPANDED)):
        ref = check(eng, t, max_steps=limit)
        assert int(ref["mols"]["flags"][0]) == flags, (limit, int(ref["mols"]["flags"][0]))


def test_engine_formula_pack_sizes_itself(eng, batch):
    t, ref = batch
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}
    for caps in (None, (1, 1, 1)):
        out = eng.formula_pack(rec, caps=caps)
        same_mols(out["mols"], ref["mols"])
        assert out["atoms"].tobytes() == clean(ref["atoms"]) and out["bonds"].tobytes() == clean(ref["bonds"]) and out["text"] == ref["text"]
        assert out["origin"].tolist() == ref["origin"].tolist() and out["totals"].tolist() == list(ref["totals"]) + [0]
    limited = eng.formula_pack(dict(zip(("mols", "atoms", "bonds", "text"), H.tables_of(["C[CH2CH3]"]))), max_steps=3)
    assert int(limited["mols"]["flags"][0]) == MOL_FORMULA_LEFT | MOL_FORMULA_LIMIT and int(limited["mols"]["n_atoms"][0]) == 2


@pytest.mark.parametrize("labels,names", FH.PAIRS)
def test_a_formula_equals_its_table_name_through_the_device_chain(eng, labels, names):
    """smiles_read -> formula_pack -> expand_pack -> normalize_pack -> smiles_pack_canonical on the device: one string per pair,
    and the string of the host oracles' chain"""
    strings = [FH.CARRIER % s for s in labels + names]
    rec = eng.smiles_read(strings, keep_device=True)
    rec = eng.normalize_pack(eng.expand_pack(eng.formula_pack(rec, keep_device=True), keep_device=True), keep_device=True)
    recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
    got = [data[int(r["text0"]):int(r["text0"]) + int(r["len"])].decode() for r in recs]
    assert len(set(got)) == 1 and "*" not in got[0], dict(zip(strings, got))
    assert got == FH.chain(strings)


def test_canonical_smiles_with_formula(eng):
    from molnextr_amd.model import canonical_smiles
    strings = [FH.CARRIER % s for s in ("CH2CH3", "Et", "OCH2Ph", "OBn", "C6H5")] + ["CC"]
    plain = canonical_smiles(eng, strings, expand=True, normalize=True)
    out = canonical_smiles(eng, strings, expand=True, normalize=True, formula=True)
    assert [o["smiles"] for o in out] == FH.chain(strings)
    assert out[0]["smiles"] == out[1]["smiles"] and out[2]["smiles"] == out[3]["smiles"] and "*" in out[4]["smiles"]
    assert [o["formula_flags"] for o in out] == [MOL_FORMULA_EXPANDED, 0, MOL_FORMULA_EXPANDED, 0, MOL_FORMULA_LEFT, 0]
    assert all("formula_flags" not in o for o in plain) and plain[1] == {k: v for k, v in out[1].items() if k != "formula_flags"}
    assert "*" in plain[0]["smiles"]                                                   # without the pass the label stays


def test_formula_pack_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, SMALL)

    def refused(expect, **over):
        assert_refused(run(eng, t, (64, 64, 64), **over), "mnx_formula_pack: " + expect)

    for name in ("mols", "atoms", "bonds", "text", "mols_out", "atoms_out", "bonds_out", "text_out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, the output tables too, totals 4-byte, origin 2-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2), ("mols_out", 0), ("atoms_out", 1), ("bonds_out", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, totals=_p(t.d[0], 2))
    refused(aligned, origin=_p(t.d[0], 1))

    class Bare(Engine):                                                                # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        assert run(bare, t, (1, 1, 1)).rc == -1 and bare.lib.mnx_last_error(bare.h) == b"mnx_formula_pack: call mnx_set_symbol_tables first"
        Engine._set_symbol_tables(bare)
        assert run(bare, t, (1, 1, 1)).rc == -1 and bare.lib.mnx_last_error(bare.h) == b"mnx_formula_pack: call mnx_set_fragments first"
        Engine._set_fragments(bare)
        check(bare, t)
    finally:
        bare.close()


def written(rec):
    """the plain writer's strings of an oracle's tables, None for a molecule it refuses"""
    import smiles_ref as S
    w = S.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tables=TABLES)
    return [None if int(r["flags"]) & 0x33 else w["out"][int(r["text0"]):int(r["text0"]) + int(r["len"])].decode() for r in w["recs"]]


def test_end_to_end_predict_formula_expand_write(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: predict_pipeline(packed=True, formula=True, expand=True, smiles=True) against the oracles applied to the
    same run's packed tables; without formula the dicts are what they were; then the facade's graph_formula."""
    from molnextr_amd.model import formula_candidate, molnextr, predict_pipeline, unpack_graphs
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    f = F.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], frags=FRAGS, tables=TABLES)
    x = X.pack(f["mols"], f["atoms"], f["bonds"], f["text"], frags=FRAGS, tables=TABLES)
    assert not (f["mols"]["flags"] & MOL_FORMULA_REFUSED).any()
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, expand=True)
    grown = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, expand=True, formula=True)
    alone = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, formula=True)
    after_f = unpack_graphs(f["mols"], f["atoms"], f["bonds"], f["text"])
    after_x = unpack_graphs(x["mols"], x["atoms"], x["bonds"], x["text"])
    want_x, want_f = written(x), written(f)
    for b, (p, g, a) in enumerate(zip(plain, grown, alone)):
        assert "formula" not in p and set(g) == set(p) | {"formula"} and set(a) == set(g) - {"expanded"}
        assert p["chartok_coords"] == g["chartok_coords"] and p["bonds"] == g["bonds"]
        m = f["mols"][b]
        a0, na = int(m["atom0"]), int(m["n_atoms"])
        origin = f["origin"][a0:a0 + na].tolist()
        before = p["chartok_coords"]["symbols"]
        assert g["formula"] == a["formula"] == {
            "symbols": after_f[b]["chartok_coords"]["symbols"], "coords": after_f[b]["chartok_coords"]["coords"], "bonds": after_f[b]["bonds"],
            "origin": origin, "flags": int(m["flags"]), "replaced": sorted(f["found"][b]), "left": f["left"][b]}
        assert all(formula_candidate(before[k]) for k in f["left"][b] + sorted(f["found"][b]))
        mx = x["mols"][b]
        x0, nx = int(mx["atom0"]), int(mx["n_atoms"])
        assert g["expanded"]["symbols"] == after_x[b]["chartok_coords"]["symbols"] and g["expanded"]["bonds"] == after_x[b]["bonds"]
        assert g["expanded"]["origin"] == [origin[k] for k in x["origin"][x0:x0 + nx].tolist()]
        assert g["graph_smiles"] == want_x[b] and a["graph_smiles"] == want_f[b]
    with pytest.raises(ValueError, match="formula=True needs packed=True"):
        predict_pipeline(eng, imgs[:1], formula=True)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)          # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_formula=True needs graph_smiles=True or graph_molfile=True"):
        molnextr("synthetic", dev, graph_formula=True)
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_expand=True, graph_formula=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True, expand=True, formula=True)
        assert [o["formula"] for o in got] == [p["formula"] for p in want] and [o["expanded"] for o in got] == [p["expanded"] for p in want]
        m.graph_formula = False                                                        # the default: the label stays
        assert all("formula" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()
