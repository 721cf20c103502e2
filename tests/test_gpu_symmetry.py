"""GPU (-m gpu): mnx_smiles_pack_symmetric — the canonical graph SMILES with the symmetry rule for its marks — against the oracle
of tests/symmetry_ref.py, byte for byte and word for word (recs, order, rank, sym_class, atom_marks, text, totals; no
tolerances), for marks 0..3: the strings that pin the rule, the generated molecules of the CPU tests, the device against its
own mnx_smiles_pack_canonical, molecules at odd offsets and the refusal cases, the largest molecule, the protocol, and one
end-to-end run."""
import numpy as np
import pytest

import canon_ref as K
import ez_ref as E
import smiles_ref as S
import stereo_ref as T
import symmetry_ref as Y
import test_canon_host as H
import test_symmetry_host as HS
from molnextr_amd import weights as W
from molnextr_amd.engine import ATOM_MARKS_NONE, SMILES_REFUSED, SMILES_SYM_DROPPED
from packed_tables import (FILL, WORD_FILL, Tables, _p, assert_refused, call_text, compare_text, dev, device_texts, eng,  # noqa: F401
                           same_results, texts)

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the plain writer's end-to-end test
MODES = (0, 1, 2, 3)
NAME = "mnx_smiles_pack_symmetric: "


def oracle(t, marks, **sizes):
    return Y.pack(t.mols, t.atoms, t.bonds, t.text, marks, order_fill=WORD_FILL, marks_fill=FILL, **sizes)


@pytest.fixture(scope="module")
def pinned(dev):
    """the pinned molecules, each drawing, as one batch of molecules of at most 8 atoms"""
    mols = []
    for name in sorted(HS.PINNED):
        mol, _, mirror = HS.PINNED[name][:3]
        mols += [mol] + ([HS.mirrored(mol, *mirror)] if mirror else [])
    assert max(len(m[0]) for m in mols) <= 8
    return mols, Tables(dev, mols)


@pytest.fixture(scope="module")
def generated(dev):
    """the generated molecules of the CPU test as one batch, and the oracle's result for every set of marks"""
    mols = T.generated_set(100) + E.generated_set(100) + Y.generated_set()
    t = Tables(dev, mols)
    return mols, t, {m: oracle(t, m) for m in MODES}


def run(eng, t, out_cap, marks=0, fn="mnx_smiles_pack_symmetric", **over):
    """fn = "mnx_smiles_pack_canonical": the older call, which has no atom_marks"""
    return call_text(fn, eng, t, out_cap, marks=marks, **over)


def check(eng, t, marks, ref=None):
    """the device's recs, order, rank, sym_class, atom_marks, bytes and totals equal the oracle's at the exact capacity; returns
    the oracle's"""
    ref = ref or oracle(t, marks)
    compare_text(run(eng, t, ref["total"], marks), ref, "SMILES")
    return ref


@pytest.mark.parametrize("marks", MODES)
def test_pinned_molecules_in_one_batch(eng, pinned, marks):
    mols, t = pinned
    ref = check(eng, t, marks)
    k = 0
    for name in sorted(HS.PINNED):
        mol, at_marks, mirror, before, after, set_bits, clear_bits = HS.PINNED[name]
        for d in range(2 if mirror else 1):
            if marks == at_marks:
                assert texts(ref)[k] == (after if isinstance(after, str) else after[d]), (name, d)
                f = int(ref["recs"]["flags"][k])
                assert f & set_bits == set_bits and not f & clear_bits, (name, d, f)
            k += 1
    assert k == t.n


@pytest.mark.parametrize("marks", MODES)
def test_generated_molecules_in_one_call(eng, generated, marks):
    mols, t, refs = generated
    ref = refs[marks]
    dropped = (ref["recs"]["flags"] & SMILES_SYM_DROPPED).astype(bool).sum()
    assert (dropped == 0) if marks == 0 else (dropped >= 30), dropped
    assert ((ref["recs"]["flags"] & SMILES_REFUSED) == 0).all() and t.n == 200 + 160
    check(eng, t, marks, ref)


def test_device_against_its_own_canonical_call(eng, generated):
    """bytes and flags equal mnx_smiles_pack_canonical on every molecule with bit 15 clear, everywhere with marks == 0; order,
    rank, sym_class, n_rings and the flag bits of invariant 1 equal it everywhere; the strip invariant"""
    mols, t, refs = generated
    plain = None
    for marks in MODES:
        cap = refs[marks]["total"] + 16384                  # the canonical strings are longer where marks were dropped
        new = run(eng, t, cap, marks)
        old = run(eng, t, cap, marks, fn="mnx_smiles_pack_canonical")
        assert new.rc == old.rc == 0 and new.totals[1] == old.totals[1] == 0
        assert all(np.array_equal(getattr(new, k), getattr(old, k)) for k in ("order", "rank", "sym_class"))
        assert np.array_equal(new.recs["n_rings"], old.recs["n_rings"])
        assert np.array_equal(new.recs["flags"] & Y.KEPT_BITS, old.recs["flags"] & Y.KEPT_BITS)
        got, was = (device_texts(x.recs, x.out) for x in (new, old))
        plain = got if marks == 0 else plain
        fired = 0
        for b, (g, w) in enumerate(zip(got, was)):
            if not new.recs["flags"][b] & SMILES_SYM_DROPPED:
                assert g == w and new.recs["flags"][b] == old.recs["flags"][b], (marks, b)
            else:
                fired += 1
            assert E.strip(g.replace("@", "")) == plain[b], (marks, b)
        assert fired == 0 if marks == 0 else fired >= 30
        if marks == 0:
            assert new.recs.tobytes() == old.recs.tobytes() and np.array_equal(new.out, old.out) and not new.atom_marks.any()


CHAIN = ([b"O", b"C", b"C"], [(0, 0), (10, 0), (20, 0)], [(0, 1, 1, 1), (1, 2, 1, 1)])
DUPLICATE = (H.DIFLUORO[0], H.DIFLUORO[1], H.CHAIN3 + [(2, 1, 1, 1)])
MANY_RINGS = ([b"C"] * 102, [(k, 0) for k in range(102)], [(0, k, 1, 1) for k in range(1, 102)] + [(k, k + 1, 1, 1) for k in range(1, 101)])
EMPTY = ([], [], [])


def test_molecule_offsets_and_edges(eng, dev, pinned):
    """n = 1; molecules that start at odd atom0; an empty molecule; a duplicate bond (0xFF in atom_marks exactly where order is
    0xFFFF); more than 99 ring numbers (no string, 0xFF, valid ranks)"""
    fluoropropane, diene = HS.PINNED["2-fluoropropane"][0], HS.PINNED["a diene with a symmetric end"][0]
    for mol in (fluoropropane, EMPTY, DUPLICATE):
        check(eng, Tables(dev, [mol]), 3)
    batch = [CHAIN, fluoropropane, diene, EMPTY, DUPLICATE, diene, CHAIN, MANY_RINGS, fluoropropane, HS.PINNED["1,1-dimethylcyclopropane"][0]]
    t = Tables(dev, batch)
    assert [int(m["atom0"]) % 2 for m in t.mols[:7]] == [0, 1, 1, 0, 0, 0, 1]
    for marks in MODES:
        ref = check(eng, t, marks)
        assert np.array_equal(ref["atom_marks"] == ATOM_MARKS_NONE, ref["order"] == S.NO_POSITION)
    a0 = [int(m["atom0"]) for m in t.mols]
    assert set(ref["atom_marks"][a0[4]:a0[5]].tolist()) == set(ref["atom_marks"][a0[7]:a0[8]].tolist()) == {ATOM_MARKS_NONE}
    assert set(ref["rank"][a0[4]:a0[5]].tolist()) == {K.NO_RANK} and sorted(ref["rank"][a0[7]:a0[8]].tolist()) == list(range(102))
    flags = ref["recs"]["flags"].tolist()
    assert flags[4] == S.FLAG_DUPLICATE and flags[7] == S.FLAG_RINGS | K.FLAG_TIE and flags[3] == 0
    assert all(flags[k] & SMILES_SYM_DROPPED for k in (1, 2, 5, 8, 9)) and not any(flags[k] & SMILES_SYM_DROPPED for k in (0, 3, 4, 6, 7))


def test_the_largest_molecule(eng, dev):
    """a chain of 999 carbons that ends in a marked gem-dimethyl carbon: the serial low pass and the rank loop at their bound"""
    symbols = [b"C"] * 996 + [b"[C@H]", b"C", b"C"]
    xy = [(k // 30, 2 * (k % 30)) for k in range(996)] + [(40, 10), (45, 4), (45, 16)]
    bonds = [(k, k + 1, 1, 1) for k in range(996)] + [(996, 997, 5, 6), (996, 998, 1, 1)]
    ref = check(eng, Tables(dev, [(symbols, xy, bonds)]), 3)
    assert texts(ref) == ["C" * 996 + "[CH](C)C"] and ref["recs"]["flags"].tolist() == [SMILES_SYM_DROPPED | K.FLAG_TIE | S.FLAG_WEDGES]
    assert ref["atom_marks"].tolist() == [0] * 996 + [Y.ATOM_SYM, 0, 0]


def test_protocol(eng, generated):
    """the sizing call without a buffer, the exact size, one byte short; `order` and `atom_marks` left out"""
    mols, t, refs = generated
    ref = refs[3]
    need = ref["total"]
    a = run(eng, t, 0, 3, out=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and np.all(a.out == FILL)
    assert a.order.tobytes() == ref["order"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes() and a.sym_class.tobytes() == ref["sym_class"].tobytes()
    assert a.atom_marks.tobytes() == ref["atom_marks"].tobytes()
    a = run(eng, t, need - 1, 3)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes()
    assert a.out[:need - 1].tobytes() == ref["out"][:need - 1] and np.all(a.out[need - 1:] == FILL), "nothing is written beyond out_cap"
    assert a.atom_marks.tobytes() == ref["atom_marks"].tobytes()
    a = run(eng, t, need, 3, order=None, atom_marks=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 0] and a.recs.tobytes() == ref["recs"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes()
    assert a.out[:need].tobytes() == ref["out"] and np.all(a.out[need:] == FILL) and (a.order == WORD_FILL).all() and (a.atom_marks == FILL).all()
    assert a.sym_class.tobytes() == ref["sym_class"].tobytes()


def test_refused_calls_launch_nothing_and_name_the_new_function(eng, pinned):
    mols, t = pinned
    need = oracle(t, 3)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **{"marks": 3, **over}), NAME + expect)

    assert run(eng, t, need, 3).rc == 0
    for marks in (4, 8, 0x80000001):
        refused("marks may hold MNX_SMILES_MARK_TETRAHEDRAL and MNX_SMILES_MARK_DOUBLE_BOND only", marks=marks)
    for name in ("rank", "sym_class", "mols", "atoms", "recs", "out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    for name in ("rank", "sym_class"):
        refused("mols, atoms and bonds must be 8-byte aligned, recs and totals 4-byte, order, rank and sym_class 2-byte", **{name: _p(t.d[0], 1)})
    refused("mols, atoms and bonds must be 8-byte aligned, recs and totals 4-byte, order, rank and sym_class 2-byte", mols=_p(t.d[0], 4))


def test_two_runs_are_word_identical(eng, generated):
    mols, t, refs = generated
    for marks in (1, 3):
        a, b = run(eng, t, refs[marks]["total"], marks), run(eng, t, refs[marks]["total"], marks)
        same_results(a, b)
        assert a.rc == b.rc == 0


def test_end_to_end_predict_pipeline_and_molnextr(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images through predict_pipeline(packed, smiles, canonical, symmetry) with all marks: strings, ranks and the
    per-atom bits equal the oracle's on the returned tables; without symmetry the results are the canonical call's; and
    molnextr(graph_symmetry=True) hands them on"""
    from molnextr_amd.model import molnextr, predict_pipeline
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    ref = Y.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], 3)
    got = eng.smiles_pack(rec, stereo=True, double_bonds=True, canonical=True, symmetry=True)
    assert len(got) == 6 and got[2] == ref["out"] and got[0].tobytes() == ref["recs"].tobytes()
    for k, name in ((1, "order"), (3, "rank"), (4, "sym_class"), (5, "atom_marks")):
        assert got[k].dtype == ref[name].dtype and got[k].tobytes() == ref[name].tobytes(), name
    assert len(eng.smiles_pack(rec, stereo=True, double_bonds=True, canonical=True)) == 5
    with pytest.raises(ValueError, match="symmetry=True needs canonical=True"):
        eng.smiles_pack(rec, symmetry=True)
    conf = dict(ref_batch_size=4, packed=True, smiles=True, stereo=True, double_bonds=True, canonical=True)
    preds, plain = predict_pipeline(eng, imgs, symmetry=True, **conf), predict_pipeline(eng, imgs, **conf)
    old = K.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], 3)
    written = 0
    for b, (p, q, m) in enumerate(zip(preds, plain, rec["mols"])):
        a0, na = int(m["atom0"]), int(m["n_atoms"])
        refused = bool(ref["recs"]["flags"][b] & SMILES_REFUSED)
        assert p["graph_smiles"] == (None if refused else texts(ref)[b])
        assert p["stereo_atoms"] == (None if refused else ref["atom_marks"][a0:a0 + na].tolist())
        assert p["canonical_rank"] == q["canonical_rank"] and p["symmetry_class"] == q["symmetry_class"]
        assert q["graph_smiles"] == (None if refused else texts(old)[b]) and "stereo_atoms" not in q
        written += not refused
    assert written
    for args in ({"canonical": False}, {"smiles": False, "stereo": False, "double_bonds": False, "canonical": False}):
        with pytest.raises(ValueError, match="symmetry=True needs smiles=True and canonical=True"):
            predict_pipeline(eng, imgs, symmetry=True, **{**conf, **args})

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_symmetry=True needs graph_smiles=True and graph_canonical=True"):
        molnextr("synthetic", dev, graph_smiles=True, graph_symmetry=True)
    pages = [W.synthetic_page(c) for c in range(4)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_stereo=True, graph_double_bonds=True, graph_canonical=True,
                 graph_symmetry=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, symmetry=True, **conf)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert [o["stereo_atoms"] for o in got] == [p["stereo_atoms"] for p in want]
        m.graph_symmetry = False                               # the default: what it gave before
        before = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, **conf)
        again = m.predict_images(pages, batch_size=4)
        assert [o["predicted_smiles"] for o in again] == [p["graph_smiles"] for p in before] and "stereo_atoms" not in again[0]
    finally:
        m.engine.close()
