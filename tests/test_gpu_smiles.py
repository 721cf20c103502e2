"""GPU (-m gpu): mnx_smiles_pack — graph SMILES written on the device from the packed molecule tables — against the oracle of
tests/smiles_ref.py, byte for byte and record for record, `order` included (no tolerances), on hand-built tables uploaded with
torch: the sizes at which the kernels take another path, the limits of the walk and of the ring numbers, the capacity and
argument handling, and one end-to-end run through Engine.predict, predict_pipeline and the facade."""
import functools

import numpy as np
import pytest

import packed_tables as P
import smiles_ref as S
import test_smiles_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_REFUSED, Engine
from packed_tables import FILL, POOL, Tables, _p, assert_refused, compare_text, dev, eng, random_molecule, same_results  # noqa: F401
from packed_tables import WORD_FILL as ORDER_FILL

pytestmark = pytest.mark.gpu

# Images 500..507, the batch the molfile test takes: its molecules of 12 and 10 atoms (images 503 and 507, complete graphs like
# all of them) stay under 99 ring numbers and get a string; two of 25 atoms are refused for ring numbers, four for > 999 bonds.
E2E_FIRST_INDEX = 500


mol = functools.partial(P.mol, flat=True)                     # the plain writer reads no coordinates: every atom at (0, 0)
run = functools.partial(P.call_text, "mnx_smiles_pack")       # run(eng, t, out_cap, sizes=None, **over)


def check(eng, t, sizes=None, ref_kw=None):
    """the device's recs, order, bytes and totals equal the oracle's at the exact capacity; returns the oracle's result"""
    kw = dict(zip(("n_atom_records", "n_bond_records", "n_text_bytes"), sizes)) if sizes is not None else {}
    ref = S.pack(t.mols, t.atoms, t.bonds, t.text, order_fill=ORDER_FILL, **kw, **(ref_kw or {}))
    compare_text(run(eng, t, ref["total"], sizes), ref, "SMILES")
    return ref


def text_of(ref, b):
    r = ref["recs"][b]
    return ref["out"][r["text0"]:r["text0"] + r["len"]].decode()


def test_hand_written_strings_and_tiny_molecules(eng, dev):
    names = sorted(H.HAND)
    t = Tables(dev, [([], [], []), mol([b"[NH4+]"], [])] + [mol(*H.HAND[k][:2]) for k in names] + [([], [], []), mol([b"[Ac]"], [])])
    ref = check(eng, t)
    assert ref["out"].decode() == "[NH4+]" + "".join(H.HAND[k][2] for k in names) + "*"
    assert ref["recs"]["flags"].tolist() == [0, 0] + [H.HAND[k][3] for k in names] + [0, S.FLAG_PSEUDO]
    t = Tables(dev, [mol([b"C"] * 8, H.path(8) + [(0, 3, 1, 1), (2, 5, 1, 1), (4, 7, 1, 1)]),
                     mol([b"C"] * 5, [(0, 1, 1, 1), (1, 2, 1, 1), (0, 2, 1, 1), (2, 3, 1, 1), (3, 4, 1, 1), (2, 4, 1, 1)])])
    assert check(eng, t)["out"] == b"C1CC2C1C1C2CC1" + b"C1CC12CC2"          # a freed number comes back; not at the atom that closed it


def test_every_symbol_class_past_one_tile_of_threads(eng, dev):
    """300 atoms / 400 bonds and 257 / 255 (more than 256 atoms, slots past 512) drawn from POOL, among smaller molecules; the
    larger one once with every class of bond and once sparse enough in rings to be written"""
    rng = np.random.default_rng(31)
    big = H.random_graph(rng, 300, 400)
    tree = H.random_graph(rng, 300, 330)
    t = Tables(dev, [H.random_graph(rng, 7, 6), big, mol(list(POOL), H.path(len(POOL))), H.random_graph(rng, 257, 255), tree,
                     random_molecule(rng, 300, 400), H.random_graph(rng, 2, 1)])
    ref = check(eng, t)
    assert (ref["recs"]["flags"][1:6] & S.FLAG_PSEUDO).all() and ref["recs"]["len"][[1, 3, 4]].min() > 1000
    assert ref["recs"]["n_rings"][[1, 5]].min() > 100 and ref["recs"]["n_rings"][4] > 30
    assert b"%" in ref["out"] and ref["out"].count(b"[1*]") > 5 and ref["out"].count(b"(") > 100


def test_deepest_stack_widest_branching_and_the_size_limit(eng, dev):
    """a path of 999 atoms (the search 998 deep), a star of 999 atoms (998 neighbours in one list, 997 branches), 999 bonds in
    one molecule; 1000 atoms or bonds are refused with flag bit 0 while the neighbours stay intact"""
    rng = np.random.default_rng(32)
    syms = [POOL[k % len(POOL)] for k in range(999)]
    star = [(0, k, 1 + k % 4, 0) for k in range(998, 0, -1)]
    grid = H.path(500) + [(k, k + 2, 1, 1) for k in range(0, 998, 2)][:249] + [(k, k + 500, 2, 2) for k in range(251)]
    t = Tables(dev, [H.random_graph(rng, 5, 4), mol([b"C"] * 999, H.path(999)), mol([b"C"] * 1000, H.path(1000)), H.random_graph(rng, 6, 5),
                     mol(syms, star), mol([b"C"] * 40, [(0, 1, 1, 1)] * 1000), mol([b"c"] * 999, H.path(999, 4)[::-1]),
                     mol([b"N"] * 751, grid), H.random_graph(rng, 3, 2)])
    assert len(grid) == 999
    ref = check(eng, t)
    assert ref["recs"]["flags"].tolist()[1:3] == [0, S.FLAG_TOO_LARGE] and ref["recs"]["flags"][5] == S.FLAG_TOO_LARGE
    assert ref["recs"]["len"][[2, 5]].tolist() == [0, 0] and text_of(ref, 1) == "C" * 999 and text_of(ref, 6) == "c" * 999
    assert text_of(ref, 4).count("(") == 997 and ref["recs"]["n_rings"][7] == 249 and ref["recs"]["len"][7] > 751


def test_ring_numbers_at_the_limit_of_99(eng, dev):
    """K19 holds 97 numbers and is written, K20 would need 107; a fan of exactly 99 numbers is written, one of 100 refused"""
    t = Tables(dev, [mol(*H.complete(19)), mol(*H.complete(20)), mol(*H.fan(99)), mol(*H.fan(100)), mol(*H.complete(4))])
    ref = check(eng, t)
    assert ref["recs"]["flags"].tolist() == [0, S.FLAG_RINGS, 0, S.FLAG_RINGS, 0] and ref["recs"]["n_rings"].tolist() == [153, 171, 99, 100, 3]
    assert "%97" in text_of(ref, 0) and "%98" not in text_of(ref, 0) and text_of(ref, 2).endswith("C%97C%98C%99")
    assert ref["recs"]["len"][[1, 3]].tolist() == [0, 0] and text_of(ref, 4) == "C12C3C1C23"


def test_forty_components(eng, dev):
    t = Tables(dev, [mol([b"C", b"[Na+]"] * 20, []), mol([b"C"] * 6, [(4, 5, 2, 2), (0, 3, 1, 1)])])
    ref = check(eng, t)
    assert text_of(ref, 0) == ".".join(["C", "[Na+]"] * 20) and text_of(ref, 0).count(".") == 39 and text_of(ref, 1) == "CC.C.C.C=C"
    assert ref["order"][40:].tolist() == [0, 2, 3, 1, 4, 5]


def test_molecule_counts_past_the_scan_tile(eng, dev):
    """1025 molecules, a third of them empty: the scan over the molecules carries from its first tile of 1024 into the second"""
    rng = np.random.default_rng(33)
    sizes = rng.integers(0, 3, 1025) * rng.integers(1, 6, 1025)
    sizes[-1] = 3                                              # the molecule behind the first tile is not empty
    t = Tables(dev, [H.random_graph(rng, int(k), int(k)) if k else ([], [], []) for k in sizes])
    assert (t.mols["n_atoms"] == 0).sum() > 200
    ref = check(eng, t)
    assert ref["recs"]["text0"][-1] + ref["recs"]["len"][-1] == ref["total"] > 5000
    one = Tables(dev, arrays=(t.mols[:1], t.atoms, t.bonds, t.text))
    check(eng, one)


def test_records_beyond_the_tables(eng, dev):
    rng = np.random.default_rng(34)
    t = Tables(dev, [H.random_graph(rng, 6, 6) for _ in range(6)])
    na, nb, nt = len(t.atoms), len(t.bonds), len(t.text)
    for sizes in ((na - 1, nb, nt), (na, nb - 7, nt), (na, nb, nt - 1), (0, 0, 0), (na - 6, nb - 6, 1)):
        ref = check(eng, t, sizes=sizes)
        assert (ref["recs"]["flags"] & S.FLAG_BEYOND).any() and (ref["recs"]["len"][(ref["recs"]["flags"] & 2) != 0] == 0).all()
    mols, atoms, bonds, text = (a.copy() if isinstance(a, np.ndarray) else a for a in (t.mols, t.atoms, t.bonds, t.text))
    bonds["j"][int(mols["bond0"][1])] = 6                      # a bond to an atom the molecule does not have
    bonds["i"][int(mols["bond0"][2]) + 1] = bonds["j"][int(mols["bond0"][2]) + 1]          # a bond from an atom to itself
    atoms["sym0"][int(mols["atom0"][3]) + 2] = nt              # a symbol behind the text table
    atoms["sym_len"][int(mols["atom0"][4])] = 65535
    mols["flags"][5] = 1
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert [int(f) & 10 for f in ref["recs"]["flags"]] == [0, 2, 2, 2, 2, 8] and ref["recs"]["len"][1:5].tolist() == [0, 0, 0, 0]
    assert (ref["order"][6:30] == S.NO_POSITION).all() and sorted(ref["order"][30:].tolist()) == list(range(6))


def test_duplicate_pairs_and_unknown_classes(eng, dev):
    """the same pair in two records (in either direction) refuses the molecule, n_rings still counted; classes 0 and 7 are '~'"""
    rng = np.random.default_rng(35)
    dup = [(0, 1, 1, 1), (1, 2, 1, 1), (2, 3, 1, 1), (1, 2, 2, 2), (0, 3, 5, 5)]
    hub = [(0, k, 1, 1) for k in range(1, 300)] + [(7, 0, 2, 2)]
    t = Tables(dev, [H.random_graph(rng, 5, 5), mol([b"C", b"[R1]", b"C", b"C"], dup), mol([b"C"] * 300, hub),
                     mol([b"C", b"c", b"c"], [(0, 1, 7, 0), (1, 2, 0, 0)]), random_molecule(rng, 12, 40)])
    ref = check(eng, t)
    assert ref["recs"]["flags"].tolist()[1:4] == [S.FLAG_DUPLICATE | S.FLAG_PSEUDO, S.FLAG_DUPLICATE, S.FLAG_UNKNOWN]
    assert ref["recs"]["n_rings"].tolist()[1:4] == [2, 1, 0] and text_of(ref, 3) == "C~c~c" and ref["recs"]["flags"][4] & S.FLAG_DUPLICATE


def test_capacities(eng, dev):
    """out_cap 0, one byte short, half and exact over a 0x7F-filled buffer: totals, recs and order complete, nothing written
    beyond out_cap; the sizing call without a buffer; a call without `order`"""
    rng = np.random.default_rng(36)
    t = Tables(dev, [H.random_graph(rng, 9, 10) for _ in range(40)])
    ref = S.pack(t.mols, t.atoms, t.bonds, t.text)
    need = ref["total"]
    for cap in (0, need - 1, need // 2, need):
        a = run(eng, t, cap)
        assert a.rc == 0 and a.totals.tolist() == [need, int(cap < need)]
        assert a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
        assert a.out[:cap].tobytes() == ref["out"][:cap] and np.all(a.out[cap:] == FILL), cap
    a = run(eng, t, 0, out=None)                                # a sizing call needs no buffer
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
    a = run(eng, t, need, order=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 0] and a.recs.tobytes() == ref["recs"].tobytes() and np.all(a.order == ORDER_FILL)
    assert a.out[:need].tobytes() == ref["out"]


def test_two_runs_are_byte_identical(eng, dev):
    rng = np.random.default_rng(37)
    t = Tables(dev, [H.random_graph(rng, int(k), int(k) + 3) for k in rng.integers(0, 60, 200)])
    need = S.pack(t.mols, t.atoms, t.bonds, t.text)["total"]
    a, b = run(eng, t, need), run(eng, t, need)
    same_results(a, b)
    assert a.rc == b.rc == 0 and a.totals.tolist() == b.totals.tolist() == [need, 0]


def test_refused_calls_leave_the_outputs_untouched(eng, dev, synth_ckpt):
    rng = np.random.default_rng(38)
    t = Tables(dev, [H.random_graph(rng, 5, 4) for _ in range(3)])
    need = S.pack(t.mols, t.atoms, t.bonds, t.text)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **over), "mnx_smiles_pack: " + expect)

    assert run(eng, t, need).rc == 0
    for name in ("mols", "atoms", "bonds", "text", "recs", "out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, recs and totals 4-byte, order 2-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, recs=_p(t.d[0], 6))
    refused(aligned, totals=_p(t.d[0], 2))
    refused(aligned, order=_p(t.d[0], 1))

    class Bare(Engine):                                      # a fresh handle that was told no symbol tables
        def _set_symbol_tables(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        refused("call mnx_set_symbol_tables first", h=bare.h)
        ok = (b"AcR1", np.array([0, 2, 4], np.uint32), np.array([2, 1], np.uint8))
        assert bare.lib.mnx_set_symbol_tables(bare.h, ok[0], ok[1].ctypes.data, ok[2].ctypes.data, 2) == 0
        two = Tables(dev, [mol([b"[Ac]", b"[R1]", b"[OMe]", b"[R2]"], H.path(4))])
        ref = S.pack(two.mols, two.atoms, two.bonds, two.text, tables={b"Ac": 2, b"R1": 1})
        a = run(eng, two, ref["total"], h=bare.h)
        assert a.rc == 0 and a.out[:ref["total"]].tobytes() == ref["out"] == b"*[1*]**" and a.recs.tobytes() == ref["recs"].tobytes()
    finally:
        bare.close()


def test_end_to_end_predict_pack_smiles(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: Engine.predict -> graph_pack -> smiles_pack against the oracle over the same records; then
    predict_pipeline(packed=True, smiles=True) and the facade's 'predicted_smiles'. The synthetic checkpoint's bond head marks
    nearly every atom pair, so most of its molecules hold more than 99 ring numbers and are refused: equality with the oracle
    is the assertion, and at least one of the eight is small enough to be written."""
    from molnextr_amd.model import molnextr, predict_pipeline
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    out = eng.predict(imgs, ref_batch=4)
    rec = eng.graph_pack(out, keep_device=True)
    assert rec["totals"][0] > 8 and rec["totals"][1] > 0
    ref = S.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"])
    for r, cap in ((rec, None), ({k: v for k, v in rec.items() if k != "device"}, 1)):     # from the device tables; uploaded, grown once
        recs, order, data = eng.smiles_pack(r, cap=cap)
        assert data == ref["out"] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
    written = [b for b in range(8) if not ref["recs"]["flags"][b] & SMILES_REFUSED]
    assert written and any(ref["recs"]["len"][b] for b in written), ref["recs"]
    preds = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True)
    for b, (p, m) in enumerate(zip(preds, rec["mols"])):
        want = text_of(ref, b) if b in written else None
        assert p["graph_smiles"] == want and isinstance(want, (str, type(None)))
        assert p["graph_smiles_order"] == (ref["order"][m["atom0"]:m["atom0"] + m["n_atoms"]].tolist() if b in written else None)
        if want:
            atoms, bonds = S.read(want)                        # a valid string that holds the molecule's atoms and bonds
            assert len(atoms) == m["n_atoms"] and len(bonds) == m["n_bonds"] and sorted(p["graph_smiles_order"]) == list(range(len(atoms)))
    assert "graph_smiles" not in predict_pipeline(eng, imgs[:2], ref_batch_size=2, packed=True)[0]

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert all(o["predicted_molfile"] is None for o in got)
        m.graph_smiles = False                                 # the default: no SMILES without RDKit
        assert all(o["predicted_smiles"] is None for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()

