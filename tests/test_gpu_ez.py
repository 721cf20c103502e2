"""GPU (-m gpu): mnx_smiles_pack_marks — the graph SMILES with '/' and '\\' at double bonds (and '@' / '@@') written on the device —
against the oracle of tests/ez_ref.py, byte for byte and record for record, `order` included (no tolerances), with marks == 2
and marks == 3: the strings that pin the rule, the generated molecules of the CPU tests, the sizes at which the kernel's loops
take another turn, the capacity and argument handling, marks == 0 and 1 against the two older calls, the strip invariants on the
device, and one end-to-end run."""
import numpy as np
import pytest

import ez_ref as E
import stereo_ref as T
import test_ez_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_EZ, SMILES_EZ_IMPLIED, SMILES_EZ_UNRESOLVED, SMILES_REFUSED, Engine
from packed_tables import (FILL, Tables, _p, assert_refused, call_text, compare_text, dev, device_texts, eng, random_molecule,  # noqa: F401
                           same_results, texts)
from packed_tables import WORD_FILL as ORDER_FILL

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the plain writer's end-to-end test: two of its eight molecules are written
MODES = (2, 3)


@pytest.fixture(scope="module")
def generated(dev):
    mols = E.generated_set()
    t = Tables(dev, mols)
    return mols, t, {m: E.pack(t.mols, t.atoms, t.bonds, t.text, m, order_fill=ORDER_FILL) for m in MODES}


@pytest.fixture(scope="module")
def pool(dev):
    """random graphs over every class of symbol, bond classes 1-6 with any `rev`, many refused"""
    rng = np.random.default_rng(53)
    return Tables(dev, [random_molecule(rng, int(n), int(n) + int(rng.integers(-2, 3))) for n in rng.integers(3, 40, 200)])


def run(eng, t, out_cap, marks=2, fn="mnx_smiles_pack_marks", **over):
    """the older calls (fn) take no marks"""
    return call_text(fn, eng, t, out_cap, **({"marks": marks} if fn == "mnx_smiles_pack_marks" else {}), **over)


def check(eng, t, marks, ref=None):
    """the device's recs, order, bytes and totals equal the oracle's at the exact capacity; returns the oracle's result"""
    ref = ref or E.pack(t.mols, t.atoms, t.bonds, t.text, marks, order_fill=ORDER_FILL)
    compare_text(run(eng, t, ref["total"], marks), ref, "SMILES")
    return ref


@pytest.mark.parametrize("marks", MODES)
def test_pinned_strings_and_flag_cases(eng, dev, marks):
    names, cases = sorted(H.PINNED), sorted(H.FLAG_CASES)
    t = Tables(dev, [H.PINNED[k][:3] for k in names] + [H.FLAG_CASES[k][0] for k in cases])
    ref = check(eng, t, marks)
    assert texts(ref) == [H.PINNED[k][3] for k in names] + [H.FLAG_CASES[k][1] for k in cases]
    assert ref["recs"]["flags"].tolist() == [H.PINNED[k][4] for k in names] + [H.FLAG_CASES[k][2] for k in cases]


@pytest.mark.parametrize("marks", MODES)
def test_generated_molecules_in_one_call(eng, generated, marks):
    mols, t, refs = generated
    ref = refs[marks]
    flags = ref["recs"]["flags"]
    assert t.n == 300 and ref["out"].count(b"/") > 1000 and ref["out"].count(b"\\") > 500 and (flags & SMILES_EZ).astype(bool).sum() > 200
    assert (flags & SMILES_EZ_UNRESOLVED).astype(bool).sum() > 100 and (flags & SMILES_EZ_IMPLIED).astype(bool).sum() >= 20
    assert (ref["out"].count(b"@") > 100) == (marks == 3)
    check(eng, t, marks, ref)


def polyene(rng):
    """600 atoms: a zigzag backbone of 400 with every other bond double and a branch at every other backbone atom (some of them
    on the line of the double bond), so every double bond is a candidate and all but the first resolved one take their flip from
    the one before; the atoms then numbered at random"""
    syms, xy, bonds = [], [], []
    for k in range(400):
        syms.append(b"C")
        xy.append((20 + 10 * k, 100 + 10 * (k % 2)))
        if k:
            bonds.append((k - 1, k, 2, 2) if k % 2 else (k - 1, k, 1, 1))
    for k in range(1, 400, 2):
        syms.append((b"F", b"N", b"c")[k % 3])
        on_the_line = k % 23 == 5                            # behind its atom, on the line of the atom's double bond k - 1, k
        xy.append((xy[k][0] + 10, xy[k][1] + 10) if on_the_line else (xy[k][0], xy[k][1] + 10))
        bonds.append((k, len(syms) - 1, 1, 1))
    perm = [int(p) for p in rng.permutation(600)]
    return T.renumber((syms, xy, bonds), perm, rng)


@pytest.mark.parametrize("marks", MODES)
def test_600_atoms_candidates_in_every_stride(eng, dev, marks):
    """one molecule of 600 atoms: the loops over the atoms stride by 256 threads and the pieces take four neighbouring written
    positions per thread, so resolved candidates and forced flips stand in every 256-block of atom indices, at every written
    position modulo 4, with a and b in two threads' pieces and in two 256-blocks"""
    mol = polyene(np.random.default_rng(51))
    text, pos, flags, _, what = E.smiles(*mol, marks)
    forced = [k for k, c in what["candidates"].items() if c["resolved"] and c["forced"]]
    assert len(forced) > 120 and sum(not c["resolved"] for c in what["candidates"].values()) >= 5
    for block in (range(0, 256), range(256, 512), range(512, 600)):
        assert sum(a in block for a, b in forced) > 10 and sum(b in block for a, b in forced) > 10
    assert {pos[a] % 4 for a, b in forced} == {0, 1, 2, 3} == {pos[x] % 4 for u, x in what["directed"]}
    assert any(pos[a] // 4 != pos[b] // 4 for a, b in forced) and any(a // 256 != b // 256 for a, b in forced)
    back = E.read_back(text, pos, mol[1])
    assert all(cis == drawn for k, c in what["candidates"].items() if c["resolved"] for _, _, cis, drawn in back[frozenset(k)])
    ref = check(eng, Tables(dev, [mol, H.PINNED["cis"][:3]]), marks)
    assert texts(ref) == [text, "F/C=C\\F"] and flags & SMILES_EZ and flags & SMILES_EZ_UNRESOLVED


def test_1030_small_molecules_past_the_scan_tile(eng, dev):
    rng = np.random.default_rng(52)
    names = sorted(H.PINNED)
    mols = []
    for k in range(1030):
        base = H.PINNED[names[k % 4]]
        mols.append(T.renumber(base[:3], [int(p) for p in rng.permutation(len(base[0]))], rng))
    for marks in MODES:
        ref = check(eng, Tables(dev, mols), marks)
        assert (ref["recs"]["flags"] & SMILES_EZ).astype(bool).sum() == 1030 and ref["recs"]["text0"][-1] + ref["recs"]["len"][-1] == ref["total"]
        assert ref["out"].count(b"/") > 1030 and ref["out"].count(b"\\") > 300


@pytest.mark.parametrize("marks", MODES)
def test_capacities(eng, generated, marks):
    """the sizing call without a buffer, the exact size, one byte short: totals, recs and order complete, nothing written beyond
    out_cap"""
    mols, t, refs = generated
    ref = refs[marks]
    need = ref["total"]
    a = run(eng, t, 0, marks, out=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
    assert np.all(a.out == FILL)
    for cap in (need, need - 1):
        a = run(eng, t, cap, marks)
        assert a.rc == 0 and a.totals.tolist() == [need, int(cap < need)]
        assert a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
        assert a.out[:cap].tobytes() == ref["out"][:cap] and np.all(a.out[cap:] == FILL), cap


def test_two_runs_are_byte_identical(eng, generated):
    mols, t, refs = generated
    for marks in MODES:
        a, b = run(eng, t, refs[marks]["total"], marks), run(eng, t, refs[marks]["total"], marks)
        same_results(a, b)
        assert a.rc == b.rc == 0 and a.totals.tolist() == b.totals.tolist() == [refs[marks]["total"], 0]


def test_marks_0_and_1_are_the_older_calls(eng, generated, pool):
    """bytes, records, order and totals of marks == 0 are mnx_smiles_pack's and of marks == 1 mnx_smiles_pack_stereo's, on the
    generated set and on random graphs with refused molecules among them"""
    for t in (generated[1], pool):
        for marks, fn in ((0, "mnx_smiles_pack"), (1, "mnx_smiles_pack_stereo")):
            need = int(run(eng, t, 0, fn=fn, out=None).totals[0])
            old, new = run(eng, t, need, fn=fn), run(eng, t, need, marks)
            same_results(old, new)
            assert old.rc == new.rc == 0 and old.totals.tolist() == new.totals.tolist() == [need, 0]
            assert not (new.recs["flags"] & 0x1C00).any() and need > 1000


def test_strip_invariants_on_the_device(eng, generated, pool):
    """the device's own four outputs: marks == 2 without '/' '\\' is marks == 0, marks == 3 without them marks == 1, marks == 3
    without '@' marks == 2; order, n_rings and the flag bits of the other kind are shared. Against the oracle on the random
    graphs too."""
    for t in (generated[1], pool):
        got = {}
        for marks in (0, 1, 2, 3):
            need = int(run(eng, t, 0, marks, out=None).totals[0])
            a = run(eng, t, need, marks)
            assert a.rc == 0 and a.totals.tolist() == [need, 0]
            got[marks] = (device_texts(a.recs, a.out), a.recs, a.order)
        for with_ez, without in ((2, 0), (3, 1)):
            assert [E.strip(s) for s in got[with_ez][0]] == got[without][0]
            assert got[with_ez][2].tobytes() == got[without][2].tobytes()
            assert got[with_ez][1]["n_rings"].tolist() == got[without][1]["n_rings"].tolist()
            assert ((got[with_ez][1]["flags"] ^ got[without][1]["flags"]) & 0x3FF == 0).all()
        assert [s.replace("@", "") for s in got[3][0]] == got[2][0]
        assert ((got[3][1]["flags"] ^ got[2][1]["flags"]) & 0x1C00 == 0).all()
        refused = (got[2][1]["flags"] & SMILES_REFUSED).astype(bool)
        assert not (got[2][1]["flags"][refused] & 0x1C00).any()
    for marks in MODES:
        check(eng, pool, marks)
    assert refused.sum() > 5 and (~refused).sum() > 50


def test_refused_calls_launch_nothing_and_name_the_new_function(eng, dev, synth_ckpt):
    t = Tables(dev, [H.PINNED[k][:3] for k in sorted(H.PINNED)])
    need = E.pack(t.mols, t.atoms, t.bonds, t.text, 3)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **{"marks": 3, **over}), "mnx_smiles_pack_marks: " + expect)

    assert run(eng, t, need, 3).rc == 0
    for marks in (4, 7, 8, 0x80000002):
        refused("marks may hold MNX_SMILES_MARK_TETRAHEDRAL and MNX_SMILES_MARK_DOUBLE_BOND only", marks=marks)
    for name in ("mols", "atoms", "bonds", "text", "recs", "out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    refused("mols, atoms and bonds must be 8-byte aligned, recs and totals 4-byte, order 2-byte", order=_p(t.d[0], 1))

    class Bare(Engine):                                      # a fresh handle that was told no symbol tables
        def _set_symbol_tables(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        refused("call mnx_set_symbol_tables first", h=bare.h)
    finally:
        bare.close()


def test_end_to_end_predict_pipeline_double_bonds(eng, dev):
    """8 synthetic images through predict_pipeline(packed=True, smiles=True, stereo=True, double_bonds=True): every graph_smiles
    equals the oracle on the same tables, and without its marks the string of a run without them. The synthetic checkpoint's
    near-complete graphs hold few candidates, so equality is the assertion, not a count."""
    from molnextr_amd.model import predict_pipeline
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    for stereo in (False, True):
        ref = E.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], 2 + stereo)
        recs, order, data = eng.smiles_pack(rec, stereo=stereo, double_bonds=True)
        assert data == ref["out"] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
    marked = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, stereo=True, double_bonds=True)
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, stereo=True)
    written = 0
    for b, (p, q, want) in enumerate(zip(marked, plain, texts(ref))):
        refused = bool(ref["recs"]["flags"][b] & SMILES_REFUSED)
        assert p["graph_smiles"] == (None if refused else want) and p["graph_smiles_order"] == q["graph_smiles_order"]
        assert (E.strip(p["graph_smiles"]) if not refused else None) == q["graph_smiles"]
        written += not refused
    assert written
