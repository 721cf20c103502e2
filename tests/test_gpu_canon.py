"""GPU (-m gpu): mnx_smiles_pack_canonical — canonical atom ranks, symmetry classes and the graph SMILES written on those ranks —
against the oracle of tests/canon_ref.py, byte for byte and word for word (recs, order, rank, sym_class, text, totals; no
tolerances), for marks 0..3: the strings that pin the rule, the generated molecules of the CPU tests, the device against its own
older call on the renumbered tables, renumbered and shuffled tables, the sizes at which the kernel's loops take another turn,
the refusal cases, the protocol, the two molecules that make the ranking run longest, and one end-to-end run."""
import numpy as np
import pytest

import canon_ref as K
import ez_ref as E
import smiles_ref as S
import stereo_ref as T
import test_canon_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_CANON_TIE, SMILES_CANON_TIE_INDEX, SMILES_REFUSED
from packed_tables import (FILL, WORD_FILL, Tables, _p, assert_refused, call_text, compare_text, dev, eng, random_molecule,  # noqa: F401
                           same_results, texts)

pytestmark = pytest.mark.gpu

TIE_BITS = SMILES_CANON_TIE | SMILES_CANON_TIE_INDEX
E2E_FIRST_INDEX = 500          # the batch of the plain writer's end-to-end test
MODES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def generated(dev):
    """the pinned molecules and the two generated sets as one batch, and the oracle's result for every set of marks"""
    mols = [H.PINNED[k][0] for k in sorted(H.PINNED)] + T.generated_set() + E.generated_set()
    t = Tables(dev, mols)
    return mols, t, {m: K.pack(t.mols, t.atoms, t.bonds, t.text, m, order_fill=WORD_FILL) for m in MODES}


def run(eng, t, out_cap, marks=0, **over):
    return call_text("mnx_smiles_pack_canonical", eng, t, out_cap, marks=marks, **over)


def check(eng, t, marks, ref=None):
    """the device's recs, order, rank, sym_class, bytes and totals equal the oracle's at the exact capacity; returns the oracle's"""
    ref = ref or K.pack(t.mols, t.atoms, t.bonds, t.text, marks, order_fill=WORD_FILL)
    compare_text(run(eng, t, ref["total"], marks), ref, "SMILES")
    return ref


@pytest.mark.parametrize("marks", MODES)
def test_pinned_and_generated_molecules_in_one_call(eng, generated, marks):
    mols, t, refs = generated
    ref = refs[marks]
    names = sorted(H.PINNED)
    assert t.n == len(names) + 600
    for k, (name, text) in enumerate(zip(names, texts(ref))):
        if marks in H.PINNED[name][1]:
            assert text == H.PINNED[name][1][marks], name
    flags = ref["recs"]["flags"]
    assert 100 < (flags & SMILES_CANON_TIE).astype(bool).sum() < 500 and ((flags & SMILES_REFUSED) == 0).all()
    check(eng, t, marks, ref)


def renumbered_tables(t, rank):
    """the same tables with atom a of every ranked molecule moved to record rank[a]; bond records with the lower number as i,
    `type` and `rev` swapped where the ends swap"""
    atoms, bonds = t.atoms.copy(), t.bonds.copy()
    for m in t.mols:
        a0, na, b0, nb = int(m["atom0"]), int(m["n_atoms"]), int(m["bond0"]), int(m["n_bonds"])
        r = rank[a0:a0 + na].astype(np.int64)
        if na == 0 or r[0] == K.NO_RANK:
            continue
        atoms[a0 + r] = t.atoms[a0:a0 + na]
        for k in range(b0, b0 + nb):
            i, j = int(r[t.bonds[k]["i"]]), int(r[t.bonds[k]["j"]])
            if i < j:
                bonds[k]["i"], bonds[k]["j"] = i, j
            else:
                bonds[k]["i"], bonds[k]["j"], bonds[k]["type"], bonds[k]["rev"] = j, i, t.bonds[k]["rev"], t.bonds[k]["type"]
    return atoms, bonds


@pytest.mark.parametrize("marks", MODES)
def test_device_against_its_own_older_call_on_the_renumbered_tables(eng, dev, generated, marks):
    """the tables renumbered by the returned ranks go through mnx_smiles_pack_marks: the same bytes, lengths and n_rings, the
    same flags apart from the tie bits, and `order` carried over through the ranks"""
    mols, t, refs = generated
    need = refs[marks]["total"]
    a = run(eng, t, need, marks)
    assert a.rc == 0 and a.totals.tolist() == [need, 0]
    recs, order, rank = a.recs, a.order, a.rank
    atoms, bonds = renumbered_tables(t, rank)
    moved = Tables(dev, arrays=(t.mols, atoms, bonds, t.text))
    b = call_text("mnx_smiles_pack_marks", eng, moved, need, marks=marks)
    assert b.rc == 0 and b.totals.tolist() == [need, 0]
    recs2, order2 = b.recs, b.order
    assert np.array_equal(a.out[:need], b.out[:need])
    for name in ("text0", "len", "n_rings"):
        assert np.array_equal(recs[name], recs2[name]), name
    assert np.array_equal(recs["flags"] & ~np.uint32(TIE_BITS), recs2["flags"]) and (recs["flags"] & SMILES_CANON_TIE).any()
    for m in t.mols:
        a0, na = int(m["atom0"]), int(m["n_atoms"])
        assert np.array_equal(order[a0:a0 + na], order2[a0:a0 + na][rank[a0:a0 + na]])


def test_renumbered_and_bond_shuffled_tables_give_identical_bytes(eng, dev, generated):
    """every molecule of the batch in a new numbering, its bond records in a new order with their ends swapped where the numbers
    ask for it: the same bytes, lengths, n_rings and flags for every set of marks, and the same ranks on the moved atoms. A
    molecule in which the atom index decided a tie (bit 14) is outside the claim and stays as it was."""
    mols, t, refs = generated
    rng = np.random.default_rng(81)
    by_index = (refs[0]["recs"]["flags"] & SMILES_CANON_TIE_INDEX).astype(bool)
    assert by_index.sum() <= len(mols) // 20
    perms = [list(range(len(m[0]))) if by_index[b] else [int(p) for p in rng.permutation(len(m[0]))] for b, m in enumerate(mols)]
    t2 = Tables(dev, [m if by_index[b] else T.renumber(m, perms[b], rng) for b, m in enumerate(mols)])
    for marks in MODES:
        need = refs[marks]["total"]
        a, b = run(eng, t, need, marks), run(eng, t2, need, marks)
        assert a.rc == b.rc == 0 and a.totals.tolist() == b.totals.tolist() == [need, 0]
        assert a.recs.tobytes() == b.recs.tobytes() and np.array_equal(a.out, b.out)
        for m, p in zip(t.mols, perms):
            a0, na = int(m["atom0"]), int(m["n_atoms"])
            for w in ("order", "rank", "sym_class"):          # atom k is now atom p[k]
                assert np.array_equal(getattr(a, w)[a0:a0 + na], getattr(b, w)[a0:a0 + na][p])


def chain(n, rng):
    syms = [(b"C", b"C", b"N", b"O")[int(k)] for k in rng.integers(0, 4, n)]
    return syms, [(int(x), int(y)) for x, y in rng.integers(0, 2048, (n, 2))], [(k, k + 1, 1, 1) for k in range(n - 1)]


def tree(n, rng):
    syms = [(b"C", b"C", b"C", b"N", b"c", b"[nH]", b"R")[int(k)] for k in rng.integers(0, 7, n)]
    bonds = [(int(rng.integers(0, k)), k, int(rng.integers(1, 7)), int(rng.integers(0, 7))) for k in range(1, n)]
    return syms, [(int(x), int(y)) for x, y in rng.integers(0, 2048, (n, 2))], bonds


def star(degree):
    return [b"C"] * (degree + 1), [(k, 2 * k % 41) for k in range(degree + 1)], [(0, k, 1 + k % 4, 1) for k in range(1, degree + 1)]


def many_ring_numbers():
    """a hub bonded to 101 atoms of a path: more than 99 ring numbers open at the hub"""
    return ([b"C"] * 102, [(k, 0) for k in range(102)],
            [(0, k, 1, 1) for k in range(1, 102)] + [(k, k + 1, 1, 1) for k in range(1, 101)])


DUPLICATE = (H.DIFLUORO[0], H.DIFLUORO[1], H.CHAIN3 + [(2, 1, 1, 1)])
EMPTY = ([], [], [])


@pytest.mark.parametrize("size", (1, 2, 255, 256, 257, 999))
def test_sizes_at_which_the_loops_take_another_turn(eng, dev, size):
    """a chain and a random tree (every bond class, pseudo-atoms, aromatic atoms) of `size` atoms, renumbered at random: 256
    threads take the atoms in strides, four atoms to a thread in the rank rounds"""
    rng = np.random.default_rng(82 + size)
    mols = [T.renumber(f(size, rng), [int(p) for p in rng.permutation(size)], rng) for f in (chain, tree)]
    t = Tables(dev, mols)
    ref = check(eng, t, 3)
    assert not (ref["recs"]["flags"] & SMILES_REFUSED).any() and sorted(ref["rank"][:size].tolist()) == list(range(size))
    check(eng, t, 0)


def test_refused_and_special_molecules_alone_and_in_one_batch(eng, dev):
    """1000 atoms (refused: 0xFFFF), a star of degree 40, a duplicate bond (0xFFFF in rank), more than 99 ring numbers (no string,
    valid ranks), an empty molecule, random graphs of every symbol class, and ordinary molecules between them"""
    rng = np.random.default_rng(83)
    too_large = chain(1000, rng)
    special = [too_large, star(40), DUPLICATE, many_ring_numbers(), EMPTY]
    for mol in special[1:]:
        check(eng, Tables(dev, [mol]), 3)
    pool = [random_molecule(rng, int(n), int(n) + int(rng.integers(-2, 3))) for n in rng.integers(3, 40, 40)]
    batch = []
    for k, mol in enumerate(special + pool):
        batch += [mol, H.PINNED[sorted(H.PINNED)[k % len(H.PINNED)]][0]]
    t = Tables(dev, batch)
    for marks in MODES:
        ref = check(eng, t, marks)
    flags = ref["recs"]["flags"][:10:2].tolist()
    assert flags[0] == S.FLAG_TOO_LARGE and flags[2] == S.FLAG_DUPLICATE and flags[3] & S.FLAG_RINGS and flags[3] & SMILES_CANON_TIE
    assert flags[4] == 0 and not flags[1] & SMILES_REFUSED
    a0 = [int(m["atom0"]) for m in t.mols]
    assert set(ref["rank"][a0[0]:a0[1]].tolist()) == set(ref["sym_class"][a0[0]:a0[1]].tolist()) == {K.NO_RANK}
    assert set(ref["rank"][a0[4]:a0[5]].tolist()) == {K.NO_RANK} and set(ref["order"][a0[6]:a0[7]].tolist()) == {S.NO_POSITION}
    assert sorted(ref["rank"][a0[6]:a0[7]].tolist()) == list(range(102))
    assert (ref["recs"]["flags"][10::2] & SMILES_REFUSED).astype(bool).sum() > 3


def test_records_beyond_the_tables_are_refused(eng, dev):
    """the sizes of the tables one record short of the last molecule's: that molecule is refused on bit 1 and its atoms inside the
    table hold 0xFFFF; the others are untouched"""
    mols = [H.PINNED[k][0] for k in sorted(H.PINNED)]
    t = Tables(dev, mols)
    for short in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        names = {"na": "n_atom_records", "nb": "n_bond_records", "nt": "n_text_bytes"}
        ref = K.pack(t.mols, t.atoms, t.bonds, t.text, 3, order_fill=WORD_FILL, **{names[k]: v for k, v in short.items()})
        a = run(eng, t, ref["total"], 3, **short)
        assert a.rc == 0 and a.totals.tolist() == [ref["total"], 0] and a.recs.tobytes() == ref["recs"].tobytes()
        assert ref["recs"]["flags"][-1] == S.FLAG_BEYOND and a.out[:ref["total"]].tobytes() == ref["out"]
        n = len(ref["rank"])
        for name in ("order", "rank", "sym_class"):
            got = getattr(a, name)
            assert np.array_equal(got[:n], ref[name]) and (got[n:] == WORD_FILL).all(), name


def test_tie_decided_by_the_index(eng, dev):
    on_one_bin = (H.DIFLUORO[0], [(0, 20), (10, 10), (10, 10), (30, 0)], H.CHAIN3)
    methyls = ([b"C"] * 5, [(10, 10), (0, 10), (20, 10), (20, 10), (10, 20)], [(0, k, 1, 1) for k in range(1, 5)])
    ref = check(eng, Tables(dev, [on_one_bin, H.DIFLUORO, methyls]), 3)
    assert [int(f) & TIE_BITS for f in ref["recs"]["flags"]] == [TIE_BITS, SMILES_CANON_TIE, TIE_BITS]


def test_protocol(eng, generated):
    """the sizing call without a buffer, the exact size, one byte short; `order` and `sym_class` left out"""
    mols, t, refs = generated
    ref = refs[3]
    need = ref["total"]
    a = run(eng, t, 0, 3, out=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and np.all(a.out == FILL)
    assert a.order.tobytes() == ref["order"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes() and a.sym_class.tobytes() == ref["sym_class"].tobytes()
    a = run(eng, t, need - 1, 3)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes()
    assert a.out[:need - 1].tobytes() == ref["out"][:need - 1] and np.all(a.out[need - 1:] == FILL)
    a = run(eng, t, need, 3, order=None, sym_class=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 0] and a.recs.tobytes() == ref["recs"].tobytes() and a.rank.tobytes() == ref["rank"].tobytes()
    assert a.out[:need].tobytes() == ref["out"] and (a.order == WORD_FILL).all() and (a.sym_class == WORD_FILL).all()


def test_refused_calls_launch_nothing_and_name_the_new_function(eng, dev):
    t = Tables(dev, [H.PINNED[k][0] for k in sorted(H.PINNED)])
    need = K.pack(t.mols, t.atoms, t.bonds, t.text, 3)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **{"marks": 3, **over}), "mnx_smiles_pack_canonical: " + expect)

    assert run(eng, t, need, 3).rc == 0
    for marks in (4, 8, 0x80000001):
        refused("marks may hold MNX_SMILES_MARK_TETRAHEDRAL and MNX_SMILES_MARK_DOUBLE_BOND only", marks=marks)
    for name in ("rank", "mols", "atoms", "recs", "out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    refused("mols, atoms and bonds must be 8-byte aligned, recs and totals 4-byte, order, rank and sym_class 2-byte", rank=_p(t.d[0], 1))


def test_two_runs_are_word_identical(eng, generated):
    mols, t, refs = generated
    for marks in (0, 3):
        a, b = run(eng, t, refs[marks]["total"], marks), run(eng, t, refs[marks]["total"], marks)
        same_results(a, b)
        assert a.rc == b.rc == 0


def test_the_two_molecules_that_rank_longest(eng, dev):
    """999 identical isolated atoms (998 ties, one round each) and a ring of 999 (two ties, about a thousand rounds): the most
    passes and the most rounds the ranking's loops can take"""
    xy = [(k // 40, k % 40) for k in range(999)]            # ascending in k: the isolated atoms keep their order
    isolated = ([b"C"] * 999, xy, [])
    ring = ([b"C"] * 999, xy, [(k, k + 1, 1, 1) for k in range(998)] + [(0, 998, 1, 1)])
    ref = check(eng, Tables(dev, [isolated, ring]), 0)
    assert texts(ref) == ["C" + ".C" * 998, "C1" + "C" * 997 + "C1"] and ref["recs"]["flags"].tolist() == [SMILES_CANON_TIE] * 2
    assert ref["sym_class"].tolist() == [0] * 1998 and ref["rank"][:999].tolist() == list(range(999))


def test_end_to_end_predict_pipeline_and_molnextr(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images through predict_pipeline(packed=True, smiles=True, canonical=True) with and without marks: strings,
    order, ranks and classes equal the oracle's on the returned tables; without canonical the bytes are the older call's; and
    molnextr(graph_canonical=True) hands them on"""
    from molnextr_amd.model import molnextr, predict_pipeline
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    written = 0
    for stereo, double_bonds in ((False, False), (True, True)):
        marks = stereo + 2 * double_bonds
        ref = K.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], marks)
        recs, order, data, rank, sym_class = eng.smiles_pack(rec, stereo=stereo, double_bonds=double_bonds, canonical=True)
        assert data == ref["out"] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
        assert rank.tobytes() == ref["rank"].tobytes() and sym_class.tobytes() == ref["sym_class"].tobytes()
        preds = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, stereo=stereo, double_bonds=double_bonds, canonical=True)
        plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, stereo=stereo, double_bonds=double_bonds)
        old = E.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], marks)
        for b, (p, q, m) in enumerate(zip(preds, plain, rec["mols"])):
            a0, na = int(m["atom0"]), int(m["n_atoms"])
            refused = bool(ref["recs"]["flags"][b] & SMILES_REFUSED)
            assert p["graph_smiles"] == (None if refused else texts(ref)[b])
            ranked = ref["rank"][a0] != K.NO_RANK if na else True
            assert p["canonical_rank"] == (ref["rank"][a0:a0 + na].tolist() if ranked else None)
            assert p["symmetry_class"] == (ref["sym_class"][a0:a0 + na].tolist() if ranked else None)
            assert q["graph_smiles"] == (None if old["recs"]["flags"][b] & SMILES_REFUSED else texts(old)[b]) and "canonical_rank" not in q
            written += not refused
    assert written

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(4)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_canonical=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True, canonical=True)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert [o["canonical_rank"] for o in got] == [p["canonical_rank"] for p in want]
        assert [o["symmetry_class"] for o in got] == [p["symmetry_class"] for p in want]
        m.graph_canonical = False                              # the default: the bytes it gave before
        before = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True)
        again = m.predict_images(pages, batch_size=4)
        assert [o["predicted_smiles"] for o in again] == [p["graph_smiles"] for p in before] and "canonical_rank" not in again[0]
    finally:
        m.engine.close()
