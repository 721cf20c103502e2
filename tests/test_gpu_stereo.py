"""GPU (-m gpu): mnx_smiles_pack_stereo — the graph SMILES with '@' / '@@' written on the device — against the oracle of
tests/stereo_ref.py, byte for byte and record for record, `order` included (no tolerances): the strings that pin the rule, the
generated molecules of the CPU tests, the sizes at which the kernel's loops take another turn, the capacity and argument
handling of the sibling call, the property that removing the marks gives mnx_smiles_pack's output, and one end-to-end run."""
import numpy as np
import pytest

import smiles_ref as S
import stereo_ref as T
import test_stereo_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_REFUSED, SMILES_STEREO, SMILES_STEREO_UNRESOLVED, Engine
from packed_tables import (FILL, Tables, _p, assert_refused, call_text, compare_text, dev, device_texts, eng, random_molecule,  # noqa: F401
                           same_results, texts)
from packed_tables import WORD_FILL as ORDER_FILL

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the plain writer's end-to-end test: two of its eight molecules are written


@pytest.fixture(scope="module")
def generated(dev):
    mols = T.generated_set()
    t = Tables(dev, mols)
    return mols, t, T.pack(t.mols, t.atoms, t.bonds, t.text, order_fill=ORDER_FILL)


def run(eng, t, out_cap, fn="mnx_smiles_pack_stereo", **over):
    return call_text(fn, eng, t, out_cap, **over)


def check(eng, t, ref=None):
    """the device's recs, order, bytes and totals equal the oracle's at the exact capacity; returns the oracle's result"""
    ref = ref or T.pack(t.mols, t.atoms, t.bonds, t.text, order_fill=ORDER_FILL)
    compare_text(run(eng, t, ref["total"]), ref, "SMILES")
    return ref


def test_pinned_strings_and_flag_cases(eng, dev):
    names, cases = sorted(H.PINNED), sorted(H.FLAG_CASES)
    t = Tables(dev, [H.PINNED[k][:3] for k in names] + [H.FLAG_CASES[k][0] for k in cases])
    ref = check(eng, t)
    assert texts(ref)[:len(names)] == [H.PINNED[k][3] for k in names]
    assert ref["recs"]["flags"].tolist() == [H.PINNED[k][4] for k in names] + [H.FLAG_CASES[k][1] for k in cases]


def test_generated_molecules_in_one_call(eng, generated):
    mols, t, ref = generated
    assert t.n == 300 and ref["out"].count(b"@@") > 100 and (ref["recs"]["flags"] & SMILES_STEREO).sum() > 200
    check(eng, t, ref)


def test_600_atoms_centres_in_every_stride(eng, dev):
    """one molecule of 600 atoms: the loops over the atoms stride by 256 threads and the pieces take four atoms per thread, so
    marked centres stand below index 256, past it, past 512 and at the last atom"""
    rng = np.random.default_rng(41)
    mol = T.generate(rng, 600, 40)
    marked = sorted(c for c, r in T.smiles(*mol)[4].items() if r["mark"])
    perm = [int(p) for p in rng.permutation(600)]
    other = perm.index(599)
    perm[other], perm[marked[0]] = perm[marked[0]], 599                    # a marked centre becomes the last atom
    mol = T.renumber(mol, perm, rng)
    text, pos, flags, _, centre = T.smiles(*mol)
    now = sorted(c for c, r in centre.items() if r["mark"])
    assert now[-1] == 599 and now[0] < 256 and any(256 <= c < 512 for c in now) and any(512 <= c < 599 for c in now) and len(now) > 60
    for c, (mark, hand, _) in T.read_back(text, pos, mol[1], mol[2]).items():
        assert mark == hand
    ref = check(eng, Tables(dev, [mol, H.PINNED["2"][:3]]))
    assert texts(ref) == [text, "N[C@@H](C)C(=O)O"]


def test_1030_small_molecules_past_the_scan_tile(eng, dev):
    rng = np.random.default_rng(42)
    mols = []
    for k in range(1030):
        perm = [int(p) for p in rng.permutation(5)]
        xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (5, 2))]
        base = H.PINNED["1"] if k % 2 else ([b"N", b"[C@H]", b"C", b"O", b"C"], None, [(0, 1, 1, 1), (1, 2, 5, 6), (1, 3, 1, 1), (3, 4, 1, 1)])
        mols.append(T.renumber((base[0], xy, base[2]), perm, rng))
    ref = check(eng, Tables(dev, mols))
    assert (ref["recs"]["flags"] & SMILES_STEREO).sum() > 1000 and ref["recs"]["text0"][-1] + ref["recs"]["len"][-1] == ref["total"]
    assert ref["out"].count(b"@@") > 300 and ref["out"].count(b"@") - 2 * ref["out"].count(b"@@") > 300


def test_a_centre_with_a_neighbour_beyond_the_table_is_refused(eng, dev):
    t = Tables(dev, [H.PINNED["1"][:3], H.PINNED["2"][:3], H.PINNED["3"][:3]])
    mols, atoms, bonds, text = (a.copy() if isinstance(a, np.ndarray) else a for a in (t.mols, t.atoms, t.bonds, t.text))
    bonds["j"][int(mols["bond0"][1]) + 1] = 6                  # the wedge of molecule 1's centre ends at an atom it does not have
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert ref["recs"]["flags"].tolist() == [T.FLAG_STEREO, S.FLAG_BEYOND, T.FLAG_STEREO] and ref["recs"]["len"][1] == 0
    assert texts(ref) == ["F[C@](Cl)(Br)I", "", "[C@H]1(CC1)F"] and (ref["order"][5:11] == S.NO_POSITION).all()


def test_capacities(eng, generated):
    """the sizing call without a buffer, the exact size, one byte short: totals, recs and order complete, nothing written beyond
    out_cap"""
    mols, t, ref = generated
    need = ref["total"]
    a = run(eng, t, 0, out=None)
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
    for cap in (need, need - 1):
        a = run(eng, t, cap)
        assert a.rc == 0 and a.totals.tolist() == [need, int(cap < need)]
        assert a.recs.tobytes() == ref["recs"].tobytes() and a.order.tobytes() == ref["order"].tobytes()
        assert a.out[:cap].tobytes() == ref["out"][:cap] and np.all(a.out[cap:] == FILL), cap


def test_two_runs_are_byte_identical(eng, generated):
    mols, t, ref = generated
    a, b = run(eng, t, ref["total"]), run(eng, t, ref["total"])
    same_results(a, b)
    assert a.rc == b.rc == 0 and a.totals.tolist() == b.totals.tolist() == [ref["total"], 0]


def test_without_the_marks_it_is_the_plain_writer(eng, dev, generated):
    """on the generated set and on random graphs over every class of symbol: the stereo call's strings with '@' removed, its
    order, n_rings and flag bits 0-5 and 7 are those of mnx_smiles_pack on the same tables"""
    rng = np.random.default_rng(43)
    pool = Tables(dev, [random_molecule(rng, int(n), int(n) + int(rng.integers(-2, 3))) for n in rng.integers(3, 40, 200)])
    for t in (generated[1], pool):
        ref = check(eng, t)
        a = run(eng, t, ref["total"], fn="mnx_smiles_pack")
        assert a.rc == 0
        recs, plain = a.recs, device_texts(a.recs, a.out)
        assert [s.replace("@", "") for s in texts(ref)] == plain and a.order.tobytes() == ref["order"].tobytes()
        assert recs["n_rings"].tolist() == ref["recs"]["n_rings"].tolist()
        assert ((recs["flags"] ^ ref["recs"]["flags"]) & 0xBF == 0).all() and not (recs["flags"] & 0x300).any()
        assert (ref["recs"]["len"] - recs["len"]).tolist() == [s.count("@") for s in texts(ref)]
    written = ~(ref["recs"]["flags"] & SMILES_REFUSED).astype(bool)
    assert written.sum() > 50 and (ref["recs"]["flags"] & SMILES_STEREO_UNRESOLVED).any() and (~written).sum() > 5


def test_refused_calls_launch_nothing_and_name_the_new_function(eng, dev, synth_ckpt):
    t = Tables(dev, [H.PINNED[k][:3] for k in ("1", "2", "3")])
    need = T.pack(t.mols, t.atoms, t.bonds, t.text)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **over), "mnx_smiles_pack_stereo: " + expect)

    assert run(eng, t, need).rc == 0
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


def test_end_to_end_predict_pipeline_stereo(eng, dev):
    """8 synthetic images through predict_pipeline(packed=True, smiles=True, stereo=True): every graph_smiles equals the oracle on
    the same tables, and without its marks the string of a stereo=False run. The synthetic checkpoint's near-complete graphs
    resolve few centres, so equality is the assertion, not a count."""
    from molnextr_amd.model import predict_pipeline
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    ref = T.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"])
    recs, order, data = eng.smiles_pack(rec, stereo=True)
    assert data == ref["out"] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
    marked = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, stereo=True)
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True)
    written = 0
    for b, (p, q, want) in enumerate(zip(marked, plain, texts(ref))):
        refused = bool(ref["recs"]["flags"][b] & SMILES_REFUSED)
        assert p["graph_smiles"] == (None if refused else want) and p["graph_smiles_order"] == q["graph_smiles_order"]
        assert (p["graph_smiles"].replace("@", "") if not refused else None) == q["graph_smiles"]
        written += not refused
    assert written
