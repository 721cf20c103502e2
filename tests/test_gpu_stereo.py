"""GPU (-m gpu): mnx_smiles_pack_stereo — the graph SMILES with '@' / '@@' written on the device — against the oracle of
tests/stereo_ref.py, byte for byte and record for record, `order` included (no tolerances): the strings that pin the rule, the
generated molecules of the CPU tests, the sizes at which the kernel's loops take another turn, the capacity and argument
handling of the sibling call, the property that removing the marks gives mnx_smiles_pack's output, and one end-to-end run."""
import ctypes as C

import numpy as np
import pytest
import torch

import molfile_ref as M
import smiles_ref as S
import stereo_ref as T
import test_stereo_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_DTYPE, SMILES_REFUSED, SMILES_STEREO, SMILES_STEREO_UNRESOLVED, Engine
from packed_tables import FILL, GUARD, POOL, Tables, _p, compare, random_molecule

pytestmark = pytest.mark.gpu

ORDER_FILL = FILL | FILL << 8
E2E_FIRST_INDEX = 500          # the batch of the plain writer's end-to-end test: two of its eight molecules are written


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    yield e
    e.close()


@pytest.fixture(scope="module")
def generated(dev):
    mols = T.generated_set()
    t = Tables(dev, mols)
    return mols, t, T.pack(t.mols, t.atoms, t.bonds, t.text, order_fill=ORDER_FILL)


def run(eng, t, out_cap, fn="mnx_smiles_pack_stereo", **over):
    """One call into FILL-filled outputs with GUARD bytes behind each: (rc, recs, order, the whole out arena, totals)"""
    na, nb, nt = len(t.atoms), len(t.bonds), len(t.text)
    recs = torch.full((t.n * 16 + GUARD,), FILL, dtype=torch.uint8, device=t.dev)
    order = torch.full((na * 2 + GUARD,), FILL, dtype=torch.uint8, device=t.dev)
    out = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device=t.dev)
    totals = torch.full((8,), FILL, dtype=torch.uint8, device=t.dev)
    a = {"h": eng.h, "mols": _p(t.d[0]), "n": t.n, "atoms": _p(t.d[1]), "na": na, "bonds": _p(t.d[2]), "nb": nb, "text": _p(t.d[3]),
         "nt": nt, "recs": _p(recs), "order": _p(order), "out": _p(out), "out_cap": out_cap, "totals": _p(totals),
         "stream": C.c_void_p(torch.cuda.current_stream().cuda_stream)}
    a.update(over)
    rc = getattr(eng.lib, fn)(*a.values())
    torch.cuda.synchronize()
    r, o, w = recs.cpu().numpy(), out.cpu().numpy(), order.cpu().numpy()
    assert np.all(r[t.n * 16:] == FILL), "bytes behind recs were overwritten"
    assert np.all(w[na * 2:] == FILL), "bytes behind order were overwritten"
    return rc, r[:t.n * 16].view(SMILES_DTYPE), w[:na * 2].view(np.uint16), o, totals.cpu().numpy().view(np.uint32)


def check(eng, t, ref=None):
    """the device's recs, order, bytes and totals equal the oracle's at the exact capacity; returns the oracle's result"""
    ref = ref or T.pack(t.mols, t.atoms, t.bonds, t.text, order_fill=ORDER_FILL)
    rc, recs, order, out, totals = run(eng, t, ref["total"])
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert totals.tolist() == [ref["total"], 0]
    compare(recs, ref["recs"], out, ref["out"], ref["total"], "SMILES")
    bad = np.nonzero(order != ref["order"])[0]
    assert bad.size == 0, ("order", bad[:5], order[bad[:5]], ref["order"][bad[:5]])
    return ref


def texts(ref):
    return [ref["out"][r["text0"]:r["text0"] + r["len"]].decode() for r in ref["recs"]]


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
    rc, recs, order, _, totals = run(eng, t, 0, out=None)
    assert rc == 0 and totals.tolist() == [need, 1] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
    for cap in (need, need - 1):
        rc, recs, order, out, totals = run(eng, t, cap)
        assert rc == 0 and totals.tolist() == [need, int(cap < need)]
        assert recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
        assert out[:cap].tobytes() == ref["out"][:cap] and np.all(out[cap:] == FILL), cap


def test_two_runs_are_byte_identical(eng, generated):
    mols, t, ref = generated
    a, b = run(eng, t, ref["total"]), run(eng, t, ref["total"])
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert np.array_equal(a[3], b[3]) and a[4].tolist() == b[4].tolist() == [ref["total"], 0]


def test_without_the_marks_it_is_the_plain_writer(eng, dev, generated):
    """on the generated set and on random graphs over every class of symbol: the stereo call's strings with '@' removed, its
    order, n_rings and flag bits 0-5 and 7 are those of mnx_smiles_pack on the same tables"""
    rng = np.random.default_rng(43)
    pool = Tables(dev, [random_molecule(rng, int(n), int(n) + int(rng.integers(-2, 3))) for n in rng.integers(3, 40, 200)])
    for t in (generated[1], pool):
        ref = check(eng, t)
        rc, recs, order, out, totals = run(eng, t, ref["total"], fn="mnx_smiles_pack")
        assert rc == 0
        plain = [out[r["text0"]:r["text0"] + r["len"]].tobytes().decode() for r in recs]
        assert [s.replace("@", "") for s in texts(ref)] == plain and order.tobytes() == ref["order"].tobytes()
        assert recs["n_rings"].tolist() == ref["recs"]["n_rings"].tolist()
        assert ((recs["flags"] ^ ref["recs"]["flags"]) & 0xBF == 0).all() and not (recs["flags"] & 0x300).any()
        assert (ref["recs"]["len"] - recs["len"]).tolist() == [s.count("@") for s in texts(ref)]
    written = ~(ref["recs"]["flags"] & SMILES_REFUSED).astype(bool)
    assert written.sum() > 50 and (ref["recs"]["flags"] & SMILES_STEREO_UNRESOLVED).any() and (~written).sum() > 5


def test_refused_calls_launch_nothing_and_name_the_new_function(eng, dev, synth_ckpt):
    t = Tables(dev, [H.PINNED[k][:3] for k in ("1", "2", "3")])
    need = T.pack(t.mols, t.atoms, t.bonds, t.text)["total"]

    def refused(expect, **over):
        rc, recs, order, out, totals = run(eng, t, need, **over)
        msg = eng.lib.mnx_last_error(over.get("h", eng.h)).decode()
        assert rc == -1 and msg == "mnx_smiles_pack_stereo: " + expect, (over, rc, msg)
        assert np.all(recs.view(np.uint8) == FILL) and np.all(out == FILL) and np.all(totals.view(np.uint8) == FILL), over
        assert np.all(order == ORDER_FILL), over

    assert run(eng, t, need)[0] == 0
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
