"""GPU (-m gpu): mnx_molfile_pack — V2000 molfiles written on the device from the packed molecule tables — against the oracle
of tests/molfile_ref.py, byte for byte and record for record (no tolerances), on hand-built tables uploaded with torch: the
sizes at which the kernels take another path, the capacity and argument handling, and one end-to-end run through
Engine.predict, predict_pipeline and the facade. The kernel's rounding is never seen at an exact tie here: the engine's 64
coordinate bins give the odd den = 63, and 2 * bin * S is even (tests/test_molfile_host.py::test_coordinate_rule shows it and
covers the tie in the oracle with den = 64); the kernel rounds with the same integer expression."""
import functools

import numpy as np
import pytest

import molfile_ref as R
import smiles_ref as S
import test_molfile_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import Engine
from packed_tables import (FILL, POOL, UTF2, Tables, _p, assert_refused, call_text, compare_text, dev, eng, random_molecule,  # noqa: F401
                           same_results)

pytestmark = pytest.mark.gpu

# run(eng, t, out_cap, sizes=None, **over); the result's `recs` are the `files`; scale: an int array [n, 2] or a raw pointer
run = functools.partial(call_text, "mnx_molfile_pack")


def check(eng, t, scale=None, sizes=None, ref_kw=None):
    """the device's files, bytes and totals equal the oracle's at the exact capacity; returns the oracle's result"""
    kw = dict(zip(("n_atom_records", "n_bond_records", "n_text_bytes"), sizes)) if sizes is not None else {}
    ref = R.pack(t.mols, t.atoms, t.bonds, t.text, scale=scale, **kw, **(ref_kw or {}))
    compare_text(run(eng, t, ref["total"], sizes, scale=scale), ref, "molfiles")
    return ref


def test_hand_written_blocks_and_tiny_molecules(eng, dev):
    names = sorted(H.HAND)
    t = Tables(dev, [([], [], []), ([b"[NH4+]"], [(5, 9)], [])] + [H.HAND[k][0] for k in names] + [([], [], [])])
    ref = check(eng, t)
    empty = b"\n  MolNexTR          2D\n\n  0  0  0  0  0  0  0  0  0  0999 V2000\nM  END\n"
    assert ref["out"].startswith(empty + b"\n  MolNexTR          2D\n\n  1  0  0") and ref["out"].endswith(empty)
    assert ref["out"][2 * len(empty) + 70 + 18:] == b"".join(H.HAND[k][1].encode() for k in names) + empty


def test_every_symbol_class_past_one_tile_of_threads(eng, dev):
    """300 atoms and 400 bonds (more than 256 of each) drawn from POOL, among smaller molecules"""
    rng = np.random.default_rng(11)
    t = Tables(dev, [random_molecule(rng, 7, 6), random_molecule(rng, 300, 400), ([s for s in POOL], [(1, 2)] * len(POOL), []),
                     random_molecule(rng, 257, 255), random_molecule(rng, 2, 1)])
    ref = check(eng, t)
    assert (ref["files"]["flags"][1:4] & R.FLAG_PSEUDO).all() and ref["out"].count(b"M  CHG") > 5 and ref["out"].count(b"\nA  ") > 100


def test_three_digit_limits(eng, dev):
    """999 atoms / bonds are written, 1000 are refused with flag bit 0 and length 0 while the neighbours stay intact; 999 entries
    in each of the three property sections fill their 10-bit counters"""
    rng = np.random.default_rng(12)
    pair = lambda n: [(0, 1, 1 + k % 6, k % 7) for k in range(n)]                                  # noqa: E731
    xy = lambda n: [(k % 64, k // 16 % 64) for k in range(n)]                                        # noqa: E731
    rich = [b"[13CH3+]", b"[R7]", b"[18O-]"]
    t = Tables(dev, [random_molecule(rng, 5, 4), ([b"C", b"[C@H]"] + [b"N"] * 38, xy(40), pair(999)),
                     ([b"C"] * 40, xy(40), pair(1000)), random_molecule(rng, 6, 5),
                     ([rich[k % 3] for k in range(999)], xy(999), pair(3)), ([b"C"] * 1000, xy(1000), pair(3)),
                     ([b"[13CH3+]"] * 999, xy(999), []), ([b"[R999]", b"[R12]"] * 499, xy(998), pair(2)), random_molecule(rng, 3, 2)])
    ref = check(eng, t)
    assert ref["files"]["flags"].tolist()[1:6] == [0, R.FLAG_TOO_LARGE, ref["files"]["flags"][3], R.FLAG_PSEUDO, R.FLAG_TOO_LARGE]
    assert ref["files"]["len"][[2, 5]].tolist() == [0, 0] and ref["files"]["len"][[1, 4, 6]].min() > 13 * 999
    assert b"M  CHG  7 993   1 994   1 995   1 996   1 997   1 998   1 999   1\n" in ref["out"]


def test_seventeen_charges_make_three_lines(eng, dev):
    t = Tables(dev, [([b"[O-]", b"C"] * 17, [(k, k) for k in range(34)], [(k, k + 1, 1, 1) for k in range(33)])])
    ref = check(eng, t)
    assert [ln[:9] for ln in ref["out"].decode().split("\n") if ln.startswith("M  CHG")] == ["M  CHG  8", "M  CHG  8", "M  CHG  1"]


def test_alias_lengths(eng, dev):
    """70 bytes whole, 71 cut to 70, a two-byte character that would straddle byte 70 dropped whole, and one well inside"""
    a70, a71 = b"[" + b"x" * 70 + b"]", b"y" * 71
    straddle, inside = b"z" * 69 + UTF2 + b"w", b"[q" + UTF2 + b"q]"
    t = Tables(dev, [([a70, a71, straddle, inside, b"C"], [(k, k) for k in range(5)], [(0, 4, 1, 1)])])
    ref = check(eng, t)
    lines = ref["out"].split(b"\n")
    assert [lines[lines.index(b"A  %3d" % k) + 1] for k in (1, 2, 3, 4)] == [b"x" * 70, b"y" * 70, b"z" * 69, b"q" + UTF2 + b"q"]


def test_molecule_counts_past_the_scan_tile(eng, dev):
    """1025 molecules, a third of them empty: the scan over the molecules carries from its first tile of 1024 into the second"""
    rng = np.random.default_rng(13)
    sizes = rng.integers(0, 3, 1025) * rng.integers(1, 6, 1025)
    sizes[-1] = 3                                              # the molecule behind the first tile is not empty
    t = Tables(dev, [random_molecule(rng, int(k), int(k)) if k else ([], [], []) for k in sizes])
    assert (t.mols["n_atoms"] == 0).sum() > 200
    ref = check(eng, t)
    assert ref["files"]["text0"][-1] + ref["files"]["len"][-1] == ref["total"] > 100000
    one = Tables(dev, arrays=(t.mols[:1], t.atoms, t.bonds, t.text))
    check(eng, one)


def test_records_beyond_the_tables(eng, dev):
    rng = np.random.default_rng(14)
    ms = [random_molecule(rng, 6, 6) for _ in range(6)]
    t = Tables(dev, ms)
    na, nb, nt = len(t.atoms), len(t.bonds), len(t.text)
    for sizes in ((na - 1, nb, nt), (na, nb - 7, nt), (na, nb, nt - 1), (0, 0, 0), (na - 6, nb - 6, 1)):
        ref = check(eng, t, sizes=sizes)
        assert (ref["files"]["flags"] & R.FLAG_BEYOND).any() and (ref["files"]["len"][(ref["files"]["flags"] & 2) != 0] == 0).all()
    mols, atoms, bonds, text = (a.copy() if isinstance(a, np.ndarray) else a for a in (t.mols, t.atoms, t.bonds, t.text))
    bonds["j"][int(mols["bond0"][1])] = 6                      # a bond to an atom the molecule does not have
    atoms["sym0"][int(mols["atom0"][3]) + 2] = nt              # a symbol behind the text table
    atoms["sym_len"][int(mols["atom0"][4])] = 65535
    mols["flags"][5] = 1
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert [int(f) & 10 for f in ref["files"]["flags"]] == [0, 2, 0, 2, 2, 8] and ref["files"]["len"][[1, 3, 4]].tolist() == [0, 0, 0]


def test_self_bond_one_table_two_writers(eng, dev):
    """The one rule on which the two writers of the packed tables differ: the molfile writes a bond from an atom to itself as the
    record stands, the graph SMILES has no way to write it and refuses the molecule. One table through both writers at the
    oracles' exact capacities, byte for byte; the neighbour is written by both."""
    xy = [(3, 4), (10, 4), (3, 11), (10, 11)]
    t = Tables(dev, [([b"C", b"N", b"O", b"C"], xy, [(0, 1, 1, 1), (2, 2, 1, 1), (2, 3, 2, 2)]), ([b"C", b"C"], xy[:2], [(0, 1, 1, 1)])])
    ref = check(eng, t)
    assert ref["files"]["flags"].tolist() == [0, 0] and ref["files"]["len"].tolist() == [391, 225] and b"\n  3  3  1  0\n" in ref["out"]
    ref = S.pack(t.mols, t.atoms, t.bonds, t.text)
    assert ref["recs"]["flags"].tolist() == [S.FLAG_BEYOND, 0] and ref["recs"]["len"].tolist() == [0, 2] and ref["out"] == b"CC"
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text, "device": tuple(t.d)}
    recs, order, data = eng.smiles_pack(rec, cap=ref["total"])
    assert data == ref["out"] and recs.tobytes() == ref["recs"].tobytes() and order.tobytes() == ref["order"].tobytes()
    assert order.tolist() == [S.NO_POSITION] * 4 + [0, 1]


def test_capacities(eng, dev):
    """out_cap 0, one byte short and exact over a 0x7F-filled buffer: totals and files complete, nothing written beyond out_cap"""
    rng = np.random.default_rng(15)
    t = Tables(dev, [random_molecule(rng, 9, 9) for _ in range(40)])
    ref = R.pack(t.mols, t.atoms, t.bonds, t.text)
    need = ref["total"]
    for cap in (0, need - 1, need // 2, need):
        a = run(eng, t, cap)
        assert a.rc == 0 and a.totals.tolist() == [need, int(cap < need)]
        assert a.recs.tobytes() == ref["files"].tobytes()
        assert a.out[:cap].tobytes() == ref["out"][:cap] and np.all(a.out[cap:] == FILL), cap
    a = run(eng, t, 0, out=None)                                # a sizing call needs no buffer
    assert a.rc == 0 and a.totals.tolist() == [need, 1] and a.recs.tobytes() == ref["files"].tobytes()


def test_scales_and_clamped_bins(eng, dev):
    rng = np.random.default_rng(16)
    ms = [random_molecule(rng, 8, 7) for _ in range(12)]
    t = Tables(dev, ms)
    t.atoms["x_bin"][:5] = [64, 65535, 63, 0, 1000]            # garbage bins are clamped to 0..63
    t.atoms["y_bin"][:5] = [65535, 64, 0, 63, 32768]
    t.atoms["x_bin"][8] = 63                                   # the second molecule reaches the right edge
    t = Tables(dev, arrays=(t.mols, t.atoms, t.bonds, t.text))
    plain = check(eng, t)
    assert plain["out"].split(b"\n")[4].startswith(b"   10.0000    0.0000    0.0000 ")
    same = check(eng, t, scale=np.full((12, 2), 100000))
    assert same["out"] == plain["out"]
    scale = np.array([[1, 1], [10000000, 10000000], [33333, 100000], [177778, 100000], [99999, 100001], [1, 10000000],
                      [0, -5], [20000000, 2 ** 31 - 1], [-2 ** 31, 10000001], [63, 126], [123457, 7], [31, 5000000]])
    other = check(eng, t, scale=scale)                         # rows 6-8 lie outside 1..10 000 000: clamped
    assert other["out"] != plain["out"] and b" 1000.0000" in other["out"]


def test_two_runs_are_byte_identical(eng, dev):
    rng = np.random.default_rng(17)
    t = Tables(dev, [random_molecule(rng, int(k), int(k) + 3) for k in rng.integers(0, 60, 200)])
    need = R.pack(t.mols, t.atoms, t.bonds, t.text)["total"]
    a, b = run(eng, t, need), run(eng, t, need)
    same_results(a, b)
    assert a.rc == b.rc == 0


def test_refused_calls_leave_the_outputs_untouched(eng, dev, synth_ckpt):
    rng = np.random.default_rng(18)
    t = Tables(dev, [random_molecule(rng, 5, 4) for _ in range(3)])
    need = R.pack(t.mols, t.atoms, t.bonds, t.text)["total"]

    def refused(expect, **over):
        assert_refused(run(eng, t, need, **over), "mnx_molfile_pack: " + expect)

    assert run(eng, t, need).rc == 0
    for name in ("mols", "atoms", "bonds", "text", "files", "out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, files, scale and totals 4-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, scale=_p(t.d[0], 2))
    refused(aligned, files=_p(t.d[0], 6))

    class Bare(Engine):                                      # a fresh handle that was told no symbol tables
        def _set_symbol_tables(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        refused("call mnx_set_symbol_tables first", h=bare.h)
        lib, ok = bare.lib, (b"AcR1", np.array([0, 2, 4], np.uint32), np.array([2, 1], np.uint8))

        def set_tables(text, offsets, kinds, n):
            rc = lib.mnx_set_symbol_tables(bare.h, text, offsets.ctypes.data, kinds.ctypes.data, n)
            return rc, lib.mnx_last_error(bare.h).decode()
        for text, offsets, kinds, n, why in (
                (b"R1Ac", ok[1], ok[2], 2, "strictly ascending"), (b"AcAc", ok[1], ok[2], 2, "strictly ascending"),
                (b"AAc", np.array([0, 1, 3], np.uint32), ok[2], 2, None), (b"Ac", np.array([0, 2, 2], np.uint32), ok[2], 2, "is empty or longer"),
                (b"A" * 17 + b"B", np.array([0, 17, 18], np.uint32), ok[2], 2, "is empty or longer"),
                (ok[0], ok[1], np.array([2, 3], np.uint8), 2, "kinds[1] must be 1"), (ok[0], np.array([1, 2, 4], np.uint32), ok[2], 2, "offsets[0]"),
                (ok[0], ok[1], ok[2], 513, "n outside 0..512"), (ok[0], ok[1], ok[2], -1, "n outside 0..512")):
            rc, msg = set_tables(text, offsets, kinds, n)
            assert (rc, why in msg) == (-1, True) if why else rc == 0, (text, rc, msg)
        assert lib.mnx_set_symbol_tables(bare.h, None, ok[1].ctypes.data, ok[2].ctypes.data, 2) == -1
        rc, msg = set_tables(*ok, 2)
        assert rc == 0, msg
        assert set_tables(b"R1Ac", ok[1], ok[2], 2)[0] == -1                          # a refused table leaves the last one in place
        two = Tables(dev, [([b"[Ac]", b"[R1]", b"[OMe]", b"Ph"], [(1, 1)] * 4, [])])
        ref = R.pack(two.mols, two.atoms, two.bonds, two.text, tables={b"Ac": 2, b"R1": 1})
        a = run(eng, two, ref["total"], h=bare.h)
        assert a.rc == 0 and a.out[:ref["total"]].tobytes() == ref["out"] and a.recs.tobytes() == ref["files"].tobytes()
        assert ref["out"].count(b"\nA  ") == 4 and b"M  RGP  1   2   1" in ref["out"]   # 'OMe', 'Ph': no table, no parse
        assert lib.mnx_set_symbol_tables(bare.h, None, None, None, 0) == 0            # no names at all: everything is parsed
        ref = R.pack(two.mols, two.atoms, two.bonds, two.text, tables={})
        a = run(eng, two, ref["total"], h=bare.h)
        assert a.rc == 0 and a.out[:ref["total"]].tobytes() == ref["out"] and b" Ac " in ref["out"] and b"M  RGP" not in ref["out"]
    finally:
        bare.close()


def test_end_to_end_predict_pack_molfile(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: Engine.predict -> graph_pack -> molfile_pack against the oracle over the same records; then
    predict_pipeline(packed=True, molfile=True) and the facade's 'predicted_molfile'"""
    from molnextr_amd.model import molnextr, page_scale, predict_pipeline
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    out = eng.predict(imgs, ref_batch=4)
    rec = eng.graph_pack(out, keep_device=True)
    assert rec["totals"][0] > 8 and rec["totals"][1] > 0
    scale = np.array([[100000 + 7777 * k, 100000 - 999 * k] for k in range(8)])
    for sc in (None, scale):
        ref = R.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], scale=sc)
        for r, cap in ((rec, None), ({k: v for k, v in rec.items() if k != "device"}, 1)):     # from the device tables; uploaded, grown once
            files, data = eng.molfile_pack(r, scale=sc, cap=cap)
            assert data == ref["out"] and files.tobytes() == ref["files"].tobytes()
    preds = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, molfile=True, molfile_scale=scale)
    for p, f in zip(preds, ref["files"]):              # a molecule without a molfile (more than 999 bonds, say): None
        want = ref["out"][f["text0"]:f["text0"] + f["len"]].decode() if f["len"] else None
        assert p["molfile"] == want and isinstance(want, (str, type(None)))
    written = [p["molfile"] for p in preds if p["molfile"] is not None]
    assert written and all(w.endswith("M  END\n") for w in written)
    assert "molfile" not in predict_pipeline(eng, imgs[:2], ref_batch_size=2, packed=True)[0]

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_molfile=True)
    try:
        m.group_images = 4                                     # two groups: the page scales travel with their group
        got = m.predict_images(pages, batch_size=4)
        want = []
        for g in (pages[:4], pages[4:]):
            want += predict_pipeline(m.engine, m._transform(g), m.tokenizer, ref_batch_size=4, packed=True, molfile=True,
                                     molfile_scale=[page_scale(p) for p in g])
        assert [o["predicted_molfile"] for o in got] == [p["molfile"] for p in want] and all(o["predicted_smiles"] is None for o in got)
        written = [o["predicted_molfile"] for o in got if o["predicted_molfile"] is not None]
        assert written and all(w.startswith("\n  MolNexTR          2D\n\n") for w in written)
        assert len({page_scale(p) for p in pages}) > 1
        m.graph_molfile = False                                # the default: no molfile without RDKit
        assert all(o["predicted_molfile"] is None for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()
