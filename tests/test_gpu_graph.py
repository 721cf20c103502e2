"""GPU (-m gpu): mnx_graph_pack — the packed atom / bond / text tables of the molecules — against the numpy oracle of
tests/graph_ref.py (integers and bytes equal, scores bit for bit), its capacity and argument handling, and the packed mode of
predict_pipeline / molnextr against the dense one."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ref
from molnextr_amd import weights as W
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE, Engine, vocab_text
from packed_tables import Inputs, _p, call_tables, dev, eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    from molnextr_amd.tokenizer import get_tokenizer
    return get_tokenizer()["chartok_coords"]


class Case:
    """Dense inputs of one mnx_graph_pack call on the host and on the device, and the oracle's records for them."""

    def __init__(self, tok, dev, toks, lens, kmax, rng, scores=True):
        self.toks, self.lens, self.kmax, self.n = toks, lens, kmax, len(lens)
        self.atom_idx, self.n_atoms = graph_ref.dense_atoms(tok, toks, lens, kmax)
        self.edges = graph_ref.random_edges(rng, self.n_atoms, kmax)
        self.sc = (rng.random((self.n, kmax)), rng.random((self.n, kmax, kmax)), rng.random(self.n)) if scores else (None,) * 3
        self.ref = graph_ref.pack(tok, toks, lens, self.edges, kmax, *self.sc)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
        self.d = [up(a) for a in (toks, lens, self.atom_idx, self.n_atoms, self.edges) + self.sc]

    def rows(self, n):
        """the first n rows as a case of their own, without scores (shares the device arrays)"""
        c = object.__new__(Case)
        c.n, c.kmax, c.sc = n, self.kmax, (None,) * 3
        c.d = self.d[:5] + [None] * 3
        return c


def call(eng, case, caps, **over):
    """One mnx_graph_pack call on the dense inputs of `case`: the harness's named result; over: arguments by name"""
    tk, ln, ai, na, ed, s0, s1, s2 = case.d
    head = {"tokens": _p(tk), "lengths": _p(ln), "n": case.n, "T": tk.shape[1], "atom_idx": _p(ai), "n_atoms": _p(na), "edges": _p(ed),
            "kmax": case.kmax, "atom_scores": _p(s0), "edge_scores": _p(s1), "overall": _p(s2)}
    return call_tables("mnx_graph_pack", eng, Inputs(tk.device, case.n, head), caps, **over)


def run_pack(eng, dev, case, caps):
    """One mnx_graph_pack call into arenas of exactly `caps` records / bytes with guard bytes behind each; returns
    (rc, {'mols', 'atoms', 'bonds', 'text', 'totals'} as read back, the arenas as raw bytes)."""
    got = call(eng, case, caps)
    out = {"mols": got.mols, "totals": got.totals, "atoms": got.atoms.view(ATOM_DTYPE), "bonds": got.bonds.view(BOND_DTYPE),
           "text": got.text.tobytes()}
    return got.rc, out, [got.atoms, got.bonds, got.text, got.mols.view(np.uint8)]


def assert_records_equal(got, ref, n_atoms=None, n_bonds=None, n_text=None):
    """every field of every record equal, scores as bit patterns; the n_* cut both sides to what a small arena holds"""
    for name in MOL_DTYPE.names:
        a, b = got["mols"][name], ref["mols"][name]
        assert np.array_equal(a.view(np.uint64) if name == "overall_score" else a, b.view(np.uint64) if name == "overall_score" else b), name
    for key, dt, cut in (("atoms", ATOM_DTYPE, n_atoms), ("bonds", BOND_DTYPE, n_bonds)):
        a, b = got[key][:cut], ref[key][:cut]
        assert len(a) == len(b), key
        for name in dt.names:
            x, y = (a[name].view(np.uint64), b[name].view(np.uint64)) if name == "score" else (a[name], b[name])
            bad = np.nonzero(x != y)[0]
            assert bad.size == 0, (key, name, bad[:5], x[bad[:5]], y[bad[:5]])
    assert got["text"][:n_text] == ref["text"][:n_text]


def exact_caps(ref):
    return tuple(int(v) for v in ref["totals"][:3])


def _hand_rows(tok):
    s = tok.stoi
    xy = lambda a, b: [101 + a, 165 + b]                                         # noqa: E731
    C_, N, O = s["C"], s["N"], s["O"]
    return [
        [2],                                                                     # '<eos>' at position 0
        [C_] + xy(1, 2) + [0, N] + xy(3, 4) + [2],                               # '<pad>' mid-row ends the molecule
        [C_] + xy(5, 6) + [s["="]] * 509,                                        # 512 ids, no '<eos>'
        [C_, s["l"]] + xy(0, 63) + [s["B"], s["r"]] + xy(63, 0) + [C_] + xy(7, 7) + [2],
        [3] + xy(1, 1) + [s["["], 3, s["H"], s["]"]] + xy(2, 2) + [2],           # '<unk>' alone and inside brackets
        [s["["], N, s["H"]] + xy(9, 9) + [C_] + xy(8, 8) + [2],                  # unclosed '[' runs into a coordinate
        [s["ŕ"]] + xy(4, 4) + [C_] + xy(5, 5) + [s["ŕ"], O] + xy(6, 6) + [2],    # the two-byte name
        [C_] + xy(1, 1) + [1, 4, O] + xy(2, 2) + [2],                            # '<sos>' and '<mask>' inside a row
        [C_] + xy(1, 1) + [O, 2],                                                # last atom without x y: SMILES only
        [C_] + xy(1, 1) + [O] + xy(2, 2),                                        # last atom with x y but no next position
        sum(([a] + xy(i, i) for i, a in enumerate([C_, N, O, C_, N, O])), []) + [2],   # 6 atoms > kmax = 4
        [C_, N, s["="], O, 2],                                                   # atoms without coordinates: 0 atoms
    ]


@pytest.fixture(scope="module")
def hand(tok, dev):
    rows = _hand_rows(tok)
    T, kmax = 512, 4
    toks = np.zeros((len(rows), T), np.int32)
    lens = np.array([len(r) for r in rows], np.int32)
    for b, r in enumerate(rows):
        toks[b, :len(r)] = r
    return Case(tok, dev, toks, lens, kmax, np.random.default_rng(1))


@pytest.fixture(scope="module")
def fuzz(tok, dev):
    """about 2000 rows from the whole vocabulary under the grammar mask, T = 200, kmax = 24 (long rows exceed it), with scores"""
    rng = np.random.default_rng(7)
    toks, lens = graph_ref.fuzz_rows(tok, rng, 2000, 200)
    return Case(tok, dev, toks, lens, 24, rng)


def test_hand_written_rows(eng, dev, hand):
    ref = hand.ref
    m = ref["mols"]
    assert m["n_atoms"].tolist() == [0, 1, 1, 3, 2, 2, 3, 2, 1, 1, 4, 0] and m["flags"].tolist() == [0] * 10 + [1, 0]
    assert m["smiles_len"][2] == 510 and m["smiles_len"][6] == 6 and ref["text"].decode().startswith("CC" + "=" * 509 + "ClBrC<unk>[<unk>H]")
    rc, got, _ = run_pack(eng, dev, hand, exact_caps(ref))
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert got["totals"].tolist() == ref["totals"].tolist()
    assert_records_equal(got, ref)
    a = got["atoms"][int(m["atom0"][5])]                                         # '[NH': the symbol is a substring of the text
    t0 = int(m["text0"][5])
    assert got["text"][t0 + a["sym0"]:t0 + a["sym0"] + a["sym_len"]] == b"[NH" and (a["x_bin"], a["y_bin"], a["index"]) == (9, 9, 5)


def test_fuzzed_rows_in_one_call_and_twice_the_same_bytes(eng, dev, fuzz):
    ref = fuzz.ref
    assert ref["mols"]["flags"].sum() > 20 and (ref["mols"]["n_atoms"] == 0).sum() > 20 and ref["totals"][1] > 20000
    rc, got, raw = run_pack(eng, dev, fuzz, exact_caps(ref))
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert got["totals"].tolist() == ref["totals"].tolist()
    assert_records_equal(got, ref)
    rc2, _, raw2 = run_pack(eng, dev, fuzz, exact_caps(ref))
    assert rc2 == 0 and all(np.array_equal(x, y) for x, y in zip(raw, raw2)), "two runs differ"
    pad = raw[0][:len(got["atoms"]) * 24].reshape(-1, 24)[:, 12:16]
    assert not pad.any() and not raw[1][:len(got["bonds"]) * 16].reshape(-1, 16)[:, 6:8].any(), "padding bytes are not zero"


@pytest.mark.parametrize("n", [1, 1025])
def test_image_counts_without_scores(eng, dev, tok, fuzz, n):
    """n = 1025 takes the scan over the images past one workgroup's width; no score pointers: zeros in the records"""
    case = fuzz.rows(n)
    ref = graph_ref.pack(tok, fuzz.toks[:n], fuzz.lens[:n], fuzz.edges[:n], fuzz.kmax)
    rc, got, _ = run_pack(eng, dev, case, exact_caps(ref))
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert got["totals"].tolist() == ref["totals"].tolist()
    assert_records_equal(got, ref)
    assert not got["atoms"]["score"].any() and not got["bonds"]["score"].any() and not got["mols"]["overall_score"].any()


def test_dense_edges_cases(eng, dev, tok):
    """fully connected, empty, a pair whose two directions disagree, and a set diagonal that must not appear"""
    s = tok.stoi
    row = sum(([s["C"], 101 + i, 165 + i] for i in range(6)), []) + [2]
    toks = np.tile(np.array(row, np.int32), (3, 1))
    case = Case(tok, dev, toks, np.full(3, len(row), np.int32), 8, np.random.default_rng(2))
    e = case.edges
    e[0, :6, :6] = 1
    e[1, :6, :6] = 0
    e[2, :6, :6] = 0
    e[2, 1, 4], e[2, 4, 1] = 5, 5                              # the bond head's symmetrisation would give 6 here
    e[2, 2, 2] = e[2, 5, 5] = 3
    e[2, 3, 0] = 2                                             # lower triangle only: no record
    case.ref = graph_ref.pack(tok, toks, case.lens, e, 8, *case.sc)
    case.d[4] = torch.from_numpy(e).to(dev)
    assert case.ref["mols"]["n_bonds"].tolist() == [15, 0, 1]
    rc, got, _ = run_pack(eng, dev, case, exact_caps(case.ref))
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert_records_equal(got, case.ref)
    b = got["bonds"][15]
    assert (b["i"], b["j"], b["type"], b["rev"]) == (1, 4, 5, 5) and b["score"] == case.sc[1][2, 1, 4]


def test_capacities_one_short_then_exact(eng, dev, tok, fuzz):
    n = 64
    sc = tuple(a[:n] for a in fuzz.sc)
    case = fuzz.rows(n)
    case.d = fuzz.d[:5] + [t[:n].contiguous() for t in fuzz.d[5:]]
    ref = graph_ref.pack(tok, fuzz.toks[:n], fuzz.lens[:n], fuzz.edges[:n], fuzz.kmax, *sc)
    need = exact_caps(ref)
    assert min(need) > 1
    rc, got, _ = run_pack(eng, dev, case, tuple(c - 1 for c in need))         # run_pack checks the canaries
    assert rc == 0, eng.lib.mnx_last_error(eng.h)
    assert got["totals"].tolist() == list(need) + [1]
    assert_records_equal(got, ref, need[0] - 1, need[1] - 1, need[2] - 1)    # mols complete, the tables up to the capacity
    for short in range(3):                                                   # each capacity on its own reports too
        caps = tuple(c - (i == short) for i, c in enumerate(need))
        assert run_pack(eng, dev, case, caps)[1]["totals"].tolist() == list(need) + [1]
    rc, got, _ = run_pack(eng, dev, case, (0, 0, 0))                          # sizing call: nothing fits, the needed sizes come back
    assert rc == 0 and got["totals"].tolist() == list(need) + [1]
    rc, got, _ = run_pack(eng, dev, case, need)
    assert rc == 0 and got["totals"].tolist() == list(need) + [0]
    assert_records_equal(got, ref)


def test_engine_graph_pack_grows_once(eng, fuzz):
    """Engine.graph_pack from a first capacity that is too small: one repeat sized by totals, the oracle's records"""
    keys = ("tokens", "lengths", "atom_idx", "n_atoms", "edges", "atom_scores", "edge_scores", "overall_score")
    out = dict(zip(keys, fuzz.d))
    for caps in ((1, 1, 1), None):
        rec = eng.graph_pack(out, caps=caps)
        assert rec["totals"].tolist() == fuzz.ref["totals"].tolist()
        assert_records_equal(rec, fuzz.ref)


def _call(eng, case, **over):
    got = call(eng, case, (64, 64, 64), **over)
    return got.rc, got.error


def test_argument_checks(eng, dev, synth_ckpt, tok, hand):
    assert _call(eng, hand)[0] == 0
    for name in ("tokens", "lengths", "atom_idx", "n_atoms", "edges", "mols", "atoms", "bonds", "text", "totals"):
        rc, msg = _call(eng, hand, **{name: None})
        assert rc == -1 and msg == "mnx_graph_pack: null pointer", (name, rc, msg)
    for over in ({"n": 0}, {"n": 65537}, {"T": 0}, {"T": 513}, {"kmax": 0}, {"kmax": eng.max_atoms + 1}):
        rc, msg = _call(eng, hand, **over)
        assert rc == -1 and msg.startswith("mnx_graph_pack: 1 <= n <= 65536, 1 <= T <= 512"), (over, rc, msg)
    for name in ("atom_scores", "edge_scores", "overall"):
        rc, msg = _call(eng, hand, **{name: None})
        assert rc == -1 and "all three or none" in msg, (name, rc, msg)
    rc, msg = _call(eng, hand, atoms=C.c_void_p(hand.d[0].data_ptr() + 4))
    assert rc == -1 and "8-byte aligned" in msg, (rc, msg)

    class Bare(Engine):                                      # a fresh handle that was told nothing about the vocabulary
        def _set_token_classes(self):
            pass

        def _set_vocab_text(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        rc, msg = _call(eng, hand, h=bare.h)
        assert rc == -1 and msg == "mnx_graph_pack: call mnx_set_token_classes first", (rc, msg)
        ids = [tok.stoi[c] for c in "[]ClBr"]
        assert bare.lib.mnx_set_token_classes(bare.h, Engine.token_class_flags(tok), tok.offset, *ids) == 0
        rc, msg = _call(eng, hand, h=bare.h)
        assert rc == -1 and msg == "mnx_graph_pack: call mnx_set_vocab_text first", (rc, msg)
        off = np.arange(tok.offset + 1, dtype=np.uint32) + 8          # every name one byte, but the first: nine
        off[0] = 0
        assert bare.lib.mnx_set_vocab_text(bare.h, b"x" * int(off[-1]), off.ctypes.data, tok.offset) == -1
        assert "name of id 0 is longer than 8 bytes" in bare.lib.mnx_last_error(bare.h).decode()
        assert bare.lib.mnx_set_vocab_text(bare.h, None, off.ctypes.data, 1) == -1
        assert bare.lib.mnx_set_vocab_text(bare.h, b"x", off.ctypes.data, 257) == -1
        text, offsets, n = vocab_text(tok)                   # a table one name short would spell shortened SMILES: refused
        assert bare.lib.mnx_set_vocab_text(bare.h, text, offsets.ctypes.data, n - 1) == -1
        assert f"n = {n - 1} names, but the vocabulary has cfg.sym_offset = {n}" in bare.lib.mnx_last_error(bare.h).decode()
        rc, msg = _call(eng, hand, h=bare.h)
        assert rc == -1 and msg == "mnx_graph_pack: call mnx_set_vocab_text first", (rc, msg)
        Engine._set_vocab_text(bare)
        assert _call(eng, hand, h=bare.h)[0] == 0
    finally:
        bare.close()


@pytest.mark.parametrize("mode", ["plain", "confidence", "guided"])
def test_pipeline_packed_equals_dense(eng, dev, tok, mode):
    """40 images in reference batches of 16: predict_pipeline(packed=True) field by field against packed=False"""
    from molnextr_amd.model import predict_pipeline
    from molnextr_amd.tokenizer import coords_labels
    imgs = W.synthetic_images(40, first_index=500).to(dev)
    kw = {"ref_batch_size": 16, "compute_confidence": mode != "plain"}
    if mode == "guided":
        smiles = ["CCO", "C1CC1", "", "[Na+].[Cl-]", "c1ccccc1O", "BrCCCl", "C", "CC(=O)O"]
        kw["labels"] = coords_labels(tok, [smiles[i % len(smiles)] for i in range(40)], eng.max_len)[0]
    dense = predict_pipeline(eng, imgs, **kw)
    packed = predict_pipeline(eng, imgs, packed=True, **kw)
    graph_ref.assert_packed_equals_dense(packed, dense, kw["compute_confidence"])
    assert sum(len(p["bonds"]) for p in packed) > 0 and sum(len(p["chartok_coords"]["symbols"]) for p in packed) > 40


def test_facade_packed_results_equal_the_default(dev, synth_ckpt, monkeypatch):
    from molnextr_amd.model import molnextr
    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(10)]
    a, b = molnextr("synthetic", dev, max_batch=4), molnextr("synthetic", dev, max_batch=4, packed_results=True)
    try:
        assert a.packed_results is False and b.packed_results is True
        for m in (a, b):
            m.group_images = 4
        want = a.predict_images(pages, return_atoms_bonds=True, return_confidence=True, batch_size=4)
        got = b.predict_images(pages, return_atoms_bonds=True, return_confidence=True, batch_size=4)
        assert got == want and sum(len(o["bond_sets"]) for o in got) > 0
        assert b.predict_images(pages[:5], batch_size=4) == a.predict_images(pages[:5], batch_size=4)
        smiles = ["CCO", "c1ccccc1O", "", "BrCCCl"]
        assert b.predict_coords(pages[:4], smiles, return_confidence=True, batch_size=4) == \
            a.predict_coords(pages[:4], smiles, return_confidence=True, batch_size=4)
    finally:
        a.engine.close()
        b.engine.close()
