"""CPU: the host side of the packed molecule tables — model.unpack_graphs on the oracle's records (tests/graph_ref.py) against
the dicts the dense code of predict_pipeline / _assemble builds, the record layouts against include/molnextr_hip.h, and the
refusal of packed results with beam search."""
import ctypes
import os
import re

import numpy as np
import pytest

import graph_ref
from molnextr_amd import engine
from molnextr_amd.model import molnextr, predict_pipeline, unpack_graphs
from molnextr_amd.tokenizer import get_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tok():
    return get_tokenizer()["chartok_coords"]


@pytest.fixture(scope="module")
def dense(tok):
    """300 fuzzed rows with random bonds and scores: the dense arrays a predict call would return, on the host."""
    rng = np.random.default_rng(3)
    kmax = 64
    toks, lens = graph_ref.fuzz_rows(tok, rng, 300, 160)
    s = tok.stoi
    hand = [[s["C"], s["l"], 101, 165, s["ŕ"], s["["], 3, s["]"], 110, 170, s["="], s["O"], 120, 180, 2],
            [2], [s["C"], s["N"], 2], [1, 4, s["C"], 101, 165, 0, s["C"], 101, 165, 2]]
    for b, r in enumerate(hand):
        toks[b] = 0
        toks[b, :len(r)] = r
        lens[b] = len(r)
    _, n_atoms = graph_ref.dense_atoms(tok, toks, lens, kmax)
    assert n_atoms.max() < kmax and (n_atoms == 0).any() and n_atoms.max() > 10
    edges = graph_ref.random_edges(rng, n_atoms, kmax)
    return {"toks": toks, "lens": lens, "n_atoms": n_atoms, "edges": edges, "kmax": kmax,
            "atom_scores": rng.random((300, kmax)), "edge_scores": rng.random((300, kmax, kmax)), "overall": rng.random(300)}


@pytest.mark.parametrize("with_scores", [False, True])
def test_unpack_of_reference_records_equals_dense_dicts(tok, dense, with_scores):
    d = dense
    sc = (d["atom_scores"], d["edge_scores"], d["overall"]) if with_scores else (None, None, None)
    rec = graph_ref.pack(tok, d["toks"], d["lens"], d["edges"], d["kmax"], *sc)
    got = unpack_graphs(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tok.maxx, with_scores)
    want = graph_ref.dense_preds(tok, d["toks"], d["lens"], d["n_atoms"], d["edges"], *sc)
    graph_ref.assert_packed_equals_dense(got, want, with_scores)
    assert got[0]["chartok_coords"]["symbols"] == ["Cl", "[<unk>]", "O"] and got[0]["chartok_coords"]["smiles"] == "Clŕ[<unk>]=O"
    assert rec["totals"][0] == d["n_atoms"].sum() and rec["totals"][2] == len(rec["text"])


@pytest.mark.parametrize("with_scores", [False, True])
def test_assemble_from_records_equals_assemble_from_dense(tok, dense, with_scores):
    """_assemble builds the same 'atom_sets' / 'bond_sets' from bond records as from the dense matrices (no engine needed)."""
    d = dense
    sc = (d["atom_scores"], d["edge_scores"], d["overall"]) if with_scores else (None, None, None)
    rec = graph_ref.pack(tok, d["toks"], d["lens"], d["edges"], d["kmax"], *sc)
    packed = unpack_graphs(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tok.maxx, with_scores)
    want = graph_ref.dense_preds(tok, d["toks"], d["lens"], d["n_atoms"], d["edges"], *sc)
    m = object.__new__(molnextr)
    a = m._assemble(packed, [None] * len(packed), True, with_scores)
    b = m._assemble(want, [None] * len(want), True, with_scores)
    assert a == b
    assert sum(len(o["bond_sets"]) for o in a) == rec["totals"][1] > 0


def test_record_layouts_match_the_header():
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    ctype = {"uint32_t": ("<u4", 4), "uint16_t": ("<u2", 2), "uint8_t": ("u1", 1), "double": ("<f8", 8)}
    for name, size, cs, nd in (("mnx_mol", 40, engine.MnxMol, engine.MOL_DTYPE), ("mnx_atom", 24, engine.MnxAtom, engine.ATOM_DTYPE),
                               ("mnx_bond", 16, engine.MnxBond, engine.BOND_DTYPE)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields, off = [], 0                                  # natural C layout, worked out from the declarations
        for decl in body.split(";"):
            if not decl.strip():
                continue
            ty, names = decl.split(None, 1)
            fmt, sz = ctype[ty]
            for nm in names.split(","):
                off = -(-off // sz) * sz
                fields.append((nm.strip(), fmt, off))
                off += sz
        assert -(-off // 8) * 8 == size == ctypes.sizeof(cs) == nd.itemsize, name
        assert [(n, getattr(cs, n).offset) for n, _, _ in fields] == [(n, o) for n, _, o in fields], name
        assert [f[0] for f in cs._fields_] == list(nd.names) == [n for n, _, _ in fields], name
        assert [(nd.fields[n][0].str.lstrip("|"), nd.fields[n][1]) for n, _, _ in fields] == [(f.lstrip("|"), o) for _, f, o in fields]


def test_vocab_text_table(tok):
    text, offsets, n = engine.vocab_text(tok)
    assert n == tok.offset == 101 and offsets[0] == 0 and offsets[-1] == len(text)
    names = [text[offsets[i]:offsets[i + 1]].decode() for i in range(n)]
    assert names == [tok.itos[i] for i in range(n)] and names[:5] == ["<pad>", "<sos>", "<eos>", "<unk>", "<mask>"]
    assert sorted(i for i in range(n) if offsets[i + 1] - offsets[i] > 1) == [0, 1, 2, 3, 4, tok.stoi["ŕ"]]


def test_packed_with_beam_is_refused():
    with pytest.raises(NotImplementedError, match="packed"):
        predict_pipeline(None, None, beam_size=2, packed=True)
