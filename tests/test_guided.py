"""CPU: label-guided decoding (coordinate prediction for a known molecule) — the tokenizer's smiles_to_sequence, the CPU
restatement of the guided loop (tests/guided_ref.py) against fixtures made by the reference's own classes
(tests/golden/guided.*, tools/gen_golden.py guided), the new C-ABI symbols, and the Python layer's refusals."""
import json
import os
import re

import numpy as np
import pytest
import torch

from molnextr_amd import engine
from molnextr_amd import weights as W
from molnextr_amd.tokenizer import MASK_ID, get_tokenizer

from guided_ref import guided_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGP_TOL = 1e-3


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "guided.npz")))
    with open(os.path.join(golden_dir, "guided.json")) as f:
        g.update(json.load(f))
    return g


@pytest.fixture(scope="module")
def tok():
    return get_tokenizer()["chartok_coords"]


@pytest.mark.parametrize("case", ["ar", "px"])
def test_smiles_to_sequence_equals_the_reference(case, gold, tok):
    lab = gold[f"{case}_labels"]
    for b, s in enumerate(gold[case]["smiles"]):
        labels, indices = tok.smiles_to_sequence(s, mask_ratio=1)
        assert labels == lab[b, :len(labels)].tolist() and not lab[b, len(labels):].any(), (b, s)
        assert indices == gold[case]["indices"][b], (b, s)
    assert (3 in lab or case != "ar") and MASK_ID in lab   # '<unk>' (a character outside the vocabulary) and '<mask>' are covered


def test_smiles_to_sequence_options(tok):
    plain, _ = tok.smiles_to_sequence("CCl")
    assert plain == [1, tok.stoi["C"], tok.stoi["C"], tok.stoi["l"], 2]
    lab, idx = tok.smiles_to_sequence("C=O", coords=[[0.0, 1.0], [1.0, 0.0]])
    assert lab == [1, tok.stoi["C"], tok.x_to_id(0.0), tok.y_to_id(1.0), tok.stoi["="], tok.stoi["O"], tok.x_to_id(1.0),
                   tok.y_to_id(0.0), 2] and idx == [3, 7]
    assert tok.smiles_to_sequence("C=O", atom_only=True)[0] == [1, tok.stoi["C"], tok.stoi["O"], 2]
    with pytest.raises(ValueError):
        tok.smiles_to_sequence("CC", mask_ratio=0.5)


def test_cpu_restatement_equals_the_reference(gold, synth_ckpt):
    """ids and lengths exact at every step, own-pick log-probs below 1e-3; the fixture's smallest margin is >= 2e-3"""
    margin = gold["ar_margin"]
    assert margin[np.isfinite(margin)].min() >= 2e-3
    feats = W.hash_normal("guided_features", (12, 144, 1024), 0.5)
    r = guided_decode(feats, synth_ckpt["decoder"], gold["ar_labels"])
    err = 0.0
    for b in range(12):
        n = int(gold["ar_lens"][b])
        assert r.tokens[b] == gold["ar_ids"][b, :n].tolist(), b
        err = max(err, float(np.abs(np.array(r.token_logp[b]) - gold["ar_token_logp"][b, :n]).max()))
    print("guided cpu restatement: max |token_logp - reference|", err)
    assert err < LOGP_TOL


def test_merged_sequences_detokenise_to_the_fixture(gold, tok):
    """sequence_to_smiles of each merged sequence of the pixel case returns the symbols and indices the reference's own
    Decoder.decode derived from it (an atom whose masked positions the model did not fill with an x and a y is dropped
    by both, so these need not be smiles_to_sequence's indices)"""
    for b, p in enumerate(gold["px"]["preds"]):
        n = int(gold["px_lens"][b])
        d = tok.sequence_to_smiles(gold["px_ids"][b, :n].tolist())
        assert d["symbols"] == p["symbols"] and d["indices"] == p["indices"] and d["smiles"] == p["smiles"], b


def test_header_symbols_and_library_exports():
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    if not os.path.exists(engine.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = engine.load_library()
    for name in ("mnx_decode_guided", "mnx_predict_guided"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in engine.SYMBOLS and hasattr(lib, name), name
    assert lib.mnx_abi_version() == 7
    assert lib.mnx_decode_guided(None, None, 1, None, 8, None, 2, None, None, None, None, None, None) == -1   # null handle


def test_predict_coords_rejects_mismatched_lists():
    from molnextr_amd.model import molnextr
    m = molnextr.__new__(molnextr)            # no engine needed: the lists are checked first
    with pytest.raises(ValueError, match="same length"):
        m.predict_coords([np.zeros((8, 8, 3), np.uint8)] * 2, ["C"])


def test_label_rows_without_eos_raise():
    lab = torch.tensor([[1, 9, 4, 4, 2], [1, 9, 4, 4, 9]])
    with pytest.raises(ValueError, match="eos"):
        engine.check_labels(lab, 2)
    assert engine.check_labels(lab, 2, free_run=True).dtype == torch.int32
    with pytest.raises(ValueError):
        engine.check_labels(lab[:, :1], 2, free_run=True)


def test_free_run_exempts_single_rows():
    lab = torch.tensor([[1, 9, 4, 4, 2], [1, 9, 4, 4, 9]])
    assert engine.check_labels(lab, 2, free_run=[False, True]).shape == (2, 5)
    with pytest.raises(ValueError, match="rows \\[1\\]"):
        engine.check_labels(lab, 2, free_run=[True, False])
    with pytest.raises(ValueError, match="one per label row"):
        engine.check_labels(lab, 2, free_run=[True, False, True])


def test_coords_labels_cut_and_pad(tok):
    """predict_coords' labels: mask_ratio=1, cut to max_len ids (dataset.py:473), padded to a common L; only a row the cut
    shortened is marked (it has lost its '<eos>') — every other row still meets the engine's refusal."""
    from molnextr_amd.tokenizer import coords_labels
    lab, cut = coords_labels(tok, ["CCO", "C" * 30, ""], 16)
    assert lab.shape == (3, 16) and lab.dtype == np.int32 and cut.tolist() == [False, True, False]
    assert lab[0, :11].tolist() == tok.smiles_to_sequence("CCO", mask_ratio=1)[0] and not lab[0, 11:].any()
    assert lab[1].tolist() == tok.smiles_to_sequence("C" * 30, mask_ratio=1)[0][:16] and 2 not in lab[1]
    assert lab[2].tolist() == [1, 2] + [0] * 14
    engine.check_labels(lab, 3, free_run=cut)
    with pytest.raises(ValueError, match="eos"):
        engine.check_labels(lab, 3)
    lab, cut = coords_labels(tok, ["", ""], 480)
    assert lab.tolist() == [[1, 2], [1, 2]] and not cut.any()
