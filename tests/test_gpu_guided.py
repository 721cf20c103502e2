"""GPU: label-guided decoding through the C ABI (mnx_decode_guided / mnx_predict_guided) against the reference's fixtures
(tests/golden/guided.*), the CPU restatement (tests/guided_ref.py) and exactness properties that need no reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from molnextr_amd import weights as W

from guided_ref import guided_decode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tokens", "lengths", "n_atoms", "atom_idx", "edges")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "guided.npz")))
    with open(os.path.join(golden_dir, "guided.json")) as f:
        g.update(json.load(f))
    return g


@pytest.fixture(scope="module")
def eng(synth_ckpt):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=64, dec_slots=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    return W.synthetic_images(64)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if v is not None}


def _same(a, b, keys, what):
    for k in keys:
        x, y = a[k], b[k]
        if k in ("tokens", "token_logp", "hidden"):        # entries beyond a row's length are undefined in decode_* outputs
            for r, n in enumerate(a["lengths"]):
                assert np.array_equal(x[r, :n], y[r, :n]), (what, k, r)
        else:
            assert np.array_equal(x, y), (what, k)


def _labels_for(n, tok, smiles):
    seqs = [tok.smiles_to_sequence(smiles[i % len(smiles)], mask_ratio=1)[0] for i in range(n)]
    lab = np.zeros((n, max(len(s) for s in seqs)), np.int32)
    for r, s in enumerate(seqs):
        lab[r, :len(s)] = s
    return lab


def _eq_pred(a, b, what=""):
    """predict outputs equal bit for bit (bond classes and their scores are defined inside n_atoms x n_atoms only)"""
    for k in a:
        if k in ("edges", "edge_scores"):
            for r, n in enumerate(a["n_atoms"]):
                assert np.array_equal(a[k][r, :n, :n], b[k][r, :n, :n]), (what, k, r)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def _decode_vs_reference(gold, eng, dev, what="default"):
    """mnx_decode_guided on the fixture's features and labels: ids and lengths exact at every step; token_logp < 1e-3,
    hidden_head < 1e-3, hidden_sum < 2e-2 (the tolerances test_gpu_parity.py applies to decoder_greedy)."""
    feats = W.hash_normal("guided_features", (12, 144, 1024), 0.5).to(dev)
    o = _np(eng.decode_guided(feats, gold["ar_labels"], trace_logits=True))
    lens = gold["ar_lens"]
    assert o["lengths"].tolist() == lens.tolist()
    lp_err = hh_err = hs_err = lg_err = 0.0
    for b, n in enumerate(lens):
        assert o["tokens"][b, :n].tolist() == gold["ar_ids"][b, :n].tolist(), b
        lp_err = max(lp_err, float(np.abs(o["token_logp"][b, :n] - gold["ar_token_logp"][b, :n]).max()))
        m = min(8, n)
        hh_err = max(hh_err, float(np.abs(o["hidden"][b, :m] - gold["ar_hidden_head"][b, :m]).max()))
        hs_err = max(hs_err, float(np.abs(o["hidden"][b, :n].astype(np.float64).sum(0) - gold["ar_hidden_sum"][b]).max()))
    for s in range(4):
        alive = [b for b in range(12) if lens[b] > s]
        lg_err = max(lg_err, float(np.abs(o["logits"][s][alive] - gold[f"ar_logits_step{s}"]).max()))
    print("guided decode vs reference", what, json.dumps({"token_logp": lp_err, "hidden_head": hh_err, "hidden_sum": hs_err,
                                                    "logits_steps0-3": lg_err}))
    assert lp_err < 1e-3 and hh_err < 1e-3 and hs_err < 2e-2 and lg_err < 1e-3


def test_decode_guided_vs_reference(gold, eng, dev):
    _decode_vs_reference(gold, eng, dev)


def _predict_vs_reference(gold, eng, images, dev, what="default"):
    """One reference batch of 40 rows from pixels (the fixture's fp32 images): tokens, atoms and bonds are the reference's,
    confidences within test_gpu_confidence.py's tolerances."""
    B = 40
    lab = gold["px_labels"]
    x = images[:B].to(dev)
    o = _np(eng.predict(x, ref_batch=B, confidence=True, labels=lab))
    assert o["lengths"].tolist() == gold["px_lens"].tolist()
    preds = gold["px"]["preds"]
    offs = np.cumsum([0] + [len(p["symbols"]) ** 2 for p in preds])
    toffs = np.cumsum([0] + [len(p["symbols"]) * (len(p["symbols"]) + 1) // 2 for p in preds])
    lp_err = 0.0
    for r, p in enumerate(preds):
        n, k = int(gold["px_lens"][r]), len(p["symbols"])
        assert o["tokens"][r, :n].tolist() == gold["px_ids"][r, :n].tolist(), r
        assert o["n_atoms"][r] == k and o["atom_idx"][r, :k].tolist() == p["indices"], r
        assert np.array_equal(o["edges"][r, :k, :k].ravel(), gold["px_edges"][offs[r]:offs[r + 1]]), r
        lp_err = max(lp_err, float(np.abs(o["token_logp"][r, :n] - gold["px_token_logp"][r, :n]).max()))
        np.testing.assert_allclose(o["atom_scores"][r, :k], p["atom_scores"], rtol=2e-4)
        assert abs(o["overall_score"][r] - p["overall_score"]) <= 1e-6 + 1e-3 * abs(p["overall_score"])
        np.testing.assert_allclose(o["edge_scores"][r, :k, :k][np.triu_indices(k)], gold["px_edge_scores"][toffs[r]:toffs[r + 1]],
                                   atol=1e-5)
    print("guided predict vs reference", what, "token_logp", lp_err)
    assert lp_err < 1e-3


def test_predict_guided_from_pixels_vs_reference(gold, eng, images, dev):
    """The fixture's 40-row batch on its fp32 images; then both image formats on the same bytes (pages -> gray bytes and ->
    fp32 by the engine's own transform) along the fixture's labels: bit for bit equal."""
    _predict_vs_reference(gold, eng, images, dev)
    pages = [W.synthetic_page(i % len(W.PAGE_CASES)) for i in range(40)]
    lab = gold["px_labels"]
    a = _np(eng.predict(eng.preprocess_batch(pages, out="fp32"), ref_batch=40, confidence=True, labels=lab))
    b = _np(eng.predict(eng.preprocess_batch(pages, out="gray8"), ref_batch=40, confidence=True, labels=lab))
    _eq_pred(a, b, "fp32 vs gray8")


INK_PAGES = (0, 1, 4, 5, 6, 7, 11, 14)      # the ink-bearing pages tests/test_gpu_pages.py decodes against the oracle
PAGE_SMILES = ["CCO", "[Na+].[Cl-]", "c1ccccc1", "", "BrCCCl", "C{Si}C", "CC(=O)O", "C1CC1"]


def test_predict_guided_gray8_and_fp32_pages_vs_the_cpu_restatement(eng, synth_ckpt, dev):
    """Gray-byte input has no reference fixture of its own (the fixture's images are not gray bytes), so both formats are
    pinned on pages against the CPU chain: host transform_image -> oracle encoder -> guided restatement -> sequence_to_smiles
    -> oracle bond head. Tokens, atoms and bonds exact; own-pick log-probs within the 1e-3 the fixture comparison applies."""
    from molnextr_amd.preprocess import transform_image
    from molnextr_amd.tokenizer import get_tokenizer
    from oracle.edges import predict_edges
    from oracle.swin import encoder_forward
    tok = get_tokenizer()["chartok_coords"]
    pages = [W.synthetic_page(c) for c in INK_PAGES]
    lab = _labels_for(len(pages), tok, PAGE_SMILES)
    img = torch.from_numpy(np.stack([transform_image(p) for p in pages]))
    ref = guided_decode(encoder_forward(img, synth_ckpt["encoder"]), synth_ckpt["decoder"], lab)
    for fmt in ("gray8", "fp32"):
        o = _np(eng.predict(eng.preprocess_batch(pages, out=fmt), ref_batch=len(pages), confidence=True, labels=lab))
        lp_err = 0.0
        for r in range(len(pages)):
            n = int(o["lengths"][r])
            assert o["tokens"][r, :n].tolist() == ref.tokens[r], (fmt, r)
            d = tok.sequence_to_smiles(ref.tokens[r])
            k = len(d["indices"])
            assert int(o["n_atoms"][r]) == k and o["atom_idx"][r, :k].tolist() == list(d["indices"]), (fmt, r)
            e_ref, _ = predict_edges(ref.hidden[r], d["indices"], synth_ckpt["decoder"])
            assert np.array_equal(o["edges"][r, :k, :k], e_ref), (fmt, r)
            lp_err = max(lp_err, float(np.abs(o["token_logp"][r, :n] - np.array(ref.token_logp[r], np.float32)).max()))
        print("guided pages vs cpu restatement", fmt, "token_logp", lp_err)
        assert lp_err < 1e-3, fmt


def _guided_is_greedy(eng, images, dev):
    """labels = <sos> + the engine's own greedy output: the guided heads reproduce mnx_decode_greedy and mnx_predict bit
    for bit (tokens, lengths, log-probs, hidden, edges) — and the unguided outputs are what they were."""
    x = images[:32].to(dev)
    feats = eng.encode(x)
    g = _np(eng.decode_greedy(feats, max_len=96))
    assert len(set(g["lengths"].tolist())) > 2            # rows finish at different steps: compaction renumbers them
    L = int(g["lengths"].max()) + 1
    lab = np.zeros((32, L), np.int32)
    lab[:, 0] = 1
    for r, n in enumerate(g["lengths"]):
        lab[r, 1:1 + n] = g["tokens"][r, :n]
    o = _np(eng.decode_guided(feats, lab, max_len=96, free_run=True))
    _same(g, o, ("lengths", "tokens", "token_logp", "hidden"), "decode")
    p = _np(eng.predict(x, ref_batch=32, max_len=96, confidence=True))
    q = _np(eng.predict(x, ref_batch=32, max_len=96, confidence=True, labels=lab, free_run=True))
    _eq_pred(p, q, "greedy vs guided")
    p2 = _np(eng.predict(x, ref_batch=32, max_len=96, confidence=True))     # unguided after guided: unchanged
    _eq_pred(p, p2, "unguided after guided")


def test_guided_along_own_greedy_output_is_greedy(eng, images, dev):
    _guided_is_greedy(eng, images, dev)


@pytest.mark.parametrize("rb", [16, 32])
def test_predict_guided_equals_per_batch_decode_guided(rb, gold, eng, images, dev):
    from molnextr_amd.tokenizer import get_tokenizer
    tok = get_tokenizer()["chartok_coords"]
    n = 64
    lab = _labels_for(n, tok, gold["ar"]["smiles"])
    x = images[:n].to(dev)
    o = _np(eng.predict(x, ref_batch=rb, confidence=True, labels=lab))
    for c in range(0, n, rb):
        feats = eng.encode(x[c:c + rb])
        d = _np(eng.decode_guided(feats, lab[c:c + rb]))
        for r in range(rb):
            m = int(d["lengths"][r])
            assert o["lengths"][c + r] == m
            assert np.array_equal(o["tokens"][c + r, :m], d["tokens"][r, :m]), (c, r)
            assert np.array_equal(o["token_logp"][c + r, :m], d["token_logp"][r, :m]), (c, r)
    # the job split across two calls at a batch boundary
    a = _np(eng.predict(x[:rb], ref_batch=rb, confidence=True, labels=lab[:rb]))
    b = _np(eng.predict(x[rb:], ref_batch=rb, confidence=True, labels=lab[rb:]))
    _eq_pred(o, {k: np.concatenate([a[k], b[k]]) for k in o}, "split across two calls")


def test_large_batch_and_free_running_equal_the_cpu_restatement(gold, eng, images, synth_ckpt, dev):
    """A reference batch above 32 rows (48: two tiles, one ragged) equals the CPU restatement's ids; so do rows whose
    labels end without '<eos>' and go on free-running beyond L (the engine's extension)."""
    from molnextr_amd.tokenizer import get_tokenizer
    tok = get_tokenizer()["chartok_coords"]
    n = 48
    lab = _labels_for(n, tok, ["CCO", "C1CC1", "", "[Na+].[Cl-]", "c1ccccc1O", "BrCCCl", "C"])
    x = images[:n].to(dev)
    feats = eng.encode(x)
    o = _np(eng.predict(x, ref_batch=n, labels=lab))
    r = guided_decode(feats.cpu(), synth_ckpt["decoder"], lab)
    for b in range(n):
        assert o["tokens"][b, :o["lengths"][b]].tolist() == r.tokens[b], b
    cut = lab[:12, :6].copy()                               # rows longer than 6 ids lose their '<eos>': free-running beyond L
    assert (cut == 2).any(axis=1).sum() < 12
    f = _np(eng.decode_guided(feats[:12].contiguous(), cut, max_len=40, free_run=True))
    r = guided_decode(feats[:12].cpu(), synth_ckpt["decoder"], cut, max_len=40)
    for b in range(12):
        assert f["tokens"][b, :f["lengths"][b]].tolist() == r.tokens[b], b


_NO_GRAPH_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from molnextr_amd import weights as W
from molnextr_amd.engine import Engine
ck = W.synthetic_checkpoint(0)
e = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=64, dec_slots=256)
lab = torch.from_numpy(np.load(sys.argv[2])["lab"])
o = e.predict(W.synthetic_images(40).cuda(), ref_batch=40, confidence=True, labels=lab)
np.savez(sys.argv[3], **{k: v.cpu().numpy() for k, v in o.items()})
e.close()
"""


def test_results_equal_without_graphs(gold, eng, images, dev, tmp_path):
    """MNX_NO_GRAPH (read when an engine is created): a fresh process decodes the same job launch by launch"""
    lab = gold["px_labels"]
    o = _np(eng.predict(images[:40].to(dev), ref_batch=40, confidence=True, labels=lab))
    np.savez(tmp_path / "lab.npz", lab=lab)
    script = tmp_path / "child.py"
    script.write_text(_NO_GRAPH_CHILD)
    env = dict(os.environ, MNX_NO_GRAPH="1")
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "lab.npz"), str(tmp_path / "out.npz")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _eq_pred(o, dict(np.load(tmp_path / "out.npz")), "graph vs no graph")


def test_guided_argument_checks(eng, images, dev):
    from molnextr_amd.engine import MnxError
    x = images[:2].to(dev)
    with pytest.raises(ValueError):
        eng.predict(x, labels=np.array([[1, 2], [1, 2]]), beam=2)
    lib, h = eng.lib, eng.h
    assert lib.mnx_predict_guided(h, None, 0, 2, 2, 8, None, 1, None, None, None, None, None, 8, None, None, None, None, None) == -1


# -- every tick form the greedy path runs --------------------------------------------------------------------------------
# The default engine above decodes these jobs on the fused tick alone (capacities of 32 to 64 rows: dec_head4_guided_kernel).
# The knobs below are the ones tests/test_gpu_parity.py and tests/test_gpu_refbatch.py force the greedy forms with.
FORMS = {"unfused": {"MNX_DEC_TILE": "0"},                                       # decoder.hip tick: dec_head_guided_kernel
         "mid": {"MNX_DEC_FUSED_MAX": "16", "MNX_DEC_MID_MAX": "4096"},          # 32-row ticks and beyond on the mid form
         "crossing": {"MNX_DEC_FUSED_MAX": "64", "MNX_DEC_MID_MAX": "128"}}      # <= 64 fused, <= 128 mid, beyond: decoder.hip


def _engine_with_env(synth_ckpt, env, **kw):
    from molnextr_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)             # read when the engine is created
    try:
        return Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=["unfused", "mid"])
def form_eng(request, synth_ckpt):
    e = _engine_with_env(synth_ckpt, FORMS[request.param], max_batch=64, dec_slots=256)
    e.form = request.param
    yield e
    e.close()


def test_decode_guided_vs_reference_in_every_tick_form(gold, form_eng, dev):
    _decode_vs_reference(gold, form_eng, dev, form_eng.form)


def test_predict_guided_from_pixels_vs_reference_in_every_tick_form(gold, form_eng, images, dev):
    _predict_vs_reference(gold, form_eng, images, dev, form_eng.form)


def test_guided_along_own_greedy_output_is_greedy_in_every_tick_form(form_eng, images, dev):
    _guided_is_greedy(form_eng, images, dev)


def test_one_guided_job_crosses_the_tick_forms(gold, eng, synth_ckpt, dev):
    """160 images at ref_batch 32 on 256 slots with the fused limit at 64 rows and the mid limit at 128: the job starts on
    the decoder.hip tick (capacity 192: dec_head_guided_kernel), passes through the mid form and drains on the fused one
    (tests/test_gpu_parity.py::test_fused_and_unfused_ticks_mix_in_one_job is its greedy sibling). Ids equal the CPU
    restatement's in every reference batch; tokens, atoms and bonds equal the default engine's, whose forms differ."""
    from molnextr_amd.tokenizer import get_tokenizer
    tok = get_tokenizer()["chartok_coords"]
    n, rb = 160, 32
    x = W.synthetic_images(n, first_index=500).to(dev)
    lab = _labels_for(n, tok, gold["ar"]["smiles"])
    e = _engine_with_env(synth_ckpt, FORMS["crossing"], max_batch=32, dec_slots=256)
    try:
        o = _np(e.predict(x, ref_batch=rb, labels=lab))
    finally:
        e.close()
    for c in range(0, n, rb):
        r = guided_decode(eng.encode(x[c:c + rb].contiguous()).cpu(), synth_ckpt["decoder"], lab[c:c + rb])
        for b in range(rb):
            assert o["tokens"][c + b, :o["lengths"][c + b]].tolist() == r.tokens[b], (c, b)
    d = _np(eng.predict(x, ref_batch=rb, labels=lab))
    for k in ("lengths", "tokens", "n_atoms", "atom_idx"):
        assert np.array_equal(o[k], d[k]), k
    for r, k in enumerate(o["n_atoms"]):
        assert np.array_equal(o["edges"][r, :k, :k], d["edges"][r, :k, :k]), r


# -- the facade ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp32", "gray8"])
def test_predict_coords_equals_engine_predict_with_labels(fmt, dev):
    """molnextr.predict_coords on 11 pages in reference batches of 4 and engine groups of 8 (a group boundary inside, a ragged
    last batch), one SMILES longer than max_len: symbols, coordinates, atom and bond sets and confidences are those of
    Engine.predict(labels=...) group by group along labels tokenised, cut and padded here."""
    from molnextr_amd.model import BOND_TYPES, molnextr
    m = molnextr("synthetic", device=dev, image_format=fmt)
    try:
        m.group_images = 8
        tok = m.tokenizer["chartok_coords"]
        T = m.engine.max_len
        pages = [W.synthetic_page(c % len(W.PAGE_CASES)) for c in range(11)]
        smiles = ["CCO", "C" * 200, "", "[Na+].[Cl-]", "c1ccccc1O", "BrCCCl", "C", "C{Si}C", "CC(=O)O", "C1CC1", "N#C"]
        out = m.predict_coords(pages, smiles, return_confidence=True, batch_size=4)
        seqs = [tok.smiles_to_sequence(s, mask_ratio=1)[0] for s in smiles]
        assert len(seqs[1]) > T and all(len(q) <= T for i, q in enumerate(seqs) if i != 1)
        lab = np.zeros((11, T), np.int32)                      # the long row fills max_len ids and has lost its '<eos>'
        for i, q in enumerate(seqs):
            lab[i, :min(len(q), T)] = q[:T]
        assert len(out) == 11
        for g0, g1 in ((0, 8), (8, 11)):
            x = m.engine.preprocess(pages[g0:g1])
            o = _np(m.engine.predict(x, ref_batch=4, confidence=True, labels=lab[g0:g1], free_run=[i == 1 for i in range(g0, g1)]))
            for r in range(g1 - g0):
                d = tok.sequence_to_smiles(o["tokens"][r, :o["lengths"][r]].tolist())
                k = len(d["symbols"])
                got = out[g0 + r]
                assert [a["atom_symbol"] for a in got["atom_sets"]] == d["symbols"], g0 + r
                assert [a["coords"] for a in got["atom_sets"]] == [(round(c[0], 3), round(c[1], 3)) for c in d["coords"]], g0 + r
                assert [a["confidence"] for a in got["atom_sets"]] == o["atom_scores"][r, :k].tolist(), g0 + r
                bonds = [(i, j, BOND_TYPES[o["edges"][r, i, j]], float(o["edge_scores"][r, i, j]))
                         for i in range(k - 1) for j in range(i + 1, k) if o["edges"][r, i, j] != 0]
                assert [(*b["endpoints"], b["bond_type"], b["confidence"]) for b in got["bond_sets"]] == bonds, g0 + r
        assert len(out[2]["atom_sets"]) == 0 and len(out[0]["atom_sets"]) <= 3
        assert any(len(p["atom_sets"]) > 0 for p in out)
    finally:
        m.engine.close()


def test_evaluate_predict_coords_writes_the_known_structures(dev, tmp_path):
    """evaluate --predict_coords on a CSV with an empty SMILES cell: image_id, SMILES (the input strings, the empty cell as
    the empty string), node_coords; no score file (there is no predicted string to score)."""
    import pandas as pd
    from PIL import Image
    smiles = ["CCO", "", "c1ccccc1"]
    for i in range(3):
        Image.fromarray(W.synthetic_page(INK_PAGES[i])).save(tmp_path / f"p{i}.png")
    pd.DataFrame({"file_path": [f"p{i}.png" for i in range(3)], "SMILES": smiles}).to_csv(tmp_path / "t.csv", index=False)
    child = "import sys; sys.path.insert(0, sys.argv[1]); from molnextr_amd import evaluate; evaluate.main(sys.argv[2:])"
    r = subprocess.run([sys.executable, "-c", child, ROOT, "--data_path", str(tmp_path), "--test_file", "t.csv", "--save_path",
                        str(tmp_path / "out"), "--load_path", "synthetic", "--batch_size", "2", "--predict_coords"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = pd.read_csv(tmp_path / "out" / "prediction_t.csv", keep_default_na=False)
    assert list(got.columns) == ["image_id", "SMILES", "node_coords"]
    assert got["SMILES"].tolist() == smiles and got["image_id"].tolist() == ["p0", "p1", "p2"]
    assert got["node_coords"][1] == "[]" and not [f for f in os.listdir(tmp_path / "out") if f.startswith("eval_scores")]
