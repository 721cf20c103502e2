"""GPU (-m gpu): confidences on the continuous-batching path (mnx_predict_confidence, mnx_confidence) against the reference
golden, the host formula of decode_batch (model.py; the definition: reference components.py:456-469,485-491) and the
per-batch path encode + decode_batch(compute_confidence=True)."""
import json
import os
import random

import numpy as np
import pytest
import torch

from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    yield e
    e.close()


@pytest.fixture(scope="module")
def tok():
    from molnextr_amd.tokenizer import get_tokenizer
    return get_tokenizer()["chartok_coords"]


def _host_conf(logp_row, n, symbols, indices, es):
    """decode_batch's formulas (model.py) on one sequence: (atom_scores, overall_score)."""
    ts = np.exp(logp_row[:n].astype(np.float64))
    idx = np.array(indices) - 3
    atoms = [float(np.prod(ts[i - len(s) + 1:i + 1]) ** (1 / len(s))) for s, i in zip(symbols, idx)]
    k = len(indices)
    overall = float(np.exp(np.mean(logp_row[:n].astype(np.float64)))) * float(np.sqrt(np.prod(es[:k, :k])))
    return atoms, overall


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


def _check_device_vs_host(tok, toks, lens, logp, es, atom_scores, overall, kmax, tol=1e-12):
    for b in range(len(lens)):
        n = int(lens[b])
        d = tok.sequence_to_smiles(toks[b, :n].tolist())
        k = len(d["indices"])
        atoms, ov = _host_conf(logp[b], n, d["symbols"], d["indices"], es[b])
        assert _rel(atom_scores[b, :k], atoms) <= tol, (b, atom_scores[b, :k], atoms)
        assert np.all(atom_scores[b, k:kmax] == 0.0), b
        assert _rel([overall[b]], [ov]) <= tol, (b, overall[b], ov)


def _atoms_of(tok, toks, lens, kmax):
    n = len(lens)
    idx = np.zeros((n, kmax), np.int32)
    cnt = np.zeros(n, np.int32)
    for b in range(n):
        d = tok.sequence_to_smiles(toks[b, :lens[b]].tolist())
        cnt[b] = len(d["indices"])
        idx[b, :cnt[b]] = d["indices"]
    return torch.from_numpy(idx), torch.from_numpy(cnt)


def test_device_confidence_vs_reference_golden_and_host_formula(golden_dir, eng, dev, tok):
    """mnx_decode_greedy(log-probs) + mnx_edges(scores) + mnx_confidence on the golden features: the reference's own scores at
    the tolerances of test_confidence_outputs_vs_reference_golden, the host formula on the same inputs to 1e-12."""
    with open(os.path.join(golden_dir, "predict_e2e_conf.json")) as f:
        gold = json.load(f)["preds"]
    feats = W.hash_normal("conf_features", (3, 144, 1024), 0.5).to(dev)
    out = eng.decode_greedy(feats, want_logp=True)
    toks, lens = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy()
    idx, cnt = _atoms_of(tok, toks, lens, eng.max_atoms)
    _, scores = eng.edges(out["hidden"], idx, cnt, want_scores=True)
    a_dev, o_dev = eng.confidence(out["tokens"], out["lengths"], out["token_logp"], idx, cnt, scores)
    a_dev, o_dev = a_dev.cpu().numpy(), o_dev.cpu().numpy()
    es = scores.cpu().numpy()
    _check_device_vs_host(tok, toks, lens, out["token_logp"].cpu().numpy(), es, a_dev, o_dev, eng.max_atoms)
    for b, g in enumerate(gold):
        k = int(cnt[b])
        assert tok.sequence_to_smiles(toks[b, :lens[b]].tolist())["indices"] == g["indices"]
        np.testing.assert_allclose(a_dev[b, :k], g["atom_scores"], rtol=2e-4)
        assert abs(o_dev[b] - g["overall_score"]) <= 1e-6 + 1e-3 * abs(g["overall_score"])
        if g["edge_scores"] is not None:
            np.testing.assert_allclose(es[b, :k, :k], np.array(g["edge_scores"]), atol=1e-5)


def _fuzz_rows(tok, rng, n_rows, T):
    s = tok.stoi
    atom = lambda: s[rng.choice("CNOPSc")]                                    # noqa: E731
    xy = lambda: [101 + rng.randint(0, 63), 165 + rng.randint(0, 63)]         # noqa: E731
    rows = []
    for p in range(5):                                     # '<unk>' atom at positions 0..4: its span reaches before the start
        rows.append([atom()] * p + [3] + xy() + [atom()] + xy() + [s["="], 3] + xy() + [5, 2])
    rows.append([s["["], 3, s["H"], s["]"]] + xy() + [s["["], s["N"], 3, s["]"]] + xy() + [3] + xy() + [2])   # in brackets
    rows.append([s["C"], s["l"]] + xy() + [s["B"], s["r"]] + xy() + [s["C"]] + xy() + [s["C"], s["l"], 2])    # Cl / Br
    rows.append([s["C"], s["N"], s["O"], s["="], 2])                          # atoms without coordinates: k = 0
    rows.append([2])                                                          # EOS only: k = 0
    while len(rows) < n_rows:
        seq = []
        n = rng.randint(1, 200)
        while len(seq) < n:
            r = rng.random()
            if r < 0.55:
                sym = rng.choice(["C", "N", "O", "Cl", "Br", "[", "c", "*", "<unk>", "B", "Cr"])
                if sym == "[":
                    seq += [s["["], rng.choice([3, s[rng.choice("CNOH@+-23")]]), s[rng.choice("CNOH@+-23]")], s["]"]]
                elif sym == "<unk>":
                    seq.append(3)
                else:
                    seq += [s[c] for c in sym]
                if rng.random() < 0.9:
                    seq += xy()
            else:
                seq.append(rng.randint(5, 228))
        seq.append(2)
        rows.append(seq)
    for _ in range(4):                                     # cut at T without EOS, atoms up to the end
        seq = []
        while len(seq) < T:
            seq += [rng.choice([3, s["C"], s["N"]])] + xy() + [s["="]]
        rows.append(seq[:T])
    return rows


def test_device_confidence_fuzz_vs_host_formula(eng, dev, tok):
    """mnx_confidence on constructed id sequences ('<unk>' spans reaching before the start or inside brackets, Cl / Br, atoms
    without coordinates, rows cut at T, k = 0) with random log-probs in [-20, 0] and random edge scores: the host formula to
    1e-12 relative, exact zeros beyond n_atoms."""
    rng = random.Random(11)
    T, kmax = 480, eng.max_atoms
    rows = _fuzz_rows(tok, rng, 300, T)
    n = len(rows)
    toks = np.zeros((n, T), np.int32)
    lens = np.zeros(n, np.int32)
    for b, r in enumerate(rows):
        toks[b, :len(r)] = r
        lens[b] = len(r)
    g = np.random.default_rng(5)
    logp = (-20.0 * g.random((n, T))).astype(np.float32)
    idx, cnt = _atoms_of(tok, toks, lens, kmax)
    assert int(cnt.max()) <= kmax and int((cnt == 0).sum()) >= 2 and int(cnt.max()) > 100
    es = 1.0 - 0.02 * g.random((n, kmax, kmax))                              # winning-class probabilities (product stays normal)
    small = cnt.numpy() <= 6
    es[small] = 1.0 / 7 + (6.0 / 7) * g.random((int(small.sum()), kmax, kmax))
    a_dev, o_dev = eng.confidence(torch.from_numpy(toks).to(dev), torch.from_numpy(lens), torch.from_numpy(logp), idx, cnt,
                                  torch.from_numpy(es))
    _check_device_vs_host(tok, toks, lens, logp, es, a_dev.cpu().numpy(), o_dev.cpu().numpy(), kmax)


def _encode_all(eng, imgs):
    step = eng.max_batch
    return torch.cat([eng.encode(imgs[i:i + step].contiguous()) for i in range(0, imgs.shape[0], step)])


def _assert_dicts_equal_but_floats(p, q, tol):
    a, b = dict(p), dict(q)
    ca, cb = dict(a.pop("chartok_coords")), dict(b.pop("chartok_coords"))
    assert _rel(ca.pop("atom_scores"), cb.pop("atom_scores")) <= tol
    assert ca == cb
    assert _rel(np.ravel(a.pop("edge_scores")), np.ravel(b.pop("edge_scores"))) <= tol
    assert _rel([a.pop("overall_score")], [b.pop("overall_score")]) <= tol
    assert a == b


def test_pipeline_confidence_equals_per_batch_confidence(eng, dev, tok):
    """40 images, reference batches of 16 (at most 128 sequences: one tick form): predict_pipeline(compute_confidence=True)
    against encode + decode_batch(compute_confidence=True). Tokens / indices / edges equal, log-probs and edge scores
    bit-identical, confidences within 1e-12."""
    from molnextr_amd.model import decode_batch, predict_pipeline
    imgs = W.synthetic_images(40, first_index=500).to(dev)
    out = eng.predict(imgs, ref_batch=16, confidence=True)
    feats = _encode_all(eng, imgs)
    ref = decode_batch(eng, feats, ref_batch_size=16, compute_confidence=True)
    for first in (0, 32):                                  # decode_batch's own engine calls: 2 reference batches, then 1
        f = feats[first:first + 32].contiguous()
        r = eng.decode_greedy(f, chunk_id=torch.arange(f.shape[0], dtype=torch.int32) // 16, want_logp=True)
        n = f.shape[0]
        lens = r["lengths"].cpu().numpy()
        assert np.array_equal(out["lengths"][first:first + n].cpu().numpy(), lens)
        lp_ref = r["token_logp"].cpu().numpy()
        lp = out["token_logp"][first:first + n].cpu().numpy()
        for b in range(n):
            assert np.array_equal(lp[b, :lens[b]], lp_ref[b, :lens[b]]), f"image {first + b}: log-probs"
        for b in range(n):
            k = len(ref[first + b]["edges"])
            es = out["edge_scores"][first + b, :k, :k].cpu().numpy()
            assert np.array_equal(es, np.array(ref[first + b]["edge_scores"]).reshape(k, k)), f"image {first + b}: edge scores"
    preds = predict_pipeline(eng, imgs, ref_batch_size=16, compute_confidence=True)
    assert len(preds) == len(ref) == 40
    for p, q in zip(preds, ref):
        _assert_dicts_equal_but_floats(p, q, 1e-12)


def test_confidence_job_across_tick_forms(eng, dev, tok):
    """320 images, reference batches of 32 (the tick form changes with the alive-row count): asking for confidences changes no
    token / atom / bond of mnx_predict; the device confidences equal the host formula on the returned log-probs and edge scores
    (1e-12); against encode + decode_batch they agree to the run-to-run tolerance of the log-probs."""
    from molnextr_amd.model import decode_batch
    imgs = W.synthetic_images(320, first_index=900).to(dev)
    plain = eng.predict(imgs, ref_batch=32)
    conf = eng.predict(imgs, ref_batch=32, confidence=True)
    for key in ("lengths", "n_atoms"):
        assert torch.equal(plain[key], conf[key]), key
    p = {k: v.cpu().numpy() for k, v in plain.items()}
    c = {k: v.cpu().numpy() for k, v in conf.items()}
    for i, (n, k) in enumerate(zip(p["lengths"], p["n_atoms"])):
        assert np.array_equal(p["tokens"][i, :n], c["tokens"][i, :n]), f"image {i}: tokens"
        assert np.array_equal(p["atom_idx"][i, :k], c["atom_idx"][i, :k]), f"image {i}: atom positions"
        assert np.array_equal(p["edges"][i, :k, :k], c["edges"][i, :k, :k]), f"image {i}: bonds"
    _check_device_vs_host(tok, c["tokens"], c["lengths"], c["token_logp"], c["edge_scores"], c["atom_scores"],
                          c["overall_score"], eng.max_atoms)
    ref = decode_batch(eng, _encode_all(eng, imgs), ref_batch_size=32, compute_confidence=True)
    for i, q in enumerate(ref):
        k = int(c["n_atoms"][i])
        assert q["chartok_coords"]["indices"] == c["atom_idx"][i, :k].tolist(), f"image {i}"
        np.testing.assert_allclose(c["atom_scores"][i, :k], q["chartok_coords"]["atom_scores"], rtol=2e-4)
        if k:
            np.testing.assert_allclose(c["edge_scores"][i, :k, :k], np.array(q["edge_scores"]), atol=1e-5)
        assert abs(c["overall_score"][i] - q["overall_score"]) <= 1e-3 * abs(q["overall_score"])


def test_facade_confidences_on_the_throughput_path(dev):
    """predict_images(return_confidence=True) in several engine calls (batch_size 4, groups of 4): the reference's output keys,
    and the confidences of encode + decode_batch on the same transformed images."""
    from molnextr_amd.model import BOND_TYPES, decode_batch, molnextr
    m = molnextr("synthetic", dev, max_batch=4)
    try:
        pages = [W.synthetic_page(c) for c in range(10)]
        m.group_images = 4
        out = m.predict_images(pages, return_atoms_bonds=True, return_confidence=True, batch_size=4)
        x = m._transform(pages)
        ref = []
        for i in range(0, len(pages), 4):                  # the per-batch path the facade took before: one decode per 4
            ref += decode_batch(m.engine, m.engine.encode(x[i:i + 4].contiguous()), ref_batch_size=4,
                                compute_confidence=True)
        assert len(out) == len(ref) == 10
        for o, q in zip(out, ref):
            assert set(o) == {"predicted_smiles", "predicted_molfile", "atom_sets", "bond_sets"}
            for a in o["atom_sets"]:
                assert set(a) == {"atom_number", "atom_symbol", "coords", "confidence"}
            for b in o["bond_sets"]:
                assert b["bond_type"] in BOND_TYPES[1:] and b["endpoints"][0] < b["endpoints"][1]
            assert [a["atom_symbol"] for a in o["atom_sets"]] == q["chartok_coords"]["symbols"]
            assert _rel([a["confidence"] for a in o["atom_sets"]], q["chartok_coords"]["atom_scores"]) <= 1e-12
            want = [q["edge_scores"][i][j] for i in range(len(q["edges"])) for j in range(i + 1, len(q["edges"]))
                    if q["edges"][i][j] != 0]
            assert _rel([b["confidence"] for b in o["bond_sets"]], want) <= 1e-12
    finally:
        m.engine.close()
