"""CPU: the oracle (oracle/) against the golden vectors generated from the reference itself
(tools/gen_golden.py, run in the build container). This is what pins the oracle."""
import json
import os

import numpy as np
import pytest
import torch

from molnextr_amd import weights as W
from oracle import SwinConfig
from oracle.decoder import greedy_decode, grammar_mask, sinusoid_pe
from oracle.edges import edge_logits, predict_edges, symmetrise
from oracle.swin import encoder_forward, relative_position_index

TINY_W = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
TINY_O = SwinConfig(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
P = "decoder.chartok_coords."


def test_swin_tiny_every_block(golden_dir):
    g = np.load(os.path.join(golden_dir, "swin_tiny.npz"))
    sd = W.synthetic_encoder_state(0, TINY_W)
    img = W.hash_normal("swin_tiny_img", (2, 3, 96, 96), 1.0)
    taps = {}
    feats = encoder_forward(img, sd, TINY_O, tap=lambda n, t: taps.__setitem__(n, t.clone()))
    for name in ("patch_embed", "s0b0", "s0b1", "merge0", "s1b0", "s1b1"):
        np.testing.assert_allclose(taps[name].numpy(), g[name], rtol=0, atol=2e-5, err_msg=name)
    np.testing.assert_allclose(feats.numpy(), g["features"], rtol=0, atol=2e-5)


def test_swin_full_384(golden_dir, synth_ckpt):
    g = np.load(os.path.join(golden_dir, "swin_full.npz"))
    img = W.synthetic_images(2)
    f, hid = encoder_forward(img, synth_ckpt["encoder"], return_hiddens=True)
    f = f.numpy()
    assert f.shape == (2, 144, 1024)
    np.testing.assert_allclose(f[:, :4, :], g["features_head"], atol=5e-5, rtol=0)
    np.testing.assert_allclose(f[:, ::9, ::16], g["features_strided"], atol=5e-5, rtol=0)
    np.testing.assert_allclose(np.abs(f).sum(axis=(1, 2)), g["features_abs_sum"], rtol=1e-5)
    np.testing.assert_allclose(hid[0].numpy()[:, ::512, ::8], g["hidden0_strided"], atol=5e-5, rtol=0)
    np.testing.assert_allclose(hid[2].numpy()[:, ::36, ::32], g["hidden2_strided"], atol=1e-4, rtol=0)


def test_relative_position_index_matches_contract():
    assert torch.equal(relative_position_index(12), W.relative_position_index(12))
    idx = relative_position_index(12)
    assert idx[0, 0] == 11 * 23 + 11 and idx[0, 143] == 0 and idx[143, 0] == 528


def _check_greedy(g, res, max_len):
    B = g["ids"].shape[0]
    for b in range(B):
        n = int(g["lens"][b])
        assert res.tokens[b] == g["ids"][b, :n].tolist(), f"row {b} token ids differ"
        np.testing.assert_allclose(np.array(res.token_logp[b], dtype=np.float32), g["token_logp"][b, :n], atol=2e-4)
        np.testing.assert_allclose(res.hidden[b][:8].numpy(), g["hidden_head"][b, :min(8, n)], atol=2e-5)
        np.testing.assert_allclose(res.hidden[b].double().sum(0).numpy(), g["hidden_sum"][b], atol=2e-3)
    np.testing.assert_allclose(np.array(res.scores), g["scores"], rtol=1e-4)


def test_decoder_greedy_with_compaction(golden_dir, synth_ckpt):
    """B=6, rows finish at different steps: exercises the batch-row positional-encoding quirk under compaction."""
    g = np.load(os.path.join(golden_dir, "decoder_greedy.npz"))
    feats = W.hash_normal("decoder_greedy_features", (6, 144, 1024), 0.5)
    res = greedy_decode(feats, synth_ckpt["decoder"], trace=True)
    assert len(set(g["lens"].tolist())) > 3, "fixture must contain rows of different length"
    _check_greedy(g, res, 480)
    # rtol 1e-6 (~8 fp32 ulps): the logits reach |80|, and the host BLAS picks its fp32 summation order by CPU (an AVX2 sgemm
    # path lands up to 7.6e-5 off the golden on those, 3.6e-7 relative beyond the 5e-5); every logit near 0 is still held to 5e-5
    for s in range(4):
        alive, logits = res.logits_trace[s]
        np.testing.assert_allclose(logits.numpy(), g[f"logits_step{s}"], atol=5e-5, rtol=1e-6)


def test_decoder_max_length_finish(golden_dir, synth_ckpt):
    g = np.load(os.path.join(golden_dir, "decoder_short.npz"))
    feats = W.hash_normal("decoder_short_features", (3, 144, 1024), 0.5)
    res = greedy_decode(feats, synth_ckpt["decoder"], max_len=24)
    _check_greedy(g, res, 24)
    assert all(len(t) == 24 for t in res.tokens)


def test_embedding_row_indexed_pe(golden_dir, synth_ckpt):
    """emb[b] = W[tok_b] * 16 + pe[b]  — PE indexed by batch row (reference components.py:290, embedding.py:52-59)."""
    g = np.load(os.path.join(golden_dir, "embedding_pe.npz"))
    sd = synth_ckpt["decoder"]
    emb_w = sd[P + "embeddings.make_embedding.emb_luts.0.weight"]
    pe = sd[P + "embeddings.make_embedding.pe.pe"].reshape(-1, 256)
    ids = torch.from_numpy(g["ids"]).long()
    mine = emb_w[ids] * 16.0 + pe[: len(ids)]
    np.testing.assert_allclose(mine.numpy(), g["emb"], atol=1e-6)
    np.testing.assert_allclose(sinusoid_pe(5000, 256).numpy(), pe.numpy(), atol=0)


def test_grammar_mask_truth_table(golden_dir):
    with open(os.path.join(golden_dir, "tokenizer.json")) as f:
        t = json.load(f)
    m = grammar_mask(torch.arange(229))
    for i, row in enumerate(t["masks"]):
        assert "".join("1" if v else "0" for v in m[i].tolist()) == row, f"prev id {i}"


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_edge_head(golden_dir, synth_ckpt, name):
    g = np.load(os.path.join(golden_dir, "edges.npz"))
    T = {"a": 40, "b": 90, "c": 12, "d": 20}[name]
    hidden = W.hash_normal(f"edges_hidden_{name}", (T, 256), 1.0)
    idx = g[f"{name}_idx"]
    np.testing.assert_allclose(edge_logits(hidden, idx, synth_ckpt["decoder"]).numpy(), g[f"{name}_logits"], atol=2e-5)
    e, s = predict_edges(hidden, idx, synth_ckpt["decoder"])
    assert np.array_equal(e, g[f"{name}_edges"])
    np.testing.assert_allclose(s, g[f"{name}_scores"], atol=1e-6)


def test_edge_symmetrise_raw(golden_dir):
    g = np.load(os.path.join(golden_dir, "edges.npz"))
    e = symmetrise(g["raw_prob"])
    assert np.array_equal(np.argmax(e, axis=2), g["raw_edges"])
    np.testing.assert_allclose(np.max(e, axis=2), g["raw_scores"], atol=0)
    assert np.array_equal(symmetrise(np.zeros((0, 0, 7))), np.zeros((0, 0, 7)))


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_beam_strategy_vs_reference_class(golden_dir, case):
    """oracle.beam.BeamStrategy against the reference's BeamSearch.advance/update_finished driven with the same
    scripted log-probs (tools/gen_golden.py gen_beam_strategy): back-pointers, ids, scores, surviving images per
    step, and the final n-best lists."""
    from oracle.beam import BeamStrategy
    g = np.load(os.path.join(golden_dir, "beam_strategy.npz"))
    B, K, NB, ML, V = g[case + "_cfg"].tolist()
    z = W.hash_normal("beam_script_" + case, (ML, B, K, V), 1.0).clone()
    z[..., 2] += float(g[case + "_boost"][0])
    table = torch.log_softmax(z, dim=-1)
    st = BeamStrategy(B, K, NB, ML, eos=2)
    seqs = [[] for _ in range(B * K)]
    nsteps = int(g[case + "_nsteps"][0])
    for step in range(nsteps):
        lp = torch.stack([table[step, b, j] for b in st.origin for j in range(K)])
        sel, tok, scores, _, _ = st.advance(lp, lambda row, pt, seqs=seqs: seqs[pt[0]] + [pt[1]])
        assert np.allclose(scores.numpy(), g[f"{case}_score{step}"], rtol=0, atol=0), f"step {step}: scores"
        assert sel.tolist() == g[f"{case}_sel{step}"].tolist(), f"step {step}: back-pointers"
        assert tok.tolist() == g[f"{case}_tok{step}"].tolist(), f"step {step}: ids"
        assert st.origin == g[f"{case}_origin{step}"].tolist(), f"step {step}: surviving images"
        seqs = [seqs[p] + [t] for p, t in zip(sel.tolist(), tok.tolist())]
    assert st.done
    for b in range(B):
        for r in range(NB):
            assert st.results[b][r][1] == g[f"{case}_pred{b}_{r}"].tolist(), f"image {b} rank {r}"
            assert st.results[b][r][0] == pytest.approx(float(g[f"{case}_final{b}_{r}"][0]), abs=0)


def test_beam_decode_with_one_beam_equals_greedy(synth_ckpt):
    """The loop around the (pinned) beam strategy is ours; with beam = n_best = 1 it must collapse to the greedy search
    that IS pinned on the reference (same ids, same decoder outputs, score = sum(logp) / (tokens + 1))."""
    from oracle.beam import beam_decode
    feats = W.hash_normal("beam_eq_greedy", (3, 144, 1024), 0.5)
    g = greedy_decode(feats, synth_ckpt["decoder"], max_len=48)
    b = beam_decode(feats, synth_ckpt["decoder"], beam=1, n_best=1, max_len=48)
    for i in range(3):
        assert b.tokens[i][0] == g.tokens[i]
        assert torch.allclose(b.hidden[i][0], g.hidden[i], atol=1e-5)
        assert b.scores[i][0] == pytest.approx(sum(g.token_logp[i]) / (len(g.tokens[i]) + 1), rel=1e-5)


def test_beam_decode_hypotheses_are_ordered_and_grammatical(synth_ckpt):
    from oracle.beam import beam_decode
    feats = W.hash_normal("beam_props", (2, 144, 1024), 0.5)
    b = beam_decode(feats, synth_ckpt["decoder"], beam=4, n_best=3, max_len=40)
    for i in range(2):
        assert len(b.tokens[i]) == 3 and b.scores[i] == sorted(b.scores[i], reverse=True)
        for seq in b.tokens[i]:
            seq = np.array(seq)
            assert (seq[:-1] != 2).all()                                   # EOS only as the last id
            prev_x = (seq[:-1] >= 101) & (seq[:-1] < 165)
            assert (seq[1:][prev_x] >= 165).all()                          # grammar mask holds inside the beam


def test_beam_decode_records_how_close_its_choices_were(synth_ckpt):
    """BeamResult.min_gap: per image and step, the smallest score gap among the best K + 1 candidates. Over 160 steps the
    4 x 3 case of the GPU beam test passes through a gap of ONE fp32 ulp between rank 0 and rank 1 (step 101): an oracle
    choice that only one particular fp32 summation order reproduces — the reason beam search keeps the arithmetic it was
    validated with, and a reminder that agreement on such a fixture is agreement to the last bit."""
    from oracle.beam import beam_decode
    feats = W.hash_normal("beam_features_4_3", (4, 144, 1024), 0.5)
    b = beam_decode(feats, synth_ckpt["decoder"], beam=3, n_best=2, max_len=160)
    assert [len(g) for g in b.min_gap] == [160, 160, 78, 160]              # image 2 leaves the batch at step 78
    assert all(g >= 0.0 for gaps in b.min_gap for g in gaps)
    assert b.min_gap[0][100] < 5e-7 and min(b.min_gap[0][:100]) > 1e-5     # decided everywhere before, a tie at step 101


def test_oracle_from_pixels_vs_reference_golden(golden_dir, synth_ckpt):
    """The oracle's composition encoder_forward -> greedy_decode on 6 synthetic images against the reference's own
    Encoder + Decoder run on the same pixels (pixels_e2e.*): features, every token, every log-prob."""
    import json
    from molnextr_amd import weights as W
    from molnextr_amd.tokenizer import get_tokenizer
    from oracle.decoder import greedy_decode
    from oracle.edges import predict_edges
    from oracle.swin import encoder_forward
    g = np.load(os.path.join(golden_dir, "pixels_e2e.npz"))
    with open(os.path.join(golden_dir, "pixels_e2e.json")) as f:
        preds = json.load(f)["preds"]["m6"]
    feats = encoder_forward(W.synthetic_images(6), synth_ckpt["encoder"])
    assert np.abs(feats[:, ::9, ::16].numpy() - g["feat_strided"][:6]).max() < 1e-5
    out = greedy_decode(feats, synth_ckpt["decoder"])
    tok = get_tokenizer()["chartok_coords"]
    for b in range(6):
        n = int(g["m6_lens"][b])
        assert out.tokens[b] == g["m6_ids"][b, :n].tolist(), f"row {b}"
        assert np.abs(np.array(out.token_logp[b]) - g["m6_token_logp"][b, :n]).max() < 1e-4
        d = tok.sequence_to_smiles(out.tokens[b])
        assert d["smiles"] == preds[b]["smiles"] and d["indices"] == preds[b]["indices"] and d["coords"] == preds[b]["coords"]
        if d["indices"]:
            e, _ = predict_edges(out.hidden[b], d["indices"], synth_ckpt["decoder"])
            assert np.asarray(e).astype(int).tolist() == preds[b]["edges"], f"row {b}: bonds"


def test_oracle_from_pixels_on_the_stress_checkpoint_vs_reference_golden(golden_dir):
    """The same composition on the hostile checkpoint (W.synthetic_checkpoint(1, stress=True): LayerNorm gains 0.1-8 with x50
    outliers, per-matrix weight scales over 40x, relative-position biases to +-8) against the reference's own classes on the
    same pixels (pixels_stress.*): features of 4 images, tokens and log-probs of the first 96 steps of the first four rows of
    its batch (a prefix of a reference batch keeps every row's positional-encoding rank)."""
    from molnextr_amd import weights as W
    from oracle.decoder import greedy_decode
    from oracle.swin import encoder_forward
    g = np.load(os.path.join(golden_dir, "pixels_stress.npz"))
    ck = W.synthetic_checkpoint(1, stress=True)
    feats = encoder_forward(W.synthetic_images(4, first_index=700), ck["encoder"])
    assert abs(float(g["feat_rms"][0]) - 1.0) < 0.05, "the stress encoder's output norm is rescaled to unit rms"
    assert np.abs(feats[:, ::9, ::16].numpy() - g["feat_strided"][:4]).max() < 2e-5
    T = 96          # the first 96 steps (row 0 finishes at 76, the other three run on): enough to pin the composition on the CPU
    out = greedy_decode(feats, ck["decoder"], max_len=T)
    for b in range(4):
        n = min(int(g["s16_lens"][b]), T)
        assert out.tokens[b] == g["s16_ids"][b, :n].tolist(), f"row {b}"
        assert np.abs(np.array(out.token_logp[b]) - g["s16_token_logp"][b, :n]).max() < 1e-4
