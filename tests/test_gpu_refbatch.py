"""Reference batches of more than 32 rows on the greedy predict path (mnx_predict / mnx_predict_confidence).

The reference numbers positional-encoding rows inside the whole (compacted) batch, so a batch of 64 gives rows 32..63
pe[32..63] at step 0 — two batches of 32 would not. These tests pin the engine's multi-tile chunks against the reference's
own output on one batch of 64 and one of 40 (tests/golden/pixels_refbatch.*, tools/gen_golden.py refbatch), against the
CPU oracle on one batch of 512, against per-chunk calls under tile pressure, and the bounds.
Measured values are printed (one JSON line per test, prefixed "refbatch"; run with -s to see them)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-3          # a divergence from the reference is allowed only from a step where its own margin is below this
LOGP_TOL = 1e-4          # token log-probs vs the reference (default operand mode fp16x3)
SCORE_RTOL = 1e-4        # atom / edge / overall confidences vs the reference, relative
SAME_PATH_TOL = 1e-5     # the same rows decoded at different tick capacities (fused vs unfused tick)
ORACLE_LOGP_TOL = 2.5e-4


def _report(name, rec):
    print("refbatch", name, json.dumps(rec))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "pixels_refbatch.npz")))
    with open(os.path.join(golden_dir, "pixels_refbatch.json")) as f:
        g["preds"] = json.load(f)["preds"]
    return g


@pytest.fixture(scope="module")
def images512():
    return W.synthetic_images(512)          # image i is a pure function of i: [:64] are the fixture's images


@pytest.fixture(scope="module")
def eng64(synth_ckpt):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=64, dec_slots=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng96(synth_ckpt):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=192, dec_slots=128)
    yield e
    e.close()


def _first_divergence(ids, n, g_ids, g_n):
    """First step where the engine's ids leave the reference's (None: identical sequences)."""
    m = min(n, g_n)
    bad = np.nonzero(ids[:m] != g_ids[:m])[0]
    if len(bad):
        return int(bad[0])
    return None if n == g_n else m


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


@pytest.mark.parametrize("name,B", [("m64", 64), ("m40", 40)])
def test_reference_batch_from_pixels_vs_reference(name, B, ref, images512, eng64, dev):
    """One reference batch of 64 (the README's evaluation: --batch_size 32) and of 40 rows (a full tile and a ragged one),
    from pixels: every token, atom and bond is the reference's, log-probs and confidences within 1e-4."""
    from molnextr_amd.model import predict_pipeline
    x = images512[:B].to(dev)
    out = eng64.predict(x, ref_batch=B, confidence=True)
    toks, lens, lp = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy(), out["token_logp"].cpu().numpy()
    g_ids, g_lens, g_lp, g_margin = (ref[f"{name}_{k}"] for k in ("ids", "lens", "token_logp", "margin"))
    diverged, lp_err = {}, 0.0
    for r in range(B):
        n, gn = int(lens[r]), int(g_lens[r])
        d = _first_divergence(toks[r], n, g_ids[r], gn)
        upto = gn if d is None else d
        lp_err = max(lp_err, float(np.abs(lp[r, :upto] - g_lp[r, :upto]).max(initial=0.0)))
        if d is not None:
            diverged[r] = (d, float(g_margin[r, d]))
    preds = predict_pipeline(eng64, x, ref_batch_size=B, compute_confidence=True)
    offs = np.cumsum([0] + [len(p["symbols"]) ** 2 for p in ref["preds"][name]])
    toffs = np.cumsum([0] + [len(p["symbols"]) * (len(p["symbols"]) + 1) // 2 for p in ref["preds"][name]])
    atom_err = edge_err = overall_err = 0.0
    for r, (p, g) in enumerate(zip(preds, ref["preds"][name])):
        if r in diverged:
            continue
        c, k = p["chartok_coords"], len(g["symbols"])
        assert c["smiles"] == g["smiles"] and c["symbols"] == g["symbols"] and c["indices"] == g["indices"], f"row {r}"
        assert np.allclose(c["coords"], g["coords"], rtol=0, atol=1e-9), f"row {r}: coordinates"
        assert p["edges"] == ref[f"{name}_edges"][offs[r]:offs[r + 1]].reshape(k, k).astype(int).tolist(), f"row {r}: bonds"
        atom_err = max(atom_err, _rel(c["atom_scores"], g["atom_scores"]))
        es = np.array(p["edge_scores"], np.float64).reshape(k, k)
        edge_err = max(edge_err, _rel(es[np.triu_indices(k)], ref[f"{name}_edge_scores"][toffs[r]:toffs[r + 1]]))
        overall_err = max(overall_err, _rel([p["overall_score"]], [g["overall_score"]]))
    rec = {"rows": B, "steps": int(g_lens.sum()), "logp_max_err": lp_err, "atom_score_max_rel": atom_err,
           "edge_score_max_rel": edge_err, "overall_max_rel": overall_err,
           "diverged_rows": {str(r): {"step": d, "reference_margin": m} for r, (d, m) in diverged.items()}}
    _report(f"reference_{name}", rec)
    for r, (d, m) in diverged.items():
        assert m < NEAR_TIE, f"row {r} leaves the reference at step {d} where its margin is {m} (not a near-tie)"
    assert lp_err < LOGP_TOL, rec
    assert atom_err < SCORE_RTOL and edge_err < SCORE_RTOL and overall_err < SCORE_RTOL, rec


def test_pe_row_passes_32(images512, eng64, dev):
    """The same 64 images as one batch of 64 and as two batches of 32: rows 32..63 see other PE rows (their log-probs differ
    from step 0 on), rows 0..31 are the same rows in both (a row's rank counts only the rows below it)."""
    x = images512[:64].to(dev)
    a = eng64.predict(x, ref_batch=64, confidence=True)
    b = eng64.predict(x, ref_batch=32, confidence=True)
    lp64, lp32 = a["token_logp"].cpu().numpy(), b["token_logp"].cpu().numpy()
    assert (lp64[32:, 0] != lp32[32:, 0]).all(), "rows 32..63 of a 64-row batch must not get pe[0..31]"
    for k in ("tokens", "lengths", "n_atoms", "atom_idx", "edges"):
        assert torch.equal(a[k][:32], b[k][:32]), k
    err = float(np.abs(lp64[:32] - lp32[:32]).max())
    changed = int(sum(not torch.equal(a["tokens"][r], b["tokens"][r]) for r in range(32, 64)))
    _report("pe_row_passes_32", {"rows_0_31_logp_max_diff": err, "rows_32_63_with_other_tokens": changed,
                                 "rows_32_63_step0_logp_max_diff": float(np.abs(lp64[32:, 0] - lp32[32:, 0]).max())})
    assert err < SAME_PATH_TOL


def test_512_rows_vs_oracle(synth_ckpt, images512, dev):
    """One reference batch of 512 (the reference main.py's default --batch_size 256) against the CPU oracle on the same
    features: rows exact or diverging only at an oracle near-tie, log-probs within 2.5e-4."""
    from molnextr_amd.engine import Engine
    from oracle.decoder import greedy_decode
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=512, dec_slots=512)
    try:
        x = images512.to(dev)
        feats = e.encode(x).cpu()                  # the encoder is batch-invariant: predict() computes these same features
        out = e.predict(x, ref_batch=512, confidence=True)
    finally:
        e.close()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    t0 = time.time()
    o = greedy_decode(feats, synth_ckpt["decoder"], trace=True)
    cpu_s = time.time() - t0
    toks, lens, lp = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy(), out["token_logp"].cpu().numpy()
    lp_err, diverged, exact = 0.0, {}, 0
    for r in range(512):
        g = np.array(o.tokens[r], np.int32)
        d = _first_divergence(toks[r], int(lens[r]), g, len(g))
        upto = len(g) if d is None else d
        lp_err = max(lp_err, float(np.abs(lp[r, :upto] - np.array(o.token_logp[r][:upto], np.float32)).max(initial=0.0)))
        if d is None:
            exact += 1
            continue
        alive, lg = o.logits_trace[d]
        top = torch.log_softmax(lg[alive.index(r)].double(), -1).topk(2).values
        diverged[r] = (d, float(top[0] - top[1]))
    rec = {"rows": 512, "rows_exact": exact, "steps": int(sum(len(t) for t in o.tokens)), "logp_max_err": lp_err,
           "oracle_cpu_seconds": round(cpu_s, 1), "cpu_threads": torch.get_num_threads(),
           "diverged_rows": {str(r): {"step": d, "oracle_raw_margin": m} for r, (d, m) in diverged.items()}}
    _report("oracle_512", rec)
    for r, (d, m) in diverged.items():
        assert m < NEAR_TIE, f"row {r} leaves the oracle at step {d} where its margin is {m}"
    assert lp_err < ORACLE_LOGP_TOL, rec


def _bit_exact_engine(synth_ckpt, max_batch, dec_slots):
    """An engine whose greedy ticks all run on one arithmetic (fused up to 128 rows, the bit-identical mid form beyond:
    MNX_DEC_MID_MAX), so that a row's numbers do not depend on how many rows share its tick."""
    from molnextr_amd.engine import Engine
    old = os.environ.get("MNX_DEC_MID_MAX")
    os.environ["MNX_DEC_MID_MAX"] = "4096"
    try:
        return Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=max_batch, dec_slots=dec_slots)
    finally:
        if old is None:
            os.environ.pop("MNX_DEC_MID_MAX")
        else:
            os.environ["MNX_DEC_MID_MAX"] = old


def _per_chunk(eng, x, rb):
    outs = [eng.predict(x[i:i + rb].contiguous(), ref_batch=rb, confidence=True) for i in range(0, x.shape[0], rb)]
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def _assert_same_rows(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def test_scheduling_under_tile_pressure(synth_ckpt, images512, dev):
    """Many multi-tile chunks through a small slot pool equal per-chunk calls, bit for bit (on engines whose ticks run one
    arithmetic at every capacity; with the default tick forms the same rows differ by up to 1e-5 in log-probs between a
    crowded and a lone run, and a bond class at a near-tie can follow): 1000 images at ref_batch=64 on 256 slots (15 full
    chunks and a ragged one of 40, tiles reused, admission waiting for whole chunks), and ref_batch=96 on 128 slots (3 of 4
    tiles per chunk, tiles handed back in another order, a ragged one-tile chunk beside a full one)."""
    x = torch.cat([images512, images512.flip(0)])[:1000].contiguous().to(dev)
    e = _bit_exact_engine(synth_ckpt, 64, 256)
    try:
        _assert_same_rows(e.predict(x, ref_batch=64, confidence=True), _per_chunk(e, x, 64), "ref_batch 64, dec_slots 256")
    finally:
        e.close()
    y = x[:308].contiguous()                      # chunks of 96, 96, 96 and 20 rows
    e = _bit_exact_engine(synth_ckpt, 96, 128)
    try:
        _assert_same_rows(e.predict(y, ref_batch=96, confidence=True), _per_chunk(e, y, 96), "ref_batch 96, dec_slots 128")
    finally:
        e.close()


def test_reference_batch_bounds(images512, eng64, eng96, dev):
    """ref_batch beyond max_batch, dec_slots or 512 is refused with the bound named; beam search keeps its 32."""
    from molnextr_amd.engine import MnxError
    x = images512[:4].to(dev)
    assert eng64.max_ref_batch == 64 and eng96.max_ref_batch == 128
    with pytest.raises(MnxError, match="exceeds cfg.max_batch = 64"):
        eng64.predict(x, ref_batch=65)
    with pytest.raises(MnxError, match="exceeds cfg.max_batch = 64"):
        eng64.predict(x, ref_batch=65, confidence=True)
    with pytest.raises(MnxError, match="exceeds cfg.dec_slots = 128"):
        eng96.predict(x, ref_batch=160)
    with pytest.raises(MnxError, match="exceeds MAX_REF_BATCH = 512"):
        eng64.predict(x, ref_batch=513)          # checked first: 513 is beyond max_batch too
    with pytest.raises(MnxError, match="32"):
        eng64.predict(x, ref_batch=33, beam=5)
