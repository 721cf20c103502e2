"""GPU (-m gpu): the greedy head's tie rule — topk(1): the LOWEST index among equal maxima — through the real decoder.

The checkpoint is the synthetic one with output_layer.weight = 0: the logits of every row at every step are the bias,
exactly (256 fmaf of a finite hidden value with 0, then + bias). The bias is piecewise constant, so the maximum of every
step is a tie whose members lie in more than one 64-lane wave of the head's arg-max (thread = id):
    ids 60..70    0.5   waves 0 and 1   (the maximum after a y-bin: the grammar mask removes ids >= 101)
    ids 101..164  2.0   waves 1 and 2   (the maximum after anything else)
    ids 165..228  1.0   waves 2 and 3   (the maximum after an x-bin: the mask leaves the y-bins only)
Three comparisons carry the rule in each head — the shuffle reduction's `oi < bi`, the per-wave merge on thread 0 — and a
wrong one picks another member of the tie here, where it picks the same id on every other fixture of the suite.

Tick forms (tests/test_gpu_parity.py::_engine_with_tick). MNX_DEC_TILE = 0 runs the 8-launches-per-layer tick, whose head is
dec_head_kernel (dec_head_body.inc). The fused tick (tiles 4 x 4 and 2 x 8) and its mid form (fused up to 16 rows only, mid
beyond: a decode call ticks 32 rows of capacity) end in dec_head4_kernel (dec_head4_body.inc). Both are reached.

token_logp against float64. u = 2^-24. The logits are exact, their maximum m = 2 is exact and so is every logit - m. The
sum S = sum_i e^(logit_i - m) has 229 positive terms, each from expf (taken as 2 ulp = 4 u relative); summed in ANY order
its relative error is at most 228 u more: 232 u, which is the absolute error it leaves in log S. S is about 102 and log S
about 4.6, below 8, where an ulp is 2^-21 = 8 u: logf (2 ulp) adds 16 u, and the roundings of m + log S and of
logit - lse, both results below 8 in magnitude, add 4 u each. 232 + 16 + 4 + 4 = 256 u = 2^-16 = 1.53e-5: the bound.
The head's sums are trees (6 shuffle levels and 3 adds), so the measured error is far smaller; it is printed. Measured on
an MI355X: 8.2e-8 = 1.4 u in all four forms (the two heads give the same words here)."""
import numpy as np
import pytest
import torch

from molnextr_amd import weights as W
from test_gpu_parity import _engine_with_tick

pytestmark = pytest.mark.gpu

V, EOS, X0, Y0 = 229, 2, 101, 165
TOL = 2.0 ** -16
# (MNX_DEC_TILE, MNX_DEC_TILE_FF, fused_max, mid_max) -> the head kernel the 32-row tick of decode_greedy ends in
FORMS = {"unfused": ((0, 4, 128, 0), "dec_head_kernel"), "fused_4x4": ((4, 4, 128, 0), "dec_head4_kernel"),
         "fused_2x8": ((2, 8, 128, 0), "dec_head4_kernel"), "mid": ((4, 4, 16, 4096), "dec_head4_kernel")}


def crafted_bias():
    b = torch.zeros(V)
    b[60:71] = 0.5
    b[X0:Y0] = 2.0
    b[Y0:V] = 1.0
    return b


def expected(bias, max_len):
    """The rule restated: float64 log-softmax of the bias, the grammar mask (after an x-bin only y-bins, after a y-bin no
    coordinate bins), <eos> banned at t = 0, first maximum. -> ids, their float64 log-probs"""
    z = bias.double().numpy()
    lp = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
    ids, logp, prev = [], [], 1                 # <sos>
    for t in range(max_len):
        row = lp.copy()
        if X0 <= prev < Y0:
            row[:Y0] = -10000.0
        elif prev >= Y0:
            row[X0:] = -10000.0
        if t == 0:
            row[EOS] = -1e20
        prev = int(np.argmax(row))              # the first of equal maxima
        ids.append(prev)
        logp.append(row[prev])
    return ids, np.array(logp)


@pytest.fixture(scope="module")
def crafted_ckpt(synth_ckpt):
    dec = dict(synth_ckpt["decoder"])
    (wk,) = [k for k in dec if k.endswith("output_layer.weight")]
    (bk,) = [k for k in dec if k.endswith("output_layer.bias")]
    assert tuple(dec[wk].shape) == (V, 256)
    dec[wk] = torch.zeros_like(dec[wk])
    dec[bk] = crafted_bias()
    return {"encoder": synth_ckpt["encoder"], "decoder": dec}


def test_expected_sequence_walks_the_three_ties():
    ids, logp = expected(crafted_bias(), 12)
    assert ids == [101, 165, 60] * 4 and np.isfinite(logp).all() and (logp > -10.0).all()


@pytest.mark.parametrize("form", list(FORMS))
def test_greedy_head_picks_the_lowest_index_of_a_tie(crafted_ckpt, form):
    (tile, tile_ff, fused_max, mid_max), _kernel = FORMS[form]
    dev = torch.device("cuda:0")
    e = _engine_with_tick(crafted_ckpt, tile, tile_ff, fused_max=fused_max, mid_max=mid_max)
    try:
        feats = W.hash_normal("head_ties_features", (5, 144, 1024), 0.5).to(dev)
        out = e.decode_greedy(feats, max_len=e.max_len, stop_on_eos=False)
        ids, logp = expected(crafted_bias(), e.max_len)
        toks, got = out["tokens"].cpu().numpy(), out["token_logp"].cpu().numpy().astype(np.float64)
        assert out["lengths"].cpu().tolist() == [e.max_len] * 5
        for b in range(5):
            assert toks[b].tolist() == ids, f"{form} row {b}: first difference at step " \
                                            f"{int(np.argmax(toks[b] != np.array(ids)))}"
        err = float(np.abs(got - logp[None, :]).max())
        print(f"{form} ({_kernel}): max |token_logp - float64| = {err:.3e} = {err / 2.0 ** -24:.1f} u; bound {TOL:.3e}")
        assert err <= TOL, (form, err)
    finally:
        e.close()
