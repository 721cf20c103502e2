"""CPU: the decoder's K / V cache format (csrc/kvq.h) restated on the host (oracle/kvq.py), the study emulation round_block
held to it, and the teacher-forced decode oracle that tests/test_gpu_kvcache.py compares the engine with."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import torch

from molnextr_amd import weights as W
from oracle import decoder as OD
from oracle import kvq as KQ

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import study_split_terms as ST  # noqa: E402

F32 = np.float32


def _quant_exact(row):
    """kvq_quant read off the header in exact rational arithmetic (independent of numpy's rounding): (q list, scale)."""
    vals = [float(v) for v in row]
    amax = max(abs(v) for v in vals)
    e = math.frexp(amax)[1] if amax != 0 else 0
    e = min(max(e, -100), 120)
    q = []
    for v in vals:
        x = Fraction(v) * Fraction(2) ** (23 - e)
        x = min(max(x, Fraction(-2 ** 23)), Fraction(2 ** 23 - 1))
        q.append(round(x))                       # Fraction rounds half to even
    return q, 2.0 ** (e - 23)


def test_restatement_reads_kvq_h_exactly():
    rows = KQ.edge_rows()
    for name, r in rows.items():
        q, sc = KQ.quant(r)
        qe, sce = _quant_exact(r)
        assert q.tolist() == qe and float(sc) == sce, name
        assert sc.dtype == np.float32 and np.isfinite(sc)
        assert q.min() >= -2 ** 23 and q.max() <= 2 ** 23 - 1, name
    # the cases by hand
    q, sc = KQ.quant(rows["zeros"])
    assert not q.any() and sc == 2.0 ** -23                              # amax = 0: e = 0
    q, sc = KQ.quant(rows["below_pow2_7"])
    assert sc == 2.0 ** (7 - 23) and q[0] == 2 ** 23 - 1 and q[1] == -2 ** 23
    q, sc = KQ.quant(rows["above_pow2_0"])
    assert sc == 2.0 ** -22 and q[0] == 2 ** 22 and q[1] == -2 ** 22       # 2^22 + 1/2 -> even
    q, sc = KQ.quant(rows["pow2_0"])
    assert sc == 2.0 ** -22 and q[2:8].tolist() == [0, 2, -2, -4, 1000, -1002]
    q, sc = KQ.quant(rows["denormal"])
    assert sc == 2.0 ** -123 and not q.any()                             # exponent clamped at -100: zeros
    q, sc = KQ.quant(rows["low_clamp_110"])
    assert sc == 2.0 ** -123 and q[0] == round(1.3 * 2.0 ** 13) and q[1] == -2 ** 12
    q, sc = KQ.quant(rows["high_clamp_121"])
    assert sc == 2.0 ** 97 and q[0] == 2 ** 23 - 1 and q[1] == -2 ** 23 and q[2] == 4 and q[3] == 0   # 3.5 -> 4


def test_restatement_of_nonfinite_rows():
    """What kvq.h documents: NaN stores -2^23 (fmaxf drops it), the row max ignores NaN, every word and scale is finite."""
    for name, r in KQ.nonfinite_rows().items():
        q, sc = KQ.quant(r)
        assert np.isfinite(sc), name
        assert (q[np.isnan(r)] == -2 ** 23).all(), name
        assert q.min() >= -2 ** 23 and q.max() <= 2 ** 23 - 1, name
    q, sc = KQ.quant(KQ.nonfinite_rows()["nan_in_row"])
    assert sc == 2.0 ** (2 - 23) and q[1] == 3 * 2 ** 20                 # amax = 3 (NaN ignored): e = 2
    q, sc = KQ.quant(KQ.nonfinite_rows()["pos_inf"])
    assert sc == 2.0 ** -23 and q[0] == 2 ** 23 - 1                      # frexp(inf): e = 0


def test_block_layout_round_trip():
    g = np.random.default_rng(3)
    for nk in (4, 144, 512):
        q = g.integers(-2 ** 23, 2 ** 23, size=(nk, 32))
        sc = np.ldexp(F32(1), g.integers(-123, 97, size=nk)).astype(F32)
        raw = KQ.pack_block(q, sc)
        assert raw.shape == (nk * 100,)
        q2, sc2 = KQ.parse_block(raw, nk)
        assert np.array_equal(q, q2) and np.array_equal(sc, sc2)
        # hi is q >> 8 at byte 64 * key + 2 * c, lo is q & 255 at 64 nk + 32 key + c, the scale at 96 nk + 4 key
        assert raw[64 * 3 + 2 * 5:64 * 3 + 2 * 5 + 2].view(np.int16)[0] == q[3, 5] >> 8
        assert raw[64 * nk + 32 * 3 + 5] == q[3, 5] & 255
        assert raw[96 * nk + 4 * 3:96 * nk + 4 * 3 + 4].view(np.float32)[0] == sc[3]


def test_round_block_24_is_the_cache():
    """round_block(., 24) (the study emulation behind kvq.h's numbers) equals the restatement on every finite row; before it
    took its exponent from float32 log2, which rounds up just below a power of two (1024 (1 - 2^-24) -> e = 11, not 10)."""
    rows = KQ.edge_rows()
    x = torch.from_numpy(np.stack(list(rows.values())))
    got = ST.round_block(x, 24).numpy()
    q, sc = KQ.quant(x.numpy())
    want = KQ.dequant(q, sc)
    for i, name in enumerate(rows):
        assert np.array_equal(got[i], want[i]), name
    # and on a batch of random rows over 60 binary orders of magnitude, with the [L][B][h][dh] layout the study uses
    g = torch.Generator().manual_seed(5)
    y = torch.randn(3, 4, 8, 32, generator=g) * torch.exp2(torch.randint(-30, 30, (3, 4, 8, 1), generator=g).float())
    q, sc = KQ.quant(y.numpy())
    assert np.array_equal(ST.round_block(y, 24).numpy(), KQ.dequant(q, sc))


def _prefixed(sd):
    return {k if k.startswith(OD.P) else OD.P + k: v for k, v in sd.items()}


def test_forced_oracle_repeats_greedy_decode():
    """oracle.decoder.forced_decode in float32, forced along greedy_decode's own tokens, gives greedy_decode's logits bit for
    bit at every step: the same loop, the same PE rank of a row in the compacted batch, the same operations."""
    sd = _prefixed(W.synthetic_checkpoint(0)["decoder"])
    feats = W.hash_normal("forced_oracle_b", (8, 144, 1024), 3.0)
    g = OD.greedy_decode(feats, sd, max_len=128, trace=True)
    lens = [len(t) for t in g.tokens]
    assert min(lens[:-1]) < min(lens[-1], 128), lens    # a row finishes before a later one: that row's PE rank changes
    ids = torch.zeros(8, max(lens), dtype=torch.long)
    for b, t in enumerate(g.tokens):
        ids[b, :len(t)] = torch.tensor(t)
    lg = OD.forced_decode(feats, sd, ids, lens, dtype=torch.float32)
    assert lg.dtype == torch.float32
    for step, (alive, logits) in enumerate(g.logits_trace):
        for i, r in enumerate(alive):
            assert torch.equal(lg[r, step], logits[i]), (r, step)
    for b, n in enumerate(lens):
        assert torch.isnan(lg[b, n:]).all()


def test_boundary_tolerance_sees_a_coarser_cache_and_a_dropped_key():
    """tests/test_gpu_kvcache.py holds the engine's logits to KQ.logit_tolerance of a float64 oracle along the key-boundary
    decode. On the same features and trajectories, a decode that rounds every cached K / V row to 16-bit block fixed point,
    or that drops key 32, 160 or 256 from the self-attention softmax once a row has passed it, must miss by at least ten
    times that tolerance: a reader that loses a key or a writer that loses the low byte cannot pass."""
    sd = W.synthetic_checkpoint(0)["decoder"]
    feats, ids, lens = KQ.boundary_case()
    ref = OD.forced_decode(feats, sd, ids, lens)
    tol = KQ.logit_tolerance(ref)
    err = lambda lg: float(torch.nan_to_num((lg - ref).abs(), nan=0.0).max())      # noqa: E731
    ratios = {"int16 cache": err(OD.forced_decode(feats, sd, ids, lens, kv=lambda t: ST.round_block(t, 16).double()))}
    for j in (32, 160, 256):
        ratios[f"drop key {j}"] = err(OD.forced_decode(feats, sd, ids, lens, drop_key=j))
    ratios = {k: v / tol for k, v in ratios.items()}
    print(f"tolerance {tol:.3e}; error / tolerance: " + ", ".join(f"{k} {v:.1f}" for k, v in ratios.items()))
    assert all(v >= 10 for v in ratios.values()), ratios
    # and the float32 oracle, with or without the 24-bit cache, stays inside it
    f32 = OD.forced_decode(feats, sd, ids, lens, dtype=torch.float32, kv=lambda t: ST.round_block(t, 24))
    assert err(f32.double()) < tol / 2
