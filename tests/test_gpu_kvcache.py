"""GPU (-m gpu): the decoder's K / V cache (csrc/kvq.h) read back bit for bit from every writer, and the decoder's logits
against a float64 oracle at every key count where the attention readers change behaviour, up to 512 keys.

Writers: kvq_pack_kernel (memory K / V, every engine), dec_linear_kernel EPI 0 (the 8-launch tick: tile 0, and max_len 512,
where it is forced), dec_fa_kernel (the fused tick) and dec_ma_kernel (the mid form). A decode call ticks 32 rows of
capacity whatever B, so MNX_DEC_FUSED_MAX = 16 with MNX_DEC_MID_MAX = 4096 sends every tick to the mid form. The engines
run at max_len 511, so that Tq = kvq_rows(511) = 512 != T, or at 512.

Crafted heads. In every layer three heads get zero K / V / query weight rows, zero query biases and zero final_linear
columns, in both attentions: every writer's fp32 row for them is then the bias slice exactly, their scores are 0 and
nothing downstream depends on them. Their K / V biases carry the rows of oracle.kvq.edge_rows / nonfinite_rows (ties,
rows just below / above a power of two, denormals, both exponent clamps, NaN and infinities; the weight contract takes
any float). The other heads stay random: the decode remains a real one. Rows whose largest element is 2^119 or more are
stored as keys and memory values but not as self-attention values: the readers sum P.V unnormalised (sum_j e^(s_j - m) v_j,
divided by sum_j e^(s_j - m) afterwards), so 257 or more keys of values near 2^120 overflow to Inf where the reference,
which normalises P first, stays finite (144 memory keys stay below 2^128). This test found that range limit; no trained
checkpoint's values come near it.

Tolerance of the logits (test_logits_match_float64_at_every_key_boundary). u = 2^-24, the fp32 unit roundoff; M = max
|logit| of the float64 decode. A logit is a 256-term dot product of the final LayerNorm's output; its error is the
residual stream's relative error carried through that product, i.e. at most (n + 4) u M for a stream that went through n
relative roundings of size u, plus the fp32 output product itself (a 256-long chain of fmaf: 4 u M in the four-way
chain). Per layer the stream takes 2 LayerNorms (2 each), the self-attention (score 1, exponential and normalisation 2,
P.V 1, final_linear 1) and the cross-attention (the same, 5), the feed-forward (2 products, GELU: 3) and three residual
sums (3): about 5 + 5 + 2 + 3 + 3 -> 4 layers of slack aside, 6 layers x ~4.5 ~= 28. The cache adds 2^-24 of a row's
largest element per K / V element, the size of the fp32 rounding of that element, read once per key: it stays in the same
budget. tol = 32 u M (oracle.kvq.LOGIT_TOL_C). The float32 oracle with the 24-bit cache measures 11 u M on the
molecule-like checkpoint; tests/test_kvq_host.py shows that a 16-bit cache (15 x tol) and a dropped key 32 / 160 / 256
(>1000 x tol) fail it. Measured on an MI355X (printed by the test): the fused tick at R = 4 and R = 2 and the mid form
3.7e-5 = 7.2 u M (bitwise the same logits), tile 0 and max_len 512 (the 8-launch tick) 6.6e-5 = 13.0 u M; tol = 1.6e-4.
"""
import os
import time

import numpy as np
import pytest
import torch

from oracle import decoder as OD
from oracle import kvq as KQ

pytestmark = pytest.mark.gpu

L, H, S = 6, 8, 144
SLOTS = 64                        # dec_slots: two 32-row tiles, so that slots and memory blocks at or past B exist
P = "decoder.transformer_layers."
WHICH = ("self_k", "self_v", "mem_k", "mem_v")
# (max_len, MNX_DEC_TILE, MNX_DEC_FUSED_MAX, MNX_DEC_MID_MAX)
FORMS = {"fused": (511, -1, 128, 0), "fused_r4": (511, 4, 128, 0), "fused_r2": (511, 2, 128, 0), "mid": (511, 4, 16, 4096),
         "tile0": (511, 0, 128, 0), "len512": (512, -1, 128, 0)}


def crafted_heads(layer):
    return (layer % H, (layer + 3) % H, (layer + 6) % H)


def crafted_rows():
    """{(layer, head, which): float32 [32]}: every edge row, then the non-finite ones, then random rows at a spread of scales.
    Rows of 2^119 and more go to keys and memory values only (module docstring)."""
    g = np.random.default_rng(17)
    keys = [(l, h, w) for l in range(L) for h in crafted_heads(l) for w in WHICH]
    pending = list(KQ.edge_rows().values()) + list(KQ.nonfinite_rows().values())
    while len(pending) < len(keys) + 8:
        pending.append((g.standard_normal(32) * 2.0 ** int(g.integers(-60, 60))).astype(np.float32))
    huge = lambda r: np.abs(r[np.isfinite(r)]).max(initial=0.0) >= 2.0 ** 119          # noqa: E731
    out = {}
    for k in keys:
        out[k] = pending.pop(next(i for i, r in enumerate(pending) if k[2] != "self_v" or not huge(r)))
    return out


def _prefix(dec):
    return next(k for k in dec if k.endswith(P + "0.self_attn.linear_keys.weight"))[:-len(P + "0.self_attn.linear_keys.weight")]


def crafted_decoder(dec, rows, zero_bias=False):
    d = {k: v.clone() for k, v in dec.items()}
    pre = _prefix(d)
    for l in range(L):
        for h in crafted_heads(l):
            c = slice(32 * h, 32 * h + 32)
            for att in ("self_attn", "context_attn"):
                a = f"{pre}{P}{l}.{att}."
                for lin in ("linear_keys", "linear_values", "linear_query"):
                    d[a + lin + ".weight"][c] = 0.0
                d[a + "linear_query.bias"][c] = 0.0
                d[a + "final_linear.weight"][:, c] = 0.0
                for lin, w in (("linear_keys", "k"), ("linear_values", "v")):
                    which = ("self_" if att == "self_attn" else "mem_") + w
                    d[a + lin + ".bias"][c] = 0.0 if zero_bias else torch.from_numpy(rows[(l, h, which)])
    return d


def make_engine(ckpt_enc, dec, form):
    from molnextr_amd.engine import Engine
    max_len, tile, fmax, mmax = FORMS[form]
    keys = {"MNX_DEC_TILE": str(tile), "MNX_DEC_FUSED_MAX": str(fmax), "MNX_DEC_MID_MAX": str(mmax)}
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        return Engine(ckpt_enc, dec, device=0, max_batch=1, dec_slots=SLOTS, max_len=max_len, dtype="fp32")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    return KQ.boundary_case()


def _batch(case, max_len, dev):
    """the boundary rows an engine of max_len holds (the 512 row only at 512: it is the last row, so dropping it changes no
    other row's PE rank) as (features, forced ids [B, max_len], lengths)"""
    feats, ids, lens = case
    B = sum(n <= max_len for n in lens)
    return feats[:B].contiguous().to(dev), ids[:B, :max_len].to(torch.int32).contiguous().to(dev), lens[:B]


def _forced(eng, case, dev):
    f, ids, lens = _batch(case, eng.max_len, dev)
    out = eng.decode_forced(f, ids, max_len=eng.max_len, trace_logits=True)
    torch.cuda.synchronize()
    assert out["lengths"].cpu().tolist() == lens
    return out["logits"].cpu().double().permute(1, 0, 2), lens          # [B, max_len, V]


def _blocks(eng, which, owners, heads, dev):
    """[layer][owner][head] raw blocks (uint8 on the device)"""
    nk = KQ.rows(eng.max_len if which.startswith("self") else S)
    buf = torch.empty(L, len(owners), len(heads), nk * KQ.ROW_BYTES, dtype=torch.uint8, device=dev)
    for l in range(L):
        for i, o in enumerate(owners):
            for j, h in enumerate(heads):
                eng.kv_block(which, l, o, h, out=buf[l, i, j])
    torch.cuda.synchronize()
    return buf, nk


def _check_cache(eng, rows, lens, dev):
    """the stored bits of every crafted row, the zero bytes of everything no writer may have touched"""
    B, n_mem_blocks = len(lens), SLOTS
    for which in WHICH:
        self_ = which.startswith("self")
        buf, nk = _blocks(eng, which, range(SLOTS if self_ else n_mem_blocks), range(H), dev)
        assert not buf[:, B:].any(), f"{which}: a slot / memory block at or past B = {B} was written"
        if self_:   # positions at or past a row's length: hi, lo and scale bytes still zero
            for b, n in enumerate(lens):
                blk = buf[:, b]
                for lo_, hi_ in ((n * 64, nk * 64), (nk * 64 + n * 32, nk * 96), (nk * 96 + n * 4, nk * 100)):
                    assert not blk[..., lo_:hi_].any(), f"{which} slot {b} (length {n}): bytes {lo_}..{hi_} written"
        host = buf[:, :B].cpu().numpy()
        bad = []
        for l in range(L):
            for h in crafted_heads(l):
                v = rows[(l, h, which)]
                want_q, want_s = KQ.quant(v)
                finite = bool(np.isfinite(v).all())
                for b, n in enumerate(lens):
                    q, sc = KQ.parse_block(host[l, b, h], nk)
                    m = n if self_ else S
                    q, sc = q[:m], sc[:m]
                    if finite:
                        ok = (q == want_q).all() and (sc == want_s).all()
                    else:   # what kvq.h documents for non-finite rows, nothing more
                        ok = np.isfinite(sc).all() and (q[:, np.isnan(v)] == -2 ** 23).all()
                    if not ok:
                        pos = np.nonzero((q != want_q).any(-1) | (sc != want_s))[0]
                        p0 = int(pos[0])
                        bad.append((which, l, h, b, n, f"{len(pos)} positions from {p0}: q {q[p0, :4].tolist()} scale "
                                    f"{sc[p0]!r}, want {want_q[:4].tolist()} {want_s!r}"))
        assert not bad, f"{len(bad)} crafted (which, layer, head, owner, length) rows differ from kvq_quant, first {bad[:6]}"


@pytest.fixture(scope="module")
def crafted(synth_ckpt):
    rows = crafted_rows()
    return rows, crafted_decoder(synth_ckpt["decoder"], rows), crafted_decoder(synth_ckpt["decoder"], rows, zero_bias=True)


@pytest.mark.parametrize("form", ["fused", "tile0", "mid", "len512"])
def test_every_writer_stores_kvq_quant_bit_for_bit(form, synth_ckpt, crafted, case, dev):
    """dec_fa (fused), dec_linear EPI 0 (tile0, len512), dec_ma (mid), and kvq_pack on every engine: the crafted heads' rows
    equal the host restatement bit for bit at every (layer, K / V, slot, position < length) and in all 144 rows of every
    memory block; on a fresh engine nothing at or past a row's length, no slot and no memory block at or past B is written;
    and the logits equal those of the same checkpoint with the crafted K / V biases zero (the crafted rows are isolated)."""
    rows, dec, dec0 = crafted
    t0 = time.time()
    eng = make_engine(synth_ckpt["encoder"], dec, form)
    try:
        lg, lens = _forced(eng, case, dev)
        _check_cache(eng, rows, lens, dev)
    finally:
        eng.close()
    eng = make_engine(synth_ckpt["encoder"], dec0, form)
    try:
        lg0, lens0 = _forced(eng, case, dev)
    finally:
        eng.close()
    assert lens == lens0
    for b, n in enumerate(lens):
        assert torch.isfinite(lg[b, :n]).all(), f"row {b}: a non-finite crafted row reached the logits"
        assert torch.equal(lg[b, :n], lg0[b, :n]), f"row {b}: the crafted heads' K / V rows change the logits"
    print(f"{form}: {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def oracle_logits(synth_ckpt, case):
    feats, ids, lens = case
    return OD.forced_decode(feats, synth_ckpt["decoder"], ids, lens)


@pytest.mark.parametrize("form", ["fused_r4", "fused_r2", "mid", "tile0", "len512"])
def test_logits_match_float64_at_every_key_boundary(form, synth_ckpt, case, oracle_logits, dev):
    """decode_forced's raw logits at every (row, step < length) against the float64 oracle, rows of 2, 31, 32, 33, 160, 161,
    256, 257 and 511 (and 512) steps: 32-key value blocks, the end of the value prefetch, the second key per thread, a full
    score array. Tolerance: the module docstring."""
    t0 = time.time()
    eng = make_engine(synth_ckpt["encoder"], synth_ckpt["decoder"], form)
    try:
        lg, lens = _forced(eng, case, dev)
    finally:
        eng.close()
    ref = oracle_logits[:len(lens)]
    tol = KQ.logit_tolerance(ref)
    unit = tol / KQ.LOGIT_TOL_C
    worst, where = 0.0, None
    for b, n in enumerate(lens):
        e = (lg[b, :n] - ref[b, :n]).abs().amax(-1)
        s = int(e.argmax())
        if float(e[s]) > worst:
            worst, where = float(e[s]), (b, s)
    print(f"{form}: max |logit - float64| = {worst:.3e} = {worst / unit:.1f} u M at (row, step) {where}; tol {tol:.3e} "
          f"({KQ.LOGIT_TOL_C} u M); {time.time() - t0:.1f} s")
    assert worst <= tol, (form, worst, tol, where)


def test_kv_block_rejects_out_of_range_arguments(synth_ckpt, dev):
    """mnx_kv_block: every index is checked against the engine's sizes; MNX_ERR_INVALID_ARG with a message, nothing copied"""
    from molnextr_amd.engine import MnxError
    eng = make_engine(synth_ckpt["encoder"], synth_ckpt["decoder"], "len512")
    try:
        out = torch.zeros(KQ.rows(512) * KQ.ROW_BYTES, dtype=torch.uint8, device=dev)
        eng.kv_block("self_k", L - 1, SLOTS - 1, H - 1, out=out)
        eng.kv_block("mem_v", L - 1, SLOTS - 1, H - 1, out=out)
        torch.cuda.synchronize()
        for which, layer, owner, head in ((4, 0, 0, 0), (-1, 0, 0, 0), (0, L, 0, 0), (1, -1, 0, 0), (0, 0, SLOTS, 0),
                                          (2, 0, SLOTS, 0), (3, 0, -1, 0), (0, 0, 0, H), (2, 0, 0, -1)):
            rc = eng.lib.mnx_kv_block(eng.h, which, layer, owner, head, out.data_ptr(), None)
            assert rc == -1, (which, layer, owner, head, rc)
            assert eng.lib.mnx_last_error(eng.h).startswith(b"mnx_kv_block: ")
        assert eng.lib.mnx_kv_block(eng.h, 0, 0, 0, 0, None, None) == -1
        with pytest.raises(MnxError):
            eng.kv_block("self_v", 0, SLOTS, 0, out=out)
    finally:
        eng.close()
