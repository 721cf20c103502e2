"""CPU: what tests/test_gpu_dec_linear.py judges dec_linear_kernel with (tests/dec_linear_ref.py derives it) is neither vacuous
nor tight, shown on the GPU test's own shapes before a kernel is ever judged:
  * the fp32 restatement of every form (two-pass LayerNorm, torch's fp32 matmul, fp32 erf-GELU, oracle.kvq's quantiser) stays
    within its tolerance of the float64 reference;
  * each named wrong variant leaves it: eps 1e-5 on the low-variance row, the unbiased variance, the last K chunk dropped,
    the bias in every slice or in none, the 32^-1/2 scale omitted, a tanh GELU;
  * torch's fp32 0.5 x (1 + erf(x / sqrt 2)) stays inside the GELU arithmetic bound over [-6, 6], cancelling tail included, and
    the tanh form does not;
  * the crafted hand-over partials tell the summation orders apart in at least half of the elements, the probes reach every
    residue mod 256 and every 256-chunk, and the scripts make row index, slot and PE rank three different numbers.
Nothing here loads the library.
"""
import numpy as np
import pytest
import torch

import dec_linear_ref as L
import encoder_ops_ref as R
from molnextr_amd import weights as W

M = max(c for c, _ in L.TICKS)          # the rows of the largest tick; every smaller tick is a prefix of it


def _case(pro, N, K):
    Wt, bias, gamma, beta = L.weights(N, K)
    if pro == 0:
        x, res = L.plain_rows(M, K)
        return x, res[:, :N], Wt, bias, gamma, beta
    return L.stream_rows(M), None, Wt, bias, gamma, beta


def _apply(epi, z32, res):
    if epi == 1:
        return res + z32
    if epi == 2:
        return z32 * torch.tensor(L.SCALE32)
    return L.gelu_fp32(z32)


@pytest.mark.parametrize("pro,epi,N,K", [(p, e, n, k) for (p, e) in L.FORMS if e in (1, 2, 3) for (n, k) in L.FORM_SHAPES[(p, e)]])
def test_store_forms_have_margin_and_power(pro, epi, N, K):
    x, res, Wt, bias, gamma, beta = _case(pro, N, K)
    z, tz = L.product_ref(pro, x, Wt, bias, gamma, beta)
    ref, tol = L.epilogue_ref(epi, z, tz, res)
    assert torch.isfinite(tol).all() and (tol > 0).all()
    r = L.ratio(_apply(epi, L.product_fp32(pro, x, Wt, bias, gamma, beta), res), ref, tol)
    print(f"<{pro},{epi}> ({N}, {K}): fp32 restatement at {r:.3f} of tol")
    assert r <= 1.0, r
    wrong = {}
    if pro:
        wrong["eps 1e-5"] = _apply(epi, L.product_fp32(pro, x, Wt, bias, gamma, beta, eps=1e-5), res)
        o = R.ln_reference(x, gamma, beta, eps=L.LN_EPS, ddof=1)[0]
        wrong["unbiased variance"] = _apply(epi, (o @ Wt.double().t() + bias.double()).float(), res)
    if K > 256:
        wrong["last K chunk dropped"] = _apply(epi, x[:, :K - 256] @ Wt[:, :K - 256].t() + bias, res)
    if epi == 2:
        wrong["scale omitted"] = L.product_fp32(pro, x, Wt, bias, gamma, beta)
    if epi == 3:
        wrong["tanh GELU"] = L.gelu_tanh(L.product_fp32(pro, x, Wt, bias, gamma, beta))
    for name, got in wrong.items():
        w = L.ratio(got, ref, tol)
        print(f"<{pro},{epi}> ({N}, {K}): {name} at {w:.1f} tol")
        assert w > 1.0, (name, w)
    if pro:      # the eps mutant is caught ON the low-variance row (row 1 of stream_rows), the row it is about
        w = L.ratio(wrong["eps 1e-5"][1], ref[1], tol[1])
        assert w > 1.0, w


@pytest.mark.parametrize("pro", [1, 2])
def test_qkv_scatter_has_margin_and_power(pro):
    """EPI 0: q within the scaled bound, the K / V rows as the cache gives them back within bound + quantum. PRO 2's stream is
    x0 = emb * 16 + pe of the synthetic checkpoint under the largest script."""
    N, K = L.FORM_SHAPES[(pro, 0)][0]
    Wt, bias, gamma, beta = L.weights(N, K)
    if pro == 1:
        x = L.stream_rows(M)
    else:
        dec = W.DecoderDims()
        sd = W.synthetic_checkpoint(0, enc=W.EncoderDims(img_size=96, embed_dim=32, depths=(2, 2), heads=(1, 2)),
                                    dec=W.DecoderDims(enc_dim=64))["decoder"]
        p = "decoder.chartok_coords.embeddings.make_embedding."
        ent, rank = L.row_view(L.script(65, dec.vocab))
        x = torch.from_numpy(L.embed_stream(sd[p + "emb_luts.0.weight"].numpy(), sd[p + "pe.pe"].numpy(), ent[:, 2], rank))
    z, tz = L.product_ref(pro, x, Wt, bias, gamma, beta)
    q, tq, kv, tkv = L.qkv_ref(z, tz)
    z32 = L.product_fp32(pro, x, Wt, bias, gamma, beta)
    r = max(L.ratio(z32[:, :256] * torch.tensor(L.SCALE32), q, tq), L.ratio(L.kv_fp32(z32[:, 256:]), kv, tkv))
    print(f"<{pro},0>: fp32 restatement at {r:.3f} of tol")
    assert r <= 1.0, r
    assert L.ratio(z32[:, :256], q, tq) > 1.0                                  # scale omitted
    o = R.ln_reference(x, gamma, beta, eps=L.LN_EPS, ddof=1)[0]
    z_unb = (o @ Wt.double().t() + bias.double()).float()
    assert L.ratio(L.kv_fp32(z_unb[:, 256:]), kv, tkv) > 1.0 and L.ratio(z_unb[:, :256] * L.SCALE32, q, tq) > 1.0
    z_eps = L.product_fp32(pro, x, Wt, bias, gamma, beta, eps=1e-5)
    if pro == 1:                                                               # (x0 has no low-variance row)
        assert L.ratio(L.kv_fp32(z_eps[1:2, 256:]), kv[1:2], tkv[1:2]) > 1.0
    # a 16-bit cache (fp16 values) is outside the bound + quantum: the quantum term is not what lets things through
    assert L.ratio(z32[:, 256:].half().float(), kv, tkv) > 1.0


def test_slices_have_margin_and_power():
    """EPI 4: every plane within the slice bound; the bias in every slice, in none, and a dropped last chunk are outside"""
    N, K = L.FORM_SHAPES[(0, 4)][0]
    x, _, Wt, bias, _, _ = _case(0, N, K)
    ref, tol = L.slice_ref(x, Wt, bias)
    assert ref.shape == (K // 256, M, N)
    honest = torch.stack([x[:, k:k + 256] @ Wt[:, k:k + 256].t() + (bias if k == 0 else 0.0) for k in range(0, K, 256)])
    r = L.ratio(honest, ref, tol)
    print(f"<0,4>: fp32 restatement at {r:.3f} of tol")
    assert r <= 1.0, r
    every = honest.clone()
    every[1:] += bias
    none = honest.clone()
    none[0] -= bias
    dropped = honest.clone()
    dropped[-1] = 0.0
    for name, got in (("bias in every slice", every), ("bias in no slice", none), ("last K chunk dropped", dropped)):
        w = L.ratio(got, ref, tol)
        print(f"<0,4>: {name} at {w:.1f} tol")
        assert w > 1.0, (name, w)
    # and the planes add up to the unsplit product within its bound
    z, tz = R.sgemm_tol(x, Wt, bias)
    assert L.ratio(honest.double().sum(0), z, tz) <= 1.0


def test_gelu_bound_admits_erf_and_refuses_tanh():
    z = torch.cat([torch.linspace(-6.0, 6.0, 48001), torch.linspace(-6.0, -3.0, 12001)]).float()
    ref, tol = L.gelu64(z.double()), L.gelu_arith_tol(z.double())
    r = L.ratio(L.gelu_fp32(z), ref, tol)
    tail = z < -3
    rt = L.ratio(L.gelu_fp32(z)[tail], ref[tail], tol[tail])
    print(f"fp32 erf-GELU at {r:.3f} of its arithmetic bound over [-6, 6], {rt:.3f} in the tail z < -3")
    assert r <= 1.0 and rt <= 1.0
    w = L.ratio(L.gelu_tanh(z), ref, tol)
    print(f"tanh GELU at {w:.0f}")
    assert w > 10.0
    assert abs(L.SCALE32 - 0.17677669529663687) < 2.0 ** -27 and np.float32(0.17677669529663687) == np.float32(L.SCALE32)
    # sup |gelu'| is below GELU_SLOPE
    zz = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    slope = 0.5 * (1 + torch.erf(zz / 2 ** 0.5)) + zz * torch.exp(-zz * zz / 2) / (2 * np.pi) ** 0.5
    assert 1.12 < slope.abs().max().item() < L.GELU_SLOPE


def test_integer_families_are_exact_and_the_probes_cover_k():
    for N, K in ((256, 256), (256, 1024)):
        Wt, bias = L.int_weights(N, K)
        x, res = L.int_rows(M, K, N)
        assert x.abs().max() <= 7 and Wt.abs().max() <= 7 and Wt.abs().min() >= 1 and bias.abs().max() <= 100
        want = L.int_product(x, Wt, bias)
        # fp32 in two different orders of summation gives the same words
        fwd = (x @ Wt.t() + bias)
        rev = (x.flip(1) @ Wt.flip(1).t() + bias)
        assert torch.equal(fwd, want) and torch.equal(rev, want)
        planes = L.int_slices(x, Wt, bias)
        assert torch.equal(planes.sum(0), want) and planes.shape == (K // 256, M, N)
        seen = set()
        for base in L.PROBE_BASES:
            k = L.probe_k(64, K, base)
            p = L.probe_rows(64, K, base)
            assert ((p != 0).sum(1) == 1).all() and (p[torch.arange(64), torch.from_numpy(k)] != 0).all()
            seen.update(k.tolist())
            got = L.int_product(p, Wt, bias)
            # a swapped chunk (k + 256 mod K) or a neighbouring k-slot changes words of every probe row
            for shift in ([1, 4, 16, 64] + ([256, 512] if K > 256 else [])):
                moved = L.int_product(torch.roll(p, shift, dims=1), Wt, bias)
                assert (moved != got).any(1).all(), (K, base, shift)
        assert {k % 256 for k in seen} == set(range(256)) and {k // 256 for k in seen} == set(range(K // 256))


def test_handover_partials_tell_the_orders_apart():
    parts, x = L.handover_crafted(M)
    want = L.handover_chain(parts, x)
    assert np.isfinite(want).all() and parts.dtype == np.float32 and want.dtype == np.float32
    assert (np.abs(parts) >= 2.0 ** 20).mean() > 0.3 and (np.abs(parts) <= 64).mean() > 0.3
    for name, f in L.HANDOVER_WRONG.items():
        frac = (f(parts, x) != want).mean()
        print(f"{name}: differs in {frac:.2f} of the elements")
        assert frac >= 0.5, (name, frac)
    # random partials: the chain is what float64 gives within four roundings, and zero partials leave the crafted rows alone
    p, s = L.part_rows(M), L.stream_rows(M)
    chain = L.handover_chain(p.numpy(), s.numpy())
    exact = p.double().sum(0) + s.double()
    assert (torch.from_numpy(chain).double() - exact).abs().max() <= 4 * 2.0 ** -24 * (p.double().abs().sum(0) + s.double().abs()).max()
    assert np.array_equal(chain[:4].view(np.int32), s[:4].numpy().view(np.int32))


def test_embed_stream_is_one_rounding_either_way():
    g = np.random.default_rng(3)
    emb, pe = g.standard_normal((50, 256)).astype(np.float32), g.standard_normal((70, 256)).astype(np.float32)
    tok, rank = g.integers(0, 50, 65), g.integers(0, 70, 65)
    x0 = L.embed_stream(emb, pe, tok, rank)
    fma = (emb[tok].astype(np.float64) * 16.0 + pe[rank].astype(np.float64)).astype(np.float32)     # one rounding of the exact value
    assert x0.dtype == np.float32 and np.array_equal(x0.view(np.int32), fma.view(np.int32))


@pytest.mark.parametrize("capacity,n_alive", L.TICKS)
def test_scripts_separate_row_slot_and_rank(capacity, n_alive):
    vocab = W.DecoderDims().vocab
    for with0 in (False, True):
        rows = L.script(n_alive, vocab, with_slot0=with0)
        assert rows.shape == (n_alive, 4) and n_alive <= capacity <= L.DEC_SLOTS and capacity % 32 == 0
        assert len(set(rows[:, 0].tolist())) == n_alive and len(set(rows[:, 3].tolist())) == n_alive
        assert rows[:, 0].min() >= (0 if with0 else 1) and rows[:, 0].max() < L.DEC_SLOTS
        assert (rows[:, 1] >= 0).all() and (rows[:, 1] < L.MAX_LEN).all() and (rows[:, 2] < vocab).all() and (rows[:, 3] < 512).all()
        ent, rank = L.row_view(rows)
        assert (np.diff(ent[:, 0]) > 0).all() and sorted(rank.tolist()) == list(range(n_alive))
        if n_alive >= 31:
            r = np.arange(n_alive)
            assert (ent[:, 0] != r).mean() > 0.9 and (rank != r).mean() > 0.9 and (ent[:, 0] != rank).mean() > 0.9
            assert (np.diff(ent[:, 0]) > 1).any() and not np.array_equal(rows[:, 0], ent[:, 0])
