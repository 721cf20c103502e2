"""CPU: the tolerances of tests/test_gpu_encoder_ops.py (tests/encoder_ops_ref.py derives them) are neither vacuous nor
tight, shown before they ever judge a kernel. For every shape of the GPU tests,
  * an honest fp32 restatement of the operation (two-pass LayerNorm, torch's fp32 matmul) stays within HALF the tolerance
    of the float64 reference (measured: LayerNorm <= 0.44 of it at every C, merge <= 0.38, patch embedding <= 0.06,
    SGEMM <= 0.19), and
  * each named wrong variant, restated in float64, lies at least TEN tolerances away on some element (measured: >= 80).
"""
import itertools

import pytest
import torch

import encoder_ops_ref as R


def _ratio(got, ref, tol):
    return ((got.double() - ref).abs() / tol).max().item()


@pytest.mark.parametrize("C", sorted(R.LN_SHAPES))
def test_layernorm_tolerance_has_margin_and_power(C):
    x, g, b = R.ln_inputs(C, max(R.LN_SHAPES[C]))
    ref, tol = R.ln_tol(x, g, b)
    assert torch.isfinite(tol).all() and (tol > 0).all()
    r = _ratio(R.ln_fp32_restatement(x, g, b), ref, tol)
    print(f"C = {C}: fp32 restatement at {r:.3f} of tol")
    assert r <= 0.5, r
    for name, kw in [("eps = 0", dict(eps=0.0)), ("eps = 1e-6", dict(eps=1e-6)), ("variance over C - 1", dict(ddof=1))]:
        w = _ratio(R.ln_reference(x, g, b, **kw)[0], ref, tol)
        print(f"C = {C}: {name} at {w:.0f} tol")
        assert w >= 10, (name, w)


@pytest.mark.parametrize("B,H,W", R.MERGE_SHAPES)
@pytest.mark.parametrize("Cin", R.MERGE_CIN)
def test_merge_tolerance_has_margin_and_power(Cin, B, H, W):
    x, g, b = R.merge_inputs(B, H, W, Cin)
    rows = R.merge_gather(x)
    assert rows.shape == (B * (H // 2) * (W // 2), 4 * Cin)
    ref, tol = R.ln_tol(rows, g, b)
    r = _ratio(R.ln_fp32_restatement(rows, g, b), ref, tol)
    assert r <= 0.5, r
    for i, j in itertools.combinations(range(4), 2):        # every transposition of the concat order
        order = list(R.MERGE_ORDER)
        order[i], order[j] = order[j], order[i]
        w = _ratio(R.ln_reference(R.merge_gather(x, order), g, b)[0], ref, tol)
        assert w >= 10, (order, w)
    # swapped strides (H for W): the gather of the transposed map, where it is a different one
    if H != W:
        w = _ratio(R.ln_reference(R.merge_gather(x.reshape(B, W, H, Cin)), g, b)[0], ref, tol)
        assert w >= 10, w


def test_merge_gather_is_the_oracles_concat():
    """merge_gather restates oracle/swin.py's PatchMerging concat (x0, x1, x2, x3) = (0,0), (1,0), (0,1), (1,1)"""
    x = torch.arange(2 * 4 * 6 * 3, dtype=torch.float32).reshape(2, 4, 6, 3)
    x0, x1, x2, x3 = x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]
    assert torch.equal(R.merge_gather(x), torch.cat([x0, x1, x2, x3], -1).reshape(-1, 12))


@pytest.mark.parametrize("S", R.PE_S)
@pytest.mark.parametrize("C", R.PE_C)
def test_patch_embed_tolerance_has_margin_and_power(C, S):
    w, bias, g, b = R.pe_weights(C)
    img = R.pe_images(2, S)
    ref, tol = R.patch_embed_tol(img, w, bias, g, b)
    assert ref.shape == (2, (S // 4) ** 2, C)
    r = _ratio(R.patch_embed_fp32_restatement(img, w, bias, g, b), ref, tol)
    assert r <= 0.5, r
    wrong = R.patch_embed_tol(img, w.transpose(2, 3).contiguous(), bias, g, b)[0]      # (ky, kx) transposed taps
    assert _ratio(wrong, ref, tol) >= 10


def test_patch_embed_reference_is_the_convolution():
    """the unfold + matmul restatement against torch's own conv2d, and w_t against the layout [48][C]"""
    w, bias, g, b = R.pe_weights(32)
    img = R.pe_images(1, 16)
    z = torch.nn.functional.conv2d(img.double(), w.double(), bias.double(), stride=4).flatten(2).transpose(1, 2)
    mine = R.pe_patches(img).double() @ w.reshape(32, 48).double().t() + bias.double()
    assert (z - mine).abs().max() < 1e-12
    wt = R.pe_w_t(w)
    assert wt.shape == (48, 32) and wt[(1 * 4 + 2) * 4 + 3, 5] == w[5, 1, 2, 3]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", R.SGEMM_SHAPES)
def test_sgemm_tolerance_has_margin_and_power(M, N, K, bias):
    A, W, b = R.sgemm_inputs(M, N, K)
    b = b if bias else None
    ref, tol = R.sgemm_tol(A, W, b)
    got = A @ W.t() + (b if bias else 0.0)
    assert _ratio(got, ref, tol) <= 0.5
    wrong = A.double() @ W.double().roll(1, dims=1).t() + (b.double() if bias else 0.0)     # W read one k off
    assert _ratio(wrong, ref, tol) >= 10
    if bias:                                                                              # the bias left out
        assert _ratio(A.double() @ W.double().t(), ref, tol) >= 10


def test_sgemm_perm_index_is_a_permutation_of_the_documented_layout():
    for (M, N, K), S in R.SGEMM_PERM.items():
        idx = R.sgemm_perm_index(M, N, S)
        assert sorted(idx.flatten().tolist()) == list(range(M * N))
        lay = torch.arange(M * N).reshape(M // S, N // 256, 8, S, 32)       # [M/S][N/256][8][S][32]
        m, n = M - 1, N - 33
        assert lay[m // S, n // 256, (n % 256) // 32, m % S, n % 32] == idx[m, n]


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_split_planes_restate_two_roundings(name):
    """split_planes: hi + lo reproduces v to u^2 (or the fp16 subnormal step), and the cast inputs hold what they claim"""
    td = R.RN16[name]
    u = 2.0 ** -11 if td == torch.float16 else 2.0 ** -8
    x = R.cast_inputs(1024, td)
    x = x[x.abs() < 6e4]
    hi, lo = R.split_planes(x, td)
    err = (hi.double() + lo.double() - x.double()).abs()
    assert (err <= u * u * x.double().abs() + 2.0 ** -25).all()
    sp = R.cast_inputs(1024, torch.float16)
    assert (sp == 0).sum() >= 2 and torch.signbit(sp[1]) and (sp == 65520.0).any()
    assert (sp.to(torch.float16).float() == float("inf")).any()
    sub = sp[(sp != 0) & (sp.abs() < 2.0 ** -14)]
    assert len(sub) >= 4                                                    # fp16 subnormals
    assert R.cast_inputs(4, td).shape == (4,)
