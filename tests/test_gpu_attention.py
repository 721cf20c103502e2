"""GPU (-m gpu): the encoder's window attention by itself (mnx_window_attn) against a float64 restatement of the reference's
WindowAttention, at the four Swin-B stage shapes and in every operand mode; the persistent split kernel at groups whose qkv
planes pass 2^32 bytes; and whole encoder groups at production size (max_batch 512 / 608) against the 32-image engine.

The reference (MolNexTR/models/transformers.py:221-280, oracle/swin.py): roll by -shift, q * 32^-1/2 . k^T, the
relative-position bias, -100 between the shift regions, softmax, . v, roll back. It is fed the kernel's own inputs (in the
split modes the hi + lo planes summed in float64, in the plain modes the 16-bit values), so the only error measured is the
kernel's.

Tolerances. u is the unit roundoff of the operand format (fp16 2^-11, bf16 2^-8, fp32 2^-24) and e = 2^-24 that of the
fp32 arithmetic around it; V = max|v|, A = 32^-1/2 max over (query, key) of sum_i |q_i| |k_i| (a bound on |score| before
the bias), b = max|bias|. An error d_j on score j moves the output by sum_j p_j d_j (v_j - o), at most 2 V max|d|.
  * split modes, terms = 3: the products drop only kl.ql (|d| <= u^2 A on a score), vl.pl (<= u^2 V on an output); P and
    the output leave as hi + lo planes, whose residuals are <= u^2 p and u^2 |o|. fp32: n_s = 6 roundings on a score of
    magnitude <= A + b + 1 (3 MFMA accumulations, scale, bias, exponent argument), n_o = 58 on an output (15 MFMA
    accumulations, the 144-term sum, exponential, normalisation):
        tol3 = V [(2A + 4) u^2 + (2 n_s (A + b + 1) + n_o) e]
  * split modes, terms = 1 (kh.qh and vh.ph alone): |d| <= 2uA per score, the dropped lo planes of P and v u V each:
        tol1 = V [(4A + 2) u + (2A + 4) u^2 + (8 (A + b + 1) + 48) e]
  * plain modes (window_attn_kernel): P and the output are rounded to the operand type (u V each); fp32 as above with the
    16-bit MFMA (1 per score, 5 per output) or eight fp32 MFMA steps per 16-bit one (fp32 mode):
        tol = V [2u + (2 n_s (A + b + 1) + n_o) e],  n_s = 4, n_o = 48 (fp16 / bf16);  n_s = 11, n_o = 83 (fp32)
The split inputs carry lo planes of nearly half an ulp of hi (the largest a split can hold), with hi's sign: on them a
dropped lo term moves every output coherently, and the terms = 1 error must exceed tol3 tenfold (the tests check it), so
a kernel that loses a lo term cannot pass.
"""
import pytest
import torch

from molnextr_amd import weights as W
from oracle.swin import from_windows, relative_position_index, shift_region_ids, to_windows

pytestmark = pytest.mark.gpu

WS, HD = 12, 32
EPS = 2.0 ** -24
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
OPERAND = {"fp16x3": torch.float16, "bf16x3": torch.bfloat16, "fp16": torch.float16, "bf16": torch.bfloat16,
           "fp32": torch.float32}
SPLIT = ("fp16x3", "bf16x3")
# (H, W, heads) of the four Swin-B stages at 384^2, and a non-square grid (nWh = 3, nWw = 5: swapped window counts show)
STAGES = [(96, 96, 4), (48, 48, 8), (24, 24, 16), (12, 12, 32)]
SHAPES = STAGES + [(36, 60, 4)]
FORCE_SPLIT = 0x100        # mnx_window_attn: window_attn_split_kernel at terms = 3
TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    """One small engine per compute dtype: mnx_window_attn uses nothing of an engine but its compute dtype."""
    from molnextr_amd.engine import Engine
    dec = W.DecoderDims(enc_dim=TINY.num_features)
    ck = W.synthetic_checkpoint(0, enc=TINY, dec=dec)
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Engine(ck["encoder"], ck["decoder"], max_batch=2, enc=TINY, dec=dec, dtype=dtype, dec_slots=64)
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _full_lo(hi):
    """lo plane of nearly half an ulp of hi (0.499 ulp, hi's sign): hi + lo still rounds to hi."""
    td = hi.dtype
    p = 11 if td == torch.float16 else 8
    _, e = torch.frexp(hi.float())
    ulp = torch.ldexp(torch.ones_like(hi, dtype=torch.float32), e - p)
    if td == torch.float16:
        ulp = ulp.clamp(min=2.0 ** -24)
    lo = (0.499 * ulp * torch.sign(hi.float())).to(td).float()
    if td == torch.float16:     # a subnormal lo may round up to half an ulp: one subnormal step back
        lo = torch.where(lo.abs() >= 0.5 * ulp, lo - torch.sign(lo) * 2.0 ** -24, lo)
    return lo.to(td)


def _fill(dst, n_rows, C, td, split, seed):
    """qkv rows into dst ([2, n_rows, 3C] split, [n_rows, 3C] plain): q, k ~ N(0, 0.25), v ~ N(0, 1)."""
    g = torch.Generator(device=dst.device).manual_seed(seed)
    step = 1 << 16
    sd = torch.tensor([0.5] * (2 * C) + [1.0] * C, device=dst.device)
    for r0 in range(0, n_rows, step):
        r1 = min(n_rows, r0 + step)
        x = torch.randn(r1 - r0, 3 * C, generator=g, device=dst.device) * sd
        hi = x.to(td)
        if split:
            dst[0, r0:r1] = hi
            dst[1, r0:r1] = _full_lo(hi)
        else:
            dst[r0:r1] = hi


def _table(heads, seed, dev):
    g = torch.Generator().manual_seed(seed)
    # bias ~ N(0, 9): sharp attention rows, through which a dropped lo plane of v reaches the output nearly undamped
    return (3.0 * torch.randn((2 * WS - 1) ** 2, heads, generator=g)).to(dev)


def _values(qkv, split):
    """The kernel's inputs as float64 [rows, 3C]"""
    return (qkv[0].double() + qkv[1].double()) if split else qkv.double()


# ---- float64 reference ----------------------------------------------------------------------------------------------
def _windows(x, B, H, Wd, heads, shift):
    """[B*H*Wd, C] -> [B*nW, heads, 144, 32] of the rolled map"""
    x = x.reshape(B, H, Wd, -1)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = to_windows(x, WS)
    return xw.reshape(xw.shape[0], WS * WS, heads, HD).permute(0, 2, 1, 3)


def reference(qkv64, table, B, H, Wd, heads, shift):
    """float64 WindowAttention on [B*H*Wd, 3C] -> ([B*H*Wd, C], A, V, b) with the bounds of the module docstring"""
    C = heads * HD
    q, k, v = (_windows(qkv64[:, i * C:(i + 1) * C], B, H, Wd, heads, shift) for i in range(3))
    s = (q * HD ** -0.5) @ k.transpose(-2, -1)
    A = ((q.abs() * HD ** -0.5) @ k.abs().transpose(-2, -1)).max().item()
    t = table.double()
    s = s + t[relative_position_index(WS).reshape(-1).to(t.device)].reshape(WS * WS, WS * WS, heads).permute(2, 0, 1)
    if shift:
        rid = to_windows(shift_region_ids(H, Wd, WS, shift).reshape(1, H, Wd, 1).double(), WS)[..., 0].to(s.device)
        mask = torch.where(rid[:, None, :] != rid[:, :, None], -100.0, 0.0)        # [nW, 144, 144]
        nW = mask.shape[0]
        s = (s.reshape(B, nW, heads, WS * WS, WS * WS) + mask[None, :, None]).reshape(s.shape)
    o = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(-1, WS * WS, C)
    o = from_windows(o, WS, B, H, Wd)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B * H * Wd, C), A, v.abs().max().item(), t.abs().max().item()


def tolerance(kind, td, A, V, b):
    u = UNIT[td]
    if kind == "split3":
        return V * ((2 * A + 4) * u * u + (12 * (A + b + 1) + 58) * EPS)
    if kind == "split1":
        return V * ((4 * A + 2) * u + (2 * A + 4) * u * u + (8 * (A + b + 1) + 48) * EPS)
    ns, no = (11, 83) if td == torch.float32 else (4, 48)
    return V * (2 * u + (2 * ns * (A + b + 1) + no) * EPS)


def _run(e, dtype, qkv, table, B, H, Wd, heads, shift, terms):
    C = heads * HD
    M = B * H * Wd
    if dtype in SPLIT:
        out = torch.full((2, M, C), float("nan"), device=qkv.device, dtype=OPERAND[dtype])
        e.window_attn(qkv, table, out, B, H, Wd, heads, shift, terms=terms, qkv_lo=M * 3 * C, out_lo=M * C)
        torch.cuda.synchronize()
        return out
    out = torch.full((M, C), float("nan"), device=qkv.device, dtype=OPERAND[dtype])
    e.window_attn(qkv, table, out, B, H, Wd, heads, shift, terms=1)
    torch.cuda.synchronize()
    return out


def _inputs(dtype, B, H, Wd, heads, seed, dev):
    C, M = heads * HD, B * H * Wd
    split = dtype in SPLIT
    qkv = torch.empty((2, M, 3 * C) if split else (M, 3 * C), device=dev, dtype=OPERAND[dtype])
    _fill(qkv, M, C, OPERAND[dtype], split, seed)
    return qkv, _table(heads, seed, dev)


# ---- every mode, every stage shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("H,Wd,heads", SHAPES)
@pytest.mark.parametrize("dtype", SPLIT)
def test_split_window_attention_vs_float64_reference(engines, dev, dtype, H, Wd, heads, shift):
    """fp16x3 / bf16x3: the persistent kernel (terms = 3; the masked and unmasked instantiations when shift > 0) within
    tol3 of the reference; the non-persistent kernel at terms = 3 bit for bit equal to it; at terms = 1 within tol1, and
    at least 10 x tol3 away (a dropped lo term cannot pass)."""
    B = 3 if H * Wd <= 48 * 48 else 2
    e = engines(dtype)
    td = OPERAND[dtype]
    qkv, table = _inputs(dtype, B, H, Wd, heads, 1000 * H + Wd + heads + shift, dev)
    ref, A, V, b = reference(_values(qkv, True), table, B, H, Wd, heads, shift)
    pipe = _run(e, dtype, qkv, table, B, H, Wd, heads, shift, 3)
    err3 = (pipe[0].double() + pipe[1].double() - ref).abs().max().item()
    tol3 = tolerance("split3", td, A, V, b)
    assert err3 <= tol3, (err3, tol3, A, V, b)
    split3 = _run(e, dtype, qkv, table, B, H, Wd, heads, shift, 3 | FORCE_SPLIT)
    assert torch.equal(pipe.view(torch.int16), split3.view(torch.int16)), \
        "window_attn_pipe_kernel and window_attn_split_kernel differ at terms = 3"
    one = _run(e, dtype, qkv, table, B, H, Wd, heads, shift, 1)
    err1 = (one[0].double() + one[1].double() - ref).abs().max().item()
    assert err1 <= tolerance("split1", td, A, V, b), (err1, A, V, b)
    assert err1 >= 10 * tol3, f"terms = 1 error {err1:.3e} is not 10 x the terms = 3 tolerance {tol3:.3e}"


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("H,Wd,heads", SHAPES)
@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_plain_window_attention_vs_float64_reference(engines, dev, dtype, H, Wd, heads, shift):
    B = 3 if H * Wd <= 48 * 48 else 2
    qkv, table = _inputs(dtype, B, H, Wd, heads, 7 * H + Wd + heads + shift, dev)
    ref, A, V, b = reference(_values(qkv, False), table, B, H, Wd, heads, shift)
    out = _run(engines(dtype), dtype, qkv, table, B, H, Wd, heads, shift, 1)
    err = (out.double() - ref).abs().max().item()
    tol = tolerance("plain", OPERAND[dtype], A, V, b)
    assert err <= tol, (err, tol, A, V, b)


def test_window_attention_rejects_bad_arguments(engines, dev):
    from molnextr_amd.engine import MnxError
    H = Wd = 24
    heads = 16
    qkv, table = _inputs("fp16x3", 1, H, Wd, heads, 5, dev)
    e = engines("fp16x3")
    M, C = H * Wd, heads * HD
    out = torch.zeros(2, M, C, device=dev, dtype=torch.float16)
    good = dict(qkv_lo=M * 3 * C, out_lo=M * C)
    for kw, words in [(dict(terms=2), "terms"), (dict(terms=1 | FORCE_SPLIT), "terms"), (dict(shift=12), "shift"),
                      (dict(H=30), "multiples"), (dict(qkv_lo=M * 3 * C - 8), "qkv_lo"), (dict(out_lo=0), "out_lo"),
                      (dict(heads=8), "head_dim")]:
        a = dict(B=1, H=H, Wd=Wd, heads=heads, shift=0, terms=3, **good)
        a.update(kw)
        with pytest.raises(MnxError, match=words) as ex:
            if "heads" in kw:       # C = heads * 32 is derived by the wrapper: call the ABI with a mismatched C
                rc = e.lib.mnx_window_attn(e.h, qkv.data_ptr(), a["qkv_lo"], table.data_ptr(), out.data_ptr(), a["out_lo"],
                                           1, H, Wd, C, 8, 0, 3, None)
                e._check(rc, "mnx_window_attn")
            else:
                e.window_attn(qkv, table, out, a["B"], a["H"], a["Wd"], a["heads"], a["shift"], terms=a["terms"],
                              qkv_lo=a["qkv_lo"], out_lo=a["out_lo"])
        assert ex.value.code == -1
    with pytest.raises(MnxError, match="terms"):            # plain engines take terms = 1 only
        engines("fp16").window_attn(qkv[0], table, out[0], 1, H, Wd, heads, 0, terms=3)
    assert torch.count_nonzero(out) == 0                      # nothing ran


# ---- groups past 4 GiB of qkv plane ---------------------------------------------------------------------------------
BIG_B = 608                        # Swin-B stage 1: 7 077 888 bytes of qkv plane per image; 2^32 falls inside image 606
BIG_IMAGES = [0, 302, 303, 304, 605, 606, 607]
H1, W1, HEADS1 = STAGES[0]


@pytest.fixture(scope="module", params=SPLIT)
def big_group(request, dev):
    """stage-1 qkv planes of BIG_B images (4.30 GB each), filled on the device"""
    dtype = request.param
    C, M = HEADS1 * HD, BIG_B * H1 * W1
    qkv = torch.empty((2, M, 3 * C), device=dev, dtype=OPERAND[dtype])
    assert qkv[0].numel() * qkv.element_size() > 2 ** 32
    _fill(qkv, M, C, OPERAND[dtype], True, 4242)
    yield dtype, qkv, _table(HEADS1, 4242, dev)
    del qkv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shift", [0, 6])
def test_window_attention_group_past_4gib(engines, dev, big_group, shift):
    """B = 608 at the stage-1 shape: images 0, 302-304 and 605-607 (around 2^31 and 2^32 bytes of qkv plane) within tol3
    of the float64 reference, and bit for bit equal to the same images' output of one B = 8 call."""
    dtype, qkv, table = big_group
    td = OPERAND[dtype]
    C, L = HEADS1 * HD, H1 * W1
    out = _run(engines(dtype), dtype, qkv, table, BIG_B, H1, W1, HEADS1, shift, 3)
    imgs = BIG_IMAGES + [BIG_B // 2 + 1]                      # eight images
    rows = torch.cat([torch.arange(i * L, (i + 1) * L, device=dev) for i in imgs])
    small_in = qkv[:, rows].contiguous()
    big_out = out[:, rows].contiguous()
    del out
    small_out = _run(engines(dtype), dtype, small_in, table, len(imgs), H1, W1, HEADS1, shift, 3)
    differ = [i for j, i in enumerate(imgs)
              if not torch.equal(big_out[:, j * L:(j + 1) * L].view(torch.int16), small_out[:, j * L:(j + 1) * L].view(torch.int16))]
    assert not differ, f"images {differ} of the B = {BIG_B} call differ from the same images in a B = 8 call"
    for j, i in enumerate(BIG_IMAGES):
        ref, A, V, b = reference(_values(small_in[:, j * L:(j + 1) * L], True), table, 1, H1, W1, HEADS1, shift)
        got = big_out[0, j * L:(j + 1) * L].double() + big_out[1, j * L:(j + 1) * L].double()
        err, tol = (got - ref).abs().max().item(), tolerance("split3", td, A, V, b)
        assert err <= tol, (i, err, tol)


# ---- whole encoder groups at production size ------------------------------------------------------------------------
def _group_images(n):
    """n images from 64 synthetic ones, mirrored in every other block of 64 (128 distinct); image i is a function of i"""
    base = W.synthetic_images(64, first_index=300)
    idx = torch.arange(n)
    imgs = base[idx % 64]
    flip = ((idx // 64) % 2 == 1)
    imgs[flip] = imgs[flip].flip(-1)
    return imgs.contiguous()


@pytest.fixture(scope="module")
def group_images():
    return _group_images(608)


@pytest.fixture(scope="module")
def oracle_features(group_images, synth_ckpt):
    from oracle.swin import encoder_forward
    cache = {}

    def get(i):
        if i not in cache:
            cache[i] = encoder_forward(group_images[i:i + 1], synth_ckpt["encoder"])[0]
        return cache[i]
    return get


@pytest.fixture(scope="module")
def small_features(group_images, synth_ckpt, dev):
    """features of every image from max_batch = 32 engines, 32 images per call (fp16x3 and bf16x3)"""
    from molnextr_amd.engine import Engine
    made = {}

    def get(dtype):
        if dtype not in made:
            e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dec_slots=64, dtype=dtype)
            try:
                made[dtype] = torch.cat([e.encode(group_images[i:i + 32].contiguous().to(dev))
                                         for i in range(0, len(group_images), 32)])
            finally:
                e.close()
        return made[dtype]
    return get


def _workspace_estimate(synth_ckpt, max_batch, dtype):
    """bytes an engine of max_batch images needs: from two small engines, the workspace is affine in max_batch"""
    from molnextr_amd.engine import Engine
    ws = []
    for mb in (32, 64):
        e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=mb, dec_slots=64, dtype=dtype)
        ws.append(e.workspace_bytes)
        e.close()
    return ws[0] + (ws[1] - ws[0]) * (max_batch - 32) // 32


@pytest.mark.parametrize("dtype,max_batch", [("fp16x3", 608), ("bf16x3", 608), ("fp16x3", 512)])
def test_encoder_group_at_production_size_is_bitwise_batch_invariant(dtype, max_batch, group_images, small_features,
                                                                       oracle_features, synth_ckpt, dev):
    """An engine of max_batch 608 (qkv planes past 2^32 bytes) or 512 (bench.py's default group) encodes its whole group in
    one call: every image's features equal, bit for bit, those of the 32-image engine run 32 at a time, and the last
    image's are within the encoder's 5e-5 of the oracle."""
    from molnextr_amd.engine import Engine
    ref = small_features(dtype)[:max_batch]
    need = _workspace_estimate(synth_ckpt, max_batch, dtype) + group_images[:max_batch].numel() * 4 + ref.numel() * 4
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{free / 2**30:.1f} GiB of device memory free, a max_batch={max_batch} engine needs {need / 2**30:.1f} GiB")
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=max_batch, dec_slots=64, dtype=dtype)
    try:
        print(f"{dtype} max_batch={max_batch}: mnx_workspace_bytes {e.workspace_bytes} ({e.workspace_bytes / 2**30:.2f} GiB)")
        f = e.encode(group_images[:max_batch].contiguous().to(dev))
        torch.cuda.synchronize()
    finally:
        e.close()
    differ = [i for i in range(max_batch) if not torch.equal(f[i], ref[i])]
    assert not differ, f"{len(differ)} images differ from the 32-image engine's features, first {differ[:8]}"
    last = max_batch - 1
    err = (f[last].cpu() - oracle_features(last)).abs().max().item()
    assert err < 5e-5, err
