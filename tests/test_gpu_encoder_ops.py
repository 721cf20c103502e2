"""GPU (-m gpu): the encoder's patch embedding, LayerNorm, patch-merging LayerNorm and operand cast, and the decoder's fp32
SGEMM, each by itself on caller buffers (mnx_patch_embed, mnx_layernorm16, mnx_merge_ln16, mnx_cast16, mnx_sgemm_tn) against
a float64 restatement of the reference operation fed the kernel's own fp32 inputs. The restatements, the inputs and the
derivation of every tolerance are in tests/encoder_ops_ref.py; tests/test_encoder_ops_host.py shows on the CPU that each
tolerance leaves an honest fp32 evaluation a factor of two and catches each named wrong variant tenfold.

What is compared how:
  * fp32 results: per element within the derived tolerance of float64.
  * 16-bit results: bit for bit the round-to-nearest-even cast (torch's) of the fp32 result of the same arithmetic — the
    y32 output of the same call (LayerNorm), the FP32 engine's output (merge, which has no fp32 output), the scaled input
    (cast). Split modes: hi == RN16(v) and lo == RN16(v - float(hi)) as 16-bit words, the two-rounding split of ONE fp32
    value (csrc/common.h split16x4); planes = 1 writes the same hi plane and not one byte of the lo plane.
  * every output lies between two guards of 64 elements and is filled with 0x7F bytes before the call: what a call must not
    write (guards, the lo plane at planes = 1, everything after a refused call) is compared with that fill bit for bit.
Each test prints its largest error / tolerance ratio ("ratio <family> <value>": pytest -s shows them;
profiles/encoder_ops_tolerances.json records a run).
"""
import functools
import json

import numpy as np
import pytest
import torch

import encoder_ops_ref as R
from encoder_ops_ref import words
from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu

TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
OUT_T = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "bf16x3": torch.bfloat16,
         "fp16x3": torch.float16}
GUARD = 64
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    """One tiny engine per compute dtype: the entry points use nothing of an engine but its device and compute dtype."""
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
    print("encoder_ops ratios " + json.dumps({k: round(v, 4) for k, v in sorted(RATIOS.items())}))


def _sync():
    torch.cuda.synchronize()


def _note(family, got, ref, tol):
    """largest |got - ref| / tol; printed and kept per kernel family"""
    r = ((got.double() - ref).abs() / tol).max().item()
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"ratio {family} {r:.4f}")
    return r


class Guarded:
    """n elements of dtype td on the device between two guards of 64 elements, every byte 0x7F before the call"""

    def __init__(self, n, td, dev):
        size = torch.empty((), dtype=td).element_size()
        self.raw = torch.full(((n + 2 * GUARD) * size,), 0x7F, dtype=torch.uint8, device=dev)
        self.all = self.raw.view(td)
        self.t = self.all[GUARD:GUARD + n]
        self.fill = {2: 0x7F7F, 4: 0x7F7F7F7F}[size]

    def untouched(self, *written):
        """True when every element outside the (start, length) ranges of .t still holds the fill"""
        w = words(self.all).cpu()
        keep = torch.ones(w.shape, dtype=torch.bool)
        for s, n in written:
            keep[GUARD + s:GUARD + s + n] = False
        return bool((w[keep] == self.fill).all())

    def written(self, s, n):
        """True when no element of the range holds the fill any more (0x7F7F... is no value these tests produce)"""
        return bool((words(self.t[s:s + n]).cpu() != self.fill).all())


def _lo_offset(n):
    """element offset of a lo plane behind a hi plane of n elements: a multiple of 8, and 64 guard elements between them"""
    return (n + 7) // 8 * 8 + GUARD


def _same(a, b):
    return a.shape == b.shape and torch.equal(words(a), words(b))


def _check_planes(dtype, hi, lo, v32, what):
    """the 16-bit output of a kernel against the fp32 value v32 of the same arithmetic, bit for bit"""
    if dtype == "fp32":
        assert _same(hi, v32), f"{what}: the fp32 y16 differs from y32"
        return
    td = OUT_T[dtype]
    want_hi, want_lo = R.split_planes(v32, td)
    bad = (words(hi) != words(want_hi)).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements of the 16-bit (hi) plane are not RN16(y32), first {bad[:4].tolist()}"
    if lo is not None:
        bad = (words(lo) != words(want_lo)).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} elements of the lo plane are not RN16(y32 - hi), first {bad[:4].tolist()}"


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_case(C):
    x, g, b = R.ln_inputs(C, max(R.LN_SHAPES[C]))
    ref, tol = R.ln_tol(x, g, b)
    return x, g, b, ref, tol


def _ln_call(e, dtype, dev, x, g, b, want16=True, want32=True, planes=2, flag=None):
    """one mnx_layernorm16 call on guarded, pre-filled outputs -> (hi, lo or None, y32 or None) on the CPU, [M, C]"""
    M, C = x.shape
    n = M * C
    split = dtype in R.SPLIT
    y_lo = _lo_offset(n) if split else 0
    y16 = Guarded(y_lo + n, OUT_T[dtype], dev) if want16 else None
    y32 = Guarded(n, torch.float32, dev) if want32 else None
    e.layernorm16(x, g, b, y16.t if want16 else None, y32.t if want32 else None, M, C, R.LN_EPS, y_lo=y_lo, planes=planes,
                  flag=flag)
    _sync()
    hi = lo = o32 = None
    if want16:
        two = split and planes == 2
        assert y16.untouched((0, n), *([(y_lo, n)] if two else [])), "mnx_layernorm16 wrote outside its y16 planes"
        assert y16.written(0, n) and (not two or y16.written(y_lo, n)), "mnx_layernorm16 left output elements unwritten"
        hi = y16.t[:n].cpu().reshape(M, C)
        lo = y16.t[y_lo:y_lo + n].cpu().reshape(M, C) if two else None
    if want32:
        assert y32.untouched((0, n)), "mnx_layernorm16 wrote outside y32"
        assert y32.written(0, n)
        o32 = y32.t.cpu().reshape(M, C)
    return hi, lo, o32


@pytest.mark.parametrize("C,M", [(C, M) for C in sorted(R.LN_SHAPES) for M in R.LN_SHAPES[C]])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_layernorm_vs_float64_and_plane_identities(engines, dev, dtype, C, M):
    """layernorm16_kernel at every lane form (32-lane rows, NV = 1, 2, 4, 8), full and partial last quads, row counts around
    the rows per workgroup: y32 within ln_tol of float64; the 16-bit planes the two-rounding split of y32; the calls
    without y32, without y16 and with planes = 1 bit-equal to the full call in everything they write."""
    e = engines(dtype)
    xc, gc, bc, ref, tol = _ln_case(C)
    x, g, b = xc[:M].contiguous().to(dev), gc.to(dev), bc.to(dev)
    hi, lo, o32 = _ln_call(e, dtype, dev, x, g, b)
    r = _note("layernorm", o32, ref[:M], tol[:M])
    assert r <= 1.0, f"y32 is {r:.3f} tolerances from the float64 LayerNorm (C = {C}, M = {M})"
    _check_planes(dtype, hi, lo, o32, f"C = {C}, M = {M}")
    split = dtype in R.SPLIT
    hi_b, lo_b, _ = _ln_call(e, dtype, dev, x, g, b, want32=False)
    assert _same(hi_b, hi) and (not split or _same(lo_b, lo)), "the call without y32 writes other 16-bit planes"
    _, _, o32_c = _ln_call(e, dtype, dev, x, g, b, want16=False)
    assert _same(o32_c, o32), "the call without y16 writes another y32"
    if split:
        for want32 in (True, False):
            hi_p, lo_p, o32_p = _ln_call(e, dtype, dev, x, g, b, want32=want32, planes=1)
            assert lo_p is None and _same(hi_p, hi), "planes = 1 writes another hi plane than planes = 2"
            assert not want32 or _same(o32_p, o32)
    if dtype == "fp16x3":       # outputs of 2^-10: every lo value is an fp16 subnormal
        gs, bs = gc * 2.0 ** -10, bc * 2.0 ** -10
        ref_s, tol_s = R.ln_tol(xc[:M], gs, bs)
        hi_s, lo_s, o32_s = _ln_call(e, dtype, dev, x, gs.to(dev), bs.to(dev))
        assert _note("layernorm", o32_s, ref_s, tol_s) <= 1.0
        _check_planes(dtype, hi_s, lo_s, o32_s, f"gamma, beta x 2^-10, C = {C}, M = {M}")
        assert ((lo_s != 0) & (lo_s.float().abs() < 2.0 ** -14)).any(), "this case is meant to hold subnormal lo values"


@pytest.mark.parametrize("C", [96, 384])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_layernorm_nonfinite_flag(engines, dev, dtype, C):
    """The flag stays 0 on finite rows and is set by a NaN, an Inf or an overflowing variance in row 0 (first half-wave of
    the 32-lane form), 1 (second half-wave) or 8 (the odd tail); the other rows' outputs do not change by one bit."""
    e = engines(dtype)
    M = 9
    xc, gc, bc, _, _ = _ln_case(C)
    g, b = gc.to(dev), bc.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    base = _ln_call(e, dtype, dev, xc[:M].contiguous().to(dev), g, b, flag=flag)
    assert flag.item() == 0, "finite rows set the non-finite flag"
    big = torch.full((C,), 3e38)
    big[1::2] = -3e38
    for kind in ("nan", "inf", "overflow"):
        for r in (0, 1, 8):
            x = xc[:M].clone()
            if kind == "nan":
                x[r, 5 % C] = float("nan")
            elif kind == "inf":
                x[r, C - 1] = float("inf")
            else:
                x[r] = big
            flag.zero_()
            got = _ln_call(e, dtype, dev, x.to(dev), g, b, flag=flag)
            assert flag.item() == 1, f"{kind} in row {r} did not set the flag"
            rows = [i for i in range(M) if i != r]
            for a, c in zip(base, got):
                assert (a is None and c is None) or _same(a[rows], c[rows]), f"{kind} in row {r} changed other rows"


# ---- patch merging + LayerNorm --------------------------------------------------------------------------------------
def _merge_call(e, dtype, dev, x, g, b, B, H, Wd, Cin, planes=2):
    n = B * (H // 2) * (Wd // 2) * 4 * Cin
    split = dtype in R.SPLIT
    y_lo = _lo_offset(n) if split else 0
    y = Guarded(y_lo + n, OUT_T[dtype], dev)
    e.merge_ln16(x, g, b, y.t, B, H, Wd, Cin, R.LN_EPS, y_lo=y_lo, planes=planes)
    _sync()
    two = split and planes == 2
    assert y.untouched((0, n), *([(y_lo, n)] if two else [])), "mnx_merge_ln16 wrote outside its planes"
    assert y.written(0, n) and (not two or y.written(y_lo, n)), "mnx_merge_ln16 left output elements unwritten"
    shape = (n // (4 * Cin), 4 * Cin)
    return y.t[:n].cpu().reshape(shape), (y.t[y_lo:y_lo + n].cpu().reshape(shape) if two else None)


@pytest.mark.parametrize("B,H,Wd", R.MERGE_SHAPES)
@pytest.mark.parametrize("Cin", R.MERGE_CIN)
@pytest.mark.parametrize("dtype", ["fp16x3", "bf16", "fp32"])
def test_merge_layernorm_vs_float64_and_plane_identities(engines, dev, dtype, Cin, B, H, Wd):
    """The gather of the four pixels (0,0), (1,0), (0,1), (1,1) (each at its own scale) + LayerNorm(4 Cin): the FP32 engine's
    result within ln_tol of float64; the 16-bit results its RN16 / its two-rounding split, bit for bit, and by themselves
    within ln_tol plus what their own format drops."""
    xc, gc, bc = R.merge_inputs(B, H, Wd, Cin)
    ref, tol = R.ln_tol(R.merge_gather(xc), gc, bc)
    x, g, b = xc.to(dev), gc.to(dev), bc.to(dev)
    o32, _ = _merge_call(engines("fp32"), "fp32", dev, x, g, b, B, H, Wd, Cin)
    r = _note("merge_layernorm", o32, ref, tol)
    assert r <= 1.0, f"{r:.3f} tolerances from the float64 merge + LayerNorm (Cin = {Cin}, {(B, H, Wd)})"
    if dtype == "fp32":
        return
    hi, lo = _merge_call(engines(dtype), dtype, dev, x, g, b, B, H, Wd, Cin)
    if dtype == "bf16":         # RN16 moves a value by at most 2^-8 of itself (8 significant bits)
        drop = 2.0 ** -8 * (ref.abs() + tol)
        val = hi.double()
    else:                       # lo = RN16(v - hi): 2^-11 of |v - hi| <= 2^-11 |v|, or half a subnormal step
        drop = 2.0 ** -22 * (ref.abs() + tol) + 2.0 ** -25
        val = hi.double() + lo.double()
    assert ((val - ref).abs() <= tol + drop).all(), "the 16-bit result is outside ln_tol + its format's rounding"
    _check_planes(dtype, hi, lo, o32, f"Cin = {Cin}, {(B, H, Wd)}")
    if dtype in R.SPLIT:
        hi_p, lo_p = _merge_call(engines(dtype), dtype, dev, x, g, b, B, H, Wd, Cin, planes=1)
        assert lo_p is None and _same(hi_p, hi), "planes = 1 writes another hi plane than planes = 2"


# ---- cast -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CAST_N)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_cast_is_the_two_rounding_split(engines, dev, dtype, n):
    """cast16_kernel / cast16_split_kernel: hi == RN16(scale x), lo == RN16(scale x - hi) bit for bit (FP32: a copy), over
    +-0, fp16 subnormals, neighbours of 16-bit ties, 65504, 65520 (inf in fp16), and a size whose grid-stride loop runs
    twice."""
    e = engines(dtype)
    td = OUT_T[dtype]
    split = dtype in R.SPLIT
    xc = R.cast_inputs(n, td)
    x = xc.to(dev)
    for scale in (R.CAST_SCALES if split else (1.0,)):
        y_lo = _lo_offset(n) if split else 0
        y = Guarded(y_lo + n, td, dev)
        e.cast16(x, y.t, n, y_lo=y_lo, scale=scale)
        _sync()
        assert y.untouched((0, n), *([(y_lo, n)] if split else [])), "mnx_cast16 wrote outside its planes"
        v = xc * torch.tensor(scale, dtype=torch.float32)           # a power of two: exact
        hi = y.t[:n].cpu()
        lo = y.t[y_lo:y_lo + n].cpu() if split else None
        _check_planes(dtype, hi, lo, v, f"n = {n}, scale = {scale}")


# ---- patch embedding ------------------------------------------------------------------------------------------------
def _pe_call(e, dev, img, w, bias, gamma, beta, B, S, C):
    n = B * (S // 4) ** 2 * C
    out = Guarded(n, torch.float32, dev)
    e.patch_embed(img, R.pe_w_t(w).to(dev), bias.to(dev), gamma.to(dev), beta.to(dev), out.t, B, S, C)
    _sync()
    assert out.untouched((0, n)), "mnx_patch_embed wrote outside x"
    assert out.written(0, n), "mnx_patch_embed left tokens unwritten"
    return out.t.cpu().reshape(B, (S // 4) ** 2, C)


@pytest.mark.parametrize("S", R.PE_S)
@pytest.mark.parametrize("C", R.PE_C)
def test_patch_embed_vs_float64_reference(engines, dev, C, S):
    """patch_embed_kernel<C/8> on N(0, 1) images: every token (every patch row and column, chunk and image edges included)
    within patch_embed_tol of float64 Conv2d(4x4 / 4) + bias + LayerNorm. S = 96: one partial chunk, two patch rows per
    workgroup; 100: G odd, one row per workgroup; 384: exactly one chunk; 388: a second chunk of one patch; 392: two
    chunks x two rows."""
    B = 2
    w, bias, gamma, beta = R.pe_weights(C)
    img = R.pe_images(B, S)
    ref, tol = R.patch_embed_tol(img, w, bias, gamma, beta)
    got = _pe_call(engines("fp16x3"), dev, img.to(dev), w, bias, gamma, beta, B, S, C)
    r = _note("patch_embed", got, ref, tol)
    assert r <= 1.0, f"{r:.3f} tolerances from the float64 patch embedding (C = {C}, S = {S})"


@pytest.mark.parametrize("S", R.PE_S)
@pytest.mark.parametrize("C", R.PE_C)
def test_patch_embed_gray8_equals_fp32_path(engines, dev, C, S):
    """patch_embed_gray8_kernel on uniform gray bytes: bit for bit the tokens of patch_embed_kernel fed normalise_gray of the
    same bytes (the kernel's stated contract), and so within the same tolerance of float64."""
    from molnextr_amd.preprocess import normalise_gray
    B = 2
    e = engines("fp16x3")
    w, bias, gamma, beta = R.pe_weights(C)
    gray = R.pe_gray(B, S)
    img = torch.from_numpy(np.stack([normalise_gray(gray[i].numpy()) for i in range(B)]))
    assert img.shape == (B, 3, S, S) and img.dtype == torch.float32
    from_f32 = _pe_call(e, dev, img.to(dev), w, bias, gamma, beta, B, S, C)
    from_gray = _pe_call(e, dev, gray.to(dev), w, bias, gamma, beta, B, S, C)
    differ = (words(from_f32) != words(from_gray)).any(-1).nonzero()
    assert differ.numel() == 0, f"{differ.shape[0]} tokens differ between the gray8 and the fp32 path, first {differ[:4].tolist()}"
    ref, tol = R.patch_embed_tol(img, w, bias, gamma, beta)
    assert _note("patch_embed", from_gray, ref, tol) <= 1.0


# ---- SGEMM ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", R.SGEMM_SHAPES)
def test_sgemm_tn_vs_float64_and_permuted_store(engines, dev, M, N, K, bias):
    """sgemm_tn_kernel with M and N tails, with and without bias, within (K + 2) e (sum |a||w| + |bias|) of float64; with
    perm_S the same words at the places of the documented [M / S][N / 256][8][S][32] layout (scatter computed here)."""
    e = engines("fp16x3")
    A, Wt, b = R.sgemm_inputs(M, N, K)
    b = b if bias else None
    ref, tol = R.sgemm_tol(A, Wt, b)
    Ad, Wd, bd = A.to(dev), Wt.to(dev), (b.to(dev) if bias else None)
    out = Guarded(M * N, torch.float32, dev)
    e.sgemm_tn(Ad, Wd, bd, out.t, M, N, K)
    _sync()
    assert out.untouched((0, M * N)) and out.written(0, M * N)
    got = out.t.cpu().reshape(M, N)
    r = _note("sgemm_tn", got, ref, tol)
    assert r <= 1.0, f"{r:.3f} tolerances from the float64 product ({M}, {N}, {K})"
    S = R.SGEMM_PERM.get((M, N, K), 0)
    if S:
        perm = Guarded(M * N, torch.float32, dev)
        e.sgemm_tn(Ad, Wd, bd, perm.t, M, N, K, perm_S=S)
        _sync()
        assert perm.untouched((0, M * N))
        want = torch.empty(M * N, dtype=torch.int32)
        want[R.sgemm_perm_index(M, N, S).flatten()] = words(got).flatten()
        assert torch.equal(words(perm.t.cpu()), want), f"perm_S = {S}: the output is not the perm_S = 0 result scattered"


# ---- argument checks ------------------------------------------------------------------------------------------------
def _refusals(e, name, good, cases, outputs):
    """Each case replaces arguments of the valid call `good` (a dict in the ABI's argument order): the call returns -1, the
    message names the entry point, and no output byte changed."""
    fn = getattr(e.lib, name)
    for change, word in cases:
        args = dict(good)
        assert set(change) <= set(args), change
        args.update(change)
        rc = fn(e.h, *args.values())
        msg = e.lib.mnx_last_error(e.h).decode()
        assert rc == -1, (name, change, rc)
        assert msg.startswith(name + ": ") and word in msg, (change, msg)
    _sync()
    for o in outputs:
        assert o.untouched(), f"{name}: a refused call wrote to an output"
    assert fn(None, *good.values()) == -1


def test_patch_embed_rejects_bad_arguments(engines, dev):
    e = engines("fp16x3")
    B, S, C = 1, 16, 32
    img = torch.zeros(B, 3, S, S, device=dev)
    w, b4 = torch.zeros(48, C, device=dev), torch.zeros(3, C + 4, device=dev)
    out = Guarded(B * 16 * C, torch.float32, dev)
    p = out.t.data_ptr()
    good = dict(img=img.data_ptr(), fmt=0, w_t=w.data_ptr(), bias=b4[0].data_ptr(), gamma=b4[1].data_ptr(),
                beta=b4[2].data_ptr(), x=p, B=B, S=S, C=C, stream=None)
    cases = [(dict(fmt=2), "img_format"), (dict(img=None), "null"), (dict(w_t=None), "null"), (dict(x=None), "null"),
             (dict(gamma=None), "null"), (dict(x=p + 4), "aligned"), (dict(w_t=w.data_ptr() + 8), "aligned"),
             (dict(img=img.data_ptr() + 4), "aligned"), (dict(img=img.data_ptr() + 2, fmt=1), "aligned"),
             (dict(C=0), "C must"), (dict(C=48), "C must"), (dict(C=160), "C must"), (dict(C=-32), "C must"),
             (dict(S=0), "S must"), (dict(S=18), "S must"), (dict(S=-4), "S must"), (dict(B=0), "B must"),
             (dict(B=65536), "B must")]
    _refusals(e, "mnx_patch_embed", good, cases, [out])


def test_layernorm_rejects_bad_arguments(engines, dev):
    M, C = 3, 64
    x = torch.zeros(M, C, device=dev)
    gb = torch.zeros(2, C, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    for dtype in ("fp16x3", "bf16"):
        e = engines(dtype)
        split = dtype in R.SPLIT
        y_lo = _lo_offset(M * C) if split else 0
        y16 = Guarded(y_lo + M * C, OUT_T[dtype], dev)
        y32 = Guarded(M * C, torch.float32, dev)
        p16, p32 = y16.t.data_ptr(), y32.t.data_ptr()
        good = dict(x=x.data_ptr(), gamma=gb[0].data_ptr(), beta=gb[1].data_ptr(), y16=p16, y_lo=y_lo, y32=p32, M=M, C=C,
                    eps=1e-5, planes=2, flag=flag.data_ptr(), stream=None)
        cases = [(dict(x=None), "null"), (dict(gamma=None), "null"), (dict(beta=None), "null"),
                 (dict(y16=None, y32=None), "both null"), (dict(y32=p32 + 4), "aligned"), (dict(y16=p16 + 2), "aligned"),
                 (dict(x=x.data_ptr() + 4), "aligned"), (dict(flag=flag.data_ptr() + 2), "flag"), (dict(M=0), "M must"),
                 (dict(M=-3), "M must"), (dict(C=0), "C must"), (dict(C=66), "C must"), (dict(C=2052), "C must"),
                 (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(planes=0), "planes"),
                 (dict(planes=3), "planes")]
        if split:
            cases += [(dict(y_lo=M * C - 8), "y_lo"), (dict(y_lo=0), "y_lo"), (dict(y_lo=y_lo + 4), "y_lo"),
                      (dict(y_lo=-8, planes=1), "y_lo")]
        else:
            cases += [(dict(y_lo=M * C), "y_lo"), (dict(planes=1), "planes")]
        _refusals(e, "mnx_layernorm16", good, cases, [y16, y32])
        assert flag.cpu().tolist() == [0, 0]


def test_merge_layernorm_rejects_bad_arguments(engines, dev):
    B, H, Wd, C = 1, 2, 4, 32
    x = torch.zeros(B, H, Wd, C, device=dev)
    gb = torch.zeros(2, 4 * C, device=dev)
    n = B * (H // 2) * (Wd // 2) * 4 * C
    for dtype in ("fp16x3", "fp32"):
        e = engines(dtype)
        split = dtype in R.SPLIT
        y_lo = _lo_offset(n) if split else 0
        y = Guarded(y_lo + n, OUT_T[dtype], dev)
        p = y.t.data_ptr()
        good = dict(x=x.data_ptr(), gamma=gb[0].data_ptr(), beta=gb[1].data_ptr(), y16=p, y_lo=y_lo, B=B, H=H, W=Wd, C=C,
                    eps=1e-5, planes=2, stream=None)
        cases = [(dict(x=None), "null"), (dict(y16=None), "null"), (dict(gamma=None), "null"),
                 (dict(y16=p + (8 if dtype == "fp32" else 2)), "aligned"), (dict(x=x.data_ptr() + 8), "aligned"),
                 (dict(B=0), "even"), (dict(H=3), "even"), (dict(W=5), "even"), (dict(H=0), "even"), (dict(W=-2), "even"),
                 (dict(C=0), "C must"), (dict(C=30), "C must"), (dict(C=516), "C must"), (dict(eps=-1e-5), "eps"),
                 (dict(planes=0), "planes"), (dict(planes=3), "planes")]
        if split:
            cases += [(dict(y_lo=n - 8), "y_lo"), (dict(y_lo=0), "y_lo"), (dict(y_lo=y_lo + 4), "y_lo")]
        else:
            cases += [(dict(y_lo=n), "y_lo"), (dict(planes=1), "planes")]
        _refusals(e, "mnx_merge_ln16", good, cases, [y])


def test_cast_rejects_bad_arguments(engines, dev):
    n = 64
    x = torch.zeros(n + 4, device=dev)
    for dtype in ("bf16x3", "fp16", "fp32"):
        e = engines(dtype)
        split = dtype in R.SPLIT
        y_lo = _lo_offset(n) if split else 0
        y = Guarded(y_lo + n, OUT_T[dtype], dev)
        p = y.t.data_ptr()
        good = dict(x=x.data_ptr(), y16=p, y_lo=y_lo, n=n, scale=1.0, stream=None)
        cases = [(dict(x=None), "null"), (dict(y16=None), "null"), (dict(x=x.data_ptr() + 4), "aligned"),
                 (dict(y16=p + (8 if dtype == "fp32" else 4)), "aligned"), (dict(n=0), "n must"), (dict(n=-4), "n must"),
                 (dict(n=62), "n must")]
        if split:
            cases += [(dict(y_lo=n - 4), "y_lo"), (dict(y_lo=0), "y_lo"), (dict(y_lo=y_lo + 2), "y_lo"),
                      (dict(scale=0.0), "scale"), (dict(scale=-2.0), "scale"), (dict(scale=float("inf")), "scale"),
                      (dict(scale=float("nan")), "scale")]
        else:
            cases += [(dict(y_lo=n), "y_lo")]
        _refusals(e, "mnx_cast16", good, cases, [y])


def test_sgemm_tn_rejects_bad_arguments(engines, dev):
    e = engines("fp16x3")
    M, N, K = 10, 256, 32
    A, Wt, b = torch.zeros(M, K, device=dev), torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    out = Guarded(M * N, torch.float32, dev)
    p = out.t.data_ptr()
    good = dict(A=A.data_ptr(), W=Wt.data_ptr(), bias=b.data_ptr(), C=p, M=M, N=N, K=K, perm_S=5, stream=None)
    cases = [(dict(K=24), "K must"), (dict(K=0), "K >= 16"), (dict(N=254, perm_S=0), "N must"), (dict(N=0), "N >= 4"),
             (dict(N=192), "multiple of 256"), (dict(perm_S=3), "divide M"), (dict(perm_S=-1), "perm_S"),
             (dict(M=0), "M >= 1"), (dict(M=-5), "M >= 1"), (dict(A=None), "null"), (dict(W=None), "null"),
             (dict(C=None), "null"), (dict(C=p + 4), "aligned"), (dict(bias=b.data_ptr() + 8), "aligned"),
             (dict(A=A.data_ptr() + 4), "aligned")]
    _refusals(e, "mnx_sgemm_tn", good, cases, [out])
