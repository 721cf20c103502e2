"""GPU (-m gpu): every route of the encoder GEMMs against exact references, bit for bit (tests/gemm_ref.py has the method,
the case tables and the bit budget; tests/test_gemm_ref_host.py shows on the CPU which faults the method detects).

Operands are small integers (lo planes: integers times 2^-6), so every fp32 partial sum is exact in any order and the
kernel's words must EQUAL the float64 reference's: no tolerance in (a), (b) and (c). In every case that launches a kernel
the output and A, W and the bias lie between NaN sentinels (a stray write changes a sentinel, a stray read puts a NaN into
the result; the residual is the guarded C itself); every case runs twice and the two runs' words are compared. The refusal
tests (f) launch nothing: only their C is guarded, A and W are plain tensors.
"Without bias" means bias == NULL at the entry point: mnx_gemm16 (N <= 4096) and mnx_gemm16_split hand the kernels the
engine's zero vector, as the encoder does for the patch-merging reduction. No kernel here runs with a null bias pointer.

ROUTES AND THE SHAPES THAT REACH THEM (gemm_ref.route restates launch_gemm16; the host test pins the arithmetic)
  (a) 128-tile kernels gemm_tn_kernel (K % 64 != 0) and gemm_tn_glds_kernel (K % 64 == 0), BN = 64 (N >= 64 at these sizes)
      and BN = 128 (N < 64, and the wide shapes 4033 x 3208, 4096 x 2048), and gemm_f32_kernel (fp32 engines, through
      mnx_gemm16): a pairwise cover of M in {1..257} x N in {8..200} x K in {8..320}, ~84 shapes per 16-bit dtype, 64 for
      fp32; epilogues 0, 2, 3; split modes at terms 3, 2 (fp16x3), 1 with | 0x200, oscale 1 and 2^-12.
  (b) g256 (gemm256_kernel): bf16 / fp16 4096 x 4096 (256 tiles) and 6144 x 3840 (360 tiles, ragged second round), and the
      split dtypes on one term; x3 (gemm256x3_kernel, six- and four-phase): 3328 x 4096 and 53248 x 256 (208 tiles, both
      orientations of the tile walk, a round taken although not full), 7424 x 4096 (464 tiles: two rounds, the stream runs
      from one tile into the next); x3+128: 5120 x 4096 (256 tiles on the persistent kernel, rows 4096.. on the 128-tile
      kernel, the seam compared like every other row); gemm_res forced (| 0x100) at 1, 255, 256, 257 and 515 tiles.
      K = 128, 192, 320, 1024: 2, 3 and 5 K-tiles and one long K; gemm_res at the smallest K of each term form.
  (c) lo planes of A, W and C farther behind their hi planes than the adjacent offset, and 2^32 bytes + 8 KiB behind, on
      the 128-tile kernels and on the 208-tile x3 shape.
  (d) gemm_f32_kernel on Gaussian data against a float64 product, per element: |err| <= (K + 3) 2^-24 (sum |a||w| + |b| + |r|).
  (e) the GELU epilogue alone (A = 0, bias = a grid of x): plain modes against the documented 2.3e-6 of the polynomial plus
      half a 16-bit ulp; split modes and the fp32 engine (gelu_erf on the library's erff) against ERFF_BOUND.
  (f) the argument refusals of mnx_gemm16 and mnx_gemm16_split.

RESULTS (MI355X, gfx950)
  * Every exact comparison of (a), (b) and (c) holds as an equality of words. So on gfx950 v_mfma_f32_16x16x32_f16,
    v_mfma_f32_16x16x32_bf16 and v_mfma_f32_16x16x4_f32 accumulate operands inside the bit budget EXACTLY, with units down
    to 2^-6 next to sums above 2^16 and at every K-tile count tried; fp16 lo planes keep their subnormals (oscale 2^-12
    gives lo values that are multiples of 2^-18); and every 16-bit store, plain (RN-even16(v), ties such as 2049 in fp16 and
    257 in bf16 included) and split (hi = RN16(v), lo = RN16(v - hi)), rounds as cast16 and torch do.
  * A bug these tests found: a split engine on ONE term with a one-plane GELU output (epi 1 | 0x400, c_lo = 0) on a 256-tile
    shape went to gemm256_kernel, which always stores both planes: the lo plane landed on the hi plane. launch_gemm16 now
    keeps a one-plane output on the 128-tile kernel and launch_gemm256 refuses it (test_gelu_epilogue_alone
    [..-4096x4096x128-e1-t1-s0-p1-128]). gemm256x3_kernel has no one-plane bf16 form (a two-term consumer is fp16 only):
    refused by launch_gemm256x3, left out of the table. A null A, W or C used to return -1 with the previous call's error text.
  * erff: worst |hi + lo - float64| / max(1, |gelu|) over the grid on every two-plane fp16x3 route is 2.01e-7 (what two fp16
    planes cannot hold included), 1.18e-7 on the fp32 engine (gelu_erf stored as fp32): ERFF_MEASURED = 2.01e-7, and
    ERFF_BOUND = 4.02e-7 is twice that and nothing more (the margin is for the library's erff changing between ROCm
    releases). It is 1200 times below half an fp16 ulp (2^-11 = 4.9e-4), so the fp16x3 and fp32 checks do say something
    about the epilogue. The bf16x3 check does NOT meet that condition: two bf16 planes are off by up to half a bf16 ulp of
    the lo plane (about 2^-18 |v| = 3.8e-6 |v|), which is added per element and is several times the erff figure — inherent
    to the format. A one-plane output has no bound: its hi plane must equal the two-plane form's hi plane word for word.
  * Run time of this file: 227 tests in 3 s after the five tiny engines are built (4 s in all); the slowest case takes
    0.5 s (the first one: kernel load), every persistent case under 0.3 s — test_gemm_split_operand_modes' slowest case
    took 2.1 s in the same run.
"""
import ctypes
import dataclasses
import time

import pytest
import torch

import gemm_ref as R
from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu

TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
ERFF_MEASURED = 2.01e-7        # worst figure of test_gelu_epilogue_alone on the split and fp32 routes (module docstring)
ERFF_BOUND = 2 * ERFF_MEASURED
GELU_POLY_ABS = 2.3e-6         # common.h gelu_fast4, tests/test_device_math.py
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    """One tiny engine per compute dtype, built as _tiny_engine of test_gpu_parity.py builds them: mnx_gemm16 and
    mnx_gemm16_split use nothing of an engine but its device, its compute dtype and its zero bias vector."""
    from molnextr_amd.engine import Engine
    dec = W.DecoderDims(enc_dim=TINY.num_features)
    ck = W.synthetic_checkpoint(0, enc=TINY, dec=dec)
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Engine(ck["encoder"], ck["decoder"], max_batch=2, enc=TINY, dec=dec, dtype=dtype)
        return made[dtype]
    t0 = time.perf_counter()
    yield get
    for e in made.values():
        e.close()
    print(f"test_gpu_gemm: {time.perf_counter() - t0:.1f} s; worst GELU figures {WORST}")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Inputs:
    """A and W of one case on the device, planes at the case's offsets, NaN sentinels around and between them. Two terms:
    the lo plane of A stays NaN (the kernel must not read it)."""

    def __init__(self, c, o, dev):
        td = R.OPERAND_T[c.dtype]
        if c.split:
            self.A = R.Planes((c.M, c.K), td, dev, lo_off=c.M * c.K + c.a_gap).put(o["Ah"], None if c.terms == 2 else o["Al"])
            self.W = R.Planes((c.N, c.K), td, dev, lo_off=c.N * c.K + c.w_gap).put(o["Wh"], o["Wl"])
        else:
            self.A = R.Planes((c.M, c.K), td, dev).put(o["Ah"])
            self.W = R.Planes((c.N, c.K), td, dev).put(o["Wh"])
        if c.split and c.terms == 2:
            self.A.lo.view(R.WORD_T[2]).fill_(R.SENTINEL[td])

    def intact(self):
        return self.A.intact() and self.W.intact()


def _output(c, dev, res):
    if c.out16:
        two = c.split and c.planes == 2
        return R.Planes((c.M, c.N), R.OPERAND_T[c.dtype], dev, lo_off=c.M * c.N + c.c_gap if two else None)
    out = R.Planes((c.M, c.N), torch.float32, dev)
    if res is not None:
        out.hi.copy_(res)
    return out


def _launch(e, c, inp, out, bias):
    epi = c.epi | {"": 0, "128": R.FORCE_128, "gres": R.FORCE_GRES}[c.force]
    if c.split:
        if c.out16 and c.planes == 1:
            epi |= R.ONE_PLANE
        rc = e.lib.mnx_gemm16_split(e.h, epi, _ptr(inp.A.hi), inp.A.lo_off, _ptr(inp.W.hi), inp.W.lo_off, c.oscale,
                                    _ptr(out.hi), out.lo_off or 0, _ptr(bias), c.M, c.N, c.K, c.terms, _stream())
    else:
        assert c.force in ("", "gres")
        rc = e.lib.mnx_gemm16(e.h, epi, _ptr(inp.A.hi), _ptr(inp.W.hi), _ptr(out.hi), _ptr(bias), c.M, c.N, c.K, _stream())
    assert rc == 0, (c.id, rc, e.lib.mnx_last_error(e.h).decode())


def _guarded_bias(bias, dev):
    if bias is None:
        return None
    b = R.guarded(tuple(bias.shape), torch.float32, dev)
    b.copy_(bias)
    return b


def _run_twice(e, c, inp, bias, res, dev):
    """the case's launch on two fresh outputs; the second must repeat the first word for word"""
    bg = _guarded_bias(bias, dev)
    outs = []
    for _ in range(2):
        out = _output(c, dev, res)
        _launch(e, c, inp, out, bg)
        outs.append(out)
    torch.cuda.synchronize()
    a, b = outs
    assert torch.equal(R.words(a.hi), R.words(b.hi)) and (a.lo is None or torch.equal(R.words(a.lo), R.words(b.lo))), \
        f"{c.id}: two runs of the same launch differ"
    assert a.intact() and b.intact(), f"{c.id}: a write outside C"
    assert inp.intact() and (bg is None or R.guards_intact(bg)), f"{c.id}: an operand's surroundings changed"
    return a


def _check_exact(e, c, inp, acc, dev):
    bias, res = R.epilogue_operands(c, dev)
    want = R.expected(c, acc, bias, res)
    out = _run_twice(e, c, inp, bias, res, dev)
    tile = (256, 256) if c.expected_route in ("g256", "x3", "x3+128") else (256, 128) if c.expected_route == "gres" else \
        (64, 64) if c.dtype == "fp32" else (128, R.tile128_variant(*c.shape)[0])
    for key, exp in want.items():
        diff = R.first_difference(out.lo if key == "lo" else out.hi, exp, tile)
        assert diff is None, f"{c.id} [{c.expected_route}] plane {key}: {diff}"


class Shared:
    """operands, device inputs and exact term sums of one (dtype, shape), shared by the runs of that shape"""

    def __init__(self, dev):
        self.dev, self.key, self.o, self.inp, self.acc = dev, None, None, {}, {}

    def get(self, c):
        key = (c.dtype, c.shape, c.amax, c.a_gap, c.w_gap)
        if key != self.key:
            self.key, self.o, self.inp, self.acc = key, R.operands(c, self.dev), {}, {}
        two = c.split and c.terms == 2
        if two not in self.inp:
            self.inp[two] = Inputs(c, self.o, self.dev)
        if c.terms not in self.acc:
            self.acc[c.terms] = R.products(self.o, c.terms, c.split)
            if c.M * c.N * c.K <= 1 << 20:          # small shapes: the device's float64 product is the host's int64 one
                want = torch.from_numpy(R.products_int64(self.o, c.terms, c.split)).to(self.dev)
                assert torch.equal(self.acc[c.terms] * 64, want.double()), c.id
        return self.inp[two], self.acc[c.terms]


# ---- (a) the 128-tile kernels and gemm_f32_kernel: edges ----------------------------------------------------------------
def _edge_groups():
    out = []
    for dt in R.DTYPES:
        for m in sorted({c.M for c in R.EDGE_CASES[dt]}):
            out.append(pytest.param(dt, m, id=f"{dt}-M{m}"))
    return out


@pytest.mark.parametrize("dtype,M", _edge_groups())
def test_tile128_and_f32_kernels_exact_at_every_edge(engines, dev, dtype, M):
    e, sh = engines(dtype), Shared(dev)
    cases = [c for c in R.EDGE_CASES[dtype] if c.M == M]
    assert len(cases) >= 3
    for c in cases:
        assert R.in_budget(c) and c.expected_route in ("128", "f32")
        inp, acc = sh.get(c)
        _check_exact(e, c, inp, acc, dev)


@pytest.mark.parametrize("dtype,shape,force", [("fp16x3", (129, 136, 72), "128"), ("bf16x3", (3328, 4096, 192), "")])
def test_the_comparison_tells_term_counts_and_offsets_apart(engines, dev, dtype, shape, force):
    """The equality is not vacuous on the device either: the three-term output differs from the one-term and (a lo.lo term
    added) four-product references in most words, and a lo plane of A read at the adjacent offset, where the gap's NaN
    sentinels lie, does not give the reference."""
    e = engines(dtype)
    c = R.make_case(dtype, *shape, R.EPI_BIAS_F32, terms=3, force=force)
    o = R.operands(c, dev)
    inp = Inputs(c, o, dev)
    bias, _ = R.epilogue_operands(c, dev)
    out = _run_twice(e, c, inp, bias, None, dev)
    want = R.expected(c, R.products(o, 3, True), bias, None)["f32"]
    assert torch.equal(R.words(out.hi), R.words(want))
    one = R.expected(c, R.products(o, 1, True), bias, None)["f32"]
    lolo = R.value(c, R.products(o, 3, True) + o["Al"].double() @ o["Wl"].double().t(), bias, None)
    assert (out.hi != one).float().mean().item() > 0.9 and (out.hi != lolo).float().mean().item() > 0.9
    wrong, bg = _output(c, dev, None), _guarded_bias(bias, dev)
    rc = e.lib.mnx_gemm16_split(e.h, c.epi | (R.FORCE_128 if force else 0), _ptr(inp.A.hi), c.M * c.K, _ptr(inp.W.hi),
                                inp.W.lo_off, 1.0, _ptr(wrong.hi), 0, _ptr(bg), c.M, c.N, c.K, 3, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.equal(R.words(wrong.hi), R.words(want)) and bool(torch.isnan(wrong.hi).any())


# ---- (b) the persistent kernels: K-tile parity and rounds ---------------------------------------------------------------
def _persistent_groups():
    groups = {}
    for c in R.PERSISTENT_CASES:
        groups.setdefault((c.dtype, c.terms, c.M, c.N, c.K, c.force), []).append(c)
    return [pytest.param(v, id=f"{k[0]}-t{k[1]}-{k[2]}x{k[3]}x{k[4]}-{v[0].expected_route}") for k, v in groups.items()]


@pytest.mark.parametrize("cases", _persistent_groups())
def test_persistent_kernels_exact_at_every_ktile_parity_and_round(engines, dev, cases):
    e, sh = engines(cases[0].dtype), Shared(dev)
    t0 = time.perf_counter()
    for c in cases:
        assert R.in_budget(c)
        inp, acc = sh.get(c)
        _check_exact(e, c, inp, acc, dev)
    torch.cuda.synchronize()
    print(f"persistent {cases[0].expected_route} {cases[0].dtype} t{cases[0].terms} {cases[0].shape}: {len(cases)} runs x 2, "
          f"{time.perf_counter() - t0:.2f} s")


# ---- (c) plane offsets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [pytest.param(c, id=f"{c.id}-{'far' if c.a_gap >= R.FAR else 'gap'}") for c in R.OFFSET_CASES])
def test_lo_planes_at_distant_offsets(engines, dev, c):
    """a_lo, w_lo and c_lo larger than the adjacent offsets, NaN in the gaps; and lo planes of A and C that start 2^32 bytes
    + 8 KiB behind their hi planes (torch.empty, only the planes and bands around them written)"""
    assert R.in_budget(c)
    if c.a_gap >= R.FAR:
        assert (c.M * c.K + c.a_gap) * 2 >= 2 ** 32 and (c.M * c.N + c.c_gap) * 2 >= 2 ** 32
    inp, acc = Shared(dev).get(c)
    _check_exact(engines(c.dtype), c, inp, acc, dev)


# ---- (d) the fp32 kernel on real-valued data ---------------------------------------------------------------------------------
F32_GAUSS = [s for s in R.edge_shapes("fp32") if s[:2] in ((129, 136), (65, 200), (257, 56))] + [(2304, 384, 128)]


@pytest.mark.parametrize("M,N,K", F32_GAUSS)
def test_f32_kernel_on_gaussian_data_within_the_dot_product_bound(engines, dev, M, N, K):
    """Three shapes of the fp32 list of (a), and the stage-1 qkv projection of Swin-B (C = 128, so K = 128 and N = 3 C =
    384) for a batch of four 96 x 96 images: 4 (96 / 4)^2 = 2304 tokens. The bound is the standard one of an fp32 dot
    product in any order, per element: nothing measured."""
    assert len(F32_GAUSS) == 4 and all(s in R.edge_shapes("fp32") for s in F32_GAUSS[:3])
    e = engines("fp32")
    g = torch.Generator().manual_seed(M + N + K)
    A = R.Planes((M, K), torch.float32, dev).put(torch.randn(M, K, generator=g).to(dev))
    Wt = R.Planes((N, K), torch.float32, dev).put((torch.randn(N, K, generator=g) / K ** 0.5).to(dev))
    bias = _guarded_bias(torch.randn(N, generator=g).to(dev), dev)
    res = torch.randn(M, N, generator=g).to(dev)
    prod = A.hi.double() @ Wt.hi.double().t()
    for epi, b, r in ((0, bias, None), (3, bias, None), (3, None, None), (2, bias, res)):
        out = R.Planes((M, N), torch.float32, dev)
        if r is not None:
            out.hi.copy_(r)
        rc = e.lib.mnx_gemm16(e.h, epi, _ptr(A.hi), _ptr(Wt.hi), _ptr(out.hi), _ptr(b), M, N, K, _stream())
        assert rc == 0, e.lib.mnx_last_error(e.h).decode()
        torch.cuda.synchronize()
        ref = prod + (b.double() if b is not None else 0.0) + (r.double() if r is not None else 0.0)
        err, bound = (out.hi.double() - ref).abs(), R.dot_bound(A.hi, Wt.hi, b, r)
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"f32 {M}x{N}x{K} epi {epi}: worst err / bound {ratio:.3f}")
        assert bool((err <= bound).all()), (epi, ratio)
        assert out.intact() and A.intact() and Wt.intact()


# ---- (e) the GELU epilogue, isolated ---------------------------------------------------------------------------------------
def _gelu_cases():
    out = []
    t128 = ((129, 2056, 72), (129, 2056, 192), (4033, 3208, 72), (4033, 3208, 192), (257, 56, 72))   # BN 64 / 128 x plain / dma, N < 64
    for dt in R.PLAIN16:
        out += [R.Case(dt, *s, R.EPI_GELU_16) for s in t128] + [R.Case(dt, 4096, 4096, 128, R.EPI_GELU_16)]
    out += [R.Case("fp32", 129, 2056, 64, R.EPI_GELU_16), R.Case("fp32", 65, 72, 16, R.EPI_GELU_16)]
    for dt in R.SPLIT:
        for terms in ((3, 2, 1) if dt == "fp16x3" else (3, 1)):
            for planes in (2, 1):
                out += [R.Case(dt, *s, R.EPI_GELU_16, terms=terms, planes=planes, force="128") for s in t128[:4:3]]
                if planes == 1 and dt == "bf16x3" and terms == 3:
                    continue        # gemm256x3_kernel has no one-plane bf16 form (a two-term consumer is fp16 only): refused
                out.append(R.Case(dt, 3328, 4096, 128, R.EPI_GELU_16, terms=terms, planes=planes))      # x3 (one term: 128-tile)
                # one term: g256 with two planes, the 128-tile kernel with one (gemm256_kernel always stores both); else x3
                out.append(R.Case(dt, 4096, 4096, 128, R.EPI_GELU_16, terms=terms, planes=planes))
            out.append(R.Case(dt, 5120, 4096, 128, R.EPI_GELU_16, terms=terms, oscale=2.0 ** -12))      # x3+128 (one term: 128-tile)
    return out


@pytest.mark.parametrize("c", [pytest.param(c, id=f"{c.id}-{c.expected_route}") for c in _gelu_cases()])
def test_gelu_epilogue_alone(engines, dev, c):
    """A = 0, so v = bias[n] exactly on every route: the output is GELU of a grid of fp32 arguments, the same in every row."""
    e = engines(c.dtype)
    td = R.OPERAND_T[c.dtype]
    o = R.operands(c, dev)
    o["Ah"].zero_()
    if c.split:
        o["Al"].zero_()
    inp = Inputs(c, o, dev)
    x = R.gelu_grid(c.N, dev)
    out = _run_twice(e, c, inp, x, None, dev)
    ref = R.gelu64(x)
    got = out.hi.double() if out.lo is None else out.hi.double() + out.lo.double()
    assert bool((got == got[0]).all()), f"{c.id}: rows differ although every row has the same arguments"
    err = (got[0] - ref).abs()
    scale = ref.abs().clamp_min(1.0)
    if c.split and c.planes == 1:
        # the hi plane alone is the two-plane output's hi plane bit for bit (kernels.h), whatever kernel each form lands on:
        # no bound of its own — the two-plane twin is the case that is compared with float64
        twin = dataclasses.replace(c, planes=2)
        both = _run_twice(e, twin, inp, x, None, dev)
        diff = R.first_difference(out.hi, both.hi)
        assert diff is None, f"{c.id} against its two-plane twin [{twin.expected_route}]: {diff}"
        print(f"gelu {c.id} [{c.expected_route}]: hi plane equals the two-plane form's [{twin.expected_route}]")
        return
    if c.dtype in R.PLAIN16:
        bound = GELU_POLY_ABS + R.half_ulp16(ref.abs() + GELU_POLY_ABS, td)
    elif c.dtype == "bf16x3":
        # two bf16 planes cannot hold v: lo = RN16(v - hi) is off by up to half a bf16 ulp of lo (about 2^-18 |v|), which is
        # several times the erff figure. Inherent to the format; this check is NOT 100 times below half an fp16 ulp.
        bound = ERFF_BOUND * scale + R.half_ulp16(out.lo[0].double(), td)
    else:
        bound = ERFF_BOUND * scale       # fp16x3 (hi + lo, what the planes cannot hold included in the measured figure), fp32
        WORST["erff " + c.dtype] = max(WORST.get("erff " + c.dtype, 0.0), (err / scale).max().item())
    print(f"gelu {c.id} [{c.expected_route}]: worst |err| / max(1, |gelu|) {(err / scale).max().item():.3e}, "
          f"worst err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (c.id, (err / bound).max().item())


def test_erff_bound_is_far_below_half_an_fp16_ulp():
    assert ERFF_BOUND == 2 * ERFF_MEASURED and ERFF_BOUND * 100 <= 2.0 ** -11


# ---- (f) refusals ------------------------------------------------------------------------------------------------------------
def _refusals(e, name, good, cases, out):
    """Each case replaces arguments of the valid call `good` (a dict in the ABI's argument order): the call returns -1, the
    handle's error text names the entry point, and the sentinel-filled C is untouched."""
    fn = getattr(e.lib, name)
    for change, word in cases:
        args = dict(good)
        assert set(change) <= set(args), change
        args.update(change)
        rc = fn(e.h, *args.values())
        msg = e.lib.mnx_last_error(e.h).decode()
        assert rc == -1, (name, change, rc, msg)
        assert msg.startswith(name + ": ") and word in msg, (change, msg)
    torch.cuda.synchronize()
    assert out.intact() and bool((out.raw == R.SENTINEL[out.td]).all()), f"{name}: a refused call wrote to C"
    assert fn(None, *good.values()) == -1


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gemm16_rejects_bad_arguments(engines, dev, dtype):
    e = engines(dtype)
    M, N, K = 128, 128, 64
    td = R.OPERAND_T[dtype]
    A, Wt, bias = torch.zeros(M, K, device=dev, dtype=td), torch.zeros(N, K, device=dev, dtype=td), torch.zeros(N, device=dev)
    out = R.Planes((M, N), torch.float32, dev)
    good = dict(epi=3, A=A.data_ptr(), W=Wt.data_ptr(), C=out.hi.data_ptr(), bias=bias.data_ptr(), M=M, N=N, K=K, stream=None)
    cases = [(dict(K=12), "multiples of 8"), (dict(K=60), "multiples of 8"), (dict(N=12), "multiples of 8"),
             (dict(N=0), "multiples of 8"), (dict(K=0), "multiples of 8"), (dict(M=0), "M must"), (dict(M=-1), "M must"),
             (dict(A=None), "null"), (dict(W=None), "null"), (dict(C=None), "null"),
             (dict(epi=3 | 0x100), "gemm_res"), (dict(epi=2 | 0x100, M=256, N=192), "gemm_res"),
             (dict(epi=0 | 0x100, M=256), "gemm_res")]
    if dtype == "fp32":
        cases += [(dict(K=24), "multiple of 16"), (dict(K=8), "multiple of 16")]
    else:
        cases += [(dict(epi=3 | 0x100, M=256, K=64), "gemm_res")]          # plain operands: the residual prefetch needs two K-tiles
    _refusals(e, "mnx_gemm16", good, cases, out)


@pytest.mark.parametrize("dtype", ["fp16x3", "bf16x3", "fp16"])
def test_gemm16_split_rejects_bad_arguments(engines, dev, dtype):
    e = engines(dtype)
    M, N, K = 128, 128, 64
    td = R.OPERAND_T[dtype]
    A, Wt = torch.zeros(2, M, K, device=dev, dtype=td), torch.zeros(2, N, K, device=dev, dtype=td)
    bias = torch.zeros(N, device=dev)
    out = R.Planes((M, N), td, dev, lo_off=M * N + R.GAP)
    good = dict(epi=0, A=A.data_ptr(), a_lo=M * K, W=Wt.data_ptr(), w_lo=N * K, oscale=1.0, C=out.hi.data_ptr(),
                c_lo=M * N + R.GAP, bias=bias.data_ptr(), M=M, N=N, K=K, terms=3, stream=None)
    if dtype == "fp16":
        cases = [(dict(), "not a split mode"), (dict(terms=1), "not a split mode")]
    else:
        cases = [(dict(K=12), "multiples of 8"), (dict(N=12), "multiples of 8"), (dict(M=0), "M must"), (dict(M=-1), "M must"),
                 (dict(terms=0), "terms must"), (dict(terms=4), "terms must"), (dict(terms=-1), "terms must"),
                 (dict(a_lo=-8), "negative"), (dict(w_lo=-8), "negative"), (dict(c_lo=-8), "negative"),
                 (dict(A=None), "null"), (dict(W=None), "null"), (dict(C=None), "null"),
                 (dict(epi=3 | 0x100), "gemm_res"), (dict(epi=0 | 0x100, M=256), "gemm_res"),
                 (dict(epi=2 | 0x100, M=256, N=2048), "gemm_res")]
        if dtype == "bf16x3":
            cases.append((dict(terms=2), "terms must"))
    _refusals(e, "mnx_gemm16_split", good, cases, out)
