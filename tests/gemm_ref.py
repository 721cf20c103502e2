"""Exact references for the encoder GEMMs (gemm.hip, gemm256.hip, gemm_res.hip): case tables, operand builders, the
bit-budget condition, guarded buffers. Used by tests/test_gemm_ref_host.py (CPU) and tests/test_gpu_gemm.py (GPU).

THE METHOD. Every encoder GEMM kernel accumulates in fp32. The operands here are small integers (plain modes, and the
hi planes of the split modes) and small integers times 2^-6 (the lo planes), so every product and every partial sum,
in ANY order of summation, is a multiple of one unit and smaller than 2^24 units: representable in fp32. The kernel's
result then cannot depend on its tiling, its K-tile order or its term order, and must equal the integer reference BIT
FOR BIT. A dropped or doubled k, a stale LDS buffer, a tile stored twice, a lo.lo term, a lo plane read at the wrong
offset: each changes bits (tests/test_gemm_ref_host.py shows it on a numpy emulation of a tiled kernel).

    plain modes (bf16, fp16, fp32):   v = sum_k A[m,k] W[n,k] + bias[n] (+ resid[m,n])
    split modes, terms = 3:           v = oscale * sum_k (Ah.Wh + Ah.Wl + Al.Wh) + bias (+ resid)
                 terms = 2:           v = oscale * sum_k (Ah.Wh + Ah.Wl) + bias (+ resid)
                 terms = 1:           v = oscale * sum_k  Ah.Wh + bias (+ resid)

The planes are the test's own (mnx_gemm16_split does not require lo to be hi's rounding residual); a lo.lo product would
add odd multiples of 2^-12, which no reference contains. oscale is 1 or 2^-12 (a power of two: exact).

16-bit stores: plain modes store RN-even16(v) — the integers are made to hit ties on purpose (bias up to +-3000: 2049 is
a tie in fp16, 257 in bf16); split modes store hi = RN16(v), lo = RN16(v - hi), the two-rounding split of cast16.

THE BIT BUDGET is a condition, not a measurement: bit_budget() computes, from the ranges and K alone, the largest
possible |value| over the smallest unit for the accumulator and for the epilogue's value; in_budget() requires both below
2^24, and the 16-bit outputs below 2^15 (fp16) / 2^127 (bf16). tests/test_gemm_ref_host.py asserts it for every case of
every table, so no case can silently leave the exact regime.
"""
import dataclasses
import math
import zlib

import numpy as np
import torch

EPI_BIAS_16, EPI_GELU_16, EPI_RESID_F32, EPI_BIAS_F32 = 0, 1, 2, 3
FORCE_GRES, FORCE_128, ONE_PLANE = 0x100, 0x200, 0x400
PLAIN16 = ("bf16", "fp16")
SPLIT = ("fp16x3", "bf16x3")
DTYPES = ("bf16", "fp16", "fp32", "fp16x3", "bf16x3")
OPERAND_T = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "bf16x3": torch.bfloat16,
             "fp16x3": torch.float16}
LO_UNIT = 2.0 ** -6                    # the lo planes hold integers times this
PERSISTENT_CUS = 256                   # workgroups of a persistent launch (kernels.h); also gemm_res's grid limit
GAP = 64                               # sentinel elements between the planes of a buffer and around every buffer
TIE_BIAS = 3000                        # bias range of the 16-bit-output cases: v crosses 2048 (fp16 ties) and 256 (bf16)


# ---- dispatch, restated from gemm.hip (launch_gemm16, x3_main_rows, launch_t) and the *_supports functions ------------------
def x3_main_rows(dtype, epi, M, N, K, terms):
    """rows launch_gemm16 gives to gemm256x3_kernel (the rest goes to the 128-tile kernel); 0: none"""
    if dtype not in SPLIT or not (terms == 3 or (terms == 2 and dtype == "fp16x3")):
        return 0
    if not (M > 0 and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 128):
        return 0
    tn, tm = N // 256, M // 256
    tiles, tm_main = tm * tn, tm
    if tiles % PERSISTENT_CUS and (tiles % PERSISTENT_CUS) * 10 < PERSISTENT_CUS * 8:
        tm_main = (tiles // PERSISTENT_CUS) * PERSISTENT_CUS // tn
    return tm_main * 256


def gemm256_supports(dtype, epi, M, N, K):
    if dtype == "fp32" or epi not in (EPI_BIAS_16, EPI_GELU_16) or M % 256 or N % 256 or K % 64 or K < 128:
        return False
    tiles = (M // 256) * (N // 256)
    rounds = (tiles + 255) // 256
    return tiles >= 256 and tiles * 10 >= rounds * 256 * 7


def gemm_res_supports(dtype, epi, M, N, K):
    if dtype == "fp32" or epi not in (EPI_RESID_F32, EPI_BIAS_F32) or M % 256 or N % 128 or K % 64 or N > 1024:
        return False
    return dtype in SPLIT or K >= 128


def route(dtype, epi, M, N, K, terms=1, has_bias=True, planes=2):
    """which kernel(s) launch_gemm16 runs a layer on (gemm16_route of gemm.hip; "f32": gemm_f32_kernel)"""
    r = x3_main_rows(dtype, epi, M, N, K, terms)
    if r == M:
        return "x3"
    if r > 0:
        return "x3+128"
    if has_bias and gemm256_supports(dtype, epi, M, N, K) and not (dtype in SPLIT and planes == 1):   # one plane: 128-tile kernel
        return "g256"
    if dtype in PLAIN16 and gemm_res_supports(dtype, epi, M, N, K) and (M // 256) * (N // 128) >= 1024:
        return "gres"
    return "f32" if dtype == "fp32" else "128"


def tile128_variant(M, N, K):
    """(BN, K loop) of the 128-tile kernel for a shape (launch_t / launch_bn of gemm.hip): BN 64 or 128, "dma" or "plain" """
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    waves = t128 / 512.0
    frac = waves - int(waves)
    small = t128 < 512 or (waves < 3.0 and 0.0 < frac < 0.6)
    narrow = N <= 128 and K < 512
    return (64 if (small or narrow) and N >= 64 else 128), ("dma" if K % 64 == 0 else "plain")


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    dtype: str
    M: int
    N: int
    K: int
    epi: int
    terms: int = 1             # split modes: product terms (3, 2 or 1); plain modes: 1
    oscale: float = 1.0        # split modes
    planes: int = 2            # split modes, 16-bit epilogues: output planes
    has_bias: bool = True     # False: bias == NULL at the entry point, which hands the kernel the engine's zero vector
    force: str = ""            # "": the dispatch; "128": | 0x200 (split entry); "gres": | 0x100
    amax: int = 4              # A, W (hi planes) hold integers in [-amax, amax], lo planes the same times 2^-6
    bias_max: int = 8
    res_max: int = 8
    a_gap: int = GAP           # split modes: elements between the end of the hi plane and the lo plane
    w_gap: int = GAP
    c_gap: int = GAP

    @property
    def shape(self):
        return (self.M, self.N, self.K)

    @property
    def split(self):
        return self.dtype in SPLIT

    @property
    def out16(self):
        return self.epi in (EPI_BIAS_16, EPI_GELU_16) and self.dtype != "fp32"

    @property
    def id(self):
        s = f"{self.dtype}-{self.M}x{self.N}x{self.K}-e{self.epi}"
        if self.split:
            s += f"-t{self.terms}-{'s12' if self.oscale != 1.0 else 's0'}-p{self.planes}"
        return s + ("" if self.has_bias else "-nobias") + (f"-{self.force}" if self.force else "")

    @property
    def expected_route(self):
        if self.force:
            return self.force
        return route(self.dtype, self.epi, self.M, self.N, self.K, self.terms, self.has_bias, self.planes)


def make_case(dtype, M, N, K, epi, terms=None, oscale=1.0, **kw):
    """a case with the ranges that keep it in the exact regime: ties-provoking bias where the value's unit allows it"""
    split = dtype in SPLIT
    terms = (3 if terms is None else terms) if split else 1
    oscale = oscale if split else 1.0
    out16 = epi == EPI_BIAS_16 and dtype != "fp32"
    kw.setdefault("bias_max", TIE_BIAS if out16 and oscale == 1.0 else 8)
    return Case(dtype, M, N, K, epi, terms=terms, oscale=oscale, **kw)


def bit_budget(dtype, K, terms, oscale, amax, bias_max, res_max, epi):
    """(accumulator's largest |value| / unit, epilogue value's largest |value| / unit, largest |value| stored) from the ranges
    alone. Per k the terms contribute at most amax^2 (hi.hi) + amax^2 2^-6 (hi.lo) + amax^2 2^-6 (lo.hi); the accumulator's
    unit is 1 (one term) or 2^-6; the epilogue's value oscale * acc + bias (+ resid) has the unit min(1, oscale * that)."""
    t = terms if dtype in SPLIT else 1
    per_k = amax * amax * (1.0 + (LO_UNIT if t >= 2 else 0.0) + (LO_UNIT if t >= 3 else 0.0))
    acc_max, acc_unit = per_k * K, (1.0 if t == 1 else LO_UNIT)
    s = oscale if dtype in SPLIT else 1.0
    v_max = acc_max * s + bias_max + (res_max if epi == EPI_RESID_F32 else 0)
    v_unit = min(1.0, acc_unit * s)
    return acc_max / acc_unit, v_max / v_unit, v_max


def in_budget(c):
    acc_r, v_r, v_max = bit_budget(c.dtype, c.K, c.terms, c.oscale, c.amax, c.bias_max if c.has_bias else 0, c.res_max, c.epi)
    ok = acc_r < 2 ** 24 and v_r < 2 ** 24
    if c.out16:
        ok = ok and v_max < (2.0 ** 15 if OPERAND_T[c.dtype] == torch.float16 else 2.0 ** 127)
    return ok


# (a) the 128-tile kernels and gemm_f32_kernel: edges around BM = 128, BN = 64 / 128, BK = 64 and the fp32 kernel's 64x64 tile
EDGE_M = (1, 63, 64, 65, 127, 128, 129, 257)
EDGE_N = (8, 56, 64, 72, 120, 128, 136, 200)
EDGE_K = (8, 16, 24, 56, 64, 72, 128, 192, 320)
EDGE_K_F32 = tuple(k for k in EDGE_K if k % 16 == 0)
# At these sizes launch_t picks BN = 64 whenever N >= 64 (fewer than 512 tiles of 128x128), BN = 128 only for N < 64. The wide
# shapes reach BN = 128 with ragged edges in both directions (32 x 26 = 832 tiles = 1.625 rounds of 512; 32 x 16 = 512 exactly).
WIDE_SHAPES = ((4033, 3208, 72), (4033, 3208, 192), (4096, 2048, 64))


def edge_shapes(dtype):
    """pairwise-covering list over EDGE_M x EDGE_N x EDGE_K: every (M, N), (M, K) and (N, K) pair occurs (a cyclic Latin
    square on 9 symbols, the 8-value axes padded by repeating their last value), plus the wide shapes for the 16-bit types"""
    if dtype == "fp32":
        ks = EDGE_K_F32
        out = [(m, n, ks[((i + j) % 8) % len(ks)]) for i, m in enumerate(EDGE_M) for j, n in enumerate(EDGE_N)]
        return out
    ms, ns = EDGE_M + EDGE_M[-1:], EDGE_N + EDGE_N[-1:]
    out = []
    for i in range(9):
        for j in range(9):
            s = (ms[i], ns[j], EDGE_K[(i + j) % 9])
            if s not in out:
                out.append(s)
    return out + list(WIDE_SHAPES)


def edge_cases(dtype, shape, idx):
    """the runs of one shape of (a): the three exact epilogues (GELU: gelu_cases), every term count, oscale alternating
    between 1 and 2^-12, a layer without bias every third shape; split modes on the 128-tile kernel whatever the dispatch"""
    M, N, K = shape
    out = []
    if dtype not in SPLIT:
        for epi in (EPI_BIAS_16, EPI_RESID_F32, EPI_BIAS_F32):
            out.append(make_case(dtype, M, N, K, epi, has_bias=not (epi == EPI_BIAS_F32 and idx % 3 == 0)))
        return out
    for terms in ((3, 2, 1) if dtype == "fp16x3" else (3, 1)):
        for epi in (EPI_BIAS_16, EPI_RESID_F32, EPI_BIAS_F32):
            out.append(make_case(dtype, M, N, K, epi, terms=terms, oscale=1.0 if (idx + terms + epi) % 2 == 0 else 2.0 ** -12,
                                 has_bias=not (epi == EPI_BIAS_F32 and idx % 3 == 0), force="128"))
    return out


EDGE_CASES = {dt: [c for i, s in enumerate(edge_shapes(dt)) for c in edge_cases(dt, s, i)] for dt in DTYPES}

# (b) the persistent kernels: K-tile parity (2, 3, 5 K-tiles and one long K) on the smallest production-reachable shapes of each route
PERSISTENT_K = (128, 192, 320, 1024)
G256_SHAPES = ((4096, 4096), (6144, 3840))        # 256 tiles exactly; 360 tiles: a ragged second round (>= 70 % of two rounds)
X3_SHAPES = ((3328, 4096), (53248, 256))           # 208 tiles as 13 x 16 and as 208 x 1: one round, taken although not full
X3_TWO_ROUNDS = (7424, 4096)                       # 464 tiles = 29 x 16: a workgroup streams from one tile into the next
X3_SEAM = (5120, 4096)                             # 320 tiles: 256 on the persistent kernel (rows 0..4095), 64 on the 128-tile kernel
GRES_W = PERSISTENT_CUS                            # gemm_res's workgroup count: grid = min(tiles, 256) (launch_gemm_res)
# 256x128 tiles: 1, W - 1 = 255 = 51 x 5, W = 32 x 8, W + 1 = 257 x 1, 2 W + 3 = 515 = 103 x 5
GRES_SHAPES = ((256, 128), (13056, 640), (8192, 1024), (65792, 128), (26368, 640))


def persistent_cases():
    out = []
    for dt in PLAIN16:
        for (M, N) in G256_SHAPES:
            for K in PERSISTENT_K:
                out.append(make_case(dt, M, N, K, EPI_BIAS_16))
    for dt in SPLIT:                                # one term on a 256-tile shape: gemm256_kernel's split form
        out.append(make_case(dt, 4096, 4096, 192, EPI_BIAS_16, terms=1))
    for dt, terms in (("fp16x3", 3), ("bf16x3", 3), ("fp16x3", 2)):
        for si, (M, N) in enumerate(X3_SHAPES):
            for ki, K in enumerate(PERSISTENT_K):
                for epi in (EPI_BIAS_16, EPI_RESID_F32, EPI_BIAS_F32):
                    out.append(make_case(dt, M, N, K, epi, terms=terms,
                                         oscale=1.0 if (si + ki + epi) % 2 == 0 else 2.0 ** -12,
                                         has_bias=not (epi == EPI_BIAS_F32 and ki == 1)))
        for (M, N), K in ((X3_TWO_ROUNDS, 192), (X3_SEAM, 192), (X3_SEAM, 128)):
            for epi in (EPI_BIAS_16, EPI_RESID_F32, EPI_BIAS_F32):
                out.append(make_case(dt, M, N, K, epi, terms=terms, oscale=2.0 ** -12 if epi == EPI_RESID_F32 else 1.0))
    # gemm_res forced: the smallest K each term form admits (plain and one term: two K-tiles; three terms: one), every
    # tile count; odd K-tile counts at W + 1 tiles
    for dt, terms, kmin in (("bf16", 1, 128), ("fp16", 1, 128), ("fp16x3", 3, 64), ("bf16x3", 3, 64), ("fp16x3", 1, 128)):
        for (M, N) in GRES_SHAPES:
            ks = (kmin, 192, 320) if (M, N) == GRES_SHAPES[3] else (kmin,)
            for K in ks:
                for epi, bias in ((EPI_RESID_F32, True), (EPI_RESID_F32, False), (EPI_BIAS_F32, True), (EPI_BIAS_F32, False)):
                    out.append(make_case(dt, M, N, K, epi, terms=terms, has_bias=bias, force="gres",
                                         oscale=2.0 ** -12 if (dt in SPLIT and epi == EPI_BIAS_F32) else 1.0))
    return out


PERSISTENT_CASES = persistent_cases()

# (c) plane offsets: lo planes farther away than the adjacent offset (an engine with spare batch capacity), and 2^32 bytes or more
FAR = 2 ** 31 + 4096                                # elements of a 16-bit plane: 2^32 bytes + 8 KiB
OFFSET_CASES = [make_case(dt, M, N, K, epi, terms=3, force=f, a_gap=ag, w_gap=wg, c_gap=cg)
                for dt in SPLIT
                for (M, N, K, f) in ((129, 136, 72, "128"), (65, 72, 192, "128"), (3328, 4096, 192, ""))
                for epi in (EPI_BIAS_16, EPI_BIAS_F32)
                for (ag, wg, cg) in ((8, 4096, 1000 * 8), (FAR, 24, FAR))]

ALL_EXACT_CASES = [c for dt in DTYPES for c in EDGE_CASES[dt]] + PERSISTENT_CASES + OFFSET_CASES


# ---- operands and references ---------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(shape, mx, g, dev):
    return torch.randint(-mx, mx + 1, shape, generator=g, device=dev, dtype=torch.int32)


def operands(c, dev):
    """the integer operands of a shape (the same for every epilogue, term count and scale of that shape and dtype): dict of
    fp32 tensors Ah, Wh (integers) and, split modes, Al, Wl (integers times 2^-6), all exactly representable in 16 bits"""
    g = torch.Generator(device=dev)
    g.manual_seed(_seed(c.dtype, c.M, c.N, c.K, c.amax))
    o = {"Ah": _ints((c.M, c.K), c.amax, g, dev).float(), "Wh": _ints((c.N, c.K), c.amax, g, dev).float()}
    if c.split:
        o["Al"] = _ints((c.M, c.K), c.amax, g, dev).float() * LO_UNIT
        o["Wl"] = _ints((c.N, c.K), c.amax, g, dev).float() * LO_UNIT
    return o


def epilogue_operands(c, dev):
    """(bias fp32 [N] of integers or None, residual fp32 [M, N] of integers or None)"""
    g = torch.Generator(device=dev)
    g.manual_seed(_seed(c.dtype, c.M, c.N, c.K, c.epi, c.bias_max, "epi"))
    bias = _ints((c.N,), c.bias_max, g, dev).float() if c.has_bias else None
    res = _ints((c.M, c.N), c.res_max, g, dev).float() if c.epi == EPI_RESID_F32 else None
    return bias, res


def products(o, terms, split):
    """the exact sum of the product terms, float64 [M, N] (every value a multiple of 2^-6 far below 2^53)"""
    Ah, Wh = o["Ah"].double(), o["Wh"].double()
    if not split or terms == 1:
        return Ah @ Wh.t()
    acc = Ah @ (Wh + o["Wl"].double()).t()
    if terms == 3:
        acc += o["Al"].double() @ Wh.t()
    return acc


def products_int64(o, terms, split):
    """the same sum in integer arithmetic on the host, in units of 2^-6: numpy int64 [M, N] (the small shapes' reference)"""
    i = lambda t, scale: np.rint(t.cpu().numpy().astype(np.float64) * scale).astype(np.int64)      # noqa: E731
    Ah, Wh = i(o["Ah"], 1), i(o["Wh"], 1)
    acc = (Ah @ Wh.T) * 64
    if split and terms >= 2:
        acc += Ah @ i(o["Wl"], 64).T
    if split and terms == 3:
        acc += i(o["Al"], 64) @ Wh.T
    return acc


def value(c, acc64, bias, res):
    """the epilogue's value in float64 and, checked to be the same number, in fp32"""
    v = acc64 * (c.oscale if c.split else 1.0)
    if bias is not None:
        v = v + bias.double()
    if res is not None:
        v = v + res.double()
    v32 = v.float()
    assert torch.equal(v32.double(), v), "the case left the exact regime (bit_budget)"
    return v32


def split_planes(v32, td):
    """hi = RN16(v), lo = RN16(v - hi): the two-rounding split (common.h split16x4, mnx_cast16)"""
    hi = v32.to(td)
    return hi, (v32 - hi.float()).to(td)


def expected(c, acc64, bias, res):
    """dict of the output tensors a kernel must produce bit for bit: "f32", or "hi" (+ "lo" for two planes)"""
    v32 = value(c, acc64, bias, res)
    if not c.out16:
        return {"f32": v32}
    td = OPERAND_T[c.dtype]
    if not c.split:
        return {"hi": v32.to(td)}
    hi, lo = split_planes(v32, td)
    return {"hi": hi, "lo": lo} if c.planes == 2 else {"hi": hi}


def dot_bound(A, W, bias, res):
    """per-element bound of an fp32 dot product in any order plus the epilogue's additions, float64 [M, N]:
    |err| <= (K + 3) 2^-24 (sum_k |a_mk| |w_nk| + |b_n| + |r_mn|)"""
    K = A.shape[1]
    s = A.double().abs() @ W.double().abs().t()
    if bias is not None:
        s = s + bias.double().abs()
    if res is not None:
        s = s + res.double().abs()
    return (K + 3) * 2.0 ** -24 * s


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grid(n, dev):
    """n fp32 arguments: dense on [-6, 6], and +-0, +-1e-30, +-20, +-100 (n >= 16)"""
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0], dtype=torch.float32)
    x = torch.cat([torch.linspace(-6.0, 6.0, n - special.numel(), dtype=torch.float64).float(), special])
    return x.to(dev)


def half_ulp16(x, td):
    """half an ulp of the 16-bit format at |x| (float64 tensor), subnormals included"""
    p, emin = (11, -14) if td == torch.float16 else (8, -126)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return 2.0 ** (e - p)


# ---- guarded buffers -----------------------------------------------------------------------------------------------------
# NaN patterns: a stray WRITE changes them, and a stray READ of an operand carries a NaN into the output
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA}
WORD_T = {4: torch.int32, 2: torch.int16}
BAND = 1 << 16                                      # far planes: sentinel elements written and checked on each side of a plane


def words(t):
    return t.view(WORD_T[t.element_size()])


class Planes:
    """One or two planes of `shape` elements of dtype td inside one buffer: `before` sentinel elements, the hi plane, and
    (lo_off given) the lo plane lo_off elements behind the hi plane's start, `after` sentinel elements. Everything that is
    not a plane holds the sentinel; when the planes are far apart (lo_off past 2^24 elements) the buffer is torch.empty and
    only bands of BAND elements around each plane are written and checked."""

    def __init__(self, shape, td, dev, lo_off=None, before=GAP, after=GAP):
        self.n = int(np.prod(shape))
        self.td, self.before, self.lo_off = td, before, lo_off
        self.starts = [before] + ([before + lo_off] if lo_off is not None else [])
        assert lo_off is None or lo_off >= self.n
        self.total = self.starts[-1] + self.n + after
        wt = WORD_T[torch.empty((), dtype=td).element_size()]
        self.far = lo_off is not None and lo_off - self.n > (1 << 24)
        if self.far:
            self.raw = torch.empty(self.total, dtype=wt, device=dev)
            for a, b in self._outside():
                self.raw[a:b] = SENTINEL[td]
        else:
            self.raw = torch.full((self.total,), SENTINEL[td], dtype=wt, device=dev)
        view = lambda s: self.raw[s:s + self.n].view(td).view(shape)      # noqa: E731
        self.hi = view(self.starts[0])
        self.lo = view(self.starts[1]) if lo_off is not None else None

    def _outside(self):
        """the (start, end) ranges outside the planes that hold the sentinel"""
        if not self.far:
            edges = [0] + [x for s in self.starts for x in (s, s + self.n)] + [self.total]
            return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2) if edges[i + 1] > edges[i]]
        out = []
        for s in self.starts:
            out += [(max(0, s - BAND), s), (s + self.n, min(self.total, s + self.n + BAND))]
        return out

    def intact(self):
        return all(bool((self.raw[a:b] == SENTINEL[self.td]).all()) for a, b in self._outside())

    def put(self, hi, lo=None):
        self.hi.copy_(hi.to(self.td))
        if lo is not None:
            self.lo.copy_(lo.to(self.td))
        return self


def guarded(shape, dtype, dev, before=GAP, after=GAP):
    """a view of `shape` into a larger buffer whose surroundings hold the NaN sentinel; guards_intact(view) checks them"""
    return Planes(shape, dtype, dev, before=before, after=after).hi


def guards_intact(t):
    """True when every element around a guarded() view still holds the sentinel"""
    raw = torch.empty(0, dtype=WORD_T[t.element_size()], device=t.device).set_(t.untyped_storage())
    off, n, s = t.storage_offset(), t.numel(), SENTINEL[t.dtype]
    return bool((raw[:off] == s).all()) and bool((raw[off + n:] == s).all())


def first_difference(got, exp, tile=(128, 128)):
    """None when the words are equal, else a line naming the first differing element, its tile and the count"""
    gw, ew = words(got), words(exp)
    if torch.equal(gw, ew):
        return None
    bad = (gw != ew).nonzero()
    m, n = (int(x) for x in bad[0])
    return (f"{bad.shape[0]} of {gw.numel()} words differ; first at [{m}, {n}] (tile {m // tile[0]}, {n // tile[1]} of "
            f"{tile[0]}x{tile[1]}): got {got[m, n].item()!r}, expected {exp[m, n].item()!r}")


# ---- numpy emulation of a tiled kernel and its mutants (tests/test_gemm_ref_host.py) ------------------------------------------
def round16_np(v32, td, mode="rne"):
    """fp32 numpy array -> the 16-bit format's value as fp32 (bit arithmetic, independent of torch): RN-even or toward zero"""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    if td == torch.bfloat16:
        b = v32.view(np.uint32).astype(np.uint64)
        if mode == "rne":
            b = b + 0x7FFF + ((b >> 16) & 1)
        return ((b >> 16) << 16).astype(np.uint32).view(np.float32)
    h = v32.astype(np.float16)                                  # numpy converts RN-even
    if mode == "rtz":
        over = np.abs(h.astype(np.float32)) > np.abs(v32)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


MUTANTS = ("drop_last_ktile", "first_ktile_twice", "stale_slot", "lo_lo", "lo_at_MK", "round_toward_zero", "tile_transposed",
           "bias_by_row")


def emulate(c, o, bias, res, rng, mutant=None, tile=(128, 64)):
    """A tiled GEMM in numpy: K-tiles of 64 in four 16-wide k-slots, the (K-tile, term, slot) partial products added into an
    fp32 accumulator in a shuffled order; the operands are read from flat buffers with the planes at their offsets, as a
    kernel reads them. Returns the dict of expected()'s keys as fp32 numpy arrays (16-bit outputs as their fp32 values)."""
    M, N, K = c.shape
    f = lambda t: t.cpu().numpy().astype(np.float32)            # noqa: E731
    a_lo, w_lo = M * K + c.a_gap, N * K + c.w_gap
    bufA = np.full(a_lo + M * K + GAP, np.nan, np.float32)
    bufW = np.full(w_lo + N * K + GAP, np.nan, np.float32)
    bufA[:M * K], bufW[:N * K] = f(o["Ah"]).ravel(), f(o["Wh"]).ravel()
    if c.split:
        bufA[a_lo:a_lo + M * K], bufW[w_lo:w_lo + N * K] = f(o["Al"]).ravel(), f(o["Wl"]).ravel()
    plane = lambda buf, off, r: buf[off:off + r * K].reshape(r, K)        # noqa: E731
    Ah, Wh = plane(bufA, 0, M), plane(bufW, 0, N)
    Al = plane(bufA, M * K if mutant == "lo_at_MK" else a_lo, M) if c.split else None
    Wl = plane(bufW, w_lo, N) if c.split else None
    terms = [(Ah, Wh)]
    if c.split and c.terms >= 2:
        terms.append((Ah, Wl))
    if c.split and c.terms == 3:
        terms.append((Al, Wh))
    if mutant == "lo_lo" and c.split:
        terms.append((plane(bufA, a_lo, M), Wl))
    nk = (K + 63) // 64
    steps = [(kt, ti, s) for kt in range(nk) for ti in range(len(terms)) for s in range(4) if kt * 64 + s * 16 < K]
    if mutant == "drop_last_ktile":
        steps = [x for x in steps if x[0] != nk - 1]
    if mutant == "first_ktile_twice":
        steps += [x for x in steps if x[0] == 0]
    rng.shuffle(steps)
    acc = np.zeros((M, N), np.float32)
    for kt, ti, s in steps:
        A_, W_ = terms[ti]
        k0 = kt * 64 + s * 16
        k1 = min(k0 + 16, K)
        ks = k0 - 64 if (mutant == "stale_slot" and kt == nk - 1 and s == 0 and kt > 0) else k0   # the other buffer: the previous K-tile
        acc += (A_[:, ks:ks + (k1 - k0)] @ W_[:, ks:ks + (k1 - k0)].T).astype(np.float32)
    v = acc * np.float32(c.oscale if c.split else 1.0)
    if bias is not None:
        b = f(bias)
        v = v + (b[np.arange(M) % N][:, None] if mutant == "bias_by_row" else b[None, :])
    if res is not None:
        v = v + f(res)
    v = v.astype(np.float32)
    if mutant == "tile_transposed" and M > tile[0] and N > tile[1]:
        # output tile (0, 1) lands at tile coordinates (1, 0); its own place keeps what the buffer held (zero here)
        tm, tn = tile
        h, w = min(tm, M - tm), min(tn, N - tn)
        moved = v[:h, tn:tn + w].copy()
        v[:tm, tn:2 * tn] = 0
        v[tm:tm + h, :w] = moved
    if not c.out16:
        return {"f32": v}
    td = OPERAND_T[c.dtype]
    mode = "rtz" if mutant == "round_toward_zero" else "rne"
    hi = round16_np(v, td, mode)
    if not c.split:
        return {"hi": hi}
    lo = round16_np(v - hi, td, mode)
    return {"hi": hi, "lo": lo} if c.planes == 2 else {"hi": hi}
