"""Inputs, float64 references, exact restatements and derived tolerances of the decode tick's linear kernel
(dec_linear_kernel<PRO, EPI>, csrc/decoder.hip), shared by tests/test_dec_linear_host.py (CPU: shows that every tolerance is
neither vacuous nor tight and that every exact family can tell the wrong variants apart) and tests/test_gpu_dec_linear.py
(GPU: judges the kernel through mnx_dec_linear). torch and numpy on the CPU only; nothing here touches the library.

The six instantiated forms, out[r, n] = epi(pro(in)[r, :] . W[n, :] + b[n]):
  PRO 0 the input as it is | 1 LayerNorm(eps 1e-6, biased variance) of the stream, with `part` of (((p0 + p1) + p2) + p3) + x,
  which column block 0 also writes to x_write | 2 LayerNorm of x0 = emb[tok] * 16 + pe[rank], also written to x_write
  EPI 0 q * 32^-1/2 | K and V rows into the cache (oracle.kvq) | 1 out += | 2 * 32^-1/2 | 3 erf-GELU | 4 K-slice partials,
  the bias in slice 0 alone

Notation: e = 2^-24. Every tolerance is per element and is computed from the float64 reference's own quantities, never from
a kernel's output (encoder_ops_ref.py: ln_tol, sgemm_tol).

Product (PRO 0): sgemm_tol, (K + 2) e (sum_k |a_k| |W_nk| + |b_n|) — any order of K fused or unfused multiply-adds and the bias.
LayerNorm then product (PRO 1, 2): the LayerNorm's output o carries ln_tol (eps 1e-6; a lane sums 8 quads = 32 adds, the
  butterfly over the row's 8 lanes has 3 steps, and the 4 e that encoder_ops_ref's 10 e leaves beyond ITS six butterfly steps
  for the division and the final conversions: delta = (32 + 3 + 4) e), which the product passes on weighted by |W|:
      tol_z[n] = sum_k |W_nk| ln_tol_k + (K + 2) e (sum_k |o_k| |W_nk| + |b_n|)
  The LayerNorm's input is an fp32 stream that is specified word for word (x itself, the hand-over sum, x0), so the float64
  reference starts from those words.
EPI 1: tol_z + e |ref| (the residual add).
EPI 2 and the q columns of EPI 0: the reference multiplies by the fp32 number nearest 32^-1/2 (the operand every fp32
  evaluation has); tol = tol_z * 32^-1/2 + e |ref|: one more rounding.
EPI 3: gelu(z) = z Phi(z). |gelu'| <= 1.1290 (at z = sqrt 2 .. 1.4142), so the error of z arrives multiplied by at most
  GELU_SLOPE = 1.13; the evaluation 0.5 z (1 + erf(z / sqrt 2)) itself: erf to A ulp (A = 4) is A e absolute, the rounding of
  z / sqrt 2 and of the 1 + . add at most 3 e more on the bracket, times |z| / 2; two products, 2 e |gelu(z)|:
      tol = 1.13 tol_z + (A + 3) e |z| / 2 + 2 e |gelu(z)|
K / V columns of EPI 0: the value a reader sees, q * scale of the cached row (oracle.kvq), against the float64 row:
  tol_z + 2^-24 * (the largest |element| of the float64 row of 32 channels), the quantum of oracle.kvq.quant.
EPI 4: plane z is the product over k in [256 z, 256 z + 256) (+ the bias in plane 0): sgemm_tol of the slice.

Exact families (compared word for word):
  integers: in and W in [-7, 7], bias in [-100, 100], the residual of EPI 1 in [-1000, 1000]: every partial sum is an integer
    below 49 * 1024 + 1100 < 2^24, so any correct order of summation gives the int64 result exactly. Probe inputs have ONE
    non-zero element per row, at k = 256 (r mod K/256) + (base + r) mod 256: over the launches of PROBE_BASES every residue
    mod 256 and every 256-chunk is hit, so a swapped chunk, a wrong slice boundary or a k-slot paired with the wrong weight
    changes a word.
  streams: x0 = emb * 16 + pe (emb * 16 is exact, so one rounding whether or not the pair is contracted into an fma) and the
    hand-over sum (((p0 + p1) + p2) + p3) + x, both restated in numpy fp32.
"""
import math

import numpy as np
import torch

import encoder_ops_ref as R
from encoder_ops_ref import E32
from oracle import kvq as KQ

LN_EPS = 1e-6
LN_DELTA = (32 + 3 + 4) * E32
SCALE32 = float(np.float32(32.0 ** -0.5))       # the fp32 number nearest 32^-1/2 (0.17677669529663687f in the kernel)
GELU_SLOPE = 1.13
ERF_ULP = 4
D = 256                                         # d_model: the LayerNorm row, the width of the stream and of a K slice
HEADS, HEAD_DIM = 8, 32

FORMS = ((2, 0), (1, 0), (0, 1), (1, 2), (1, 3), (0, 4))
# (pro, epi) -> the (N, K) production launches it with
FORM_SHAPES = {(2, 0): ((768, 256),), (1, 0): ((768, 256),), (0, 1): ((256, 256), (256, 1024)), (1, 2): ((256, 256),),
               (1, 3): ((1024, 256),), (0, 4): ((256, 1024),)}
# (capacity, n_alive): a lone row, a partial tile, a full tile, a full + a one-row tile, two full tiles, two full + one row, and
# one full + one partial + one idle tile
TICKS = ((32, 1), (32, 31), (32, 32), (64, 33), (64, 64), (96, 65), (96, 33))
DEC_SLOTS, MAX_LEN = 128, 16
PROBE_BASES = (0, 64, 128, 192)                 # four launches of 64 probe rows


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the scripted tick ------------------------------------------------------------------------------------------------------
def script(n_alive, vocab, seed=0, with_slot0=False, max_len=MAX_LEN):
    """int32 [n_alive, 4] = {slot, t, prev_tok, rowc} in installation order: slots scattered over 1..127 (37 and 29 are
    units mod 127 and mod 512: no slot and no rowc repeats for n_alive <= 127), neither contiguous nor sorted, rowc in another
    order than the slots. with_slot0: one entry, not the first, sits in slot 0 at position 0."""
    assert 1 <= n_alive <= 127
    i = np.arange(n_alive)
    rows = np.stack([(5 + 11 * seed + 37 * i) % 127 + 1, (1 + seed + 3 * i) % max_len, (3 + 5 * seed + 7 * i) % vocab,
                     (11 + 29 * i) % 512], axis=1).astype(np.int32)
    if with_slot0:
        rows[n_alive // 2, 0] = 0
        rows[n_alive // 2, 1] = 0
    return rows


def row_view(rows):
    """What dec_begin_kernel makes of a script: (entries [n, 4] in ROW order, rank [n] of each row). Row r is the alive slot
    with the r-th smallest slot number; its PE rank is the number of alive rows (of its chunk: all) with a smaller rowc."""
    rows = np.asarray(rows)
    order = np.argsort(rows[:, 0], kind="stable")
    rank = np.argsort(np.argsort(rows[:, 3], kind="stable"), kind="stable")
    return rows[order], rank[order]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def weights(N, K, seed=0):
    """W [N, K] ~ N(0, 1 / K), bias ~ N(0, 1), gamma = 1 + N(0, 1/4), beta ~ N(0, 1/4) [256]"""
    g = _gen(31 * N + K + 7919 * seed)
    return (torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), 1.0 + 0.5 * torch.randn(D, generator=g),
            0.5 * torch.randn(D, generator=g))


def plain_rows(M, K, seed=0):
    """PRO 0 input [M, K] ~ N(0, 1) and an EPI 1 residual [M, 256]-or-wider source: (x, res [M, 1024])"""
    g = _gen(1 + 17 * K + 7919 * seed)
    return torch.randn(M, K, generator=g), torch.randn(M, 1024, generator=g)


def stream_rows(M, seed=0):
    """A residual stream [M, 256] for the LayerNorm prologue: encoder_ops_ref.ln_inputs' four crafted rows first (mean 100 and
    spread 1; variance 9e-6, where eps decides; offset -5000 at spread 1000; a single non-zero channel), then N(0, 1) rows"""
    x = R.ln_inputs(D, max(M, 4))[0][:M].clone()
    if seed:
        x[4:] = torch.randn(max(M - 4, 0), D, generator=_gen(seed))
    return x


def part_rows(M, n_part=4, seed=0):
    """random K-slice partials [n_part, M, 256] ~ N(0, 1/4); rows 0..3 are zero so that stream_rows' crafted rows survive the sum"""
    p = 0.5 * torch.randn(n_part, M, D, generator=_gen(77 + seed))
    p[:, :4] = 0.0
    return p


def int_weights(N, K, seed=0):
    """W in [-7, 7] without zeros (a probe must see every k), bias in [-100, 100]"""
    g = _gen(5 + N + 3 * K + 7919 * seed)
    Wt = torch.randint(1, 8, (N, K), generator=g) * (2 * torch.randint(0, 2, (N, K), generator=g) - 1)
    return Wt.float(), torch.randint(-100, 101, (N,), generator=g).float()


def int_rows(M, K, N, seed=0):
    """x in [-7, 7] [M, K], residual in [-1000, 1000] [M, N]"""
    g = _gen(9 + M + K + 7919 * seed)
    return torch.randint(-7, 8, (M, K), generator=g).float(), torch.randint(-1000, 1001, (M, N), generator=g).float()


def probe_k(M, K, base):
    """the one k at which probe row r is non-zero"""
    r = np.arange(M)
    return 256 * (r % (K // 256)) + (base + r) % 256


def probe_rows(M, K, base):
    """[M, K] zeros but x[r, probe_k(r)] = a non-zero integer in [-7, 7]"""
    x = torch.zeros(M, K)
    r = torch.arange(M)
    x[r, torch.from_numpy(probe_k(M, K, base))] = ((r % 7) + 1).float() * (1 - 2 * (r % 2)).float()
    return x


def int_product(x, Wt, bias=None):
    """the exact product in int64 -> fp32 (every value below 2^24)"""
    z = x.long() @ Wt.long().t()
    if bias is not None:
        z = z + bias.long()
    assert int(z.abs().max()) < 2 ** 24
    return z.float()


def int_slices(x, Wt, bias):
    """[K / 256, M, N]: the exact EPI 4 planes, the bias in plane 0 alone"""
    planes = [int_product(x[:, k:k + 256], Wt[:, k:k + 256], bias if k == 0 else None) for k in range(0, x.shape[1], 256)]
    return torch.stack(planes)


# ---- the two streams, word for word -------------------------------------------------------------------------------------------
def embed_stream(emb, pe, tok, rank):
    """x0 = emb[tok] * 16 + pe[rank] in numpy fp32 (emb [V, 256], pe [pe_len, 256] fp32 arrays) -> fp32 [n, 256]"""
    emb, pe = np.asarray(emb, np.float32), np.asarray(pe, np.float32).reshape(-1, D)
    return emb[np.asarray(tok)] * np.float32(16.0) + pe[np.asarray(rank)]


def handover_chain(parts, x):
    """(((p0 + p1) + p2) + p3) + x in numpy fp32, one rounding per add, in that order"""
    parts, x = np.asarray(parts, np.float32), np.asarray(x, np.float32)
    s = parts[0]
    for z in range(1, parts.shape[0]):
        s = s + parts[z]
    return s + x


HANDOVER_WRONG = {
    "pairwise tree": lambda p, x: ((p[0] + p[1]) + (p[2] + p[3])) + x,
    "reversed": lambda p, x: (((p[3] + p[2]) + p[1]) + p[0]) + x,
    "x first": lambda p, x: (((x + p[0]) + p[1]) + p[2]) + p[3],
}


def handover_crafted(M, seed=0):
    """(parts [4, M, 256], x [M, 256]) fp32 numpy whose sum depends on the order: every element is drawn from 5-tuples of
    2^24-scale terms that cancel beside ones, threes and halves, kept only where the chain, the pairwise tree, the reversed chain
    and the x-first chain give four answers of which the last three all differ from the first; then scaled by 2^j, j in -3..3
    (exact, so the differences stay)."""
    g = np.random.default_rng(4242)
    big = np.float32(2.0 ** 24)
    pool = np.array([big, -big, big + 2, -(big + 2), 2 * big, -2 * big, 1, -1, 3, -3, 1.5, -1.5, 0.5, 5], np.float32)
    cand = pool[g.integers(0, len(pool), size=(5, 200000))]
    p, x = cand[:4], cand[4]
    want = handover_chain(p, x)
    keep = np.ones(cand.shape[1], bool)
    for f in HANDOVER_WRONG.values():
        keep &= f(p, x) != want
    keep &= (np.abs(cand) >= big).sum(0) >= 2            # at least two large terms: a cancellation, not noise
    cand = cand[:, keep]
    assert cand.shape[1] >= 64
    g = np.random.default_rng(99 + seed)
    pick = cand[:, g.integers(0, cand.shape[1], size=M * D)] * np.exp2(g.integers(-3, 4, size=M * D)).astype(np.float32)
    return pick[:4].reshape(4, M, D).copy(), pick[4].reshape(M, D).copy()


# ---- float64 references and tolerances ----------------------------------------------------------------------------------------
def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_arith_tol(z):
    """the evaluation's own share of the EPI 3 tolerance, for an exact argument z (float64)"""
    return (ERF_ULP + 3) * E32 * z.abs() / 2 + 2 * E32 * gelu64(z).abs()


def product_ref(pro, stream, Wt, bias, gamma=None, beta=None):
    """(z, tol_z) float64 [M, N] of pro(stream) . W^T + b; stream is the fp32 [M, K] the product (PRO 0) or the LayerNorm
    (PRO 1, 2: x, the hand-over sum, x0) reads"""
    if pro == 0:
        return R.sgemm_tol(stream, Wt, bias)
    K = Wt.shape[1]
    o, tl = R.ln_tol(stream, gamma, beta, eps=LN_EPS, delta=LN_DELTA)
    Wd, b = Wt.double(), bias.double()
    return o @ Wd.t() + b, tl @ Wd.abs().t() + (K + 2) * E32 * (o.abs() @ Wd.abs().t() + b.abs())


def epilogue_ref(epi, z, tz, res=None):
    """(ref, tol) float64 of EPI 1, 2, 3 applied to (z, tol_z); EPI 0 -> kv_ref, EPI 4 -> slice_ref"""
    if epi == 1:
        ref = z + res.double()
        return ref, tz + E32 * ref.abs()
    if epi == 2:
        ref = z * SCALE32
        return ref, tz * SCALE32 + E32 * ref.abs()
    assert epi == 3
    return gelu64(z), GELU_SLOPE * tz + gelu_arith_tol(z)


def qkv_ref(z, tz):
    """EPI 0: (q_ref, q_tol [M, 256]) and (kv_ref, kv_tol [M, 512]): columns 256..767, the rows the cache holds"""
    q, tq = epilogue_ref(2, z[:, :D], tz[:, :D])
    kv = z[:, D:]
    amax = kv.abs().reshape(kv.shape[0], 2 * HEADS, HEAD_DIM).amax(-1, keepdim=True).expand(-1, -1, HEAD_DIM)
    return q, tq, kv, tz[:, D:] + E32 * amax.reshape(kv.shape)


def slice_ref(x, Wt, bias):
    """EPI 4: (ref, tol) float64 [K / 256, M, N], the bias in plane 0 alone"""
    out = [R.sgemm_tol(x[:, k:k + 256], Wt[:, k:k + 256], bias if k == 0 else None) for k in range(0, x.shape[1], 256)]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def cache_values(raw, nk, t):
    """the 32 values a reader sees in row t of one raw cache block (uint8 [nk * 100]) -> float32 [32]"""
    q, scale = KQ.parse_block(raw, nk)
    return KQ.dequant(q[t], scale[t])


# ---- fp32 restatements (what an honest kernel computes; the host test shows they pass) ------------------------------------------
def product_fp32(pro, stream, Wt, bias, gamma=None, beta=None, eps=LN_EPS):
    a = stream if pro == 0 else R.ln_fp32_restatement(stream, gamma, beta, eps=eps)
    return a @ Wt.t() + bias


def gelu_fp32(z):
    return 0.5 * z * (1.0 + torch.erf(z * torch.tensor(2.0 ** -0.5, dtype=torch.float32)))


def gelu_tanh(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def kv_fp32(kv32):
    """fp32 [M, 512] -> what the cache gives back: quantised per (row, head) as kvq_quant does"""
    v = kv32.numpy().reshape(kv32.shape[0], 2 * HEADS, HEAD_DIM)
    return torch.from_numpy(KQ.dequant(*KQ.quant(v)).reshape(kv32.shape))


def ratio(got, ref, tol):
    return ((got.double() - ref).abs() / tol).max().item()
