"""CPU restatement of the decoder's K / V cache format (molnextr_amd/csrc/kvq.h), bit for bit. Test infrastructure only.

A cached row is the 32 channels of one (owner, layer, head, position). kvq_quant stores it as
    e = frexp(amax)'s exponent (amax = max |v| over the row, NaN ignored; amax = 0 gives e = 0), clamped to [-100, 120]
    q = rint(clamp(v * 2^(23 - e), -2^23, 2^23 - 1))      (round half to even; NaN -> -2^23, as fmaxf drops it)
    scale = 2^(e - 23)
and a block (the nk rows of one owner and head) lays them out as [nk][32] int16 hi | [nk][32] uint8 lo | [nk] float32 scale,
q = hi * 256 + lo.
"""
import numpy as np

ROW_BYTES, HI_BYTES, LO_BYTES = 100, 64, 32
E_MIN, E_MAX = -100, 120


def rows(n):
    """kvq_rows: n rounded up to a multiple of 4."""
    return (n + 3) & ~3


def quant(v):
    """v float32 [..., 32] -> (q int64 [..., 32], scale float32 [...]) exactly as kvq_quant stores them."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        amax = np.fmax.reduce(np.abs(v), axis=-1)                       # fmaxf ignores NaN
        _, e = np.frexp(amax)                                           # 0 for 0, inf and NaN, as on the device
        e = np.clip(e.astype(np.int64), E_MIN, E_MAX)
        up = np.ldexp(np.float32(1.0), (23 - e).astype(np.int32)).astype(np.float32)
        scale = np.ldexp(np.float32(1.0), (e - 23).astype(np.int32)).astype(np.float32)
        x = v * up[..., None]                                           # float32, exact (power-of-two scale)
        x = np.fmin(np.fmax(x, np.float32(-8388608.0)), np.float32(8388607.0))
        q = np.rint(x).astype(np.int64)
    return q, scale


def dequant(q, scale):
    """The value a reader sees: q * scale, exact in float32."""
    return (np.asarray(q, np.float64) * np.asarray(scale, np.float64)[..., None]).astype(np.float32)


def parse_block(raw, nk):
    """Raw bytes of one block (uint8 [nk * 100]) -> (q int64 [nk, 32], scale float32 [nk])."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).reshape(-1)[:nk * ROW_BYTES])
    hi = raw[:nk * HI_BYTES].view(np.int16).reshape(nk, 32).astype(np.int64)
    lo = raw[nk * HI_BYTES:nk * (HI_BYTES + LO_BYTES)].reshape(nk, 32).astype(np.int64)
    scale = raw[nk * (HI_BYTES + LO_BYTES):].view(np.float32).copy()
    return hi * 256 + lo, scale


def pack_block(q, scale):
    """(q int [nk, 32], scale float32 [nk]) -> the raw bytes of a block, as the writers lay it out (uint8 [nk * 100])."""
    q = np.asarray(q, dtype=np.int64)
    hi = (q >> 8).astype(np.int16)
    lo = (q & 255).astype(np.uint8)
    return np.concatenate([hi.reshape(-1).view(np.uint8), lo.reshape(-1), np.asarray(scale, np.float32).view(np.uint8)])


# ---- rows the cache must store exactly (tests/test_kvq_host.py, tests/test_gpu_kvcache.py) -----------------------------------
def _row(vals, fill=0.0):
    r = np.full(32, fill, np.float32)
    r[:len(vals)] = np.asarray(vals, np.float32)
    return r


def edge_rows():
    """{name: float32 [32]} the rows the cache writers must store exactly; finite ones first (nonfinite_rows: the others)."""
    rows = {"zeros": _row([])}
    for k in (-20, -1, 0, 7, 30):
        s = 2.0 ** k
        qn = 2.0 ** (k - 22)                     # max 2^k: e = k + 1, quantum 2^(k + 1 - 23)
        # mixed signs and exact half-quantum ties, even and odd integer parts (round half to even goes both ways)
        rows[f"pow2_{k}"] = _row([s, -s / 2, 0.5 * qn, 1.5 * qn, -2.5 * qn, -3.5 * qn, 1000.5 * qn, -1001.5 * qn, s / 3, -s / 7])
        rows[f"neg_pow2_{k}"] = _row([-s, s / 2, 4.5 * qn, -5.5 * qn, 0.25 * qn, -0.75 * qn])
        below = s * (1 - 2.0 ** -24)             # just below 2^k: e = k, x = 2^23 - 1/2 -> +(2^23 - 1) and -2^23
        rows[f"below_pow2_{k}"] = _row([below, -below, s / 2, -s / 4 - 0.5 * 2.0 ** (k - 23)])
        rows[f"above_pow2_{k}"] = _row([s * (1 + 2.0 ** -23), -s * (1 + 2.0 ** -23), s / 2, 0.5 * qn])
    rows["denormal"] = _row([2.0 ** -149, -3 * 2.0 ** -149, 2.0 ** -127, -(2.0 ** -126 - 2.0 ** -149)])
    rows["low_clamp_126"] = _row([2.0 ** -126, -1.5 * 2.0 ** -127, 2.0 ** -140])
    rows["low_clamp_110"] = _row([1.3 * 2.0 ** -110, -2.0 ** -111, 2.0 ** -120, 2.0 ** -125])
    rows["low_clamp_101"] = _row([1.999 * 2.0 ** -101, -2.0 ** -124, 3 * 2.0 ** -126])
    rows["high_clamp_120"] = _row([2.0 ** 120, -1.5 * 2.0 ** 119, 2.0 ** 90, -1.0])
    rows["high_clamp_121"] = _row([1.5 * 2.0 ** 121, -2.0 ** 121, 2.0 ** 97 * 3.5, 1.0])
    rows["high_clamp_127"] = _row([np.float32(3.0e38), -np.float32(3.4e38), 2.0 ** 100, -2.0 ** 98])
    rows["large_among_tiny"] = _row([1000.0] + [1e-5 * (-1) ** i * (i + 1) for i in range(31)])
    g = np.random.default_rng(11)
    for s in (-30, -8, -1, 0, 2, 9, 30):
        rows[f"random_1e{s}"] = (g.standard_normal(32) * 10.0 ** s).astype(np.float32)
    return rows


def nonfinite_rows():
    return {"nan_in_row": _row([np.nan, 1.5, -3.0, 0.25]), "pos_inf": _row([np.inf, 1.0, -2.0]),
            "neg_inf": _row([-np.inf, 1.0, 2.0]), "all_nan": np.full(32, np.nan, np.float32),
            "nan_and_inf": _row([np.nan, np.inf, -np.inf, 7.0])}


# ---- the key-boundary decode (tests/test_kvq_host.py, tests/test_gpu_kvcache.py) -------------------------------------
# Row lengths at which the attention readers change behaviour: 32-key value blocks, the end of the value prefetch (160),
# the second key per thread (256), and the full 512-key score array. The 512 row comes last, so that leaving it out (an
# engine of max_len 511) changes no other row's rank in the compacted batch, i.e. its positional-encoding row.
BOUNDARY_LENS = (2, 31, 32, 33, 160, 161, 256, 257, 511, 512)


def boundary_case(n_mem=144, enc_dim=1024, vocab=229, eos=2, lens=BOUNDARY_LENS):
    """hash_normal features [B, n_mem, enc_dim] and forced ids [B, max(lens)] that end with EOS at lens[b] - 1 (the last row
    fills max(lens)): ids are drawn from 3 .. vocab - 1, never EOS before the end."""
    import torch
    from molnextr_amd.weights import hash_normal
    B, T = len(lens), max(lens)
    feats = hash_normal("kvq_boundary_features", (B, n_mem, enc_dim), 1.0)
    ids = torch.from_numpy(np.random.default_rng(2024).integers(3, vocab, size=(B, T))).long()
    for b, n in enumerate(lens):
        if n < T:
            ids[b, n - 1] = eos
            ids[b, n:] = eos
    return feats, ids, list(lens)


# tests/test_gpu_kvcache.py derives this tolerance; tests/test_kvq_host.py shows that a 16-bit cache or one dropped key exceeds it
# tenfold on the boundary case
LOGIT_TOL_C = 32


def logit_tolerance(ref_logits):
    """Bound on |engine logit - float64 logit| over a decode: LOGIT_TOL_C * 2^-24 * max |logit| of the float64 decode."""
    import torch
    return LOGIT_TOL_C * 2.0 ** -24 * float(torch.nan_to_num(ref_logits.abs(), nan=0.0).max())
