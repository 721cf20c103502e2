"""float64 restatement, inputs, crafted checkpoints and the derived tolerance of the bond head (edge_gather_kernel, the
512-column sgemm_tn_kernel launch, edge_pair_kernel, edge_sym_kernel), shared by tests/test_edges_host.py (CPU: shows that
the tolerance is neither vacuous nor tight and that every coverage condition holds) and tests/test_gpu_edges.py (GPU: judges
the kernels with it). torch / numpy on the CPU only; nothing here touches the library.

The reference (probs64) is the reference's own form, MolNexTR/components.py:365-377 as oracle/edges.py restates it: gather,
concat [h_i | h_j], Linear(512, 256), erf-GELU, Linear(256, 7), softmax — every step in float64 on the kernel's own fp32
inputs, not split into the two half-Linears the kernels use. symmetrise_exact is get_edge_prediction (:383-400) on fp32
probabilities: a conversion, one double add and one halving per value, then the first maximum; every step is one IEEE double
operation, so its result is unique to the last bit and is compared with the device's as words.

The probability tolerance (prob_tol). u = 2^-24. What the kernels compute per pair (i, j) and the roundings they commit:
  U_i[c] = sum_t W1[c, t] h_i[t]            a chain of 256 fmaf in the order t = 0..255 from 0 (sgemm_tn_kernel)
  V_j[c] = sum_t W1[c, 256 + t] h_j[t] + b1[c]   the same chain, then one add
  a[c]   = U_i[c] + V_j[c]                  one add
  z[c]   = 0.5 a (1 + erff(a * 0.70710678))  one product, erff, one add, one product (the halving is exact)
  o[k]   = b2[k] + sum_c z[c] W2[k, c]       a chain of 256 fmaf in the order c = 0..255 from b2[k]
  p[k]   = expf(o[k] - max o) / sum_k expf(o[k] - max o)    one subtraction, expf, 6 adds, one division
A worst-case bound is of no use here: gamma_256 = 256 u on sum |W1| |h| (about 14) already allows 2e-4 per first-layer output,
three orders of magnitude over what fp32 arithmetic does, and nothing wrong short of garbage would exceed it. The bound below
is the probabilistic one (Higham & Mary, "A new approach to probabilistic rounding error analysis", SIAM J. Sci. Comput. 41,
2019; Hoeffding's inequality): every rounding replaces a value x by x (1 + d), |d| <= u, and the d of different operations
are taken as independent with mean zero. Then a first-order error sum_n d_n x_n of any number of roundings satisfies
    |sum_n d_n x_n| <= LAMBDA u sqrt(sum_n x_n^2)    with probability >= 1 - 2 exp(-LAMBDA^2 / 2).
q(v) below is that sum of squares for a value v, built from the float64 reference's own quantities:
  a chain      every fmaf rounds its partial sum s_t:                     q(U_i[c]) = sum_t s_t^2   (s_t in the chain's order)
  V            the same, and the bias add rounds V:                       q(V) = sum_t s_t^2 + V^2
  a            q(a) = q(U) + q(V) + a^2
  GELU         z = a Phi(a), z' = Phi(a) + a phi(a). The argument's product moves Phi by a phi(a) d, so z by a^2 phi(a) d;
               erff is taken as 4 ulp: 4 u |erf|, times a / 2; the add and the last product each round about z:
               q(z) = z'(a)^2 q(a) + (a^2 phi(a))^2 + (2 a erf(a / sqrt 2))^2 + 2 z^2
  logit        the chain rounds its partial sums S_c (which start at b2[k]):   qc(o[k]) = sum_c S_c^2, and o[k] carries
               sum_c W2[k, c] dz[c] besides, the errors dz[c] of the 256 z[c] being independent (different chains)
  softmax      dp_k = p_k (do[k] - sum_d p_d do[d]). The seven logits of a pair share the dz[c], so they are NOT independent and
               the dz[c] are collected first: with wbar[c] = sum_d p_d W2[d, c],
                 dp_k / p_k = sum_c (W2[k, c] - wbar[c]) dz[c] + (1 - p_k) chain_k - sum_{d != k} p_d chain_d + (softmax's own).
               Its own arithmetic: x_k = o[k] - max o is rounded (it moves the exponential by x_k d) and expf is taken as
               2 ulp (q += 4), so every term e_k has the relative qe_k = x_k^2 + 4 and enters p_k as the chain error does;
               the 6 adds round partial sums that are at most the sum (q += 6, relative), the division rounds p (q += 1):
                 q(p_k) / p_k^2 = sum_c (W2[k, c] - wbar[c])^2 q(z[c]) + (1 - p_k)^2 (qc_k + qe_k)
                                  + sum_{d != k} p_d^2 (qc_d + qe_d) + 7
  tol_k = LAMBDA u sqrt(q(p_k)): one statement per probability.
LAMBDA. The tests compare fewer than 5e6 probabilities (7 k^2 summed over the molecules of every case, on two engines).
2 * 5e6 * exp(-LAMBDA^2 / 2) <= 1e-3 needs LAMBDA >= 6.8: LAMBDA = 7 (2e-4). Hoeffding's bound charges every rounding its
largest size u, where the standard deviation of a rounding is about 0.4 u: the largest of 1e6 honest fp32 errors (5 standard
deviations) is expected near 2 u sqrt q, 0.3 of the tolerance. tests/test_edges_host.py asserts that the fp32 CPU restatement
(oracle/edges.edge_logits + softmax) stays within half. On the synthetic checkpoint (|logit| <= 3.2) the largest tol of any
case is 3.6e-6, eight times the 4.5e-7 that restatement measures, and the tolerance of most probabilities is far smaller (it
scales with p); the wrong variants that test_edges_host.py names exceed it 118-fold (tanh-GELU) to 3e6-fold. Measured: the
restatement reaches 0.30 of the tolerance, the kernels on an MI355X 0.33 (0.41 on the crafted equal-class checkpoint, whose
logit chains start at a bias of 5); profiles/edges_tolerances.json.
"""
import functools
import math

import numpy as np
import torch

from molnextr_amd import weights as W
from oracle.edges import PE_, edge_logits, symmetrise

U32 = 2.0 ** -24
LAMBDA = 7.0
D = 256
TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
DEC = W.DecoderDims(enc_dim=TINY.num_features)


# ---- checkpoints ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def checkpoint(kind="synthetic"):
    """The tiny-encoder synthetic checkpoint (the bond head uses nothing of the encoder) and the two crafted ones:
    'equal'  rows 1 and 3 of mlp.2.weight and entries 1 and 3 of mlp.2.bias are equal and the bias is raised: o[1] == o[3] bit
             for bit on every pair, an exact tie of the two largest classes nearly everywhere — class 1 must win it.
    'wedges' bias + 3 on classes 5 and 6: with two atoms at one decoder position p_ij == p_ji word for word, so
             e5 = (p5 + p6) / 2 = e6 exactly in both triangles — class 5 must win at (i, j) and at (j, i)."""
    ck = W.synthetic_checkpoint(0, enc=TINY, dec=DEC)
    if kind == "synthetic":
        return ck
    dec = dict(ck["decoder"])
    w2, b2 = dec[PE_ + "mlp.2.weight"].clone(), dec[PE_ + "mlp.2.bias"].clone()
    if kind == "equal":
        w2[3] = w2[1]
        b2[1] = b2[3] = 5.0
    elif kind == "wedges":
        b2[5] += 3.0
        b2[6] += 3.0
    else:
        raise KeyError(kind)
    dec[PE_ + "mlp.2.weight"], dec[PE_ + "mlp.2.bias"] = w2, b2
    return {"encoder": ck["encoder"], "decoder": dec}


def head_weights(sd, dtype=torch.float64):
    return tuple(sd[PE_ + n].to(dtype) for n in ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"))


# ---- inputs ---------------------------------------------------------------------------------------------------------
class Case:
    """hidden fp32 [B, max_len, 256] unit normal; idx int32 [B, kmax] (zero beyond ks[b]); ks; ckpt kind; engine max_atoms"""

    def __init__(self, name, hidden, idx, ks, ckpt="synthetic", max_atoms=160, random=True):
        self.name, self.hidden, self.idx, self.ks, self.ckpt, self.max_atoms = name, hidden, idx, list(ks), ckpt, max_atoms
        self.random = random               # distinct-position random inputs: the coverage and margin conditions apply
        self.B, self.max_len, _ = hidden.shape
        self.kmax = idx.shape[1]

    def single(self, b):
        """molecule b as a B = 1 case of the same kmax"""
        return Case(f"{self.name}[{b}]", self.hidden[b:b + 1].contiguous(), self.idx[b:b + 1].contiguous(), [self.ks[b]],
                    self.ckpt, self.max_atoms, self.random)


def positions(tag, k, max_len):
    """k sorted decoder positions: distinct where k <= max_len, otherwise position i * max_len // k (each at most
    ceil(k / max_len) times)"""
    if k > max_len:
        return torch.arange(k, dtype=torch.int64).mul(max_len).div(k, rounding_mode="floor").int()
    order = torch.argsort(W.hash_normal(f"edges_pos_{tag}", (max_len,), 1.0))
    return torch.sort(order[:k])[0].int()


def _build(name, ks, kmax, max_len, **kw):
    hidden = W.hash_normal(f"edges_hidden_{name}", (len(ks), max_len, D), 1.0)
    idx = torch.zeros(len(ks), kmax, dtype=torch.int32)
    for b, k in enumerate(ks):
        idx[b, :k] = positions(f"{name}_{b}", k, max_len)
    return Case(name, hidden, idx, ks, **kw)


B1_KS = (1, 2, 63, 64, 65, 159, 160)
B32_KS = (0, 1, 160, 2, 3, 5, 7, 11, 16, 23, 31, 32, 33, 40, 47, 48, 55, 63, 64, 65, 70, 77, 85, 95, 96, 97, 100, 128, 9, 12,
          20, 0)
RANDOM_CASES = tuple(f"k{k}" for k in B1_KS) + ("k5_kmax8", "b3_kmax72", "b32")
BIG_CASES = ("m256",)
CRAFTED_CASES = ("equal", "wedges")
WEDGE_REPEAT = 3


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("k%d" % k for k in B1_KS):
        return _build(name, [int(name[1:])], 160, 480)
    if name == "k5_kmax8":
        return _build(name, [5], 8, 40)
    if name == "b3_kmax72":
        return _build(name, [65, 0, 7], 72, 200)
    if name == "b32":                  # max_len 96: molecules of more than 96 atoms repeat positions
        return _build(name, B32_KS, 160, 96)
    if name == "m256":
        return _build(name, [256, 255], 256, 480, max_atoms=256)
    if name == "equal":
        return _build(name, [70, 3], 72, 120, ckpt="equal", random=False)
    if name == "wedges":               # 22 positions, each held by three consecutive atoms, and one molecule without repeats
        c = _build(name, [66, 9], 72, 120, ckpt="wedges", random=False)
        c.idx[0, :66] = positions("wedges_rep", 22, 120).repeat_interleave(WEDGE_REPEAT)
        return c
    if name == "clamp":                # positions out of range among valid ones (not sorted, not distinct once clamped)
        c = _build(name, [12, 7], 16, 50, random=False)
        c.idx[0, :12] = torch.tensor([-3, 0, 49, 50, 150, 7, -1, 48, 1, 2 ** 31 - 1, -2 ** 31, 23], dtype=torch.int32)
        c.idx[1, :7] = torch.tensor([5, 50, 6, -3, 49, 150, 0], dtype=torch.int32)
        return c
    if name == "natoms":               # the last molecule fills kmax: its count is what the n_atoms test overstates
        return _build(name, [7, 5, 24], 24, 60, random=False)
    raise KeyError(name)


def clamped(c):
    """the same case with every position clamped to 0..max_len-1 on the host"""
    return Case(c.name + "_clamped", c.hidden, c.idx.clamp(0, c.max_len - 1), c.ks, c.ckpt, c.max_atoms, c.random)


# ---- the float64 reference -------------------------------------------------------------------------------------------
def _gelu64(a):
    return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


@torch.no_grad()
def probs64(hidden, idx, sd, chunk=32):
    """hidden fp32 [T, 256], idx [k] (valid positions) -> float64 [k, k, 7]: softmax(Linear(GELU(Linear([h_i | h_j]))))"""
    W1, b1, W2, b2 = head_weights(sd)
    h = hidden.double()[torch.as_tensor(idx, dtype=torch.long)]
    k = h.shape[0]
    out = torch.zeros(k, k, 7, dtype=torch.float64)
    for i0 in range(0, k, chunk):
        n = min(chunk, k - i0)
        hh = torch.cat([h[i0:i0 + n, None, :].expand(n, k, D), h[None, :, :].expand(n, k, D)], dim=-1)
        out[i0:i0 + n] = torch.softmax(_gelu64(hh @ W1.T + b1) @ W2.T + b2, dim=-1)
    return out


def _chain_q(h, Wh, chunk=32):
    """value and q of the fmaf chains sum_t Wh[c, t] h[i, t], t = 0..255 in order: -> [k, 256], [k, 256]"""
    val, q = torch.zeros(h.shape[0], Wh.shape[0], dtype=torch.float64), torch.zeros(h.shape[0], Wh.shape[0], dtype=torch.float64)
    for i0 in range(0, h.shape[0], chunk):
        s = torch.cumsum(h[i0:i0 + chunk, None, :] * Wh[None, :, :], dim=-1)
        val[i0:i0 + chunk], q[i0:i0 + chunk] = s[..., -1], (s * s).sum(-1)
    return val, q


@torch.no_grad()
def prob_tol(hidden, idx, sd, chunk=32):
    """the tolerance of the module docstring for every probability: float64 [k, k, 7]"""
    W1, b1, W2, b2 = head_weights(sd)
    h = hidden.double()[torch.as_tensor(idx, dtype=torch.long)]
    k = h.shape[0]
    Uv, Uq = _chain_q(h, W1[:, :D])
    Vv, Vq = _chain_q(h, W1[:, D:])
    Vv = Vv + b1
    Vq = Vq + Vv * Vv
    tol = torch.zeros(k, k, 7, dtype=torch.float64)
    for i0 in range(0, k, chunk):
        a = Uv[i0:i0 + chunk, None, :] + Vv[None, :, :]
        qa = Uq[i0:i0 + chunk, None, :] + Vq[None, :, :] + a * a
        phi = torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
        erf = torch.erf(a / math.sqrt(2.0))
        z = 0.5 * a * (1.0 + erf)
        dz = 0.5 * (1.0 + erf) + a * phi
        qz = dz * dz * qa + (a * a * phi) ** 2 + (2.0 * a * erf) ** 2 + 2.0 * z * z
        o, qc = [], []
        for c in range(7):
            S = b2[c] + torch.cumsum(z * W2[c], dim=-1)
            o.append(S[..., -1])
            qc.append((S * S).sum(-1))
        o, qc = torch.stack(o, -1), torch.stack(qc, -1)
        x = o - o.max(-1, keepdim=True)[0]
        p = torch.softmax(o, dim=-1)
        wbar = p @ W2                                                        # [n, k, 256]: sum_d p_d W2[d, c]
        qe = x * x + 4.0
        own = p * p                                                          # weights of the other classes' terms
        for c in range(7):
            others = (own * qc).sum(-1) - own[..., c] * qc[..., c], (own * qe).sum(-1) - own[..., c] * qe[..., c]
            q = (((W2[c] - wbar) ** 2) * qz).sum(-1) + (1.0 - p[..., c]) ** 2 * (qc[..., c] + qe[..., c]) + others[0] + \
                others[1] + 7.0
            tol[i0:i0 + chunk, :, c] = LAMBDA * U32 * p[..., c] * torch.sqrt(q)
    return tol


@torch.no_grad()
def probs32(hidden, idx, sd):
    """the fp32 CPU restatement: oracle/edges.edge_logits + softmax, as float64 [k, k, 7]"""
    if len(idx) == 0:
        return torch.zeros(0, 0, 7, dtype=torch.float64)
    return torch.softmax(edge_logits(hidden, [int(v) for v in idx], sd), dim=2).double()


def symmetrise_exact(p32):
    """fp32 probabilities [k, k, >= 7] (numpy or torch) -> (class [k, k] int64: the first maximum, score [k, k] float64) of
    get_edge_prediction in float64, exactly as oracle/edges.symmetrise"""
    e = symmetrise(np.asarray(p32, dtype=np.float32)[..., :7].astype(np.float64))
    if e.shape[0] == 0:
        return np.zeros((0, 0), dtype=np.int64), np.zeros((0, 0))
    return np.argmax(e, axis=2), np.max(e, axis=2)


class Ref:
    """per molecule of a case: p64, tol (float64 [k, k, 7]), the float64 winner after symmetrisation and its margin over the
    runner-up"""

    def __init__(self, c):
        sd = checkpoint(c.ckpt)["decoder"]
        self.p64, self.tol, self.cls, self.margin = [], [], [], []
        for b, k in enumerate(c.ks):
            idx = c.idx[b, :k].clamp(0, c.max_len - 1)
            p = probs64(c.hidden[b], idx, sd)
            e = symmetrise(p.numpy())
            top = np.sort(e, axis=2)
            self.p64.append(p.numpy())
            self.tol.append(prob_tol(c.hidden[b], idx, sd).numpy())
            self.cls.append(np.argmax(e, axis=2) if k else np.zeros((0, 0), dtype=np.int64))
            self.margin.append(top[..., 6] - top[..., 5])

    def decided(self, b):
        """the pairs whose float64 margin exceeds twice the largest tolerance of the pair (of either order)"""
        t = self.tol[b].max(axis=2)
        return self.margin[b] > 2.0 * np.maximum(t, t.T)


@functools.lru_cache(maxsize=None)
def reference(name):
    return Ref(case(name))
