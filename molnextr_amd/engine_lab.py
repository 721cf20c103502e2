"""The test and measurement aids of `class Engine` (engine.py), the Python side of csrc/engine_lab.hip: the encoder tap, the
profile and probe readers, the single-kernel entry points the kernel tests call on caller buffers, and the scripted and forced
beam searches. Nothing a prediction needs lives here; what serves both the product and the tests stays in engine.py."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .abi import IMAGE_FORMATS, _ptr, _stream


def check_beam_script(parent, token, n_best: int, vocab: int, eos: int = 2):
    """The script of Engine.decode_beam_forced as two contiguous host int32 [max_len, B, beam] tensors. ValueError for a
    shape or an element out of range and for what no top-K could have chosen (include/molnextr_hip.h): '<eos>' at step 0, a
    hypothesis that has finished as a parent, the same (parent, token) twice for one image at one step. Images are followed
    as the search will run them (an image leaves once its top hypothesis has finished at some step and n_best are stored);
    entries of an image that has left are only range-checked."""
    par = torch.as_tensor(parent).cpu()
    tok = torch.as_tensor(token).cpu()
    if par.dim() != 3 or par.shape != tok.shape or par.is_floating_point() or tok.is_floating_point():
        raise ValueError(f"script parent / token must be int [max_len, B, beam], got {tuple(par.shape)} and {tuple(tok.shape)}")
    max_len, B, K = par.shape
    if not 1 <= n_best <= K:
        raise ValueError(f"n_best must be 1..beam = {K}, got {n_best}")
    for name, a, hi in (("parent", par, K), ("token", tok, vocab)):
        bad = ((a < 0) | (a >= hi)).nonzero()
        if len(bad):
            raise ValueError(f"script {name}{bad[0].tolist()} = {int(a[tuple(bad[0])])} is outside 0..{hi - 1}")
    p, v = par.tolist(), tok.tolist()
    for b in range(B):
        finished, top, stored = [False] * K, False, 0
        for t in range(max_len):
            if t == 0 and eos in v[t][b]:
                raise ValueError(f"script: image {b} emits '<eos>' at step 0, where the head bans it")
            if any(finished[j] for j in p[t][b]):
                raise ValueError(f"script: step {t} image {b} descends from a finished hypothesis")
            if len(set(zip(p[t][b], v[t][b]))) < K:
                raise ValueError(f"script: step {t} image {b} makes the same (parent, token) choice twice")
            finished = [x == eos or t + 1 == max_len for x in v[t][b]]
            top, stored = top or finished[0], stored + sum(finished)
            if top and stored >= n_best:
                break
    return par.to(torch.int32).contiguous(), tok.to(torch.int32).contiguous()


class LabCalls:
    """A base of Engine, no object of its own: a plain class without __init__. Of the engine its methods use self.lib, self.h,
    self.device and self._check, and the dimensions the aids' buffers are sized from — self.dec (vocab, d_model), self.max_len
    and self.n_mem —, and nothing else; PROFILE_KINDS and KV_WHICH are defined here."""

    def set_tap(self, item: int, dst: Optional[torch.Tensor]):
        self._check(self.lib.mnx_set_encoder_tap(self.h, item, _ptr(dst)), "mnx_set_encoder_tap")

    def decode_beam_forced(self, features: torch.Tensor, parent, token, n_best: int = 1, want_hidden: bool = True,
                           trace_logits: bool = True, fill: float = float("nan")) -> dict:
        """Beam search whose choices are read from a script while the real decoder runs (test aid, mnx_decode_beam_forced):
        parent / token int [max_len, B, beam] — new hypothesis j of original image b at step t descends from hypothesis parent
        and emits id token (check_beam_script: what a script may not do raises ValueError). Returns decode_beam's dict and,
        with trace_logits, 'logits' [max_len, B*beam, V]: the raw logits of slot b * beam + j at step t, `fill` where the
        slot was not alive."""
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        par, tok = check_beam_script(parent, token, n_best, self.dec.vocab)
        max_len, B, beam = par.shape
        if features.shape[0] != B:
            raise ValueError(f"the script is for {B} images, features for {features.shape[0]}")
        dev = features.device
        tokens = torch.zeros(B, n_best, max_len, dtype=torch.int32, device=dev)
        lengths = torch.zeros(B, n_best, dtype=torch.int32, device=dev)
        scores = torch.zeros(B, n_best, dtype=torch.float32, device=dev)
        hidden = torch.zeros(B, n_best, max_len, self.dec.d_model, dtype=torch.float32, device=dev) if want_hidden else None
        trace = torch.full((max_len, B * beam, self.dec.vocab), fill, dtype=torch.float32, device=dev) if trace_logits else None
        rc = self.lib.mnx_decode_beam_forced(self.h, _ptr(features), B, beam, n_best, max_len, _ptr(par), _ptr(tok), par.numel(),
                                             _ptr(tokens), _ptr(lengths), _ptr(scores), _ptr(hidden), _ptr(trace), _stream())
        self._check(rc, "mnx_decode_beam_forced")
        return {"tokens": tokens, "lengths": lengths, "scores": scores, "hidden": hidden, "logits": trace}

    def beam_scripted(self, table: torch.Tensor, n_best: int = 1, eos: int = 2, trace: bool = True,
                      fill: int = -7) -> dict:
        """The beam-search strategy kernels on scripted log-probs (test aid, mnx_beam_scripted): table fp32
        [max_len, B, beam, V] on the device, row (t, b, j) = what hypothesis j of original image b sees at step t; the eos
        column of step 0 is banned, nothing else is applied. Returns tokens [B,n_best,max_len], lengths, scores as
        decode_beam does, 'steps_run', and with trace=True the per-step 'parent', 'token', 'score' [max_len,B,beam], 'alive'
        [max_len,B] and 'n_active' [max_len]: rows of images not alive at the start of a step keep `fill`."""
        assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 4
        max_len, B, beam, V = table.shape
        dev = table.device
        out = {"tokens": torch.zeros(B, n_best, max_len, dtype=torch.int32, device=dev),
               "lengths": torch.zeros(B, n_best, dtype=torch.int32, device=dev),
               "scores": torch.zeros(B, n_best, dtype=torch.float32, device=dev)}
        tr = {}
        if trace:
            tr = {"parent": torch.full((max_len, B, beam), fill, dtype=torch.int32, device=dev),
                  "token": torch.full((max_len, B, beam), fill, dtype=torch.int32, device=dev),
                  "score": torch.full((max_len, B, beam), float(fill), dtype=torch.float32, device=dev),
                  "alive": torch.full((max_len, B), fill, dtype=torch.int32, device=dev),
                  "n_active": torch.full((max_len,), fill, dtype=torch.int32, device=dev)}
        steps = C.c_int32(-1)
        rc = self.lib.mnx_beam_scripted(self.h, _ptr(table), B, beam, n_best, max_len, V, eos, _ptr(out["tokens"]),
                                        _ptr(out["lengths"]), _ptr(out["scores"]), C.byref(steps), _ptr(tr.get("parent")),
                                        _ptr(tr.get("token")), _ptr(tr.get("score")), _ptr(tr.get("alive")),
                                        _ptr(tr.get("n_active")), _stream())
        self._check(rc, "mnx_beam_scripted")
        out.update(tr)
        out["steps_run"] = steps.value
        return out

    def edge_probs(self, hidden: torch.Tensor, atom_idx: torch.Tensor, n_atoms: torch.Tensor, want_scores: bool = True):
        """edges() plus the seven class probabilities of every pair as the pair kernel left them (test aid,
        mnx_edge_probs): -> edges, scores, probs fp32 [B,kmax,kmax,8]; slot 7 and pairs beyond n_atoms[b] are undefined."""
        assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.is_contiguous()
        B, max_len, _ = hidden.shape
        atom_idx = atom_idx.to(device=hidden.device, dtype=torch.int32).contiguous()
        n_atoms = n_atoms.to(device=hidden.device, dtype=torch.int32).contiguous()
        kmax = atom_idx.shape[1]
        edges = torch.zeros(B, kmax, kmax, dtype=torch.uint8, device=hidden.device)
        scores = torch.zeros(B, kmax, kmax, dtype=torch.float64, device=hidden.device) if want_scores else None
        probs = torch.zeros(B, kmax, kmax, 8, dtype=torch.float32, device=hidden.device)
        rc = self.lib.mnx_edge_probs(self.h, _ptr(hidden), _ptr(atom_idx), _ptr(n_atoms), B, kmax, max_len, _ptr(edges),
                                     _ptr(scores), _ptr(probs), _stream())
        self._check(rc, "mnx_edge_probs")
        return edges, scores, probs

    def profile(self, enable):
        """True / n: bracket the GEMMs of every n-th encode call with HIP events (at most 16 calls); False: off."""
        self._check(self.lib.mnx_profile_enable(self.h, int(enable)), "mnx_profile_enable")

    # "gemm" = encoder GEMMs of the stages with C < 512 + the patch-merging reductions, "gemm_s34" = the block Linears
    # with C >= 512 (Swin-B stages 3 and 4: the MFMA-bound shapes); the GEMM family is the sum of the two
    PROFILE_KINDS = {"gemm": 0, "layernorm": 1, "window_attn": 2, "patch_embed": 3, "gemm_s34": 4}

    def profile_read(self, kind: str = "gemm", reset: bool = True):
        """(ms, work, launches) accumulated by HIP events for one kernel class since the last reset; work = FLOP for
        'gemm', algorithmic HBM bytes for the others."""
        ms, wk, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.mnx_profile_read(self.h, self.PROFILE_KINDS[kind], C.byref(ms), C.byref(wk), C.byref(n)),
                    "mnx_profile_read")
        if reset:
            self._check(self.lib.mnx_profile_read(self.h, -1, None, None, None), "mnx_profile_read")
        return ms.value, wk.value, n.value

    def profile_read_all(self):
        out = {k: self.profile_read(k, reset=False) for k in self.PROFILE_KINDS}
        self._check(self.lib.mnx_profile_read(self.h, -1, None, None, None), "mnx_profile_read")
        return out

    def probe_decode_attn(self, rows: int, t: int, iters: int = 20):
        """Isolated timing of the two per-row decode attention kernels: (self_ms, cross_ms) per launch."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.mnx_probe_decode_attn(self.h, rows, t, iters, C.byref(a), C.byref(b), _stream()),
                    "mnx_probe_decode_attn")
        return a.value, b.value

    def gemm_clock(self, reset: bool = True) -> float:
        """Shader clock (MHz) averaged over the persistent split-operand GEMM launches since the last reset (0.0: none ran)."""
        mhz = C.c_double()
        self._check(self.lib.mnx_gemm_clock(self.h, int(reset), C.byref(mhz)), "mnx_gemm_clock")
        return mhz.value

    def probe_mfma(self, ms: int = 30):
        """(TFLOP/s, MHz) of a register-only fp16 MFMA loop on random operands on every CU: what the matrix pipes sustain
        under this device's power budget."""
        tf, mhz = C.c_double(), C.c_double()
        self._check(self.lib.mnx_probe_mfma(self.h, ms, C.byref(tf), C.byref(mhz), _stream()), "mnx_probe_mfma")
        return tf.value, mhz.value

    def gemm16_split(self, epi: int, A2: torch.Tensor, W2: torch.Tensor, Cout: torch.Tensor,
                     bias: Optional[torch.Tensor], oscale: float = 1.0, terms: int = 3):
        """Split-mode GEMM on caller buffers: A2 [2,M,K] (terms = 2: [1,M,K] will do, the lo plane is not read) and W2 [2,N,K]
        hold the hi / lo planes (16-bit); Cout is [2,M,N] 16-bit (epi 0, 1; with epi | 0x400 [1,M,N]: hi plane only) or
        [M,N] fp32 (epi 2: bias + residual in place, 3: bias). epi | 0x200: the 128x128 kernel whatever the dispatch."""
        _, M, K = A2.shape
        N = W2.shape[1]
        c_lo = M * N if Cout.dim() == 3 and Cout.shape[0] == 2 else 0
        self._check(self.lib.mnx_gemm16_split(self.h, epi, _ptr(A2), M * K, _ptr(W2), N * K, float(oscale), _ptr(Cout), c_lo,
                                              _ptr(bias), M, N, K, terms, _stream()), "mnx_gemm16_split")
        return Cout

    def window_attn(self, qkv: torch.Tensor, table: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, heads: int,
                    shift: int, terms: int = 3, qkv_lo: int = 0, out_lo: int = 0):
        """The encoder's window attention on caller buffers (test aid, mnx_window_attn): qkv [B*H*W, 3C] -> out [B*H*W, C]
        in the engine's operand type, table fp32 [529, heads]. Split modes: qkv / out start with the hi planes, qkv_lo /
        out_lo are the element offsets of the lo planes from them; terms 3, 1 or 3 | 0x100 (the non-persistent kernel).
        Plain modes: terms = 1."""
        assert qkv.is_cuda and out.is_cuda and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()
        self._check(self.lib.mnx_window_attn(self.h, _ptr(qkv), qkv_lo, _ptr(table), _ptr(out), out_lo, B, H, W, heads * 32,
                                             heads, shift, terms, _stream()), "mnx_window_attn")
        return out

    KV_WHICH = {"self_k": 0, "self_v": 1, "mem_k": 2, "mem_v": 3}

    def kv_block(self, which: str, layer: int, owner: int, head: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One raw block of the decoder's K / V cache (test aid, mnx_kv_block) as uint8 bytes on the device: which is a key
        of KV_WHICH, owner the slot (self) or memory block (memory); after decode_greedy / decode_forced row b used slot b and
        memory block b. The block holds nk = kvq_rows(max_len) (self) or kvq_rows(144) (memory) rows of 100 bytes:
        [nk][32] int16 hi | [nk][32] uint8 lo | [nk] float32 scale (csrc/kvq.h)."""
        nk = ((self.max_len if which.startswith("self") else self.n_mem) + 3) & ~3
        if out is None:
            out = torch.empty(nk * 100, dtype=torch.uint8, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.uint8 and out.numel() >= nk * 100
        self._check(self.lib.mnx_kv_block(self.h, self.KV_WHICH[which], layer, owner, head, _ptr(out), _stream()),
                    "mnx_kv_block")
        return out

    # -- the encoder's non-GEMM kernels and the fp32 SGEMM on caller buffers (test aids) -----------------------------------
    # Thin: every argument goes to the library as given, which validates it (tests/test_gpu_encoder_ops.py).
    def patch_embed(self, img: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor,
                    beta: torch.Tensor, x: torch.Tensor, B: int, S: int, C_: int):
        """mnx_patch_embed: img fp32 [B,3,S,S] or uint8 [B,S,S] (gray bytes), w_t fp32 [48, C] -> x fp32 [B, (S/4)^2, C]"""
        fmt = IMAGE_FORMATS["gray8" if img.dtype == torch.uint8 else "fp32"]
        self._check(self.lib.mnx_patch_embed(self.h, _ptr(img), fmt, _ptr(w_t), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(x),
                                             B, S, C_, _stream()), "mnx_patch_embed")
        return x

    def layernorm16(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y16: Optional[torch.Tensor],
                    y32: Optional[torch.Tensor], M: int, C_: int, eps: float = 1e-5, y_lo: int = 0, planes: int = 2,
                    flag: Optional[torch.Tensor] = None):
        """mnx_layernorm16: x fp32 [M, C] -> y16 [M, C] in the engine's operand type (split modes: the hi plane, the lo plane
        y_lo elements behind it; planes = 1: hi only) and / or y32 fp32 [M, C]; flag: device int32, set on a non-finite row."""
        self._check(self.lib.mnx_layernorm16(self.h, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y16), y_lo, _ptr(y32), M, C_,
                                             float(eps), planes, _ptr(flag), _stream()), "mnx_layernorm16")

    def merge_ln16(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y16: torch.Tensor, B: int, H: int,
                   W_: int, C_: int, eps: float = 1e-5, y_lo: int = 0, planes: int = 2):
        """mnx_merge_ln16: x fp32 [B,H,W,C] -> y16 [B * H/2 * W/2, 4C], the patch-merging gather + LayerNorm(4C)"""
        self._check(self.lib.mnx_merge_ln16(self.h, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y16), y_lo, B, H, W_, C_,
                                            float(eps), planes, _stream()), "mnx_merge_ln16")

    def cast16(self, x: torch.Tensor, y16: torch.Tensor, n: int, y_lo: int = 0, scale: float = 1.0):
        """mnx_cast16: x fp32 [n] -> y16 [n] in the engine's operand type; split modes: hi / lo planes of scale * x"""
        self._check(self.lib.mnx_cast16(self.h, _ptr(x), _ptr(y16), y_lo, n, float(scale), _stream()), "mnx_cast16")

    def sgemm_tn(self, A: torch.Tensor, Wt: torch.Tensor, bias: Optional[torch.Tensor], Cout: torch.Tensor, M: int, N: int,
                 K: int, perm_S: int = 0):
        """mnx_sgemm_tn: Cout[M,N] = A[M,K] . Wt[N,K]^T + bias in fp32; perm_S > 0: the [M/S][N/256][8][S][32] layout"""
        self._check(self.lib.mnx_sgemm_tn(self.h, _ptr(A), _ptr(Wt), _ptr(bias), _ptr(Cout), M, N, K, perm_S, _stream()),
                    "mnx_sgemm_tn")

    def dec_linear(self, pro: int, epi: int, x: Optional[torch.Tensor], Wt: torch.Tensor, bias: torch.Tensor,
                   out: torch.Tensor, rows, capacity: int, N: int, K: int, gamma: Optional[torch.Tensor] = None,
                   beta: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None, n_part: int = 0,
                   part_stride: int = 0, x_write: Optional[torch.Tensor] = None):
        """mnx_dec_linear: one launch of the decode tick's linear <pro, epi> at `capacity` rows; rows = the alive sequences
        [(slot, t, prev_tok, rowc), ...] (host). Row r of x / out / x_write / part is the alive slot with the r-th smallest
        slot number. epi 0 writes the engine's layer-0 self cache (kv_block), epi 4 K / 256 planes part_stride floats apart."""
        script = torch.as_tensor(rows, dtype=torch.int32).reshape(-1, 4).contiguous()
        self._check(self.lib.mnx_dec_linear(self.h, pro, epi, _ptr(x), _ptr(Wt), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(part),
                                            n_part, part_stride, _ptr(out), _ptr(x_write), N, K, capacity, script.shape[0],
                                            _ptr(script), _stream()), "mnx_dec_linear")

    def gemm16(self, epi: int, A: torch.Tensor, Wt: torch.Tensor, Cout: torch.Tensor, bias: Optional[torch.Tensor]):
        M, K = A.shape
        N = Wt.shape[0]
        self._check(self.lib.mnx_gemm16(self.h, epi, _ptr(A), _ptr(Wt), _ptr(Cout), _ptr(bias), M, N, K, _stream()),
                    "mnx_gemm16")
        return Cout
