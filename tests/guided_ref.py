"""CPU restatement of label-guided greedy decoding, built from oracle.decoder's blocks (helper of tests/test_guided*.py).

The reference loop is TransformerDecoderAR.decode(labels=...) (components.py:284-332, greedy_search.py:76-127). Rows alive
beyond their label go on free-running (the engine's extension; the reference raises IndexError there)."""
import math

import torch
import torch.nn.functional as F

from oracle.config import DECODER_DEFAULT
from oracle.decoder import (EOS_BAN, MASK_FILL, P, GreedyResult, _lin, _ln, _mha, cross_kv, enc_transform, grammar_mask)

MASK_ID = 4


@torch.no_grad()
def guided_decode(features, sd, labels, cfg=DECODER_DEFAULT, max_len=None) -> GreedyResult:
    """One reference batch. labels: int [B, L]. tokens = merged ids, token_logp = the own picks' masked log-probs."""
    max_len = cfg.max_len if max_len is None else max_len
    labels = torch.as_tensor(labels, dtype=torch.long)
    Ll = min(labels.shape[1], max_len + 1)
    memory = enc_transform(features, sd)
    B, S, D = memory.shape
    h, dh, L = cfg.heads, cfg.d_model // cfg.heads, cfg.layers
    mem_kv = cross_kv(memory, sd, cfg)
    emb_w = sd[P + "embeddings.make_embedding.emb_luts.0.weight"]
    pe = sd[P + "embeddings.make_embedding.pe.pe"].reshape(-1, D)
    self_k = torch.zeros(L, B, h, max_len, dh)
    self_v = torch.zeros(L, B, h, max_len, dh)
    alive = list(range(B))
    prev = torch.full((B,), cfg.sos_id, dtype=torch.long)      # the id that advances the row = next input = merged output
    toks, logps = [[] for _ in range(B)], [[] for _ in range(B)]
    hid = torch.zeros(B, max_len, D)
    fin_step = [-1] * B
    for step in range(max_len):
        idx = torch.tensor(alive)
        n = len(alive)
        tok_in = prev[idx]
        x = emb_w[tok_in] * math.sqrt(D) + pe[:n]
        for l in range(L):
            lp = f"{P}decoder.transformer_layers.{l}"
            xn = _ln(x, sd, lp + ".layer_norm_1")
            self_k[l, idx, :, step] = _lin(xn, sd, lp + ".self_attn.linear_keys").reshape(n, h, dh)
            self_v[l, idx, :, step] = _lin(xn, sd, lp + ".self_attn.linear_values").reshape(n, h, dh)
            q = _lin(xn, sd, lp + ".self_attn.linear_query")
            a = _mha(q, self_k[l, idx, :, :step + 1], self_v[l, idx, :, :step + 1], sd, lp + ".self_attn", cfg)
            query = a + x
            q2 = _lin(_ln(query, sd, lp + ".layer_norm_2"), sd, lp + ".context_attn.linear_query")
            y = _mha(q2, mem_kv[l][0][idx], mem_kv[l][1][idx], sd, lp + ".context_attn", cfg) + query
            ff = lp + ".feed_forward"
            x = _lin(F.gelu(_lin(_ln(y, sd, ff + ".layer_norm"), sd, ff + ".w_1")), sd, ff + ".w_2") + y
        out = _ln(x, sd, P + "decoder.layer_norm")
        lp_ = F.log_softmax(_lin(out, sd, P + "output_layer"), dim=-1)
        lp_ = lp_.masked_fill(grammar_mask(tok_in, cfg), MASK_FILL)          # from the MIXED input id (components.py:300-303)
        if step == 0:
            lp_[:, cfg.eos_id] = EOS_BAN
        best_lp, best = lp_.max(dim=-1)
        hid[idx, step] = out
        finished = []
        for r, t, s in zip(alive, best.tolist(), best_lp.tolist()):
            inside = step + 1 < Ll
            nxt = int(labels[r, step + 1]) if inside else MASK_ID
            adv = t if nxt == MASK_ID else nxt
            toks[r].append(adv)
            logps[r].append(s)                                               # the own pick's score, forced or not
            prev[r] = adv
            fin = (nxt == cfg.eos_id) if inside else (t == cfg.eos_id)
            if fin or step + 1 == max_len:
                finished.append(r)
                fin_step[r] = step
        if finished:
            alive = [r for r in alive if r not in finished]
            if not alive:
                break
    hidden = [hid[r, :len(toks[r])].clone() for r in range(B)]
    scores = [float(torch.tensor(lp_r).mean().exp()) for lp_r in logps]
    return GreedyResult(toks, logps, hidden, scores, fin_step, None)
