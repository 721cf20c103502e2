"""GPU (-m gpu): beam search over ancestor slots — dec_attn_kernel<true>'s lookups in bm.anc, beam_pick_kernel's inheritance
and gathers, beam_begin_kernel's PE rank after an image leaves — with the real decoder running and every step's choice read
from a script (mnx_decode_beam_forced), against the float64 scripted decode of oracle/beam.py.

The scripts (tests/beam_forced_ref.py) send every row's keys and values through other slots at every key count where the
attention kernel takes another turn (32-key value blocks, 160 prefetched keys, the second key per thread from 256, the
unrolled value loop complete at 288 and its remainder from 289); tests/test_beam_forced_host.py shows on the CPU that
reading the row's own slot in any one of these ranges would miss the tolerance used here by more than 3900 tolerances.

Tolerance of the logits: oracle.kvq.logit_tolerance = 32 u M (u = 2^-24, M = max |logit| of the float64 decode), derived in
tests/test_gpu_kvcache.py's docstring; the beam tick is the 8-launch tick that docstring measures at 13.0 u M on greedy rows.
Hidden rows: 32 u H, H = max |hidden| of the float64 decode — the residual stream's relative error, which the logit bound
carries through the output product, is what the final LayerNorm's output has. Scores: the existing beam test's
1e-4 max(1, |score|) (a score of -inf — descendants of the hypotheses that start at -inf — must be -inf). Tokens, lengths and
the order of the returned hypotheses: exact. Trace rows of slots not alive at a step: the caller's fill, bit for bit.

Measured on an MI355X (printed by the tests), worst |logit - float64| and |hidden - float64| over every alive (step, slot):
    rotation   (2 x 4, 330 steps)   6.3e-5 = 11.9 u M (tol 1.68e-4)   6.2e-6 = 8.5 u H (tol 2.3e-5)
    seams      (1 x 2, 330 steps)   4.6e-5 = 10.4 u M (tol 1.41e-4)   5.3e-6 = 7.6 u H (tol 2.2e-5)
    leaving    (5 x 3,  48 steps)   4.6e-5 =  8.9 u M (tol 1.67e-4)   3.9e-6 = 5.9 u H (tol 2.1e-5)
    two_tiles  (8 x 5,  40 steps)   6.4e-5 = 12.1 u M (tol 1.68e-4)   4.9e-6 = 7.0 u H (tol 2.2e-5)
No case comes near the tolerance: the ancestor path reads what the re-ordering oracle reads. The whole module runs in 11 s.
For comparison, a scratch build whose value loop read the row's own slot from key 160 on (the loop behind the prefetch)
was run once against this module: rotation 17.3 = 3.3e6 u M, seams 9.0 = 2.0e6 u M — both fail; leaving and two_tiles, which
end before 160 keys, as above.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_forced_ref as R
from molnextr_amd import weights as W
from oracle import beam as OB
from oracle import kvq as KQ

pytestmark = pytest.mark.gpu

FILL = -7.0
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=1, dec_slots=64, dtype="fp16x3")
    yield e
    e.close()


@pytest.fixture(scope="module")
def reference(synth_ckpt):
    """name -> (case, its float64 scripted decode), computed once per case"""
    done = {}

    def get(name):
        if name not in done:
            c = R.case(name)
            done[name] = (c, OB.scripted_decode(c.features, synth_ckpt["decoder"], c.parent, c.token, n_best=c.n_best))
        return done[name]
    return get


def _run(eng, dev, c):
    out = eng.decode_beam_forced(c.features.to(dev), c.parent, c.token, n_best=c.n_best, fill=FILL)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", R.CASES)
def test_logits_and_hypotheses_match_float64(name, eng, dev, reference):
    c, ref = reference(name)
    out = _run(eng, dev, c)
    alive = ~torch.isnan(ref.logits).any(-1)                                   # [max_len, B * beam]
    assert torch.equal(alive, torch.from_numpy(R.alive_steps(c)).repeat_interleave(c.beam, dim=1))
    lg = out["logits"].double()
    assert bool((out["logits"][~alive] == FILL).all()), "a trace row of a slot that was not alive was written"
    tol = KQ.logit_tolerance(ref.logits)
    err = (lg - ref.logits)[alive].abs().amax(-1)
    worst = float(err.max())
    where = alive.nonzero()[int(err.argmax())].tolist()
    print(f"{name}: max |logit - float64| = {worst:.3e} = {worst / (tol / KQ.LOGIT_TOL_C):.1f} u M at (step, slot) {where}; "
          f"tol {tol:.3e} ({KQ.LOGIT_TOL_C} u M)")
    assert worst <= tol, (name, worst, tol, where)
    H = max(float(h.abs().max()) for hs in ref.hidden for h in hs)
    worst_h = 0.0
    for b in range(c.B):
        assert len(ref.tokens[b]) == c.n_best
        for r in range(c.n_best):
            n = int(out["lengths"][b, r])
            assert out["tokens"][b, r, :n].tolist() == ref.tokens[b][r], f"{name}: image {b} rank {r}"
            assert not out["tokens"][b, r, n:].any()
            want = ref.scores[b][r]
            got = float(out["scores"][b, r])
            assert got == want if np.isinf(want) else abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, b, r, got, want)
            worst_h = max(worst_h, float((out["hidden"][b, r, :n].double() - ref.hidden[b][r]).abs().max()))
    print(f"{name}: max |hidden - float64| = {worst_h:.3e} = {worst_h / (U * H):.1f} u H; tol {KQ.LOGIT_TOL_C * U * H:.3e}")
    assert worst_h <= KQ.LOGIT_TOL_C * U * H, (name, worst_h, H)


def test_script_replaces_the_choice_and_nothing_else(eng, dev, synth_ckpt):
    """the (4, 3, 2, 160) search of test_gpu_parity.py::test_beam_search_vs_oracle, scripted with the oracle's own picks of
    that search: every output word equals mnx_decode_beam's"""
    B, beam, n_best, max_len = 4, 3, 2, 160
    feats = W.hash_normal(f"beam_features_{B}_{beam}", (B, 144, 1024), 0.5)
    ref = OB.beam_decode(feats, synth_ckpt["decoder"], beam=beam, n_best=n_best, max_len=max_len)
    parent, token = OB.script_from_picks(ref.picks, B, beam, max_len)
    free = eng.decode_beam(feats.to(dev), beam=beam, n_best=n_best, max_len=max_len)
    forced = eng.decode_beam_forced(feats.to(dev), parent, token, n_best=n_best, trace_logits=False)
    torch.cuda.synchronize()
    assert [[free["tokens"][b, r, :int(free["lengths"][b, r])].tolist() for r in range(n_best)] for b in range(B)] == ref.tokens
    for k in ("tokens", "lengths", "scores", "hidden"):
        assert torch.equal(free[k], forced[k]), f"'{k}' of the scripted search differs from the free search it repeats"
    assert forced["logits"] is None


def test_two_runs_are_bit_identical(eng, dev):
    c = R.case("rotation")
    a, b = _run(eng, dev, c), _run(eng, dev, c)
    for k in a:
        assert torch.equal(a[k], b[k]), f"'{k}' differs between two runs of the rotation script"


def test_argument_errors(eng, dev):
    """every bound of mnx_decode_beam_forced: MNX_ERR_INVALID_ARG with a message under its name, nothing launched (the
    outputs keep their fill). The buffers are large enough for any of the refused shapes all the same."""
    from molnextr_amd.engine import MnxError
    V = eng.dec.vocab
    feats = torch.zeros(33 * 144 * 1024, device=dev)
    ints = [torch.full((1 << 20,), -5, dtype=torch.int32, device=dev) for _ in range(2)]
    flts = [torch.full((n,), -5.0, device=dev) for n in (1 << 20, 1 << 22, 1 << 22)]
    B, K, T = 2, 3, 4
    par = np.zeros(1 << 18, np.int32)
    tok = np.zeros(1 << 18, np.int32)
    par[:T * B * K] = np.tile(np.arange(K, dtype=np.int32), T * B)
    tok[:T * B * K] = 3 + np.tile(np.arange(K, dtype=np.int32), T * B)
    p = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731

    def args(B=B, beam=K, n_best=2, max_len=T, features=p(feats), parent=hp(par), token=hp(tok), n=1 << 18, tokens=p(ints[0]),
             lengths=p(ints[1]), scores=p(flts[0]), hidden=p(flts[1]), trace=p(flts[2])):
        return (features, B, beam, n_best, max_len, parent, token, n, tokens, lengths, scores, hidden, trace, None)

    def refused(e, a, needle):
        rc = e.lib.mnx_decode_beam_forced(e.h, *a)
        msg = e.lib.mnx_last_error(e.h)
        assert rc == -1, (needle, rc)
        assert msg.startswith(b"mnx_decode_beam_forced: ") and needle in msg, (needle, msg)
        torch.cuda.synchronize()
        assert all(bool((t == -5).all()) for t in ints + flts), f"{needle}: an output was written"

    def poked(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    last = T * B * K - 1
    bad_scripts = [poked(par, 0, -1), poked(par, last, K), poked(tok, 5, -1), poked(tok, last, V), poked(par, 7, 1 << 30)]
    for kw, needle in ((dict(features=None), b"null"), (dict(parent=None), b"null"), (dict(token=None), b"null"),
                       (dict(tokens=None), b"null"), (dict(lengths=None), b"null"), (dict(scores=None), b"null"),
                       (dict(B=0), b"B must be 1..32"), (dict(B=33, beam=1, n_best=1), b"B must be 1..32"),
                       (dict(beam=0, n_best=1), b"beam must be 1..8"), (dict(beam=9), b"beam must be 1..8"),
                       (dict(n_best=0), b"n_best must be 1..beam"), (dict(n_best=K + 1), b"n_best must be 1..beam"),
                       (dict(max_len=0), b"max_len must be 1..cfg.max_len"),
                       (dict(B=1, beam=1, n_best=1, max_len=eng.max_len + 1), b"max_len must be 1..cfg.max_len"),
                       (dict(B=32, beam=3), b"B x beam exceeds dec_slots"),
                       (dict(n=T * B * K - 1), b"script_len is less than"), (dict(n=-1), b"script_len is less than"),
                       (dict(n=0), b"script_len is less than"),
                       (dict(parent=hp(bad_scripts[0])), b"script_parent[0][0][0] = -1 is outside 0..beam-1"),
                       (dict(parent=hp(bad_scripts[1])), b"script_parent[3][1][2] = 3 is outside 0..beam-1"),
                       (dict(token=hp(bad_scripts[2])), b"script_token[0][1][2] = -1 is outside 0..vocab-1"),
                       (dict(token=hp(bad_scripts[3])), f"script_token[3][1][2] = {V} is outside 0..vocab-1".encode()),
                       (dict(parent=hp(bad_scripts[4])), b"script_parent[1][0][1] = 1073741824 is outside")):
        refused(eng, args(**kw), needle)
    assert eng.lib.mnx_decode_beam_forced(None, *args()) == -1
    # an element past max_len x B x beam is not part of the script
    par[T * B * K] = -1
    assert eng.lib.mnx_decode_beam_forced(eng.h, *args()) == 0             # the arguments as such are fine
    assert eng.lib.mnx_decode_beam_forced(eng.h, *args(n=T * B * K, hidden=None, trace=None)) == 0
    torch.cuda.synchronize()
    assert ints[1][:B * 2].tolist() == [T] * (B * 2) and int(ints[1][B * 2]) == -5
    assert not bool((flts[2][:T * B * K * V] == -5).any()) and bool((flts[2][T * B * K * V:] == -5).all())
    with pytest.raises(MnxError, match="B x beam exceeds dec_slots"):
        eng.decode_beam_forced(feats[:22 * 144 * 1024].view(22, 144, 1024), torch.arange(3).repeat(2, 22, 1),
                               3 + torch.arange(3).repeat(2, 22, 1))
    with pytest.raises(ValueError, match="step 0"):
        eng.decode_beam_forced(feats[:144 * 1024].view(1, 144, 1024), torch.zeros(2, 1, 2, dtype=torch.long),
                               torch.tensor([[[2, 3]], [[4, 5]]]))
