"""GPU (-m gpu): beam_begin_kernel, beam_pick_kernel and beam_gather_kernel alone, driven with scripted log-probs through
mnx_beam_scripted, against tests/beam_script_ref.py: the reference's own golden (tests/golden/beam_strategy.npz) and, for
exact ties, -inf, the pool and the longest search, oracle.beam.BeamStrategy. Everything is compared exactly — parents, ids,
the images that stay and the rows of every step, and every score as an fp32 word: (lp + cum) / len and score * len are
single correctly rounded operations on both sides. tests/test_beam_script_host.py shows that the cases reach the ties, pool
events and boundaries they are named for."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_script_ref as R
from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    assert e.max_len == R.CFG_MAX_LEN
    yield e
    e.close()


def _words(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _run(eng, dev, table, n_best):
    out = eng.beam_scripted(table.to(dev).contiguous(), n_best=n_best, eos=R.EOS, trace=True, fill=R.FILL)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _check(out, ex, case):
    assert out["steps_run"] == ex.steps_run, case
    assert np.array_equal(out["n_active"], ex.n_active), f"{case}: rows per step"
    assert np.array_equal(out["alive"], ex.alive), f"{case}: images alive after each step"
    # scores of every image that entered a step, and the fill value everywhere else, as words
    bad = np.argwhere(_words(out["score"]) != _words(ex.score))
    assert bad.size == 0, f"{case}: score words differ first at (step, image, rank) {bad[0].tolist()}: " \
                          f"{out['score'][tuple(bad[0])]!r} vs {ex.score[tuple(bad[0])]!r}"
    for name, want in (("parent", ex.parent), ("token", ex.token)):
        got = out[name]
        known = np.broadcast_to(ex.known[..., None], got.shape)
        bad = np.argwhere((got != want) & known)
        assert bad.size == 0, f"{case}: {name} differs first at (step, image, rank) {bad[0].tolist()}"
        assert (got[~ex.entered] == R.FILL).all(), f"{case}: {name} rows of images outside the step were written"
        hidden = ex.entered & ~ex.known         # the golden's leaving images: written, not known; at least in range
        assert (got[hidden] >= 0).all() and (got[hidden] < (ex.K if name == "parent" else ex.V)).all()
    assert (out["alive"][~ex.entered] == R.FILL).all()
    for b in range(ex.B):
        for r in range(ex.n_best):
            n = int(out["lengths"][b, r])
            assert out["tokens"][b, r, :n].tolist() == ex.final_ids[b][r], f"{case}: image {b} rank {r}"
            assert (out["tokens"][b, r, n:] == 0).all()
    assert np.array_equal(_words(out["scores"]), _words(ex.final_scores)), f"{case}: final scores"


@pytest.mark.parametrize("case", R.CASES)
def test_scripted_beam_matches_expectation(eng, dev, case):
    """Every case twice on one engine: both runs equal the expectation and each other byte for byte, so nothing the first
    call leaves in the engine's state (pool, ancestry, cumulative sums, alive flags) leaks into the second."""
    table, ex = R.expectation(case)
    first = _run(eng, dev, table, ex.n_best)
    _check(first, ex, case)
    second = _run(eng, dev, table, ex.n_best)
    for k, v in first.items():
        same = v == second[k] if not isinstance(v, np.ndarray) else v.tobytes() == second[k].tobytes()
        assert same, f"{case}: '{k}' differs between two calls on one engine"


def test_without_trace_gives_the_same_result(eng, dev):
    table, ex = R.expectation("ties_small")
    out = eng.beam_scripted(table.to(dev), n_best=ex.n_best, eos=R.EOS, trace=False)
    assert "parent" not in out and out["steps_run"] == ex.steps_run
    assert np.array_equal(_words(out["scores"].cpu().numpy()), _words(ex.final_scores))
    lens = out["lengths"].cpu().numpy()
    assert [[out["tokens"][b, r, :lens[b, r]].tolist() for r in range(ex.n_best)] for b in range(ex.B)] == ex.final_ids


def test_production_beam_search_after_a_scripted_call(eng, dev, synth_ckpt):
    """mnx_beam_scripted shares the engine's beam buffers and decoder state with mnx_decode_beam: after a scripted call
    (another B, K, n_best, another 'vocabulary') the (4, 3, 2, 160) search of test_gpu_parity.py still matches its oracle,
    and a scripted call after THAT still matches its expectation."""
    from oracle.beam import beam_decode
    table, ex = R.expectation("ties_full")
    _check(_run(eng, dev, table, ex.n_best), ex, "ties_full")
    B, beam, n_best, max_len = 4, 3, 2, 160
    feats = W.hash_normal(f"beam_features_{B}_{beam}", (B, 144, 1024), 0.5)
    ref = beam_decode(feats, synth_ckpt["decoder"], beam=beam, n_best=n_best, max_len=max_len)
    out = eng.decode_beam(feats.to(dev), beam=beam, n_best=n_best, max_len=max_len)
    lens, toks, sc = out["lengths"].cpu().numpy(), out["tokens"].cpu().numpy(), out["scores"].cpu().numpy()
    for i in range(B):
        for r in range(n_best):
            n = lens[i, r]
            assert toks[i, r, :n].tolist() == ref.tokens[i][r], f"image {i} rank {r}"
            assert abs(sc[i, r] - ref.scores[i][r]) < 1e-4 * max(1.0, abs(ref.scores[i][r]))
            assert (out["hidden"][i, r, :n].cpu() - ref.hidden[i][r]).abs().max().item() < 1e-3
    table, ex = R.expectation("pool_hand")
    _check(_run(eng, dev, table, ex.n_best), ex, "pool_hand")


def _refused(e, args, needle):
    rc = e.lib.mnx_beam_scripted(e.h, *args)
    msg = e.lib.mnx_last_error(e.h)
    assert rc == -1, (needle, rc)
    assert msg.startswith(b"mnx_beam_scripted: ") and needle in msg, (needle, msg)


def test_refusals(eng, dev, synth_ckpt):
    """Every bound of mnx_beam_scripted: MNX_ERR_INVALID_ARG with a message that names it, nothing launched. The buffers are
    large enough for any of the refused shapes all the same."""
    from molnextr_amd.engine import Engine, MnxError
    table = torch.zeros(1 << 22, device=dev)
    ints = [torch.zeros(1 << 20, dtype=torch.int32, device=dev) for _ in range(6)]
    flts = [torch.zeros(1 << 20, device=dev) for _ in range(2)]
    steps = C.c_int32(-1)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def args(B=2, beam=3, n_best=2, max_len=4, V=8, eos=2, table=p(table), tokens=p(ints[0]), lengths=p(ints[1]),
             scores=p(flts[0]), steps_run=C.byref(steps), trace=(p(ints[2]), p(ints[3]), p(flts[1]), p(ints[4]), p(ints[5]))):
        return (table, B, beam, n_best, max_len, V, eos, tokens, lengths, scores, steps_run, *trace, None)

    assert eng.lib.mnx_beam_scripted(eng.h, *args()) == 0 and steps.value == 4      # the arguments as such are fine
    for kw, needle in ((dict(B=33, n_best=1), b"B must be 1..32"), (dict(B=0), b"B must be 1..32"),
                       (dict(beam=0, n_best=1), b"beam must be 1..8"), (dict(beam=9), b"beam must be 1..8"),
                       (dict(n_best=0), b"n_best must be 1..beam"), (dict(n_best=4), b"n_best must be 1..beam"),
                       (dict(V=1, eos=0), b"V must be 2..256"), (dict(B=1, beam=1, n_best=1, V=257), b"V must be 2..256"),
                       (dict(eos=-1), b"eos must be 0..V-1"), (dict(eos=8), b"eos must be 0..V-1"),
                       (dict(max_len=0), b"max_len must be 1..cfg.max_len"),
                       (dict(B=1, beam=1, n_best=1, V=4, max_len=eng.max_len + 1), b"max_len must be 1..cfg.max_len"),
                       (dict(B=64, beam=8, n_best=5), b"n_best exceeds the hypotheses the pool keeps"),
                       (dict(table=None), b"null"), (dict(tokens=None), b"null"), (dict(lengths=None), b"null"),
                       (dict(scores=None), b"null"), (dict(steps_run=None), b"null"),
                       (dict(trace=(p(ints[2]), None, None, None, None)), b"trace pointers"),
                       (dict(trace=(p(ints[2]), p(ints[3]), p(flts[1]), p(ints[4]), None)), b"trace pointers")):
        _refused(eng, args(**kw), needle)
    assert eng.lib.mnx_beam_scripted(None, *args()) == -1
    with pytest.raises(MnxError, match="beam must be 1..8"):
        eng.beam_scripted(torch.zeros(4, 2, 9, 8, device=dev))
    small = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32, dtype="fp16x3")
    try:
        _refused(small, args(B=32, beam=2), b"B x beam exceeds dec_slots")
        assert small.lib.mnx_beam_scripted(small.h, *args(B=16, beam=2)) == 0
    finally:
        small.close()
