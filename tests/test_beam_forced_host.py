"""CPU: the scripted beam decode of oracle/beam.py and the scripts of tests/test_gpu_beam_forced.py (tests/beam_forced_ref.py),
so that the device agreeing with the oracle there means what it is taken to mean:
  * scripted with a free search's own picks, the oracle repeats that search (exactly in float32, to rounding in float64);
  * every script sends the rows' keys through the ancestor slots it claims to, at the key indices it claims to;
  * on the rotation script, an attention that read a row's OWN slot in any one of the key ranges [0,32), [32,160), [160,256),
    [256,288), [288,330) would miss the float64 logits by 10 tolerances and more in every row — the tolerance being
    oracle.kvq.logit_tolerance, what the device is held to;
  * Engine.decode_beam_forced's script check refuses what no top-K could have chosen."""
import numpy as np
import pytest
import torch

import beam_forced_ref as R
from molnextr_amd import weights as W
from molnextr_amd.engine import check_beam_script
from oracle import beam as OB
from oracle import kvq as KQ


@pytest.fixture(scope="module")
def dec(synth_ckpt):
    return synth_ckpt["decoder"]


@pytest.fixture(scope="module")
def rotation(dec):
    c = R.case("rotation")
    return c, OB.scripted_decode(c.features, dec, c.parent, c.token, n_best=c.n_best)


def test_scripted_with_a_searchs_own_picks_repeats_the_search(dec):
    B, beam, n_best, max_len = 3, 3, 2, 40
    feats = W.hash_normal(f"beam_features_{B}_{beam}", (B, 144, 1024), 0.5)
    free = OB.beam_decode(feats, dec, beam=beam, n_best=n_best, max_len=max_len)
    parent, token = OB.script_from_picks(free.picks, B, beam, max_len)
    check_beam_script(parent, token, n_best, R.VOCAB)
    same = OB.scripted_decode(feats, dec, parent, token, n_best=n_best, dtype=torch.float32)
    assert same.tokens == free.tokens and same.scores == free.scores
    assert all(torch.equal(a, b) for x, y in zip(same.hidden, free.hidden) for a, b in zip(x, y))
    f64 = OB.scripted_decode(feats, dec, parent, token, n_best=n_best)
    assert f64.tokens == free.tokens
    u = 2.0 ** -24
    for i in range(B):
        for r in range(n_best):
            assert abs(f64.scores[i][r] - free.scores[i][r]) <= 1e-4 * max(1.0, abs(f64.scores[i][r]))
            # the float32 stream's relative error, as for the device (tests/test_gpu_beam_forced.py)
            e = float((f64.hidden[i][r] - free.hidden[i][r]).abs().max())
            assert e <= KQ.LOGIT_TOL_C * u * float(f64.hidden[i][r].abs().max()), (i, r, e)
    # the recorded logits are those of the rows the picks name: free-running log-probs of the float32 decode, step 0
    assert not torch.isnan(f64.logits[0]).any() and tuple(f64.logits.shape) == (max_len, B * beam, R.VOCAB)


def _final_ancestry(res, c, step=None):
    """{slot: ancestry [step + 1]} of the rows alive at `step` (default: the last step anything ran)"""
    alive = R.alive_steps(c)
    step = max(t for t in range(c.max_len) if alive[t].any()) if step is None else step
    anc = res.ancestry[step]
    return {s: anc[s, :step + 1].tolist() for s in range(c.B * c.beam) if alive[step, s // c.beam]}, step


@pytest.mark.parametrize("name", R.CASES)
def test_scripts_are_legal_and_the_oracle_runs_the_images_they_describe(name, dec, rotation):
    c = R.case(name)
    check_beam_script(c.parent, c.token, c.n_best, R.VOCAB)
    res = rotation[1] if name == "rotation" else OB.scripted_decode(c.features, dec, c.parent, c.token, n_best=c.n_best,
                                                                    dtype=torch.float32)
    alive = torch.from_numpy(R.alive_steps(c)).repeat_interleave(c.beam, dim=1)
    assert torch.equal(~torch.isnan(res.logits).any(-1), alive) and torch.equal(~torch.isnan(res.logits).all(-1), alive)
    assert torch.equal(res.ancestry[..., 0] >= 0, alive)
    K = c.beam
    for t in range(c.max_len):      # ancestry names slots of the row's own image, key t is the row's own
        for s in np.nonzero(alive[t].numpy())[0]:
            a = res.ancestry[t, s, :t + 1]
            assert int(a[t]) == s and bool((a // K == s // K).all()) and bool((res.ancestry[t, s, t + 1:] == -1).all())
    for b in range(c.B):
        n = [len(x) for x in res.tokens[b]]
        assert len(n) == c.n_best
    last, step = _final_ancestry(res, c)
    if name in ("rotation", "two_tiles", "leaving"):
        ranges = R.KEY_RANGES if name == "rotation" else ((0, 32), (32, step + 1))
        for s, a in last.items():
            for lo, hi in ranges:
                hi = min(hi, step + 1)
                owners = a[lo:hi]
                elsewhere = sum(o != s for o in owners)
                if (s // K) % 2 == 0:   # a place per step: key tau of the row in slot j at step t sits (t - tau) places on
                    assert owners == [s // K * K + (s % K + step - tau) % K for tau in range(lo, hi)]
                    assert elsewhere == sum((step - tau) % K != 0 for tau in range(lo, hi))
                assert elsewhere >= (hi - lo) // 2, (name, s, lo, hi, elsewhere)
                if hi - lo >= 4 * K:
                    assert set(owners) == set(range(s // K * K, s // K * K + K)), (name, s, lo, hi)
    if name == "rotation":
        assert step == 329
    if name == "seams":
        assert step == 329
        for at, want in ((329, R.SEAM_CHANGES + (329,)), (328, R.SEAM_CHANGES), (288, R.SEAM_CHANGES[:-1]), (33, (32, 33))):
            rows, _ = _final_ancestry(res, c, at)
            for s, a in rows.items():
                assert tuple(tau for tau in range(1, at + 1) if a[tau] != a[tau - 1]) == want, (at, s)
                assert a[at] == s and set(a) <= {0, 1}
    if name == "leaving":
        left = {b: int(np.nonzero(~R.alive_steps(c)[:, b])[0][0]) for b in (1, 3)}
        assert left == {1: 4, 3: 41} and R.alive_steps(c)[:, [0, 2, 4]].all()
        assert [len(res.tokens[b][0]) for b in range(5)] == [48, 4, 48, 41, 48]
        assert res.tokens[1][0][-1] == R.EOS and res.tokens[3][0][-1] == R.EOS
        # image 4's rows are rows 6..8 of the batch by then (PE rank), its keys still live in slots 12..14
        assert set(last) == {0, 1, 2, 6, 7, 8, 12, 13, 14} and set(last[14]) == {12, 13, 14}
    if name == "two_tiles":
        assert c.B * c.beam == 40 and all(set(last[s]) == set(range(s // K * K, s // K * K + K)) for s in last)
        assert {o for s in (30, 31) for o in last[s]} == {30, 31, 32, 33, 34}      # an image across the two 32-row tiles


@pytest.mark.parametrize("lo,hi", R.KEY_RANGES)
def test_reading_the_own_slot_in_any_key_range_fails_the_tolerance_tenfold(lo, hi, dec, rotation):
    """the condition on the rotation script that gives test_gpu_beam_forced.py its teeth: were the ancestor lookup of keys
    [lo, hi) replaced by the row's own slot, EVERY row's logits would leave the float64 decode's by >= 10 tolerances"""
    c, true = rotation
    tol = KQ.logit_tolerance(true.logits)
    wrong = OB.scripted_decode(c.features, dec, c.parent, c.token, n_best=c.n_best, steps=hi, mutant=(lo, hi))
    assert torch.equal(wrong.ancestry[:hi], true.ancestry[:hi])
    if lo > 0:
        assert torch.equal(wrong.logits[:lo], true.logits[:lo])         # nothing differs before the range is reached
    per_slot = (wrong.logits[:hi] - true.logits[:hi]).abs().amax(-1).amax(0)
    print(f"keys [{lo}, {hi}): own-slot reads move the logits by {(per_slot / tol).min():.0f} .. {(per_slot / tol).max():.0f} tolerances")
    assert bool((per_slot >= 10 * tol).all()), (lo, hi, (per_slot / tol).tolist())


def test_script_check_refuses_what_a_top_k_cannot_choose():
    K, V, T = 3, R.VOCAB, 6
    parent = torch.arange(K).repeat(T, 2, 1)
    token = torch.arange(3, 3 + K).repeat(T, 2, 1)
    p, t = check_beam_script(parent, token, 2, V)
    assert p.dtype == t.dtype == torch.int32 and p.is_contiguous() and tuple(p.shape) == (T, 2, K)

    def refused(match, *edits, n_best=2):
        pp, tt = parent.clone(), token.clone()
        for which, idx, val in edits:
            (pp if which == "parent" else tt)[idx] = val
        with pytest.raises(ValueError, match=match):
            check_beam_script(pp, tt, n_best, V)
        if n_best == 2 and "outside" not in match:      # the oracle's strategy refuses the same scripts when it reaches them
            with pytest.raises(ValueError, match=match.split(".*")[-1]):
                st = OB.ScriptedStrategy(2, K, n_best, T, R.EOS, pp, tt, V)
                while not st.done:
                    st.advance(torch.zeros(len(st.origin) * K, V), lambda row, pt: None)

    refused("step 0", ("token", (0, 1, 2), R.EOS))
    refused("finished hypothesis", ("token", (2, 0, 1), R.EOS))                     # its own row goes on from it
    refused("finished hypothesis", ("token", (2, 0, 1), R.EOS), ("parent", (3, 0, 1), 0), ("token", (3, 0, 1), 9),
            ("parent", (3, 0, 2), 1))                                              # its row is refilled, another descends from it
    refused("twice", ("parent", (1, 1, 0), 1), ("token", (1, 1, 0), 4))
    refused("parent.*outside", ("parent", (5, 1, 2), K))
    refused("parent.*outside", ("parent", (0, 0, 0), -1))
    refused("token.*outside", ("token", (5, 0, 0), V))
    refused("token.*outside", ("token", (3, 1, 1), -1))
    refused("n_best", n_best=0)
    refused("n_best", n_best=K + 1)
    with pytest.raises(ValueError, match="max_len, B, beam"):
        check_beam_script(parent[0], token[0], 1, V)
    with pytest.raises(ValueError, match="max_len, B, beam"):
        check_beam_script(parent, token[:, :1], 1, V)
    with pytest.raises(ValueError, match="max_len, B, beam"):
        check_beam_script(parent.float(), token, 1, V)
    # a finished hypothesis that is not a parent is fine; so is anything in the rows of an image that has left
    pp, tt = parent.clone(), token.clone()
    tt[2, 0, 1] = R.EOS
    pp[3:, 0, 1] = 0
    tt[3:, 0, 1] = 9
    check_beam_script(pp, tt, 2, V)
    tt[1, 1, 0] = R.EOS          # image 1 leaves after step 1 with n_best = 1: what follows is not read
    tt[3, 1] = 5
    pp[3, 1] = 1
    check_beam_script(pp, tt, 1, V)
    with pytest.raises(ValueError, match="finished hypothesis"):     # with n_best = 2 it stays, and step 2 goes on from the finished row
        check_beam_script(pp, tt, 2, V)
