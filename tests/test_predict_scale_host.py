"""CPU checks of tests/predict_scale_ref.py, the helper of tests/test_gpu_predict_scale.py: the job builder keeps different
images in slots a power-of-two number of tiles apart, the expectation maps the lone calls onto the job's rows (ragged tail
included), the comparison fails on each of the errors it is there to catch, and the trace parser reads predict_impl's lines."""
import pytest
import torch

import predict_scale_ref as P

SLOTS = (1088, 3072, 4096)          # the engines of tests/test_gpu_predict_scale.py: 34, 96 and 128 tiles


def _jobs():
    return [(sl, name, rb, n) for sl in SLOTS for name, (rb, n) in P.job_images(sl).items()]


@pytest.mark.parametrize("sl,name,rb,n_img", _jobs())
def test_job_shape(sl, name, rb, n_img):
    """Full chunks cycle through the 7 pool batches in order, the last chunk is ragged, and the first wave fills the engine:
    every tile in job A, all but fewer than three tiles in job B."""
    chunks = P.job_chunks(n_img, rb)
    assert sum(r for _, r in chunks) == n_img
    assert all(r == rb for _, r in chunks[:-1]) and 0 < chunks[-1][1] < rb
    assert [b for b, _ in chunks] == [c % 7 for c in range(len(chunks))]
    if name == "A":
        assert chunks[-1][1] == 20 and len(chunks) == sl // 32 + 7 + 1
    tiles_per_chunk = rb // 32
    first_wave = sl // 32 // tiles_per_chunk
    assert len(chunks) > first_wave                       # a second wave reuses tiles
    assert sl // 32 - first_wave * tiles_per_chunk < tiles_per_chunk
    assert len(P.lone_calls(n_img, rb)) == 8              # K full batches and the tail


@pytest.mark.parametrize("sl,name,rb,n_img", _jobs())
def test_power_of_two_tile_distances_hold_different_images(sl, name, rb, n_img):
    """First wave: job row r sits in slot r. A slot and the slot 2^k tiles (32 * 2^k rows) further, k = 0 .. 6, never hold
    the same pool image; with one-tile chunks the two chunks hold different pool batches."""
    idx = P.job_index(n_img, rb)
    assert idx.shape == (n_img,) and int(idx.max()) < P.K * rb
    filled = sl // 32 // (rb // 32) * rb                  # slots the first wave fills
    for k in range(7):
        d = 32 << k
        if d >= filled:
            continue
        assert not (idx[:filled - d] == idx[d:filled]).any(), (k, d)
        if rb == 32:
            chunks = P.job_chunks(n_img, rb)[:filled // 32]
            assert all(chunks[c][0] != chunks[c + (1 << k)][0] for c in range(len(chunks) - (1 << k)))
    # and the index is what the chunk list says, row by row
    c = 0
    for batch, rows in P.job_chunks(n_img, rb):
        assert idx[c:c + rows].tolist() == list(range(batch * rb, batch * rb + rows))
        c += rows


def _lone(n_img, rb, kmax=6, T=9, seed=0):
    """Synthetic lone-call results: random words, different for every (pool batch, rows) key."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for batch, rows in P.lone_calls(n_img, rb):
        out[batch, rows] = {
            "tokens": torch.randint(0, 200, (rows, T), generator=g, dtype=torch.int32),
            "lengths": torch.randint(1, T, (rows,), generator=g, dtype=torch.int32),
            "token_logp": -torch.rand(rows, T, generator=g),
            "n_atoms": torch.randint(0, kmax, (rows,), generator=g, dtype=torch.int32),
            "atom_idx": torch.randint(0, T, (rows, kmax), generator=g, dtype=torch.int32),
            "edges": torch.randint(0, 7, (rows, kmax, kmax), generator=g).to(torch.uint8),
            "edge_scores": torch.rand(rows, kmax, kmax, generator=g, dtype=torch.float64),
            "atom_scores": torch.rand(rows, kmax, generator=g, dtype=torch.float64),
            "overall_score": torch.rand(rows, generator=g, dtype=torch.float64),
        }
    return out


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


@pytest.mark.parametrize("sl,name,rb,n_img", _jobs())
def test_expectation_maps_lone_calls_onto_rows(sl, name, rb, n_img):
    lone = _lone(n_img, rb)
    want = P.expectation(lone, n_img, rb)
    assert set(want) == set(P.KEYS)
    chunks = P.job_chunks(n_img, rb)
    for c in sorted({0, 6, 7, min(33, len(chunks) - 3), len(chunks) - 2, len(chunks) - 1}):
        batch, rows = chunks[c]
        for key in P.KEYS:
            assert torch.equal(want[key][c * rb:c * rb + rows], lone[batch, rows][key]), (c, key)
            assert want[key].shape[0] == n_img
    tail_batch, tail_rows = chunks[-1]
    assert (tail_batch, tail_rows) in lone and tail_rows == n_img % rb
    P.compare(_clone(want), want, rb, "identical")


def test_comparison_has_teeth():
    """Each of the errors the GPU test is there to catch fails the comparison, with the row and chunk named."""
    rb, n_img = P.job_images(4096)["A"]
    lone = _lone(n_img, rb)
    want = P.expectation(lone, n_img, rb)
    # chunk c replaced by chunk c + 32: a slot alias of 1024
    for c in (0, 5, 95):
        got = _clone(want)
        for key in got:
            got[key][c * rb:(c + 1) * rb] = want[key][(c + 32) * rb:(c + 33) * rb]
        with pytest.raises(AssertionError, match=rf"first job row {c * rb} = chunk {c} "):
            P.compare(got, want, rb, "alias")
    # one changed log-prob word in the last row (one unit in the last place)
    got = _clone(want)
    w = got["token_logp"].view(torch.int32)
    w[-1, 3] += 1
    assert abs(float(got["token_logp"][-1, 3] - want["token_logp"][-1, 3])) < 1e-6
    with pytest.raises(AssertionError, match=rf"'token_logp' differs in 1 of {n_img} rows, first job row {n_img - 1} "):
        P.compare(got, want, rb, "logp word")
    # a sign of zero is a changed word too
    got = _clone(want)
    got["token_logp"][7, 0] = 0.0
    ref = _clone(want)
    ref["token_logp"][7, 0] = -0.0
    with pytest.raises(AssertionError, match="'token_logp' differs in 1 of"):
        P.compare(got, ref, rb, "signed zero")
    # one changed bond class
    got = _clone(want)
    got["edges"][1500, 2, 1] = (got["edges"][1500, 2, 1] + 1) % 7
    with pytest.raises(AssertionError, match=r"'edges' differs in 1 of \d+ rows, first job row 1500 = chunk 46 "):
        P.compare(got, want, rb, "bond class")
    # a missing key, a changed score word
    got = _clone(want)
    del got["atom_scores"]
    with pytest.raises(AssertionError):
        P.compare(got, want, rb, "missing key")
    got = _clone(want)
    got["overall_score"].view(torch.int64)[4000] += 1
    with pytest.raises(AssertionError, match="'overall_score' differs in 1 of"):
        P.compare(got, want, rb, "score word")


SAMPLE = """\
0.412 seq 0 live 16 next 16 next_enc 32 done 0 free_tiles 18 scan 1024 rows_cap 512
1.873 seq 1 live 34 next 34 next_enc 42 done 0 free_tiles 0 scan 1088 rows_cap 1088
977.250 seq 240 live 3 next 42 next_enc 42 done 39 free_tiles 31 scan 1024 rows_cap 64
981.004 end host_wait_ms 803.551
"""


def test_trace_parser():
    polls, ends = P.parse_trace(SAMPLE)
    assert len(polls) == 3 and len(ends) == 1
    assert polls[1] == {"ms": 1.873, "seq": 1, "live": 34, "next": 34, "next_enc": 42, "done": 0, "free_tiles": 0,
                        "scan": 1088, "rows_cap": 1088}
    assert [p["scan"] for p in polls] == [1024, 1088, 1024] and [p["rows_cap"] for p in polls] == [512, 1088, 64]
    assert ends[0] == {"ms": 981.004, "host_wait_ms": 803.551}
    assert P.parse_trace("") == ([], [])
    with pytest.raises(ValueError):          # a line without the two fields the tests rely on is not read as a poll
        P.parse_trace("0.412 seq 0 live 16 next 16 next_enc 32 done 0 free_tiles 18\n")


def test_rows_cap_rule():
    """predict_impl's capacity: the bound rounded up to 64 up to 1024 rows, to 128 up to 2048, to 256 beyond, at most
    dec_slots. 1088 slots reach 1088 = min(1088, 1152) from the 128 step; 1088 is no capacity of a larger engine."""
    assert P.rows_cap_of(1, 4096) == 64 and P.rows_cap_of(1024, 4096) == 1024
    assert P.rows_cap_of(1025, 4096) == 1152 and P.rows_cap_of(2048, 4096) == 2048
    assert P.rows_cap_of(2049, 4096) == 2304 and P.rows_cap_of(4096, 4096) == 4096
    assert P.rows_cap_of(1025, 1088) == 1088 and P.rows_cap_of(1088, 1088) == 1088
    a = P.allowed_rows_caps(1088)
    assert sorted(a) == list(range(64, 1025, 64)) + [1088] and a[1088] == {128} and a[1024] == {64}
    a = P.allowed_rows_caps(3072)
    assert sorted(a) == list(range(64, 1025, 64)) + list(range(1152, 2049, 128)) + list(range(2304, 3073, 256))
    assert 1088 not in a and a[1280] == {128} and a[2304] == {256}
    assert max(P.allowed_rows_caps(4096)) == 4096
