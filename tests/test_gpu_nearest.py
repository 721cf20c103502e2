"""GPU (-m gpu): mnx_tanimoto_search — for every query row of fingerprints its k nearest library rows — against the oracle of
tests/nearest_ref.py (byte-table bit counts of Q & R and Q | R, a full sort, the cut), list for list and byte for byte, no
tolerance anywhere: every output and the scratch FILL-filled with GUARD bytes behind it, the shapes at which a slab, a query tile
and the walk over the slabs take another turn, exact ties across lists, the thresholds at and one double above a hit's score,
SKIP_SELF on one pointer, each nullable output, every argument error, and the Python layer up to the facade."""
import collections

import numpy as np
import pytest
import torch

import nearest_ref as N
import packed_tables
from molnextr_amd import weights as W
from molnextr_amd.abi import (FP_WORDS, NEAREST_MAX_K, NEAREST_MAX_LISTS, NEAREST_MAX_QUERIES, NEAREST_NONE,
                              NEAREST_QUERY_TILE, NEAREST_SKIP_SELF, NEAREST_SLAB_ROWS)
from packed_tables import FILL, _call, _p, _up, dev, eng  # noqa: F401

pytestmark = pytest.mark.gpu

T, S, L = NEAREST_QUERY_TILE, NEAREST_SLAB_ROWS, NEAREST_MAX_LISTS
OUTPUTS = ("count", "index", "both", "either", "similarity")
Found = collections.namedtuple("Found", "rc count index both either similarity work error")


def random_rows(rng, n):
    """n rows with about 384 of 2048 bits set, the drug-like median: a bit of (a & b) & ~(c & d) is set with probability 3/16"""
    a, b, c, d = (rng.integers(0, 1 << 32, (n, FP_WORDS), dtype=np.uint64).astype(np.uint32) for _ in range(4))
    return (a & b) & ~(c & d)


def bits_of(row):
    return [t for t in range(2048) if row[t >> 5] >> (t & 31) & 1]


def planted(seed, nq, nl):
    """(queries, library): random rows, and — as far as the library has the rows for it —
      query 0 itself at the last row of the first slab and at the first row of the last slab: equal scores in different lists;
      a row scoring n/2 / n and one scoring (n/2 + 10) / (n + 20) against query 0: exactly 1/2 in two spellings, the larger
        numbers at the LOWER index (1), the smaller at nl - 4;
      an all-zero row at 3; with more than one query the last query all zero, alone in its tile when nq = T + 1"""
    rng = np.random.default_rng(seed)
    queries, library = random_rows(rng, nq), random_rows(rng, nl)
    on = bits_of(queries[0])
    if len(on) % 2:
        queries[0][on[-1] >> 5] &= ~np.uint32(1 << (on[-1] & 31))
        on = on[:-1]
    off = [t for t in range(2048) if t not in set(on)]
    half = len(on) // 2
    if nl >= 8:
        library[3] = 0
        library[1] = N.words_of(on[:half + 10] + off[:20])
        library[nl - 4] = N.words_of(on[half:])
    elif nl == 2:
        library[1] = 0
    library[min(S - 1, nl - 1)] = queries[0]
    library[(nl - 1) // S * S] = queries[0]
    if nq > 1:
        queries[nq - 1] = 0
    return queries, library


def search(eng, dev, q_rows, l_rows, k, min_similarity=0.0, flags=0, same=False, over=None):
    """one call of mnx_tanimoto_search through packed_tables._call: the five outputs and the scratch FILL-filled with GUARD bytes
    behind them, found untouched; same: the library IS the queries, one pointer; over: {argument name: value} in the place of what
    stands here (None: a null pointer)"""
    nq, nl = len(q_rows), len(l_rows)
    d_q = _up(dev, np.ascontiguousarray(q_rows, np.uint32))
    d_l = d_q if same else _up(dev, np.ascontiguousarray(l_rows, np.uint32))
    work_bytes = int(eng.lib.mnx_tanimoto_search_work_bytes(nq, nl, k))
    assert 0 < work_bytes <= nq * k * 8 * L
    args = {"queries": _p(d_q), "nq": nq, "library": _p(d_l), "nl": nl, "k": k, "min_similarity": float(min_similarity), "flags": flags,
            **dict.fromkeys(OUTPUTS), "work": None, "work_bytes": work_bytes}
    sizes = {"count": 4 * nq, "index": 4 * nq * k, "both": 4 * nq * k, "either": 4 * nq * k, "similarity": 8 * nq * k, "work": work_bytes}
    rc, error, host = _call(eng, "mnx_tanimoto_search", dev, args, sizes, dict(over or {}))
    cut = {name: host[name][:sizes[name]] for name in sizes}
    return Found(rc, cut["count"].view(np.uint32), *(cut[name].view(np.uint32).reshape(nq, k) for name in ("index", "both", "either")),
                 cut["similarity"].view(np.float64).reshape(nq, k), cut["work"], error)


def same_as(got, want, what=""):
    """the comparison rule: count, index, both and either equal as lists, similarity equal as bytes"""
    assert got.rc == 0, f"{what}: rc {got.rc}: {got.error}"
    for name in ("count", "index", "both", "either"):
        assert getattr(got, name).tolist() == want[name].tolist(), f"{what}: {name}"
    assert got.similarity.tobytes() == want["similarity"].tobytes(), f"{what}: similarity"


def check(eng, dev, queries, library, k, what, **kw):
    """one shape: the oracle's lists and bytes, a second run with identical bytes, and every hit's (both, either, similarity)
    equal to what mnx_tanimoto returns on that (query, row) pair. Returns the oracle's result."""
    want = N.search(queries, library, k, kw.get("min_similarity", 0.0), bool(kw.get("flags", 0) & NEAREST_SKIP_SELF))
    got = search(eng, dev, queries, library, k, **kw)
    same_as(got, want, what)
    again = search(eng, dev, queries, library, k, **kw)
    for name in OUTPUTS:
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), f"{what}: the second run's {name}"
    qi, j = np.nonzero(got.index != NEAREST_NONE)
    assert [int((row != NEAREST_NONE).sum()) for row in got.index] == got.count.tolist(), what
    if len(qi):
        pairs = eng.tanimoto(np.asarray(queries)[qi], np.asarray(library)[got.index[qi, j]])
        assert pairs["both"].tolist() == got.both[qi, j].tolist() and pairs["either"].tolist() == got.either[qi, j].tolist(), what
        assert pairs["similarity"].tobytes() == got.similarity[qi, j].tobytes(), what
    return want


@pytest.mark.parametrize("nq", [1, T + 1])
@pytest.mark.parametrize("nl", [1, 2, 63, 65, S - 1, S, S + 1, 2 * S + 3])
def test_shapes_against_the_oracle(eng, dev, nl, nq):
    """every library size around a wave and a slab, with one query and with a second tile of one query, at k of 1, 3 and 64 (k
    beyond the library among them), the planted rows of planted()"""
    queries, library = planted(1000 * nl + nq, nq, nl)
    for k in (1, 3, 64):
        want = check(eng, dev, queries, library, k, f"nl {nl} nq {nq} k {k}")
        assert want["count"].tolist() == [min(k, nl)] * nq
        first, last = sorted({min(S - 1, nl - 1), (nl - 1) // S * S})[0], sorted({min(S - 1, nl - 1), (nl - 1) // S * S})[-1]
        assert want["index"][0, 0] == first and want["similarity"][0, 0] == 1.0                      # itself, the lower index first
        if k > 1 and last != first:
            assert want["index"][0, 1] == last and want["similarity"][0, 1] == 1.0
        if nq > 1:                                                                                   # the all-zero query: the first rows, 0.0
            assert want["index"][nq - 1].tolist()[:min(k, nl)] == list(range(min(k, nl))) and not want["similarity"][nq - 1].any()
    if nl >= 8:                                                                                      # 1/2 twice: the lower index first
        at = [int(np.nonzero(want["index"][0] == row)[0][0]) for row in (1, nl - 4)]
        assert at[1] == at[0] + 1 and want["similarity"][0, at].tolist() == [0.5, 0.5]
        assert want["both"][0, at[0]] == want["both"][0, at[1]] + 10 and want["either"][0, at[0]] == want["either"][0, at[1]] + 20


def test_a_workgroup_wraps_round_to_a_second_slab(eng, dev):
    """nl = L * S + S + 1: more slabs than a query may have lists, so the first two workgroups walk two slabs each; query 0 stands in
    the first slab and in the last — a slab of one row, walked second by workgroup 1"""
    nl = L * S + S + 1
    queries, library = planted(7, 2, nl)
    want = check(eng, dev, queries, library, 3, "wrap")
    assert want["index"][0].tolist()[:2] == [S - 1, nl - 1] and want["similarity"][0].tolist()[:2] == [1.0, 1.0]
    assert want["index"][1].tolist() == [0, 1, 2]


def test_one_half_and_two_quarters(eng, dev):
    """rows scoring exactly 1/2 and 2/4 against query 0, in both index orders and across slabs: the lower index comes first"""
    rng = np.random.default_rng(3)
    q = np.stack([N.words_of({0, 1})])
    for nl, lo, hi in ((2, 0, 1), (S + 2, S - 1, S), (2 * S + 3, 5, 2 * S + 2)):
        for first, second in ((N.words_of({0}), N.words_of({0, 1, 2, 3})), (N.words_of({0, 1, 2, 3}), N.words_of({0}))):
            library = random_rows(rng, nl) & ~np.uint32(3)                                           # no other row shares a bit with the query
            library[lo], library[hi] = first, second
            want = check(eng, dev, q, library, 2, f"1/2 and 2/4, nl {nl}")
            assert want["index"].tolist() == [[lo, hi]] and want["similarity"].tolist() == [[0.5, 0.5]]
            assert sorted(zip(want["both"][0].tolist(), want["either"][0].tolist())) == [(1, 2), (2, 4)]


def test_thresholds(eng, dev):
    """min_similarity of 0.0 and 1.0, the exact double of a planted hit's score (kept) and the next double above it (dropped)"""
    nl = S + 1
    queries, library = planted(11, 2, nl)
    half = 0.5
    for k in (1, 8):
        everything = check(eng, dev, queries, library, k, "min 0.0", min_similarity=0.0)
        assert everything["count"].tolist() == [k, k]
        exact = check(eng, dev, queries, library, k, "min 1.0", min_similarity=1.0)
        assert exact["count"].tolist() == [min(k, 2), 0] and exact["index"][1].tolist() == [NEAREST_NONE] * k
    kept = check(eng, dev, queries, library, 8, "min 1/2", min_similarity=half)
    assert kept["count"].tolist() == [4, 0] and kept["index"][0].tolist()[:4] == [S - 1, S, 1, nl - 4]
    dropped = check(eng, dev, queries, library, 8, "min above 1/2", min_similarity=float(np.nextafter(half, 1.0)))
    assert dropped["count"].tolist() == [2, 0] and dropped["index"][0].tolist()[2:] == [NEAREST_NONE] * 6
    # a score that is no short binary fraction: both / either of the third hit of a random query
    queries, library = planted(12, 1, nl)
    ranked = N.search(queries, library, 8)
    score = float(ranked["similarity"][0, 4])
    assert 0.0 < score < 0.5 and score == int(ranked["both"][0, 4]) / int(ranked["either"][0, 4])
    tail = int((ranked["similarity"][0] >= score).sum())
    assert check(eng, dev, queries, library, 8, "min at a hit", min_similarity=score)["count"].tolist() == [tail]
    above = check(eng, dev, queries, library, 8, "min above a hit", min_similarity=float(np.nextafter(score, 1.0)))
    assert above["count"].tolist() == [int((ranked["similarity"][0] > score).sum())] and above["count"][0] < tail


def test_skip_self_on_one_pointer(eng, dev):
    """queries == library, the same pointer, nl = S + 1, k = 2: no hit is the query's own row, and the result is the oracle's with
    row q removed; a duplicate of row 0 at row S is row 0's nearest other row, and the other way round"""
    rows = random_rows(np.random.default_rng(21), S + 1)
    rows[S] = rows[0]
    rows[7] = 0
    want = check(eng, dev, rows, rows, 2, "skip self", flags=NEAREST_SKIP_SELF, same=True)
    assert all(q not in hits for q, hits in enumerate(want["index"].tolist()))
    assert want["index"][0, 0] == S and want["index"][S, 0] == 0 and want["similarity"][[0, S], 0].tolist() == [1.0, 1.0]
    without = N.search(rows, rows, 3)
    for q in range(S + 1):
        assert [i for i in without["index"][q].tolist() if i != q][:2] == want["index"][q].tolist()
    plain = check(eng, dev, rows, rows, 2, "one pointer, no flag", same=True)
    assert plain["index"][:, 0].tolist() == [0] + list(range(1, 7)) + [0] + list(range(8, S)) + [0]   # itself, or the first of its equals


def test_each_nullable_output_null_in_turn(eng, dev):
    queries, library = planted(31, T + 1, S + 1)
    want = N.search(queries, library, 3)
    for name in ("both", "either", "similarity"):
        got = search(eng, dev, queries, library, 3, over={name: None})
        assert got.rc == 0, got.error
        for other in OUTPUTS:
            x = getattr(got, other)
            if other == name:
                assert (x.view(np.uint8) == FILL).all(), f"{name} is null and its buffer was written"
            elif other == "similarity":
                assert x.tobytes() == want[other].tobytes()
            else:
                assert x.tolist() == want[other].tolist(), (name, other)
    none = search(eng, dev, queries, library, 3, over=dict(both=None, either=None, similarity=None))
    assert none.rc == 0 and none.index.tolist() == want["index"].tolist() and none.count.tolist() == want["count"].tolist()


def test_argument_errors(eng, dev):
    """every argument error of the header with its message; nothing is launched: the outputs and the scratch are still FILL"""
    queries, library = planted(41, 2, 5)
    skew = _up(dev, np.zeros(64, np.uint8))
    work_bytes = int(eng.lib.mnx_tanimoto_search_work_bytes(2, 5, 3))

    def refused(expect, **over):
        got = search(eng, dev, queries, library, 3, over=over)
        assert got.rc == -1 and got.error == "mnx_tanimoto_search: " + expect, (over, got.rc, got.error)
        for name in OUTPUTS + ("work",):
            assert (getattr(got, name).view(np.uint8) == FILL).all(), f"{name} was written by a call refused with {expect!r}"

    for name in ("queries", "library", "count", "index", "work"):
        refused("null pointer", **{name: None})
    for nq in (0, -1, NEAREST_MAX_QUERIES + 1):
        refused("1 <= nq <= 4096 required", nq=nq)
    for nl in (0, (1 << 24) + 1, 0xFFFFFFFF):
        refused("1 <= nl <= 16777216 required", nl=nl)
    for k in (0, NEAREST_MAX_K + 1):
        refused("1 <= k <= 64 required", k=k)
    for s in (float("nan"), -1e-300, float(np.nextafter(1.0, 2.0)), float("inf"), -float("inf")):
        refused("0 <= min_similarity <= 1 required", min_similarity=s)
    for flags in (2, 3, 1 << 31):
        refused("flags may hold MNX_NEAREST_SKIP_SELF only", flags=flags)
    for short in (0, work_bytes - 1):
        refused("work_bytes is below mnx_tanimoto_search_work_bytes(nq, nl, k)", work_bytes=short)
    aligned = "queries, library, count, index, both and either must be 4-byte aligned, similarity and work 8-byte"
    for name, off in (("queries", 2), ("library", 1), ("count", 2), ("index", 3), ("both", 2), ("either", 1), ("similarity", 4), ("work", 4)):
        refused(aligned, **{name: _p(skew, off)})
    assert eng.lib.mnx_tanimoto_search(None, None, 0, None, 0, 0, 0.0, 0, None, None, None, None, None, None, 0, None) == -1
    ok = search(eng, dev, queries, library, 3, min_similarity=-0.0)                                  # minus zero is zero
    same_as(ok, N.search(queries, library, 3), "min -0.0")


# ------------------------------------------------------------------------------------ the Python layer
def test_engine_tanimoto_search_in_chunks(eng, dev):
    """Engine.tanimoto_search on numpy and on device rows, with one query more than a call takes, on a library of 65 rows"""
    nq = NEAREST_MAX_QUERIES + 1
    rng = np.random.default_rng(51)
    library = random_rows(rng, 65)
    queries = random_rows(rng, nq)
    queries[nq - 1] = library[64]                                                                    # the chunk of one finds its row
    queries[5] = 0
    want = N.search(queries, library, 3, min_similarity=0.05)
    assert want["index"][nq - 1, 0] == 64 and want["count"][5] == 0 and want["count"].max() == 3
    for rows in ((queries, library), (torch.from_numpy(queries.view(np.int32)).to(dev), torch.from_numpy(library.view(np.int32)).to(dev))):
        got = eng.tanimoto_search(*rows, k=3, min_similarity=0.05)
        assert set(got) == set(OUTPUTS) and got["index"].dtype == np.uint32 and got["similarity"].dtype == np.float64
        for name in ("count", "index", "both", "either"):
            assert got[name].tolist() == want[name].tolist(), name
        assert got["similarity"].tobytes() == want["similarity"].tobytes()
    on_device = eng.tanimoto_search(queries[:3], library, keep_device=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in on_device.values()) and on_device["index"].shape == (3, 1)
    assert on_device["index"].cpu().numpy().view(np.uint32).tolist() == N.search(queries[:3], library)["index"].tolist()
    with pytest.raises(ValueError, match="skip_self takes at most 4096 queries"):
        eng.tanimoto_search(queries, library, skip_self=True)
    own = eng.tanimoto_search(library, library, k=1, skip_self=True)
    assert own["index"].tolist() == N.search(library, library, 1, skip_self=True)["index"].tolist()
    for bad in (dict(k=0), dict(k=65)):
        with pytest.raises(ValueError, match="1 <= k <= 64"):
            eng.tanimoto_search(queries[:1], library, **bad)
    with pytest.raises(ValueError, match="words of 32 bits"):
        eng.tanimoto_search(queries[:, :63], library)


LIBRARY = ["CCO", "CCCCCC", "C1=CC=CC=C1", "CC(=O)O", "c1ccncc1", "CC(=O)Oc1ccccc1C(=O)O", "C1CCCCC1", "CN", "OC(=O)c1ccccc1O", "Cc1ccccc1"]


def test_nearest_smiles(eng):
    from molnextr_amd.graphs import nearest_smiles, smiles_fingerprints, smiles_library
    passes = dict(kekulize=True, normalize=True)
    found = nearest_smiles(eng, ["c1ccccc1", "C1CC", "CC(=O)Oc1ccccc1C(=O)O"], LIBRARY, k=3, **passes)
    assert found[0][0] == {"index": 2, "smiles": "C1=CC=CC=C1", "similarity": 1.0} and len(found[0]) == 3
    assert found[1] == []                                                                            # an unreadable query
    assert found[2][0]["index"] == 5 and found[2][0]["similarity"] == 1.0
    for hits in found:
        assert [h["similarity"] for h in hits] == sorted((h["similarity"] for h in hits), reverse=True)
        assert all(h["smiles"] == LIBRARY[h["index"]] for h in hits)
    made = smiles_library(eng, LIBRARY, **passes)
    assert set(made) == {"bits", "flags", "smiles"} and made["bits"].is_cuda and tuple(made["bits"].shape) == (10, FP_WORDS)
    assert made["smiles"] == LIBRARY and not made["flags"].any()
    assert nearest_smiles(eng, ["c1ccccc1", "C1CC", "CC(=O)Oc1ccccc1C(=O)O"], made, k=3, **passes) == found
    # by hand: the fingerprints of both sides through Engine.tanimoto_search
    prints = [np.frombuffer(x["fingerprint"], np.uint32) for x in smiles_fingerprints(eng, ["c1ccccc1"] + LIBRARY, **passes)]
    by_hand = eng.tanimoto_search(prints[:1], np.stack(prints[1:]), k=3)
    assert [h["index"] for h in found[0]] == by_hand["index"][0].tolist() and [h["similarity"] for h in found[0]] == by_hand["similarity"][0].tolist()
    assert nearest_smiles(eng, ["c1ccccc1"], LIBRARY)[0][0]["similarity"] < 1.0                      # without the passes the spellings differ
    assert nearest_smiles(eng, ["CCO"], LIBRARY, min_similarity=1.0) == [[{"index": 0, "smiles": "CCO", "similarity": 1.0}]]
    assert nearest_smiles(eng, [], LIBRARY) == []
    unread = smiles_library(eng, ["CCO", "C1CC"])
    assert unread["flags"][0] == 0 and unread["flags"][1] >> 31 == 1
    with pytest.raises(TypeError, match="nearest_smiles: no pass named"):
        nearest_smiles(eng, ["C"], LIBRARY, aromatize=True)
    with pytest.raises(ValueError, match="an empty library"):
        smiles_library(eng, [])


def test_predict_nearest_and_the_facade(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images at paths of the default length: predict_nearest's 'nearest' against Engine.tanimoto_search on the
    fingerprints predict_fingerprints returns for the same images, sorted by the order of the rule; a library as a list and as
    smiles_library's dict; the facade's attribute, and with it unset the keys of before"""
    from molnextr_amd.graphs import smiles_library
    from molnextr_amd.model import molnextr, predict_fingerprints, predict_nearest, predict_pipeline
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True)
    prints = predict_fingerprints(eng, imgs, ref_batch_size=4)
    own = [p["fingerprint"] for p in prints]
    library = smiles_library(eng, LIBRARY)
    lib_rows = library["bits"].cpu().numpy().view(np.uint32)
    # the predictions' own fingerprints join the library, so that a hit at 1.0 exists for every molecule that has one
    rows = np.stack([np.frombuffer(f or bytes(256), np.uint32) for f in own])
    both = {"bits": torch.from_numpy(np.concatenate([lib_rows, rows]).view(np.int32)).to(dev), "flags": None, "smiles": LIBRARY + [f"own {i}" for i in range(8)]}
    got = predict_nearest(eng, imgs, both, k=4, ref_batch_size=4)
    by_hand = eng.tanimoto_search(rows, both["bits"], k=4)
    for i, (p, g) in enumerate(zip(plain, got)):
        assert "nearest" not in p and set(g) == set(p) | {"nearest"}
        if own[i] is None:
            assert g["nearest"] == []
            continue
        n = int(by_hand["count"][i])
        assert [h["index"] for h in g["nearest"]] == by_hand["index"][i, :n].tolist() and n == 4
        assert [h["similarity"] for h in g["nearest"]] == by_hand["similarity"][i, :n].tolist()
        assert all(h["smiles"] == both["smiles"][h["index"]] for h in g["nearest"])
        keys = [(-h["similarity"], h["index"]) for h in g["nearest"]]
        assert keys == sorted(keys) and g["nearest"][0]["similarity"] == 1.0 and g["nearest"][0]["index"] <= 10 + i
    listed = predict_nearest(eng, imgs, LIBRARY, k=2, min_similarity=0.0, ref_batch_size=4, fingerprint=True)
    made = predict_nearest(eng, imgs, library, k=2, ref_batch_size=4)
    assert [g["nearest"] for g in listed] == [g["nearest"] for g in made] and [g["fingerprint"] for g in listed] == own
    with pytest.raises(ValueError, match="predict_nearest needs packed=True"):
        predict_nearest(eng, imgs[:1], LIBRARY, packed=False)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_kekulize=True, graph_normalize=True)
    try:
        assert m.graph_nearest is None and m.graph_nearest_k == 1
        before = m.predict_images(pages[:2], batch_size=2)
        m.graph_nearest, m.graph_nearest_k = LIBRARY, 2                            # attributes: the constructor's list is closed
        out = m.predict_images(pages, batch_size=4)
        want = predict_nearest(m.engine, m._transform(pages), LIBRARY, 2, 0.0, m.tokenizer, ref_batch_size=4, smiles=True, stereo=False,
                               kekulize=True, normalize=True)
        assert [o["nearest"] for o in out] == [p["nearest"] for p in want] and all(set(o) == set(before[0]) | {"nearest"} for o in out)
        m.graph_fingerprint = True
        assert all({"nearest", "fingerprint"} <= set(o) for o in m.predict_images(pages[:2], batch_size=2))
        m.graph_fingerprint = False
        assert m.nearest(["C1=CC=CC=C1"], LIBRARY, kekulize=True, normalize=True)[0][0]["index"] == 2
        m.graph_nearest = None                                                     # the default: the keys of before
        after = m.predict_images(pages[:2], batch_size=2)
        assert [set(o) for o in after] == [set(o) for o in before] and all("nearest" not in o for o in after)
    finally:
        m.engine.close()
