"""GPU (-m gpu): mnx_substructure_match — does a query molecule embed in a target molecule, how often and where — against the
oracle of tests/substructure_ref.py, word for word (no tolerances), guard bytes included: the hand-made pairs of the host test,
every way of pairing two tables, the shapes at which the split of the roots over the lanes, the sort of the lists and the stack take
another turn, every refusal on either side, the step limit, determinism, every argument error, the documented place behind the
chain of passes, the known limit of the canonical ranks, and one end-to-end run through predict_substructures, the facade and
evaluate's score."""
import collections
import functools
import itertools

import numpy as np
import pytest

import molfile_ref as M
import packed_tables
import substructure_ref as X
import test_canon_host as CH
import test_substructure_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import MATCH_DTYPE, MATCH_LIMIT, MATCH_MAX_QUERY, MATCH_NO_ATOM, MATCH_REFUSED, READ_REFUSED, SMILES_REFUSED, Engine
from packed_tables import Tables, _call, _p, _up, assert_refused, dev, eng, mol, random_molecule, same_array, same_mols  # noqa: F401

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the writers' end-to-end tests
Q = X.QUERY_SHIFT

MatchResult = collections.namedtuple("MatchResult", "rc recs maps error")


def run(eng, q, t, pairs, max_matches=1, max_steps=0, q_sizes=None, t_sizes=None, **over):
    """one call of mnx_substructure_match on the tables q and t (they may be the same object): both outputs FILL-filled with GUARD
    bytes behind them, found untouched; over: arguments by name (q_mols, n_t, pair_list for `pairs`, ...)"""
    pairs = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
    d_pairs = _up(t.dev, pairs)
    n = len(pairs)
    args = {**{("q_" + k if not k.startswith("n") else k + "_q"): v for k, v in q.head(q_sizes).items()},
            **{("t_" + k if not k.startswith("n") else k + "_t"): v for k, v in t.head(t_sizes).items()},
            "pair_list": _p(d_pairs), "n_pairs": n, "recs": None, "maps": None, "max_matches": max_matches, "max_steps": max_steps}
    nbytes = {"recs": n * MATCH_DTYPE.itemsize, "maps": n * MATCH_MAX_QUERY * 2}
    rc, error, host = _call(eng, "mnx_substructure_match", t.dev, args, nbytes, over)
    return MatchResult(rc, host["recs"][:nbytes["recs"]].view(MATCH_DTYPE), host["maps"][:nbytes["maps"]].view(np.uint16).reshape(n, MATCH_MAX_QUERY), error)


def arrays(t):
    return t.mols, t.atoms, t.bonds, t.text


def check(eng, q, t, pairs, ref=None, q_sizes=None, t_sizes=None, **kw):
    """the device's records and maps equal the oracle's; returns the oracle's"""
    ref = ref or X.pack(arrays(q), arrays(t), pairs, tables=H.TABLES, q_sizes=q_sizes, t_sizes=t_sizes, **kw)
    got = run(eng, q, t, pairs, q_sizes=q_sizes, t_sizes=t_sizes, **kw)
    assert got.rc == 0, f"rc {got.rc}: {got.error}"
    same_mols(got.recs, ref["match"], "recs")
    assert got.recs.tobytes() == ref["match"].tobytes()
    same_array(got.maps.reshape(-1), ref["map"].reshape(-1), "maps")
    return ref


def all_pairs(nq, nt):
    return [(i, j) for i in range(nq) for j in range(nt)]


def test_hand_made_pairs_one_per_launch_and_together(eng, dev):
    """the small graphs of the host test: every pair in one launch at 1 and at 65535 embeddings, and a part of them alone (n_pairs = 1)"""
    t = Tables(dev, H.small_molecules())
    pairs = all_pairs(t.n, t.n)
    ref = check(eng, t, t, pairs)
    assert 200 < (ref["match"]["n_matches"] > 0).sum() < len(pairs) // 2 and not (ref["match"]["flags"] & MATCH_REFUSED).any()
    check(eng, t, t, pairs, max_matches=65535)
    for p in pairs[::97]:
        check(eng, t, t, [p], max_matches=65535)                                   # n_pairs = 1
    benzene, toluene = H.SMALL.index("c1ccccc1"), H.SMALL.index("Cc1ccccc1")
    one = check(eng, t, t, [(benzene, toluene)], max_matches=65535)
    assert one["match"]["n_matches"].tolist() == [12] and one["map"][0][:7].tolist() == [1, 2, 3, 4, 5, 6, MATCH_NO_ATOM]


def test_one_against_many_many_against_one_and_a_long_pair_list(eng, dev):
    molecules = H.small_molecules()
    q, t = Tables(dev, molecules[:1]), Tables(dev, molecules)
    check(eng, q, t, [(0, j) for j in range(t.n)])                                 # one query, many targets
    check(eng, t, q, [(i, 0) for i in range(t.n)])                                 # many queries, one target
    rng = np.random.default_rng(5)
    long_list = rng.integers(0, t.n, (5 * t.n, 2))                                 # longer than either table, pairs repeated
    check(eng, t, t, long_list)
    bad = [(2, 3), (t.n, 0), (3, 9), (0, t.n), (0xFFFFFFFF, 0xFFFFFFFF), (9, 3), (70000, 2), (21, 19)]
    ref = check(eng, t, t, bad)
    assert ref["match"]["flags"].tolist() == [0, X.BAD_PAIR, 0, X.BAD_PAIR, X.BAD_PAIR, 0, X.BAD_PAIR, 0]


def test_more_roots_than_lanes_long_chains_and_a_hub(eng, dev):
    """a 300-atom chain has more roots than the 128 lanes that search; a chain of 999 atoms is admitted and one of 1000 is not; a
    hub of degree 300 makes one thread sort a list of 300 and a position try 300 candidates"""
    chain300 = H.chain([b"C", b"C", b"N"] * 100)
    hub = ([b"C"] + [b"N", b"O"] * 150, [(0, 0)] * 301, [(0, k, 1, 1) for k in range(300, 0, -1)])
    q = Tables(dev, [H.chain([b"C", b"N", b"C", b"C", b"N"]), H.chain([b"N", b"C", b"O"]), H.chain([b"C"] * 64), H.chain([b"C"] * 65),
                     H.chain([b"O", b"C", b"O"])])
    t = Tables(dev, [chain300, hub, H.chain([b"C"] * 999), H.chain([b"C"] * 1000), H.chain([b"C"] * 64)])
    ref = check(eng, q, t, [(0, 0), (1, 1), (4, 1), (2, 2), (2, 3), (2, 4), (3, 4)], max_matches=65535)
    assert ref["match"]["n_matches"].tolist() == [99 + 98, 150 * 150, 150 * 149, 2 * (999 - 63), 0, 2, 0]
    assert ref["match"]["flags"].tolist() == [0, 0, 0, 0, X.TOO_LARGE, 0, X.QUERY_TOO_LARGE]
    assert ref["map"][5].tolist() == list(range(64))
    first = check(eng, q, t, [(0, 0), (1, 1), (2, 2), (2, 4)])
    assert first["match"]["n_matches"].tolist() == [1, 1, 1, 1] and first["map"][0][:5].tolist() == [1, 2, 3, 4, 5]


def test_the_query_limits(eng, dev):
    """64 atoms and 128 bonds are a query, 65 atoms or 129 bonds are not; the admission of a large query is still reported"""
    ladder = [(k, k + 1, 1, 1) for k in range(63)] + [(k, k + 2, 1, 1) for k in range(62)] + [(0, 3, 1, 1), (1, 4, 1, 1), (2, 5, 1, 1), (3, 6, 1, 1)]
    q = Tables(dev, [([b"C"] * 64, [(0, 0)] * 64, ladder[:128]), ([b"C"] * 64, [(0, 0)] * 64, ladder[:129]), H.chain([b"C"] * 65),
                     H.chain([b"C", b"Ph"] * 40), ([b"C"] * 70, [(0, 0)] * 70, [(0, 1, 1, 1), (1, 0, 1, 1)]), H.chain([])])
    ref = check(eng, q, q, [(0, 0), (1, 1), (2, 2), (3, 3), (4, 2), (0, 1), (5, 0)], max_steps=X.MAX_STEPS)
    assert ref["match"]["flags"].tolist() == [0, X.QUERY_TOO_LARGE, X.QUERY_TOO_LARGE, X.QUERY_TOO_LARGE | X.PSEUDO << Q | X.PSEUDO, X.BAD_BOND << Q, 0,
                                              X.QUERY_EMPTY]
    assert ref["match"]["n_matches"].tolist() == [1, 0, 0, 0, 0, 1, 0] and ref["map"][0].tolist() == list(range(64))


def test_refusals_on_either_side_leave_the_pairs_around_them_alone(eng, dev):
    ok = mol([b"C", b"[NH3+]", b"O"], [(0, 1, 1, 1), (1, 2, 1, 1)])
    two = [b"C", b"N"]
    molecules = [ok, H.chain([b"C"] * 1000), mol(two, [(0, 2, 1, 1)]), mol(two, [(1, 1, 1, 1)]), mol(two, [(0, 1, 1, 1), (1, 0, 2, 2)]),
                 mol([b"C", b"Ph", b"[Xx]"], [(0, 1, 1, 1), (1, 2, 1, 1)]), mol([b"R", b"N"], [(0, 0, 1, 1)]), mol([]), H.chain([b"C"] * 65), ok]
    mols, atoms, bonds, text = M.build_tables(molecules)
    mols["flags"][9] = 1 | 1 << 10                                                 # truncated; the bits of the passes are not copied
    t = Tables(dev, arrays=(mols, atoms, bonds, text))
    pairs = [p for k in range(1, 10) for p in ((0, 0), (k, 0), (0, 0), (0, k))] + [(1, 2), (5, 5), (0, 0)]
    ref = check(eng, t, t, pairs)
    flags = ref["match"]["flags"].tolist()
    assert flags[::2][:18] == [0] * 18 and flags[-1] == 0 and (ref["map"][::2][:18, :4] == [0, 1, 2, MATCH_NO_ATOM]).all()
    assert flags[1::4][:9] == [X.TOO_LARGE << Q, X.BAD_BOND << Q, X.BAD_BOND << Q, X.BAD_BOND << Q, X.PSEUDO << Q, (X.PSEUDO | X.BAD_BOND) << Q,
                               X.QUERY_EMPTY, X.QUERY_TOO_LARGE, X.TRUNCATED << Q]
    assert flags[3::4][:9] == [X.TOO_LARGE, X.BAD_BOND, X.BAD_BOND, X.BAD_BOND, X.PSEUDO, X.PSEUDO | X.BAD_BOND, 0, 0, X.TRUNCATED]
    assert flags[36:38] == [X.TOO_LARGE << Q | X.BAD_BOND, X.PSEUDO << Q | X.PSEUDO]
    refused = (ref["match"]["flags"] & MATCH_REFUSED) != 0
    assert refused.sum() == 13 and not ref["match"]["n_matches"][refused].any() and (ref["map"][refused] == MATCH_NO_ATOM).all()
    # records beyond the tables passed, on either side: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        sizes = (cut.get("na", len(t.atoms)), cut.get("nb", len(t.bonds)), cut.get("nt", len(t.text)))
        for side in ("q_sizes", "t_sizes"):
            want = check(eng, t, t, [(0, 0), (9, 0), (0, 9), (0, 0)], **{side: sizes})
            beyond = X.TRUNCATED | X.BEYOND
            assert want["match"]["flags"].tolist() == ([0, beyond << Q, X.TRUNCATED, 0] if side == "q_sizes" else [0, X.TRUNCATED << Q, beyond, 0])
    mols, atoms, bonds, text = M.build_tables([ok, ok])
    atoms["sym0"][4] = 60000                                                       # a symbol beyond the text
    s = Tables(dev, arrays=(mols, atoms, bonds, text))
    assert check(eng, s, s, all_pairs(2, 2))["match"]["flags"].tolist() == [0, X.BEYOND, X.BEYOND << Q, X.BEYOND | X.BEYOND << Q]


def test_the_step_limit_on_a_complete_graph(eng, dev):
    """a chain of 8 carbons in K9: with S from the oracle (test_substructure_host.limit_pair: the cheapest root's steps) the pair is
    written at max_steps = S and limited at S - 1; between S and the dearest root's 29 steps some roots are broken off while one
    embedding is already counted, which is a certain yes and no limit; a query that is not there is limited one step below its S"""
    s = H.limit_pair()[2]
    q = Tables(dev, [H.chain([b"C"] * 8), H.chain([b"C"] * 7 + [b"N"])])
    t = Tables(dev, [H.complete(9), H.chain([b"C", b"O"])])
    for max_steps, n, steps, flags in ((0, 1, 29, 0), (29, 1, 29, 0), (28, 1, 29, 0), (s, 1, s + 1, 0), (s - 1, 0, s, MATCH_LIMIT)):
        ref = check(eng, q, t, [(0, 0), (0, 1)], max_steps=max_steps)
        assert (ref["match"]["n_matches"][0], ref["match"]["steps"][0], ref["match"]["flags"][0]) == (n, steps, flags), max_steps
        assert ref["match"]["flags"][1] == 0 and ref["match"]["steps"][1] == 2     # the pair behind a limited one is left alone
    most = int(X.pack(arrays(q), arrays(t), [(1, 0)], max_steps=X.MAX_STEPS, tables=H.TABLES)["match"]["steps"][0])
    assert X.DEFAULT_STEPS < most < X.MAX_STEPS                                    # 231689: every 7-chain of K9 is tried from every root
    for max_steps, flags, steps in ((most, 0, most), (most - 1, MATCH_LIMIT, most), (0, MATCH_LIMIT, X.DEFAULT_STEPS + 1)):
        ref = check(eng, q, t, [(1, 0)], max_steps=max_steps)
        assert ref["match"]["flags"].tolist() == [flags] and ref["match"]["steps"].tolist() == [steps] and ref["match"]["n_matches"].tolist() == [0]
    some = check(eng, q, t, [(0, 0)], max_matches=65535, max_steps=2000)           # every root broken off with embeddings in hand
    assert some["match"]["flags"].tolist() == [MATCH_LIMIT] and 9 < some["match"]["n_matches"][0] < 65535


# ---------------------------------------------------------------------------------------------------------------- the random batch
BATCH_SEED = 7


def piece_of(rng, molecule):
    """a random connected piece of a molecule — 2 to 10 atoms grown along its bonds from a random atom, with every bond among them
    —, renumbered by a random permutation; a molecule without atoms gives none"""
    syms, xy, bonds = molecule
    if not syms:
        return [], [], []
    around = [set() for _ in syms]
    for i, j, *_ in bonds:
        around[i].add(j)
        around[j].add(i)
    inside = [int(rng.integers(0, len(syms)))]
    want = int(rng.integers(2, 11))
    while len(inside) < want:
        rim = sorted({n for a in inside for n in around[a]} - set(inside))
        if not rim:
            break
        inside.append(rim[int(rng.integers(0, len(rim)))])
    perm = [int(p) for p in rng.permutation(len(inside))]
    new = {a: perm[k] for k, a in enumerate(inside)}
    out = [None] * len(inside)
    for a in inside:
        out[new[a]] = syms[a]
    return out, [(0, 0)] * len(inside), [(new[i], new[j], ty, rv) for i, j, ty, rv in bonds if i in new and j in new]


@functools.lru_cache(maxsize=None)
def random_batch(seed=BATCH_SEED):
    """64 random targets of 0 to 40 atoms of every symbol class (packed_tables.random_molecule; a pair drawn twice is dropped but in
    every eighth target, which may so be refused) and 64 queries: an even one is a piece of its own target, an odd one a piece of
    the target before it. (targets, queries)"""
    rng = np.random.default_rng(seed)
    targets = []
    for k in range(64):
        na = int(rng.integers(0, 41))
        syms, xy, bonds = random_molecule(rng, na, na // 2 + int(rng.integers(0, 3)))
        if k % 8 != 7:
            seen = set()
            bonds = [b for b in bonds if (b[0], b[1]) not in seen and not seen.add((b[0], b[1]))]
        targets.append((syms, xy, bonds))
    clean = [(m[0], m[1], list({(b[0], b[1]): b for b in m[2]}.values())) for m in targets]
    queries = [piece_of(rng, clean[k if k % 2 == 0 else k - 1]) for k in range(64)]
    return targets, queries


def test_64_random_pairs_and_two_runs_with_identical_bytes(eng, dev):
    targets, queries = random_batch()
    q, t = Tables(dev, queries), Tables(dev, targets)
    pairs = [(k, k) for k in range(64)]
    ref = check(eng, q, t, pairs)
    m = ref["match"]
    searched = (m["flags"] & MATCH_REFUSED) == 0
    # the condition on the seed, by the oracle: a third match, a third do not, none is limited at the default
    assert (searched & (m["n_matches"] > 0)).sum() >= 22 and (searched & (m["n_matches"] == 0)).sum() >= 22 and not (m["flags"] & MATCH_LIMIT).any()
    a, b = run(eng, q, t, pairs), run(eng, q, t, pairs)
    assert a.rc == b.rc == 0 and a.recs.tobytes() == b.recs.tobytes() and a.maps.tobytes() == b.maps.tobytes()
    all_of_them = check(eng, q, t, pairs, max_matches=65535)
    assert ((all_of_them["match"]["n_matches"] > 0) == (m["n_matches"] > 0)).all() and (all_of_them["map"] == ref["map"]).all()
    # without the oracle: a piece of a target embeds in it, and every map the device wrote satisfies the rule when checked directly
    graphs = [[H.graph(x) if not (f & X.SIDE_REFUSED) else None for x, f in zip(side, flags)]
              for side, flags in ((queries, m["flags"] >> Q), (targets, m["flags"]))]
    for k in range(64):
        if not searched[k]:
            continue
        images = a.maps[k][:len(queries[k][0])].tolist()
        assert k % 2 or a.recs["n_matches"][k] == 1, k
        assert (a.maps[k][len(queries[k][0]):] == MATCH_NO_ATOM).all()
        if a.recs["n_matches"][k]:
            assert X.is_embedding(graphs[0][k], graphs[1][k], images), (k, images)
        else:
            assert images == [MATCH_NO_ATOM] * len(images)


def test_engine_method_and_its_pairings(eng, dev):
    targets, queries = random_batch()
    q = dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables(queries)))
    t = dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables(targets)))
    arrays_of = lambda r: (r["mols"], r["atoms"], r["bonds"], r["text"])           # noqa: E731
    ref = X.pack(arrays_of(q), arrays_of(t), [(k, k) for k in range(64)], tables=H.TABLES)
    out = eng.substructure_match(q, t)                                             # equal counts: item by item
    assert out["match"].tobytes() == ref["match"].tobytes() and out["map"].dtype == np.uint16 and (out["map"] == ref["map"]).all()
    kept = eng.substructure_match(q, t, keep_device=True)
    assert kept["map"].is_cuda and (kept["map"].cpu().numpy().view(np.uint16) == ref["map"]).all()
    one = dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables(queries[:1])))
    spread = eng.substructure_match(one, t, max_matches=3)                         # one query: against every target
    want = X.pack(arrays_of(one), arrays_of(t), [(0, k) for k in range(64)], max_matches=3, tables=H.TABLES)
    assert spread["match"].tobytes() == want["match"].tobytes() and (spread["map"] == want["map"]).all()
    with pytest.raises(ValueError, match="one query with every target or item with item"):
        eng.substructure_match(dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables(queries[:2]))), t)
    listed = eng.substructure_match(q, t, pairs=[(3, 3), (2, 5), (99, 0)])
    assert listed["match"]["flags"][2] == X.BAD_PAIR and listed["match"][0] == ref["match"][3]


def test_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, H.small_molecules()[:4])
    pairs = [(0, 1), (1, 2)]

    def refused(expect, **over):
        assert_refused(run(eng, t, t, pairs, **over), "mnx_substructure_match: " + expect)

    for name in ("q_mols", "q_atoms", "q_bonds", "q_text", "t_mols", "t_atoms", "t_bonds", "t_text", "pair_list", "recs", "maps"):
        refused("null pointer", **{name: None})
    for name in ("n_q", "n_t"):
        for n in (0, -1, 65537):
            refused("1 <= nq <= 65536 and 1 <= nt <= 65536 required", **{name: n})
    for n in (0, -1, 1048577):
        refused("1 <= n_pairs <= 1048576 required", n_pairs=n)
    aligned = "mols, atoms and bonds of both sides must be 8-byte aligned, pairs and recs 4-byte, maps 2-byte"
    for side in "qt":
        for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2)):
            refused(aligned, **{side + "_" + name: _p(t.d[k], 4)})
    refused(aligned, pair_list=_p(t.d[0], 2))
    refused(aligned, recs=_p(t.d[0], 2))
    refused(aligned, maps=_p(t.d[0], 1))
    refused("max_matches must not exceed 65535", max_matches=65536)
    refused("max_steps must not exceed MNX_MATCH_MAX_STEPS (1048576)", max_steps=(1 << 20) + 1)
    assert run(eng, t, t, pairs, max_matches=65535, max_steps=1 << 20).rc == 0     # the largest values are admitted
    empty = Tables(dev, [mol([])])
    assert run(eng, empty, empty, [(0, 0)], q_atoms=None, q_bonds=None, q_text=None, t_atoms=None, t_bonds=None, t_text=None).rc == 0      # tables of 0 records

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        refused("call mnx_set_symbol_tables first", h=bare.h)
    finally:
        bare.close()


def test_the_place_behind_the_chain(eng):
    """read -> kekulize -> normalize -> match: aromatic benzene is not found in Kekule toluene as read, and is behind the two passes
    on both sides"""
    from molnextr_amd.model import smiles_substructure
    q, t = eng.smiles_read(["c1ccccc1"], keep_device=True), eng.smiles_read(["CC1=CC=CC=C1"], keep_device=True)
    assert not ((q["read"]["flags"] | t["read"]["flags"]) & READ_REFUSED).any()
    plain = eng.substructure_match(q, t)
    assert plain["match"]["flags"].tolist() == [0] and plain["match"]["n_matches"].tolist() == [0]
    last = [eng.normalize_pack(eng.kekulize_pack(x, keep_device=True), keep_device=True) for x in (q, t)]
    found = eng.substructure_match(*last, max_matches=100)
    assert found["match"]["n_matches"].tolist() == [12] and found["map"][0][:7].tolist() == [1, 2, 3, 4, 5, 6, MATCH_NO_ATOM]
    want = X.pack(*[(x["mols"], x["atoms"], x["bonds"], x["text"]) for x in last], [(0, 0)], max_matches=100, tables=H.TABLES)
    assert found["match"].tobytes() == want["match"].tobytes() and (found["map"] == want["map"]).all()
    items = smiles_substructure(eng, ["c1ccccc1"], ["CC1=CC=CC=C1", "C1CCCCC1", "C1CC"], kekulize=True, normalize=True)
    assert [x["matched"] for x in items] == [True, False, None] and items[0]["atoms"] == [1, 2, 3, 4, 5, 6] and items[1]["atoms"] is None
    assert smiles_substructure(eng, ["c1ccccc1"], ["CC1=CC=CC=C1"])[0]["matched"] is False


def test_the_known_limit_of_the_ranks_is_no_limit_here(eng, dev, monkeypatch):
    """the two drawings of C1CCCCC1.C1CC1.C1CC1 that test_canon_host pins get two canonical strings on the device too, yet they are
    the same graph; graph_isomorphic_scores counts such a pair where graph_match_scores does not"""
    from molnextr_amd import evaluate as E
    from molnextr_amd.model import _same_graph_tables, same_graph
    drawings = [CH.PINNED[k][0] for k in ("limit, six-ring drawn first", "limit, six-ring drawn last")]
    recs = [dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables([m]))) for m in drawings]
    strings = []
    for rec in recs:
        written, _, data = eng.smiles_pack(rec, canonical=True)[:3]
        assert not int(written["flags"][0]) & SMILES_REFUSED
        strings.append(bytes(data[:int(written["len"][0])]).decode())
    assert strings == ["C1CCCCC1.C1CC1.C1CC1", "C1CC1.C1CC1.C1CCCCC1"]
    assert _same_graph_tables(eng, recs[0], recs[1]) == ([True], [False])
    assert same_graph(eng, strings[:1], strings[1:]) == [True]
    assert same_graph(eng, ["C1CCCCC1.C1CC1.C1CC1", "CCO", "CCO", "C[13CH3]", "C1CC", "c1ccccc1"],
                      ["C1CCCC1.C1CCC1.C1CC1", "OCC", "CCN", "CC", "C1CC", "C1=CC=CC=C1"]) == [False, True, False, False, False, False]
    assert same_graph(eng, ["c1ccccc1"], ["C1=CC=CC=C1"], kekulize=True, normalize=True) == [True]
    with pytest.raises(ValueError, match="item with item"):
        same_graph(eng, ["C"], ["C", "C"])
    counted = []
    for drawing, gold in itertools.product(recs, strings):
        monkeypatch.setattr(E, "_both_sides", lambda engine, records, gold, chunk, d=drawing: iter([(d, engine.smiles_read(gold, keep_device=True))]))
        by_string = E.graph_match_scores(eng, np.zeros((1, 1), np.int32), [gold], kekulize=True)
        by_graph = E.graph_isomorphic_scores(eng, np.zeros((1, 1), np.int32), [gold])
        assert by_graph == {"graph_match_isomorphic": 1.0, "isomorphic_skipped": 0}
        counted.append((by_string["graph_match_device"], by_string["graph_match_kekulized"]))
    print("by string", counted)
    assert (0.0, 0.0) in counted                                                   # a correct prediction that the strings count as wrong


def test_end_to_end_predict_substructures_facade_and_evaluate(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: a query cut from each prediction's own first atoms is found, with a map onto atoms of equal symbols;
    predict_substructures against the calls made by hand; the facade's graph_substructure switched on and off; has_substructure on
    a caller's strings; evaluate's flag"""
    from molnextr_amd import evaluate as E
    from molnextr_amd.model import molnextr, predict_pipeline, predict_substructures
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4), keep_device=True)
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True)
    cuts = []
    for p in plain:
        k = min(4, len(p["chartok_coords"]["symbols"]))
        cuts.append(([s.encode() for s in p["chartok_coords"]["symbols"][:k]], [(0, 0)] * k, [b[:4] for b in p["bonds"] if b[0] < k and b[1] < k]))
    q_rec = dict(zip(("mols", "atoms", "bonds", "text"), M.build_tables(cuts)))
    own = eng.substructure_match(q_rec, rec)
    oracle = X.pack((q_rec["mols"], q_rec["atoms"], q_rec["bonds"], q_rec["text"]), (rec["mols"], rec["atoms"], rec["bonds"], rec["text"]),
                    [(k, k) for k in range(8)], tables=H.TABLES)
    assert own["match"].tobytes() == oracle["match"].tobytes() and (own["map"] == oracle["map"]).all()
    found = 0
    for p, cut, r, images in zip(plain, cuts, own["match"], own["map"]):
        if int(r["flags"]) & MATCH_REFUSED:
            continue
        assert r["n_matches"] == 1
        found += 1
        for a, s in enumerate(cut[0]):
            key = X.atom_key(s, H.TABLES)
            assert key == X.WILD or X.atom_key(p["chartok_coords"]["symbols"][images[a]].encode(), H.TABLES)[:3] == key[:3]
    print("own cuts found in", found, "of 8 predictions")
    assert found >= 1

    queries = ["C", "CC", "c1ccccc1", "*", "C1CC"]
    got = predict_substructures(eng, imgs, queries, ref_batch_size=4)
    q_read = eng.smiles_read(queries, keep_device=True)
    by_hand = eng.substructure_match(q_read, rec, pairs=[(k, t) for t in range(8) for k in range(len(queries))])
    seen = set()
    for t, (p, g) in enumerate(zip(plain, got)):
        assert "substructure" not in p and set(g) == set(p) | {"substructure"} and len(g["substructure"]) == len(queries)
        for k, item in enumerate(g["substructure"]):
            r, images = by_hand["match"][t * len(queries) + k], by_hand["map"][t * len(queries) + k]
            want = None if int(r["flags"]) & MATCH_REFUSED else bool(r["n_matches"])
            atoms = images[:int(q_read["mols"]["n_atoms"][k])].tolist() if want else None
            assert item == {"matched": want, "atoms": atoms, "coords": [p["chartok_coords"]["coords"][a] for a in atoms] if want else None}
            seen.add(want)
        assert g["substructure"][4]["matched"] is None                             # an unreadable query is the empty molecule
    assert True in seen
    both = predict_substructures(eng, imgs[:2], ["C"], ref_batch_size=2, fingerprint=True, smiles=True)
    assert all({"substructure", "fingerprint", "graph_smiles"} <= set(x) for x in both)
    with pytest.raises(ValueError, match="predict_substructures needs packed=True: the search runs in the packed tables"):
        predict_substructures(eng, imgs[:1], ["C"], packed=False)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True)
    try:
        assert m.graph_substructure is None
        assert all("substructure" not in o for o in m.predict_images(pages[:2], batch_size=2))     # the default: no such key
        m.graph_substructure = ["C", "*", "CN"]                                    # an attribute: the constructor's list is closed
        out = m.predict_images(pages, batch_size=4)
        want = predict_substructures(m.engine, m._transform(pages), ["C", "*", "CN"], m.tokenizer, ref_batch_size=4, smiles=True, stereo=False)
        assert all("substructure" in o for o in out) and [o["substructure"] for o in out] == [p["substructure"] for p in want]
        assert m.has_substructure(["CCO", "CCN", "C1CC", "OC"], "CO") == [True, False, None, True]
        assert m.has_substructure(["Cc1ccccc1"], "C1=CC=CC=C1", kekulize=True, normalize=True) == [True]
        m.graph_substructure = None
        assert all("substructure" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()
    args = E.build_parser().parse_args(["--test_file", "t.csv", "--load_path", "synthetic", "--graph_match", "--graph_isomorphic"])
    assert args.graph_isomorphic and not args.graph_tanimoto
