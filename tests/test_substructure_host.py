"""CPU: the rule of mnx_substructure_match (include/molnextr_hip.h, "Substructure search") as the oracle of
tests/substructure_ref.py states it — against a brute force that knows neither an order nor a step on every pair of a set of
hand-made graphs, the cases the rule names pinned by hand, the names the engine loads against the header, and the search of the
kernel itself (csrc/match_search.h) under the host compiler's sanitizers, as a program of its own."""
import functools
import itertools
import os
import re
import shutil
import subprocess

import molfile_ref as M
import smiles_read_ref as R
import substructure_ref as X
from molnextr_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = M.name_tables()


def molecule(smiles: str, any_bonds=()):
    """(symbols, xy, bonds) of one string by the reader's oracle; the bonds named in any_bonds get type 0, the class ANY"""
    r = R.pack([smiles.encode()])
    assert not int(r["recs"]["flags"][0]) & (R.SYNTAX | R.TOO_LARGE | R.BEYOND), smiles
    text = r["text"]
    syms = [text[int(a["sym0"]):int(a["sym0"]) + int(a["sym_len"])] for a in r["atoms"]]
    bonds = [(int(b["i"]), int(b["j"]), 0 if k in any_bonds else int(b["type"]), 0 if k in any_bonds else int(b["type"])) for k, b in enumerate(r["bonds"])]
    return syms, [(3 * k % 64, 5 * k % 64) for k in range(len(syms))], bonds


def chain(symbols, ty=1):
    return list(symbols), [(0, 0)] * len(symbols), [(k, k + 1, ty, ty) for k in range(len(symbols) - 1)]


def complete(n):
    return [b"C"] * n, [(0, 0)] * n, [(i, j, 1, 1) for i, j in itertools.combinations(range(n), 2)]


def graph(mol):
    return X.graph(mol[0], mol[2], TABLES)


def g(smiles, any_bonds=()):
    return graph(molecule(smiles, any_bonds))


# about 40 graphs of at most 7 atoms: chains, rings, branches, two components, hetero atoms, charges, isotopes, aromatic and Kekule
# spellings, wildcards, R-groups, every bond class
SMALL = ["C", "N", "CC", "C=C", "C#C", "CO", "C=O", "CCC", "C1CC1", "CCO", "OCC", "C(C)C", "CC(C)C", "CCCC", "C1CCC1", "C1CC1C", "C.C", "C.O",
         "CC.C", "c1ccccc1", "C1=CC=CC=C1", "Cc1ccccc1", "c1ccncc1", "C1CCCCC1", "CC(=O)O", "CC(=O)[O-]", "[NH4+]", "C[N+](C)C", "[13C]C", "[13CH3]O",
         "*", "*C", "[1*]", "*.*", "[R1]C", "C*C", "CC(C)(C)C", "C1CC1C1CC1", "N#CC=C", "C1=CC1", "c1cc[nH]c1", "CCCCCCC"]


@functools.lru_cache(maxsize=None)
def small_molecules():
    out = [molecule(s) for s in SMALL]
    out.append(molecule("CCC", any_bonds=(0,)))            # C~CC
    out.append(molecule("C1CC1", any_bonds=(0, 1, 2)))     # a ring of three ANY bonds
    assert all(1 <= len(m[0]) <= 7 for m in out)
    return out


def first_along_the_order(q, found):
    order, _ = X.query_order(q[1])
    return list(min(found, key=lambda images: [images[a] for a in order])) if found else None


def test_the_oracle_against_the_brute_force_on_every_pair():
    """n_matches at max_matches = 65535 is the number of injective maps that satisfy the rule, and the map is the one whose image
    sequence along the order is the smallest"""
    graphs = [graph(m) for m in small_molecules()]
    matched = 0
    for q, t in itertools.product(graphs, graphs):
        found = X.embeddings_brute(q, t) if len(q[0]) <= len(t[0]) else []
        n, steps, limited, first = X.match(q, t, max_matches=65535, max_steps=X.MAX_STEPS)
        assert n == len(found) and not limited and first == first_along_the_order(q, found)
        one = X.match(q, t)                                # at the defaults: the same map, one embedding counted
        assert one[0] == min(n, 1) and one[3] == first and not one[2] and one[1] <= steps
        assert first is None or X.is_embedding(q, t, first)
        matched += bool(found)
    assert len(graphs) ** 2 // 8 < matched < len(graphs) ** 2 // 2


def count(q, t, **kw):
    return X.match(q, t, max_matches=65535, **kw)[0]


def test_pinned_cases():
    assert count(g("c1ccccc1"), g("Cc1ccccc1")) == 12                      # six rotations, two directions
    assert X.match(g("c1ccccc1"), g("Cc1ccccc1"))[3] == [1, 2, 3, 4, 5, 6]
    assert count(g("C1=CC=CC=C1"), g("c1ccccc1")) == 0 == count(g("c1ccccc1"), g("C1=CC=CC=C1"))
    assert count(g("CCC"), g("C1CC1")) == 6 and count(g("C1CC1"), g("CCC")) == 0      # not induced
    assert count(g("C.C"), g("CC")) == 2 and count(g("C.C"), g("C")) == 0
    assert count(g("*"), g("CCO")) == 3 and count(g("[1*]"), g("CCO")) == 3 and count(g("*"), g("*")) == 1
    assert count(g("C"), g("*")) == 0 and count(g("C"), g("[R1]")) == 0 and count(g("[R1]"), g("C")) == 1
    assert count(g("[13C]"), g("C")) == 0 and count(g("C"), g("[13C]")) == 1 and count(g("[13C]"), g("[13CH3]O")) == 1
    assert count(g("[12C]"), g("[13C]")) == 0
    assert count(g("[NH4+]"), g("N")) == 0 and count(g("[NH4+]"), g("[N+]")) == 1 and count(g("N"), g("[NH2]C")) == 1     # H counts are not compared
    any_q = graph(molecule("CC", any_bonds=(0,)))
    assert count(any_q, g("C=C")) == 2 and count(any_q, g("C#C")) == 2 and count(any_q, any_q) == 2
    assert count(g("CC"), any_q) == 0                                       # a target bond of class ANY is matched by ANY alone
    assert count(g("CC"), graph(chain([b"C", b"C"], ty=5))) == 2 == count(g("CC"), graph(chain([b"C", b"C"], ty=6)))      # a wedge is a single bond


def test_the_order_and_the_steps_by_hand():
    """C(C)C: the order is 0, 1, 2 with both later atoms children of position 0. Against propane from root 1 (the middle atom): the
    root 1 step, position 1 tries 0 (accepted) and position 2 tries 0 (an image) and 2 (accepted): the first embedding after 4
    steps; all embeddings of that root take 1 + 2 + 2 + 2 = 7"""
    q, t = g("C(C)C"), g("CCC")
    assert X.query_order(q[1]) == ([0, 1, 2], [None, 0, 0])
    assert X.query_order(g("CC.C(C)C")[1]) == ([0, 1, 2, 3, 4], [None, 0, None, 2, 2])
    assert X.search_root(q, t, 1, 1, 100) == ([[1, 0, 2]], 4)
    assert X.search_root(q, t, 1, 10, 100) == ([[1, 0, 2], [1, 2, 0]], 7)
    assert X.search_root(q, t, 0, 10, 100) == ([], 3)                       # root; 1 accepted; 1 again, an image
    assert X.match(q, t, 10, 100) == (2, 7, False, [1, 0, 2])
    assert X.match(q, t, 10, 6) == (2, 7, True, [1, 0, 2])                  # broken off at the 7th step, both embeddings found: a lower bound
    assert X.match(q, t, 10, 5) == (1, 6, True, [1, 0, 2])
    assert X.match(q, t, 1, 4) == (1, 4, False, [1, 0, 2])
    assert X.match(q, t, 1, 3) == (0, 4, True, None)


@functools.lru_cache(maxsize=None)
def limit_pair():
    """a chain of 8 carbons in the complete graph on 9: (query, target, S) — S the fewest steps at which one embedding is found and
    nothing is limited: the cheapest root's. Every root has an embedding, so below the dearest root's steps some search is broken
    off while n_matches is already max_matches = 1, which is no limit by the rule; below S no root finds one."""
    q, t = graph(chain([b"C"] * 8)), graph(complete(9))
    return q, t, min(X.search_root(q, t, r, 1, X.MAX_STEPS)[1] for r in range(9))


def test_the_step_limit_pair():
    q, t, s = limit_pair()
    # no backtracking: from root 0 position k examines its k - 1 earlier images, then accepts: 1 + (1 + .. + 7); from root 8 one fewer from position 2 on
    assert X.match(q, t, 1, X.MAX_STEPS) == (1, 29, False, list(range(8))) and s == 23 == X.search_root(q, t, 8, 1, X.MAX_STEPS)[1]
    assert X.match(q, t, 1, 28) == (1, 29, False, [2, 0, 1, 3, 4, 5, 6, 7])       # roots 0 and 1 broken off at their 29th step, root 2 has one after 28: a certain yes
    assert X.match(q, t, 1, s) == (1, s + 1, False, [7, 0, 1, 2, 3, 4, 5, 6]) and X.match(q, t, 1, s - 1) == (0, s, True, None)
    full = X.match(q, t, 65535, X.MAX_STEPS)
    assert full[0] == 65535 and not full[2]                # 9!/1! = 362880 embeddings, the count capped: nothing is limited
    q7, k7 = graph(chain([b"C"] * 7 + [b"N"])), graph(complete(9))
    n, most, limited, first = X.match(q7, k7, 1, X.MAX_STEPS)
    assert n == 0 and first is None and not limited and most > 1000
    assert X.match(q7, k7, 1, most) == (0, most, False, None) and X.match(q7, k7, 1, most - 1) == (0, most, True, None)


def test_pack_admission_and_refusals():
    ok, big = chain([b"C", b"N"]), chain([b"C"] * 65)
    ring129 = ([b"C"] * 64, [(0, 0)] * 64, [(i, j, 1, 1) for i, j in itertools.combinations(range(64), 2)][:129])
    sides = M.build_tables([ok, chain([]), big, ring129, chain([b"C"] * 1000), ([b"C", b"N"], [(0, 0)] * 2, [(0, 1, 1, 1), (1, 0, 1, 1)]),
                            chain([b"C", b"Ph"]), chain([b"C"] * 64)])
    pairs = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 6), (0, 4), (0, 5), (8, 0), (0, 8), (7, 7), (0, 1), (6, 0), (0, 6)]
    out = X.pack(sides, sides, pairs, tables=TABLES)
    Q = X.QUERY_SHIFT
    assert out["match"]["flags"].tolist() == [0, X.QUERY_EMPTY, X.QUERY_TOO_LARGE, X.QUERY_TOO_LARGE, X.TOO_LARGE << Q, X.BAD_BOND << Q,
                                              X.PSEUDO | X.PSEUDO << Q, X.TOO_LARGE, X.BAD_BOND, X.BAD_PAIR, X.BAD_PAIR, 0, 0, X.PSEUDO << Q, X.PSEUDO]
    assert out["match"]["n_matches"].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0]
    assert out["map"][0].tolist() == [0, 1] + [X.NO_ATOM] * 62 and (out["map"][[1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 14]] == X.NO_ATOM).all()
    assert out["map"][11].tolist() == list(range(64)) and out["match"]["steps"][12] == 0
    assert X.pack(sides, sides, [(7, 7)], max_matches=9, tables=TABLES)["match"]["n_matches"].tolist() == [2]
    cut = X.pack(sides, sides, [(0, 7), (7, 0)], tables=TABLES, t_sizes=(len(sides[1]) - 1, len(sides[2]), len(sides[3])))
    assert cut["match"]["flags"].tolist() == [X.BEYOND, 0]
    assert engine.MATCH_REFUSED == X.REFUSED and engine.MATCH_DTYPE.itemsize == 16
    assert engine.MATCH_DTYPE.names == ("flags", "n_matches", "steps", "reserved")


def test_the_names_the_engine_loads_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "molnextr_hip.h")).read()
    assert "mnx_substructure_match" in engine.SYMBOLS and re.search(r"\bint mnx_substructure_match\s*\(", hdr)
    assert re.search(r"#define MNX_ABI_VERSION 7\b", hdr) and engine.ABI_VERSION == 7
    for name, text, value in (("MNX_MATCH_QUERY_TOO_LARGE", "32u", engine.MATCH_QUERY_TOO_LARGE), ("MNX_MATCH_QUERY_EMPTY", "64u", engine.MATCH_QUERY_EMPTY),
                              ("MNX_MATCH_QUERY_SHIFT", "8", engine.MATCH_QUERY_SHIFT), ("MNX_MATCH_LIMIT", "65536u", engine.MATCH_LIMIT),
                              ("MNX_MATCH_BAD_PAIR", "131072u", engine.MATCH_BAD_PAIR), ("MNX_MATCH_MAX_QUERY", "64u", engine.MATCH_MAX_QUERY),
                              ("MNX_MATCH_MAX_QUERY_BONDS", "128u", engine.MATCH_MAX_QUERY_BONDS),
                              ("MNX_MATCH_DEFAULT_STEPS", "%du" % X.DEFAULT_STEPS, engine.MATCH_DEFAULT_STEPS),
                              ("MNX_MATCH_MAX_STEPS", "(1u << 20)", engine.MATCH_MAX_STEPS)):
        assert "#define %s %s\n" % (name, text) in hdr, name
        assert value == int(eval(text.replace("u", ""))), name
    assert (X.QUERY_TOO_LARGE, X.QUERY_EMPTY, X.LIMIT, X.BAD_PAIR, X.QUERY_SHIFT, X.MAX_QUERY, X.MAX_QUERY_BONDS, X.DEFAULT_STEPS, X.MAX_STEPS, X.NO_ATOM) == \
        (engine.MATCH_QUERY_TOO_LARGE, engine.MATCH_QUERY_EMPTY, engine.MATCH_LIMIT, engine.MATCH_BAD_PAIR, engine.MATCH_QUERY_SHIFT,
         engine.MATCH_MAX_QUERY, engine.MATCH_MAX_QUERY_BONDS, engine.MATCH_DEFAULT_STEPS, engine.MATCH_MAX_STEPS, engine.MATCH_NO_ATOM)
    assert "NOT RDKit's HasSubstructMatch" in hdr and "not SMARTS" in hdr


# ------------------------------------------------------------------------------------ the search under the sanitizers
def word_of(key) -> int:
    """the match word of csrc/match_search.h from the oracle's key"""
    if key == X.WILD:
        return 1 << 31
    el, aromatic, charge, isotope = key
    return (ord(el[0]) - 65) | ((ord(el[1]) - 96) if len(el) > 1 else 0) << 5 | int(aromatic) << 10 | (charge + 15) << 11 | isotope << 16


def search_input(cases):
    """what tools/match_host.cpp reads, from (query, target, max_matches, max_steps) with both limits resolved"""
    lines = [str(len(cases))]
    for q, t, max_matches, max_steps in cases:
        nb = [sum(len(x) for x in side[1]) // 2 for side in (q, t)]
        lines.append("%d %d %d %d %d %d" % (len(q[0]), nb[0], len(t[0]), nb[1], max_matches, max_steps))
        for keys, around in (q, t):
            lines.append(" ".join(str(word_of(k)) for k in keys))
            lines += ["%d %d %d" % (i, j, c + 1) for i in range(len(keys)) for j, c in sorted(around[i].items()) if i < j]
    return "\n".join(lines) + "\n"


def test_the_search_header_under_the_sanitizers(tmp_path):
    """tools/match_host.cpp — a main() around csrc/match_search.h, its stack exactly the query's atoms — built with
    -fsanitize=address,undefined and run once, as a plain executable, over every pair of the small graphs at 65535 embeddings and a
    part of them at the defaults and at three steps, a 64-atom chain in a 999-atom chain, the step-limit pair at its limit and one
    below, and an empty query: counts, steps, limits and maps are the oracle's, and the sanitizers report nothing (a report ends
    the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "match_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "match_host.cpp"), "-o", exe], check=True)
    graphs = [graph(m) for m in small_molecules()]
    cases = [(q, t, 65535, X.MAX_STEPS) for q, t in itertools.product(graphs, graphs)]
    cases += [(q, t, 1, X.DEFAULT_STEPS) for q, t in itertools.product(graphs[::3], graphs[::2])]
    cases += [(q, t, 2, 3) for q, t in itertools.product(graphs[::4], graphs[::3])]
    q7, k9 = graph(chain([b"C"] * 7 + [b"N"])), graph(complete(9))
    s = X.match(q7, k9, 1, X.MAX_STEPS)[1]
    long_q, long_t = graph(chain([b"C"] * 64)), graph(chain([b"C", b"C", b"N"] * 333))
    cases += [(q7, k9, 1, s), (q7, k9, 1, s - 1), (limit_pair()[0], k9, 1, limit_pair()[2]), (limit_pair()[0], k9, 1, limit_pair()[2] - 1), (long_q, long_t, 1, X.DEFAULT_STEPS),
              (long_q, graph(chain([b"C"] * 999)), 3, X.DEFAULT_STEPS), (graph(chain([])), graphs[3], 1, 1)]
    run = subprocess.run([exe], input=search_input(cases), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(cases) + 1 and got[-1] == ""
    limited = 0
    for line, (q, t, max_matches, max_steps) in zip(got, cases):
        if not q[0]:
            assert line == "0 0 0"
            continue
        n, steps, lim, first = X.match(q, t, max_matches, max_steps)
        limited += lim
        want = [n, steps, int(lim)] + (first if first is not None else [X.NO_ATOM] * len(q[0]))
        assert [int(x) for x in line.split()] == want, (len(q[0]), len(t[0]), max_matches, max_steps)
    assert limited >= 10
    # no atom; a word of 6; a pair twice; 65 query atoms; no limits at all; cut short
    for text in ("1\n2 1 2 0 1 9\n1 2\n0 2 1\n1 2\n", "1\n2 1 2 0 1 9\n1 2\n0 1 6\n1 2\n", "1\n2 2 2 0 1 9\n1 2\n0 1 1\n1 0 1\n1 2\n",
                 "1\n65 0 1 0 1 9\n" + "1 " * 65 + "\n1\n", "1\n1 0 1 0 0 0\n1\n1\n", "1\n2 1 2 0 1 9\n1 2\n0 1 1\n1\n", ""):
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2, text
