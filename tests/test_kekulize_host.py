"""CPU: the oracle of mnx_kekulize_pack (tests/kekulize_ref.py) against outcomes written out by a person, the validity check
check_kekule() on every case and against mutants, the round trip normalize(kekulize(normalize(K))) on generated molecules, the
conditions the cases must cover (a backtrack, a pruned pairing, two systems, 999 atoms), the rule that sets
MNX_KEKULE_DEFAULT_STEPS, the step limit, and the search of molnextr_amd/csrc/kekule_search.h itself, compiled into a stand-alone
program with the host compiler's address and undefined-behaviour sanitizers and compared with the oracle on every case. A Kekule
structure is a perfect matching, which check_kekule() verifies without a toolkit; the choice among several is the project's own
order (include/molnextr_hip.h): it is not RDKit's Kekulize and no toolkit has checked these strings."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import expand_ref as X
import kekulize_ref as Q
import molfile_ref as M
import normalize_ref as N
import test_normalize_host as H

TABLES = H.TABLES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS_PROFILE = os.path.join(ROOT, "profiles", "kekulize_steps.json")

TRIANGULENE = "c12c3cccc1cc1c4c2c2c(c3)cccc2cc4ccc1"                  # 22 needy atoms, 12 of one colour and 10 of the other
# string -> the writer's string behind the oracle; the writer walks by atom index, so the atoms stand in the input's order
HAND = {
    "c1ccccc1": "C1=CC=CC=C1",
    "c1cc[nH]c1": "C=1C=CNC1",                                        # pyrrole: atom 0 takes atom 1 first, which strands atom 2
    "O=c1cccc[nH]1": "O=C1C=CC=CN1",
    "c1ccc2ccccc2c1": "C1=CC=C2C=CC=CC2=C1",
    "c1ccccc1-c1ccccc1": "C1=CC=CC=C1C1=CC=CC=C1",
    "[cH-]1cccc1": "[CH-]1C=CC=C1",
    "c1ccc2cccc2cc1": "C1=CC=C2C=CC=C2C=C1",                          # azulene
    "c1cnc[nH]1": "C1=CN=CN1",                                        # imidazole
    "c1ccc2c(c1)cc[nH]2": "C1=CC=C2C(=C1)C=CN2",                      # indole
    "c1ncc2[nH]cnc2n1": "C1=NC=C2NC=NC2=N1",                          # purine
    "[O-][n+]1ccccc1": "[O-][N+]1=CC=CC=C1",                          # pyridine N-oxide
    "s1cccc1": "S1C=CC=C1",
    "o1cccc1": "O1C=CC=C1",
    "[cH+]1cccccc1": "[CH+]1C=CC=CC=C1",                              # tropylium
    "c1ccc2ncccc2c1": "C1=CC=C2N=CC=CC2=C1",                          # quinoline
    "c12c3c4c5c6c1c1ccc2ccc3ccc4ccc5ccc6cc1": "C12=C3C4=C5C6=C1C1=CC=C2C=CC3=CC=C4C=CC5=CC=C6C=C1",      # coronene
    "Cn1cccc1": "CN1C=CC=C1",
    "c1ccccc1c1ccccc1": "C1=CC=CC=C1C1=CC=CC=C1",                     # the link is a type-4 record: one system of twelve
    "[13cH]1ccccc1": "[13CH]1=CC=CC=C1",
    "c1cc[n+](C)cc1": "C1=CC=[N+](C)C=C1",
    "[o+]1ccccc1": "[O+]1=CC=CC=C1",                                  # pyrylium
    "c1ccc2C=CC=Cc2c1": "C1=CC=C2C=CC=CC2=C1",                        # half-aromatic fused pair
    "c1cccc1-c1ccccc1": "c1cccc1C1=CC=CC=C1",                         # a failing and a succeeding system
    TRIANGULENE + ".c1ccccc1": TRIANGULENE + ".C1=CC=CC=C1",
    # atom orders in which the first choices are wrong: the search backtracks, and undoes stranding pairings at once
    "c1c2c3c(ccc4c3c(ccc4)c1)ccc2": "C1=C2C=3C(C=CC=4C3C(C=CC4)=C1)=CC=C2",                                        # pyrene
    "c1cc2ccc3c4c5c6c(ccc7c6c(c24)c1cc7)ccc5cc3": "C1=CC2=CC=C3C4=C5C=6C(C=CC=7C6C(=C24)C1=CC7)=CC=C5C=C3",      # coronene
    "c1c2c(cc3ccccc3c2)ccc1": "C1=C2C(C=C3C=CC=CC3=C2)=CC=C1",        # anthracene
}
LEFT = ["c1cccc1", TRIANGULENE, "c1ccccc1:C", "Cc", "c1ccccc1:[Ph]"]  # no matching (odd; colours); blocked by a type-4 record to no aromatic atom
UNTOUCHED = ["C1=CC=CC=C1", "CCO", "[Ph]C", "*C", "C:C", "O=C1C=CC(=O)C=C1", ""]


def kekulized(strings, **more):
    return Q.pack(*H.tables_of(strings), tables=TABLES, **more)


def checked(inp, out):
    """check_kekule finds nothing to object to"""
    bad = Q.check_kekule(inp, out, TABLES)
    assert not bad, bad[:5]


def four(rec):
    return {k: rec[k] for k in ("mols", "atoms", "bonds", "text")}


def same_tables(a, b, flags=True):
    """all four tables equal: records field by field, the text byte for byte. flags=False: but for mols['flags'], which say what
    a call changed and not what the molecule is"""
    mols = all(a["mols"][k].tolist() == b["mols"][k].tolist() for k in a["mols"].dtype.names if flags or k != "flags")
    return mols and all(H.same_records(a[k], b[k]) for k in ("atoms", "bonds")) and bytes(a["text"]) == bytes(b["text"])


@pytest.mark.parametrize("string", sorted(HAND))
def test_rows_that_are_kekulised(string):
    t = H.tables_of([string])
    out = Q.pack(*t, tables=TABLES)
    assert H.written(out) == [HAND[string]]
    flags = int(out["mols"]["flags"][0])
    assert flags & Q.KEKULIZED and not flags & Q.REFUSED
    assert bool(flags & Q.KEKULE_LEFT) == any(N.lower_case(s) for s in X.molecules(four(out))[0][0])
    checked(H.as_rec(t), out)
    # pruning removes failing branches only: a search without it finds the same matching
    plain = Q.pack(*t, tables=TABLES, prune=False, max_steps=1 << 30)
    assert same_tables(plain, out) and plain["atom_notes"].tolist() == out["atom_notes"].tolist()
    # a second call changes no table
    again = Q.pack(out["mols"], out["atoms"], out["bonds"], out["text"], tables=TABLES)
    assert X.molecules(four(again)) == X.molecules(four(out)) and H.same_records(again["bonds"], out["bonds"]) and again["text"] == out["text"]
    assert not (int(again["mols"]["flags"][0]) & Q.KEKULIZED)


@pytest.mark.parametrize("string", LEFT + UNTOUCHED)
def test_rows_that_stay_as_they_are(string):
    t = H.tables_of([string])
    out = Q.pack(*t, tables=TABLES)
    assert H.written(out) == H.written(H.as_rec(t))
    assert H.same_molecules(out, t) and H.same_records(out["bonds"], t[2])
    assert int(out["mols"]["flags"][0]) == (Q.KEKULE_LEFT if string in LEFT else 0)
    checked(H.as_rec(t), out)


def test_notes_against_a_hand_list():
    rows = {"c1cc[nH]c1": [17, 17, 17, 17, 17], "Cc1ccccc1": [64, 16, 17, 17, 17, 17, 17], "c1cccc1": [33] * 5, "O=c1cccc[nH]1": [64, 16, 17, 17, 17, 17, 17],
            "c1ccccc1:C": [33, 33, 33, 33, 33, 32, 64], "[Ph]C": [64, 64], "[cH-]1cccc1": [17] * 5, "c": [35], "[nH]": [17], "n": [16]}
    out = kekulized(list(rows))
    at = 0
    for string, want in rows.items():
        assert out["atom_notes"][at:at + len(want)].tolist() == want, string
        at += len(want)
    assert at == len(out["atom_notes"])
    assert H.written(out)[-3:] == ["c", "[NH]", "[N]"]            # systems of one: a needy atom alone fails; [nH] and n need nothing, H stays


def test_one_failing_and_one_succeeding_system_are_handled_on_their_own():
    out = kekulized([TRIANGULENE + ".c1ccccc1", "c1cccc1-c1ccccc1"])
    assert [[x["result"] for x in s] for s in out["systems"]] == [[Q.NO_MATCHING, Q.OK], [Q.NO_MATCHING, Q.OK]]
    assert out["mols"]["flags"].tolist() == [Q.KEKULIZED | Q.KEKULE_LEFT] * 2
    notes = out["atom_notes"].tolist()
    assert sorted(notes[:22]) == [32] * 10 + [33] * 12 and notes[22:] == [17] * 6 + [33] * 4 + [32] + [16] + [17] * 5
    assert len(out["systems"][0][0]["needy"]) == 22 and out["systems"][0][0]["steps"] > 0


def test_what_blocks_a_system():
    ring = [(k, (k + 1) % 6, 4, 4) for k in range(6)]
    syms = [b"c"] * 6
    blocked = [(syms + [b"C"], ring + [(0, 6, 4, 4)]),                               # a type-4 record to an upper-case atom
               (syms + [b"c"] * 2, ring + [(0, 6, 4, 4), (0, 7, 4, 4)]),             # four type-4 records at atom 0
               (syms + [b"C"], ring + [(0, 6, 1, 1), (6, 0, 1, 1)]),                 # two records to the same atom
               (syms, ring + [(2, 2, 1, 1)]),                                        # a record to itself
               (syms + [b"C"], ring + [(0, 6, 0, 0)]), (syms + [b"C"], ring + [(3, 6, 7, 7)])]      # a type outside 1..6
    free = [(syms + [b"C"], ring + [(0, 6, 5, 6)]), (syms + [b"c"], ring + [(0, 6, 1, 1)]), (syms + [b"C"] * 2, ring + [(0, 6, 1, 1), (3, 7, 1, 1)])]
    t = M.build_tables([(s, [(0, 0)] * len(s), sorted((min(i, j), max(i, j), ty, rv) for i, j, ty, rv in b)) for s, b in blocked + free])
    out = Q.pack(*t, tables=TABLES)
    assert [s[0]["result"] for s in out["systems"]] == [Q.BLOCKED] * 6 + [Q.OK] * 3
    assert out["mols"]["flags"].tolist() == [Q.KEKULE_LEFT] * 6 + [Q.KEKULIZED, Q.KEKULIZED | Q.KEKULE_LEFT, Q.KEKULIZED]
    assert X.molecules(four(out))[:6] == X.molecules(H.as_rec(t))[:6]
    assert [tuple(x.tolist()[:4]) for x in out["bonds"][-8:]] == [(0, 1, 2, 2), (0, 5, 1, 1), (0, 6, 1, 1), (1, 2, 1, 1), (2, 3, 2, 2), (3, 4, 1, 1),
                                                                  (3, 7, 1, 1), (4, 5, 2, 2)]
    wedge = int(out["mols"]["bond0"][6])                       # a wedge at a ring atom is no type-4 record and keeps its fields
    assert (0, 6, 5, 6) in [tuple(x.tolist()[:4]) for x in out["bonds"][wedge:wedge + 7]]
    checked(H.as_rec(t), out)


# ---------------------------------------------------------------------------------------------------------------- mutants
def test_check_kekule_rejects_mutants():
    t = H.tables_of(["Cc1ccc2ccccc2c1", "c1cc[nH]c1"])
    out = Q.pack(*t, tables=TABLES)
    checked(H.as_rec(t), out)

    def mutant(change):
        m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        change(m)
        return Q.check_kekule(H.as_rec(t), m, TABLES)

    def move_a_double_bond(m):                                 # C2=C3 becomes single and C3-C4 double: atom 2 loses its double bond
        ty = m["bonds"]["type"].tolist()
        k = ty.index(2)
        k1 = next(x for x in range(len(ty)) if ty[x] == 1 and x != k and {int(m["bonds"]["i"][x]), int(m["bonds"]["j"][x])} & {int(m["bonds"]["j"][k])}
                  and int(m["bonds"]["i"][x]) != 0)
        for x, v in ((k, 1), (k1, 2)):
            m["bonds"]["type"][x] = m["bonds"]["rev"][x] = v

    def respell(atom, new):
        def change(m):
            a0, t0 = int(m["mols"]["atom0"][1]), int(m["mols"]["text0"][1])
            syms = X.molecules(four(m))[1][0]
            syms[atom] = new
            text = bytes(m["text"])[:t0] + b"".join(syms)
            m["text"] = text
            off = 0
            for k, s in enumerate(syms):
                m["atoms"]["sym0"][a0 + k], m["atoms"]["sym_len"][a0 + k] = off, len(s)
                off += len(s)
            m["mols"]["smiles_len"][1] = off
        return change

    assert any("double bonds" in x for x in mutant(move_a_double_bond))
    assert any("H 1" in x for x in mutant(respell(3, b"[NH2]")))                # one H changed
    assert any("H 1" in x for x in mutant(respell(0, b"[CH2]")))
    assert any("lower case" in x for x in mutant(respell(1, b"c")))            # one atom left lower-case
    assert mutant(lambda m: m["bonds"]["type"].__setitem__(0, 2))              # a bond outside the systems changed
    assert mutant(lambda m: m["atom_notes"].__setitem__(2, 16))                # the noted H


# --------------------------------------------------------------------------------------------------- generated molecules
def aromatic_acene(rings, extra=0):
    """a chain of `rings` fused six-rings of c atoms on type-4 records (top row 0 .. 2k, bottom row 2k + 1 .. 4k + 1, a rung at
    every even position) and `extra` methanes without a bond: 4k + 2 + extra atoms on 5k + 1 bonds"""
    w = 2 * rings + 1
    bonds = [(r * w + k, r * w + k + 1, 4, 4) for r in (0, 1) for k in range(w - 1)] + [(k, w + k, 4, 4) for k in range(0, w, 2)]
    return [b"c"] * (2 * w) + [b"C"] * extra, [(0, 0)] * (2 * w + extra), sorted(bonds)


@functools.lru_cache(maxsize=None)
def generated():
    """700 molecules of the Kekule generator of test_normalize_host, of which those are kept that the normalize oracle makes
    aromatic and that hold no lower-case symbol to begin with — a stray lower-case atom in a Kekule drawing is a system of one,
    which kekulize writes in upper case where it needs nothing ([nH] -> [NH]) and normalize, which copies lower-case atoms, cannot
    bring back. Returns the kept molecules in normalised (aromatic) form, as (symbols, coordinate bins, bonds) each."""
    mols = H.kekule_batch(np.random.default_rng(21), 700)
    assert len(mols) >= 600
    normal = N.pack(*M.build_tables(mols), tables=TABLES)
    keep = [b for b, m in enumerate(mols) if int(normal["mols"]["flags"][b]) & N.AROMATIZED and not any(N.lower_case(s) for s in m[0])]
    after = X.molecules(four(normal))
    return [after[b] for b in keep]


def generated_tables():
    """the kept molecules in normalised (aromatic) form as tables"""
    return M.build_tables([(syms, xy, [b[:4] for b in bonds]) for syms, xy, bonds in generated()])


def test_round_trip_on_generated_molecules():
    t = generated_tables()
    assert len(t[0]) > 80
    once = N.pack(*t, tables=TABLES)                           # normalize_ref(K): a fixed point of normalize already
    assert X.molecules(four(once)) == X.molecules(H.as_rec(t))
    kek = Q.pack(once["mols"], once["atoms"], once["bonds"], once["text"], tables=TABLES)
    checked(four(once), kek)
    flags = kek["mols"]["flags"]                              # a few stay aromatic: normalize takes [NH]= in a six-ring, which needs no double bond here
    assert all(int(f) & (Q.KEKULIZED | Q.KEKULE_LEFT) for f in flags) and (flags & Q.KEKULIZED).astype(bool).sum() > 0.9 * len(flags)
    assert (kek["atom_notes"] & Q.NOTE_KEKULIZED).astype(bool).sum() > 500
    back = N.pack(kek["mols"], kek["atoms"], kek["bonds"], kek["text"], tables=TABLES)
    assert same_tables(back, once, flags=False)               # `once` ran on normal tables and changed nothing, `back` made rings aromatic again
    assert [bool(int(f) & N.AROMATIZED) for f in back["mols"]["flags"]] == [bool(int(f) & Q.KEKULIZED) for f in flags]
    again = Q.pack(kek["mols"], kek["atoms"], kek["bonds"], kek["text"], tables=TABLES)
    for k in ("atoms", "bonds"):
        assert H.same_records(again[k], kek[k])
    assert again["text"] == kek["text"] and not (again["mols"]["flags"] & Q.KEKULIZED).any()
    assert sum(len(s) > 1 for s in kek["systems"]) >= 5       # molecules of two systems and more


# ------------------------------------------------------------------------------------------- coverage, the default, the limit
@functools.lru_cache(maxsize=None)
def all_cases():
    """every case of this file as (tables, the oracle's result): the hand rows in one batch, the generated set, the 999 atoms"""
    hand = H.tables_of(sorted(HAND) + LEFT + UNTOUCHED)
    big = M.build_tables([aromatic_acene(199, extra=201)])
    return [(t, Q.pack(*t, tables=TABLES)) for t in (hand, generated_tables(), big)]


def succeeding_systems():
    return [s for _, out in all_cases() for systems in out["systems"] for s in systems if s["result"] == Q.OK]


def test_the_cases_cover_what_they_must():
    systems = succeeding_systems()
    assert any(s["steps"] > len(s["needy"]) // 2 for s in systems)                  # a backtrack
    assert any(s["pruned"] > 0 for s in systems)                                    # a pruned pairing
    assert any(len(m) >= 2 for _, out in all_cases() for m in out["systems"])       # two systems
    t, big = all_cases()[2]
    assert int(t[0]["n_atoms"][0]) == 999 and int(t[0]["n_bonds"][0]) == 996
    assert int(big["mols"]["flags"][0]) == Q.KEKULIZED and len(big["systems"][0][0]["needy"]) == 798
    assert big["systems"][0][0]["steps"] < Q.DEFAULT_STEPS
    checked(H.as_rec(t), big)


def largest_step_count():
    return max(s["steps"] for s in succeeding_systems())


def write_steps_profile():
    """profiles/kekulize_steps.json from the cases of this file (run by hand when the cases change)"""
    with open(STEPS_PROFILE, "w") as f:
        json.dump({"largest_step_count_of_a_succeeding_system": largest_step_count(), "MNX_KEKULE_DEFAULT_STEPS": Q.DEFAULT_STEPS,
                   "rule": "the default is at least 8 times the largest step count"}, f, indent=1)
        f.write("\n")


def test_the_default_step_limit_follows_its_rule():
    """MNX_KEKULE_DEFAULT_STEPS is at least 8 times the largest step count of any succeeding case, the hand polycyclics and the
    999 atoms included; the figure is on record in profiles/kekulize_steps.json, and header, engine and oracle hold one value"""
    largest = largest_step_count()
    with open(STEPS_PROFILE) as f:
        recorded = json.load(f)
    assert recorded["largest_step_count_of_a_succeeding_system"] == largest and recorded["MNX_KEKULE_DEFAULT_STEPS"] == Q.DEFAULT_STEPS
    assert Q.DEFAULT_STEPS >= 8 * largest
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        assert "#define MNX_KEKULE_DEFAULT_STEPS %du\n" % Q.DEFAULT_STEPS in f.read()
    from molnextr_amd import engine
    assert engine.KEKULE_DEFAULT_STEPS == Q.DEFAULT_STEPS
    assert (engine.MOL_KEKULIZED, engine.MOL_KEKULE_LEFT, engine.MOL_KEKULIZE_REFUSED) == (Q.KEKULIZED, Q.KEKULE_LEFT, Q.REFUSED)
    assert (engine.NOTE_KEKULIZED, engine.NOTE_KEKULE_LEFT, engine.NOTE_KEKULE_LIMIT, engine.NOTE_COPIED) == (16, 32, 128, 64)


def test_the_step_limit():
    t = H.tables_of(["c1ccc2ccccc2c1"])
    cut = Q.pack(*t, tables=TABLES, max_steps=2)
    assert H.written(cut) == ["c1ccc2ccccc2c1"] and cut["atom_notes"].tolist() == [161] * 3 + [160] + [161] * 4 + [160, 161]
    assert int(cut["mols"]["flags"][0]) == Q.KEKULE_LEFT and cut["systems"][0][0]["result"] == Q.LIMIT and cut["systems"][0][0]["steps"] == 3
    assert H.same_molecules(cut, t) and H.same_records(cut["bonds"], t[2])
    assert H.written(Q.pack(*t, tables=TABLES, max_steps=5)) == H.written(Q.pack(*t, tables=TABLES)) == ["C1=CC=C2C=CC=CC2=C1"]
    assert Q.pack(*t, tables=TABLES, max_steps=4)["systems"][0][0]["result"] == Q.LIMIT


def test_refusals_and_the_truncated_bit():
    ok = ([b"c", b"[CH3]"], [(0, 0), (1, 1)], [(0, 1, 1, 1)])
    big = ([b"C"] * 1000, [(0, 0)] * 1000, [])
    mols, atoms, bonds, text = M.build_tables([ok, big, ok, ([b"C", b"C"], [(0, 0)] * 2, [(0, 2, 1, 1)]), ([], [], [])])
    mols["flags"][0] = mols["flags"][1] = 1 | 2 | 4 | 16 | 32
    mols["overall_score"] = [0.5, 0.25, 0.125, 1.0, 2.0]
    out = Q.pack(mols, atoms, bonds, text, tables=TABLES)
    assert out["mols"]["flags"].tolist() == [1 | Q.KEKULE_LEFT, 1 | Q.REFUSED, Q.KEKULE_LEFT, Q.REFUSED, 0]
    assert out["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 0] and out["mols"]["atom0"].tolist() == [0, 2, 2, 4, 4]
    assert out["mols"]["overall_score"].tolist() == [0.5, 0.25, 0.125, 1.0, 2.0] and out["text"] == b"c[CH3]c[CH3]"
    cut = Q.pack(mols, atoms, bonds, text, tables=TABLES, n_text_bytes=len(text) - 1)
    assert cut["mols"]["flags"].tolist()[2:] == [Q.KEKULE_LEFT, Q.REFUSED, Q.REFUSED]


# ------------------------------------------------------------------------------------ the search core under the sanitizers
def search_input(cases, max_steps):
    """what tools/kekule_host.cpp reads: every molecule of every case, the systems that are searched named by their lowest atom"""
    lines, expect = [], []
    for t, out in cases:
        for m, systems in zip(t[0], out["systems"]):
            n = int(m["n_atoms"])
            system, adj = [1023] * n, {}
            for s in systems:
                if s["result"] != Q.BLOCKED:
                    for a in s["needy"]:
                        system[a] = s["root"]
                    adj.update(s["adj"])
            lines.append("%d %d" % (n, max_steps))
            lines += ["%d %d %s" % (system[a], len(adj.get(a, ())), " ".join(map(str, adj.get(a, ())))) for a in range(n)]
            expect.append((n, [s for s in systems if s["result"] != Q.BLOCKED and s["needy"]]))
    return "%d\n%s\n" % (len(expect), "\n".join(lines)), expect


def test_the_search_header_under_the_sanitizers(tmp_path):
    """tools/kekule_host.cpp — a main() around csrc/kekule_search.h — built with -fsanitize=address,undefined and run once, as a
    plain executable, over every case of this file at the default limit and at a limit of 4: its partners, results and step counts
    are the oracle's, and the sanitizers report nothing (a report ends the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "kekule_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "kekule_host.cpp"), "-o", exe], check=True)
    code = {Q.OK: 0, Q.NO_MATCHING: 1, Q.LIMIT: 2}
    for max_steps in (Q.DEFAULT_STEPS, 4):
        cases = all_cases() if max_steps == Q.DEFAULT_STEPS else [(t, Q.pack(*t, tables=TABLES, max_steps=max_steps)) for t, _ in all_cases()[:2]]
        text, expect = search_input(cases, max_steps)
        run = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        got = run.stdout.split("\n")
        at = 0
        for n, systems in expect:
            for s in systems:
                assert got[at].split() == [str(s["root"]), str(code[s["result"]]), str(s["steps"])], (at, s)
                at += 1
            partner = {}
            for s in systems:
                if s["result"] == Q.OK:
                    partner.update(pairs_of(s))
            assert [int(x) for x in got[at].split()] == [partner.get(a, 1023) for a in range(n)], at
            at += 1
        assert got[at:] == [""]
    assert subprocess.run([exe], input="1\n2 9\n0 1 5\n0 0\n", capture_output=True, text=True).returncode == 2     # a neighbour that is no atom


def pairs_of(system):
    """the matching of a system that succeeded, from the oracle's search on the system alone"""
    result, pairs, steps, _ = Q.first_matching(system["needy"], system["adj"], 1 << 30)
    assert result == Q.OK and steps == system["steps"]
    return pairs
