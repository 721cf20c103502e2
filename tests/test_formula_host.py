"""CPU: the oracle of mnx_formula_pack (tests/formula_ref.py) — invariants of every structure it finds on the corpus
(tests/golden/formula_corpus.json), equivalence with the hand-written fragment library through expansion, normalisation and the
canonical writer, the valence order, the reference's search (tests/golden/formula_reference.json, written by
tools/gen_formula_golden.py) where its output is a molecule, the refusals, and the tokenizer and search of
molnextr_amd/csrc/formula_search.h themselves, compiled into a stand-alone program with the host compiler's address and
undefined-behaviour sanitizers and compared with the oracle on the corpus. THE RULE IS THE PROJECT'S OWN (include/molnextr_hip.h):
no toolkit has parsed these structures.

The reference fixture is a gate only on one class of cases and a record everywhere else, because the reference's raw search output
is not chemistry: 'N(CH3)2' comes out with a triple bond ('H3' is one token of valence 1 there), 'SH' ends with 4 bonds left over,
'NCH3' tokenises as 'NC', 'H3' and fails."""
import json
import os
import re
import shutil
import subprocess

import pytest

import expand_ref as X
import formula_ref as F
import normalize_ref as N
import test_normalize_host as H

TABLES = H.TABLES
FRAGS = X.library(tables=TABLES)
GROUPS = F.group_names(FRAGS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "formula_corpus.json")) as _f:
    CORPUS = json.load(_f)["labels"]
with open(os.path.join(ROOT, "tests", "golden", "formula_reference.json")) as _f:
    REFERENCE = json.load(_f)["cases"]

# label(s) = table name(s): one canonical string on the carrier
PAIRS = [(("CH2CH3", "C2H5", "H3CH2C"), ("Et",)), (("CH(CH3)2",), ("iPr",)), (("C(CH3)3", "(H3C)3C"), ("tBu",)), (("N(CH3)2",), ("NMe2",)),
         (("OCH2CH3",), ("OEt",)), (("COOCH3",), ("CO2Me",)), (("COOC2H5",), ("CO2Et",)), (("SO2CH3",), ("SO2Me",)),
         (("Si(CH3)3",), ("SiMe3", "TMS")), (("NHCOCH3",), ("NHAc",)), (("OCOCH3",), ("OAc",)), (("CH2Ph",), ("Bn",)), (("OCH2Ph",), ("OBn",))]
CARRIER = "c1ccccc1-[%s]"          # the bond written out: the reader takes an unwritten one next to a lower-case name (iPr, tBu) as aromatic


def formula(strings, **kw):
    return F.pack(*H.tables_of(strings), frags=FRAGS, tables=TABLES, **kw)


def chain(strings):
    """formula -> expand -> normalize -> the canonical strings"""
    f = formula(strings)
    x = X.pack(f["mols"], f["atoms"], f["bonds"], f["text"], FRAGS, TABLES)
    return H.canonical(N.pack(x["mols"], x["atoms"], x["bonds"], x["text"], tables=TABLES))


def formula_counts(label):
    """(heavy atoms and group tokens in reading order, hydrogens) of a label, by a recursive descent of its own"""
    toks = re.findall(r"\(|\)|\d+|[A-Z][a-z]*|[a-z]+[A-Z][a-z]*", label)
    assert "".join(toks) == label, label

    def seq(k):
        heavy, h = [], 0
        while k < len(toks) and toks[k] != ")":
            if toks[k] == "(":
                inner, ih, k = seq(k + 1)
                k += 1
            else:
                run = toks[k]
                if run in F.VALENCES:
                    inner, ih = ([], 1) if run == "H" else ([run], 0)
                    k += 1
                else:                                   # a run that is no element: the longest group name at this position
                    rest = "".join(toks[k:])
                    name = next(rest[:n] for n in range(min(16, len(rest)), 0, -1) if rest[:n].encode() in GROUPS)
                    used = 0
                    while len("".join(toks[k:k + used])) < len(name):
                        used += 1
                    assert "".join(toks[k:k + used]) == name, (label, name)
                    inner, ih = [name], 0
                    k += used
            count = 1
            if k < len(toks) and toks[k].isdigit():
                count = int(toks[k])
                k += 1
            heavy += inner * count
            h += ih * count
        return heavy, h, k

    heavy, h, k = seq(0)
    assert k == len(toks)
    return heavy, h


EXPANDED = [(label, start) for label in CORPUS for start in (1, 2, 3) if F.search(label.encode(), start, GROUPS)[0] == F.OK]


def test_the_corpus_is_large_enough_and_mostly_expands():
    assert len(CORPUS) >= 120 and len(set(CORPUS)) == len(CORPUS)
    assert len({label for label, _ in EXPANDED}) >= 100


@pytest.mark.parametrize("label,start", EXPANDED)
def test_invariants_of_a_structure(label, start):
    status, atoms, steps = F.search(label.encode(), start, GROUPS)
    heavy, hydrogens = formula_counts(label)
    names = [a[0][1] if a[0][0] == "el" else a[0][1].decode() for a in atoms]
    # the atoms are the formula's: in reading order, or — direction -1 — in the order of the label read from the right. C with a
    # count in front of an element is written out chain-wise, which keeps the elements' multiset, so compare sorted where it occurs
    assert sorted(names) == sorted(heavy)
    if not re.search(r"C\d", label):
        assert names in (heavy, heavy[::-1]) or "(" in label
    assert sum(a[3] for a in atoms) == hydrogens
    assert atoms[0][1] is None and all(0 <= a[1] < k for k, a in enumerate(atoms) if k), "a tree: every atom hangs on an earlier one"
    assert all(1 <= a[2] <= 3 for a in atoms[1:])
    for k, (what, parent, order, h) in enumerate(atoms):
        total = (start if k == 0 else order) + sum(a[2] for a in atoms[k + 1:] if a[1] == k) + h
        assert total in (F.VALENCES[what[1]] if what[0] == "el" else (1,)), (label, k, total)
    # atom 0's surplus over its own bonds and hydrogens is the label's bond-order sum: the same statement for k = 0, said apart
    assert 1 <= steps <= F.DEFAULT_STEPS and status == F.OK


# The two left sides that the abbreviation table itself holds (with a fragment): they never reach the search on the tables —
# mnx_expand_pack replaces them — and are compared through the chain all the same; the search is asked for them directly below.
ALSO_TABLE_NAMES = {"C2H5": "CH2CH3", "OCOCH3": "OC(O)CH3"}


def test_the_left_side_of_each_pair_is_no_table_name():
    for labels, names in PAIRS:
        for label in labels:
            if label in ALSO_TABLE_NAMES:
                assert TABLES.get(label.encode()) == 2 and label.encode() in FRAGS, label
            else:
                assert label.encode() not in TABLES, label
    for label, other in ALSO_TABLE_NAMES.items():          # the search itself gives them the structure of their other spelling
        a, b = F.search(label.encode(), 1, GROUPS), F.search(other.encode(), 1, GROUPS)
        assert a[0] == b[0] == F.OK and a[1] == b[1], (label, a, b)


@pytest.mark.parametrize("labels,names", PAIRS)
def test_a_formula_equals_its_table_name(labels, names):
    strings = [CARRIER % s for s in labels + names]
    out = chain(strings)
    assert len(set(out)) == 1 and "*" not in out[0] and "[" not in out[0].replace("[Si]", ""), dict(zip(strings, out))
    f = formula(strings[:len(labels)])
    assert [int(fl) for fl in f["mols"]["flags"]] == [0 if label in ALSO_TABLE_NAMES else F.FORMULA_EXPANDED for label in labels]


def test_the_spelling_is_the_tables():
    f = formula([CARRIER % "CH2CH3", CARRIER % "Si(CH3)3"])
    syms = [s[6:] for s, _, _ in X.molecules(f)]
    assert syms == [[b"C", b"C"], [b"[Si]", b"C", b"C", b"C"]]


def test_valence_order():
    sulfur = {}
    for label in ("SH", "SCH3", "SO2NH2"):
        status, atoms, _ = F.search(label.encode(), 1, GROUPS)
        assert status == F.OK and atoms[0][0] == ("el", "S")
        sulfur[label] = 1 + sum(a[2] for a in atoms[1:] if a[1] == 0) + atoms[0][3]
    assert sulfur == {"SH": 2, "SCH3": 2, "SO2NH2": 6}
    assert F.search(b"PO3H2", 1, GROUPS)[0] == F.NO_STRUCTURE          # the chain rule gives the second O the last bonds


def _reference_graph(case):
    """the reference's heavy-atom graph: (elements, sorted bonds). The reference writes a hydrogen as a token without atoms, so its
    string holds heavy atoms only"""
    assert "H" not in case["elements"]
    return case["elements"], sorted((min(a, b), max(a, b), o) for a, b, o in case["bonds"])


def _is_a_molecule(elements, bonds, start):
    """whether the reference's graph is one the invariants of this file admit: a tree on atom 0, no order above 3, every atom's
    bond-order sum (with the label's bonds on atom 0) within a table valence"""
    if len(bonds) != len(elements) - 1 or any(not 1 <= o <= 3 for _, _, o in bonds) or any(not a < b for a, b, _ in bonds):
        return False
    if sorted(b for _, b, _ in bonds) != list(range(1, len(elements))):
        return False
    for k, el in enumerate(elements):
        total = (start if k == 0 else 0) + sum(o for a, b, o in bonds if k in (a, b))
        if total > max(F.VALENCES[el]):
            return False
    return True


# (label, start bonds) where the reference "succeeds with 0 bonds left" on a graph that is no molecule: a first atom that is a
# leaf of nothing (an O with 3 start bonds; a branch with no atom to hang on), or a branch whose double bond is not taken from the
# atom it hangs on (a carbon with 5 bonds, a phosphorus with 6)
MENDED = [("OCHF2", 3), ("O(CH2)2OH", 3), ("OCH2CH2OH", 3), ("(CH2)2OH", 2), ("(CH2)2OH", 3), ("C(O)OH", 2), ("C(O)NH2", 2), ("C(O)Cl", 2),
          ("P(O)(OH)2", 2)]


def test_against_the_reference_where_it_gives_a_molecule():
    """The cases of the fixture where every token is an element of our valence table, 'H', a count or a parenthesis, the reference
    succeeded, and the reference ended with 0 bonds left. There our element list and bond list equal the reference's exactly —
    where the reference's graph is a molecule at all. With 2 or 3 start bonds the reference also "succeeds with 0 bonds left" on
    graphs that break the invariants this file demands of every structure (test_invariants_of_a_structure), and that the rule
    repairs by its own words: a first atom hung as a leaf onto nothing ('OCHF2' with 3 bonds: an O apart from the rest), a branch
    whose raised bond order is not taken from the atom it hangs on ('C(O)OH' with 2 bonds: a carbon with 5 bonds). No structure
    can equal such a graph and keep the invariants, so on those cases — each named in MENDED, with the reason — the demand is that
    the oracle finds NO structure. At least 15 distinct labels must be in the exact-equality part."""
    ours = set(F.VALENCES)
    equal, mended = set(), []
    for c in REFERENCE:
        if "".join(c["tokens"]) != c["label"] or not all(t in ours or t.isdigit() or t in "()" for t in c["tokens"]):
            continue
        if not c["success"] or c["bonds_left"] != 0:
            continue
        assert c["elements"] is not None, c
        elements, bonds = _reference_graph(c)
        status, atoms, _ = F.search(c["label"].encode(), c["start"], GROUPS)
        if not _is_a_molecule(elements, bonds, c["start"]):
            assert status == F.NO_STRUCTURE, (c["label"], c["start"], c["raw"])
            mended.append((c["label"], c["start"]))
            continue
        assert status == F.OK, (c["label"], c["start"], c["raw"])
        assert [a[0][1] for a in atoms] == elements, (c["label"], c["start"], c["raw"])
        assert sorted((a[1], k, a[2]) for k, a in enumerate(atoms) if k) == bonds, (c["label"], c["start"], c["raw"])
        equal.add(c["label"])
    assert len(equal) >= 15, sorted(equal)
    assert sorted(mended) == sorted(MENDED), mended                # with one start bond every qualifying case is exact


REFUSED = ["CH2CH2", "C6H5", "C6H11", "CH=CH2", "C#CH", "CD3", "CH2NH3+", "CO2-", "PO3H2", "C" * 21, "C33H68", "((((CH2))))", "CH2()", "2OCH3",
           "C100", "Xy2"]


@pytest.mark.parametrize("label", REFUSED)
def test_a_label_that_stays(label):
    string = "C[%s]" % label + ("C" if label == "CH2CH2" else "")           # the two-ended label between two atoms
    f = formula([string])
    if len(label) > 20:                         # beyond the reference's bound: no candidate, so nothing is flagged
        assert int(f["mols"]["flags"][0]) == 0 and f["left"] == [[]] and F.search(label.encode(), 1, GROUPS)[0] == F.NO_STRUCTURE
    else:
        assert int(f["mols"]["flags"][0]) == F.FORMULA_LEFT and f["found"] == [{}] and f["left"] == [[1]]
    assert X.molecules(f) == X.molecules(H.as_rec(H.tables_of([string])))


def test_too_long_too_large_aromatic_bond_table_name_and_step_limit():
    assert F.search(b"CH2" * 7, 1, GROUPS)[0] == F.NO_STRUCTURE and F.search(b"CH2" * 6 + b"H", 1, GROUPS)[0] == F.OK      # 21 and 19 bytes
    assert F.search(b"CH2(CH2)19CH3", 1, GROUPS)[0] == F.OK and F.search(b"C32H65", 1, GROUPS)[0] == F.OK
    assert F.search(b"C33H67", 1, GROUPS)[0] == F.NO_STRUCTURE                                                          # 33 atoms
    # a label on a class-4 bond stays: the molecule's own tables, with the label's bond made aromatic
    t = H.tables_of(["C[CH2CH3]"])
    assert int(F.pack(*t, frags=FRAGS, tables=TABLES)["mols"]["flags"][0]) == F.FORMULA_EXPANDED
    t[2]["type"][0] = t[2]["rev"][0] = 4
    assert int(F.pack(*t, frags=FRAGS, tables=TABLES)["mols"]["flags"][0]) == F.FORMULA_LEFT
    # a table name is no candidate, with or without a fragment; neither is an R-group
    f = formula(["C[Et]", "C[R1]", "C[OMe]"])
    assert [int(x) for x in f["mols"]["flags"]] == [0, 0, 0]
    assert X.molecules(f) == X.molecules(H.as_rec(H.tables_of(["C[Et]", "C[R1]", "C[OMe]"])))
    # the step limit: CH2CH3 takes 4 placements
    assert F.search(b"CH2CH3", 1, GROUPS)[2] == 4
    for limit, flags in ((3, F.FORMULA_LEFT | F.FORMULA_LIMIT), (4, F.FORMULA_EXPANDED), (0, F.FORMULA_EXPANDED)):
        assert int(formula(["C[CH2CH3]"], max_steps=limit)["mols"]["flags"][0]) == flags
    assert F.search(b"CH2CH3", 1, GROUPS, 3) == (F.LIMIT, None, 4)


def test_tables_of_a_small_molecule_by_hand():
    """two labels in one molecule: indices, rows and text written out by a person"""
    f = formula(["[NHCH3]C[CH2Cl]"])
    (syms, xy, bonds), = X.molecules(f)
    assert syms == [b"N", b"C", b"C", b"C", b"Cl"]                      # the labels' first atoms in place, the others appended in label order
    assert [b[:3] for b in bonds] == [(0, 1, 1), (0, 3, 1), (1, 2, 1), (2, 4, 1)]
    assert f["origin"].tolist() == [0, 1, 2, 0, 2] and f["totals"] == (5, 4, 6)
    assert int(f["mols"]["flags"][0]) == F.FORMULA_EXPANDED and f["text"] == b"NCCCCl"


def test_refused_molecule_and_the_truncated_bit():
    t = H.tables_of(["C[CH2CH3]C", "C[CH2CH3]"])
    t[2][:2] = t[2][:2][::-1].copy()                                              # unsorted bond records
    t[0]["flags"][1] |= 1
    f = F.pack(*t, frags=FRAGS, tables=TABLES)
    assert [int(x) for x in f["mols"]["flags"]] == [F.FORMULA_REFUSED, 1 | F.FORMULA_EXPANDED]
    assert int(f["mols"]["n_atoms"][0]) == 0 and int(f["mols"]["n_atoms"][1]) == 3


# ------------------------------------------------------------------- the tokenizer and the search under the sanitizers
def host_names():
    """the names a group token can be, as tools/formula_host.cpp reads them: a name that begins with no letter matches nowhere"""
    return sorted(n for n in GROUPS if n[:1].isalpha())


def host_line(status, atoms, steps):
    line = "%d %d %d" % (status, steps, len(atoms) if atoms else 0)
    for what, parent, order, h in atoms or []:
        line += " %s %d %d %d" % (what[1] if what[0] == "el" else "[" + what[1].decode() + "]", parent or 0, order, h)
    return line


def test_the_search_header_under_the_sanitizers(tmp_path):
    """tools/formula_host.cpp — a main() around csrc/formula_search.h — built with -fsanitize=address,undefined and run once, as a
    plain executable, over the corpus and the refused labels with 0 to 3 start bonds, at the default limit and at a limit of 3:
    status, steps and every atom are the oracle's, and the sanitizers report nothing (a report ends the program with a status
    other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "formula_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "formula_host.cpp"), "-o", exe], check=True)
    names = host_names()
    assert all(len(n) <= 16 and not re.search(rb"\s", n) for n in names)
    cases = [(label, start, limit) for label in CORPUS + REFUSED + ["((CH3)2CH)2N", "C9H19(C9H19)9", "(CH2)99", "C2(H)99"]
             for start in (0, 1, 2, 3) for limit in (0, 3)]
    text = "%d\n%s%d\n%s" % (len(names), "".join("%s 1\n" % n.decode() for n in names), len(cases),
                             "".join("%s %d %d\n" % c for c in cases))
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(cases)
    for (label, start, limit), line in zip(cases, got):
        assert line == host_line(*F.search(label.encode(), start, GROUPS, limit)), (label, start, limit)
    assert subprocess.run([exe], input="2\nPh 1\nEt 1\n0\n", capture_output=True, text=True).returncode == 2       # names out of order
