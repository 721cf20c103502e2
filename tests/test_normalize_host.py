"""CPU: the oracle of mnx_normalize_pack (tests/normalize_ref.py) against outcomes written out by a person. Each row goes string ->
smiles_read_ref (the reader's oracle) -> normalize_ref -> smiles_ref's writer, and the string that comes out is compared with one
worked out by hand from the rule of include/molnextr_hip.h. The rule is the project's own: no toolkit has checked these strings.
Then the fixed point on aromatic input, idempotence on generated molecules, the H counts of `atom_notes`, and the generator of
Kekule-form molecules that the GPU test shares."""
import numpy as np
import pytest

import canon_ref as K
import expand_ref as X
import ez_ref as E
import molfile_ref as M
import normalize_ref as N
import smiles_read_ref as R
import smiles_ref as S
import stereo_ref as T
import test_expand_host as H

TABLES = M.name_tables()

# string -> the writer's string behind the oracle; the writer walks by atom index, so the atoms stand in the input's order
AROMATIC = {
    "C1=CC=CC=C1": "c1ccccc1",
    "CC1=C(C)C=CC=C1": "Cc1c(C)cccc1",                       # o-xylene, the double bond between the methyl carbons
    "CC=1C(C)=CC=CC1": "Cc1c(C)cccc1",                       # and the other Kekule form, the same atom order
    "C1=CC=C2C=CC=CC2=C1": "c1ccc2ccccc2c1",                 # naphthalene, the fusion bond single
    "C=1C=CC=2C=CC=CC2C1": "c1ccc2ccccc2c1",                 # and double
    "N1C=CC=C1": "[nH]1cccc1",                               # pyrrole: c1cc[nH]c1 with the walk beginning at the nitrogen
    "C1=CNC=C1": "c1c[nH]cc1",
    "CN1C=CC=C1": "Cn1cccc1",
    "C1=CC=NC=C1": "c1ccncc1",
    "O1C=CC=C1": "o1cccc1",
    "S1C=CC=C1": "s1cccc1",
    "C1=CN=CN1": "c1cnc[nH]1",
    "C1=CC=C2C(=C1)C=CN2": "c1ccc2c(c1)cc[nH]2",             # indole
    "O=C1C=CC=CN1": "O=c1cccc[nH]1",
    "[CH-]1C=CC=C1": "[cH-]1cccc1",
    "C1=CC=CC=C1C1=CC=CC=C1": "c1ccccc1-c1ccccc1",
    "C=CC1=CC=CC=C1": "C=Cc1ccccc1",
    "[13CH]1=CC=CC=C1": "[13cH]1ccccc1",
    "C1=CC=[N+](C)C=C1": "c1cc[n+](C)cc1",
}
# a string of the issue that names the same molecule with another first atom: equal as canonical strings
SAME_GRAPH = {"N1C=CC=C1": "c1cc[nH]c1", "C1=CNC=C1": "c1cc[nH]c1", "C=1C=CC=2C=CC=CC2C1": "c1ccc2ccccc2c1"}
NOT_AROMATIC = ["C1=CC=CCC1", "C1=CC=CC1", "O=C1C=CC(=O)C=C1", "C=C1C=CC=C1", "C1=COC=CC1", "C1=CC=CC=CC=C1", "[CH+]1C=CC=CC=C1",
                "C1=CC=CC=CC1", "C1=CC1", "C1=CC=C1", "C1#CC=CC=C1", "N1C=CN=NC=C1"]
BRACKETS = {"C[CH](C)F": "CC(C)F", "[CH3][CH2][OH]": "CCO", "[CH2]C": "[CH2]C", "[13CH4]": "[13CH4]", "[NH4+]": "[NH4+]", "[C]": "[C]",
            "CC(=O)[O-]": "CC(=O)[O-]", "[C:12](C)(C)(C)C": "C(C)(C)(C)C", "[NH2]C": "NC", "[N](C)(C)(C)=O": "N(C)(C)(C)=O",
            "[SH]C": "SC", "[S](C)(C)=O": "S(C)(C)=O", "[Cl]C": "ClC", "[Na+].[Cl-]": "[Na+].[Cl-]", "[BH2]C": "BC", "[Si](C)(C)(C)C": "[Si](C)(C)(C)C"}


def tables_of(strings):
    r = R.pack([s.encode() for s in strings])
    assert not (r["recs"]["flags"] & (R.SYNTAX | R.TOO_LARGE | R.BEYOND)).any(), r["recs"]["flags"]
    return r["mols"], r["atoms"], r["bonds"], r["text"]


def normalized(strings):
    return N.pack(*tables_of(strings), tables=TABLES)


def written(rec):
    """the writer's strings of packed tables"""
    w = S.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tables=TABLES)
    return [w["out"][int(r["text0"]):int(r["text0"]) + int(r["len"])].decode() for r in w["recs"]]


def canonical(rec):
    w = K.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], 0, TABLES)
    return [w["out"][int(r["text0"]):int(r["text0"]) + int(r["len"])].decode() for r in w["recs"]]


def as_rec(t):
    return dict(zip(("mols", "atoms", "bonds", "text"), t))


def same_records(a, b):
    """two record arrays field by field (the padding bytes of a host array are not set)"""
    return len(a) == len(b) and all(a[name].tolist() == b[name].tolist() for name in a.dtype.names)


def same_molecules(out, t):
    """symbols, bins and bonds of every molecule are those of the tables t (a reader's text holds more than the symbols, so the
    text and the atoms' sym0 are not compared)"""
    return X.molecules(out) == X.molecules(as_rec(t))


@pytest.mark.parametrize("string", sorted(AROMATIC))
def test_rows_that_become_aromatic(string):
    out = normalized([string])
    assert written(out) == [AROMATIC[string]]
    assert int(out["mols"]["flags"][0]) & N.AROMATIZED and not int(out["mols"]["flags"][0]) & N.REFUSED
    assert out["mols"]["n_atoms"][0] == tables_of([string])[0]["n_atoms"][0]
    # the aromatic spelling is a fixed point and names the same graph
    assert canonical(out) == canonical(as_rec(tables_of([AROMATIC[string]]))) == canonical(normalized([AROMATIC[string]]))
    if string in SAME_GRAPH:
        assert canonical(out) == canonical(as_rec(tables_of([SAME_GRAPH[string]])))
    assert canonical(as_rec(tables_of([string]))) != canonical(out)             # what the pass is for


def test_both_kekule_forms_give_one_string():
    assert written(normalized(["CC1=C(C)C=CC=C1", "CC=1C(C)=CC=CC1"])) == ["Cc1c(C)cccc1"] * 2
    a, b, c = written(normalized(["C1=CC=C2C=CC=CC2=C1", "C=1C=CC=2C=CC=CC2C1", "c1ccc2ccccc2c1"]))
    assert a == b == c == "c1ccc2ccccc2c1"
    out = normalized(["C1=CC=CC=C1C1=CC=CC=C1"])
    assert [int(x["type"]) for x in out["bonds"]].count(1) == 1 and [int(x["type"]) for x in out["bonds"]].count(4) == 12


@pytest.mark.parametrize("string", NOT_AROMATIC)
def test_rows_that_stay_as_they_are(string):
    t = tables_of([string])
    out = normalized([string])
    assert written(out) == written(as_rec(t)) == [string]
    assert same_molecules(out, t) and same_records(out["bonds"], t[2]) and not int(out["mols"]["flags"][0]) & N.AROMATIZED


@pytest.mark.parametrize("string", sorted(BRACKETS))
def test_bracket_rows(string):
    out = normalized([string])
    assert written(out) == [BRACKETS[string]]
    assert bool(int(out["mols"]["flags"][0]) & N.UNBRACKETED) == (BRACKETS[string] != string)


def test_the_chiral_symbols_are_copied():
    for string in ("[C@H]", "N[C@@H](C)O", "C[C@](N)(O)F", "[C@@]1=CC=CC=C1"):
        t = tables_of([string])
        out = normalized([string])
        assert same_molecules(out, t) and same_records(out["bonds"], t[2]) and int(out["mols"]["flags"][0]) == 0


def test_atom_notes_against_a_hand_list():
    rows = {"CC(=O)[O-]": [3, 0, 0, 0], "N1C=CC=C1": [1 | 16, 1 | 16, 1 | 16, 1 | 16, 1 | 16], "C[CH](C)F": [3, 1 | 32, 3, 0], "[NH4+]": [4],
            "CC1=CC=CC=C1": [3, 16, 17, 17, 17, 17, 17], "c1ccccc1": [64] * 6, "[nH]1cccc1": [65, 64, 64, 64, 64], "[Ph]C": [64, 3],
            "N#C": [0, 1], "O": [2], "S(=O)(=O)(O)O": [0, 0, 0, 1, 1], "[C@H](N)(O)F": [1, 2, 1, 0], "P": [3], "B": [3], "Cl": [1],
            "*C": [64, 3], "[CH2]=C": [2 | 32, 2], "N(=O)(=O)C": [0, 0, 0, 3], "C:C": [64, 64]}
    out = normalized(list(rows))
    at = 0
    for string, want in rows.items():
        assert out["atom_notes"][at:at + len(want)].tolist() == want, string
        at += len(want)
    assert at == len(out["atom_notes"])


def test_aromatic_input_is_a_fixed_point():
    strings = ["c1ccccc1", "Cc1ccccc1", "c1cc[nH]c1", "O=c1cccc[nH]1", "c1ccccc1-c1ccccc1", "[cH-]1cccc1", "c1ccc2ccccc2c1", "C=Cc1ccccc1"]
    t = tables_of(strings)
    out = normalized(strings)
    assert same_molecules(out, t) and same_records(out["bonds"], t[2]) and not out["mols"]["flags"].any()
    assert written(out) == strings
    # a half-aromatic fused ring system stays as it came: the Kekule ring of this naphthalene holds two lower-case atoms
    half = normalized(["c1ccc2C=CC=Cc2c1"])
    assert written(half) == ["c1ccc2C=CC=Cc2c1"] and int(half["mols"]["flags"][0]) == 0


def test_a_bond_of_no_class_excludes_its_atoms():
    for ty in (0, 7, 4):
        mols, atoms, bonds, text = tables_of(["C1=CC=CC=C1[CH3]"])
        bonds = bonds.copy()
        k = [(int(x["i"]), int(x["j"])) for x in bonds].index((5, 6))
        bonds["type"][k] = ty
        out = N.pack(mols, atoms, bonds, text, tables=TABLES)
        assert same_molecules(out, (mols, atoms, bonds, text)) and same_records(out["bonds"], bonds) and out["atom_notes"].tolist() == [1, 1, 1, 1, 1, 64, 64 | 3]


# ---------------------------------------------------------------------------------------------------- generated molecules
RING_POOL = [b"C"] * 200 + [b"N", b"N", b"N", b"N", b"O", b"S", b"[NH]", b"[CH]", b"[CH-]", b"[N+]", b"[C+]", b"[13C]", b"[C@H]", b"[CH+]", b"c", b"n", b"[nH]",
                          b"[NH+]", b"[C-]", b"P", b"[Se]", b"[R1]"]
SIDE_POOL = [b"C", b"C", b"C", b"N", b"O", b"O", b"F", b"Cl", b"Br", b"I", b"S", b"P", b"B", b"[O-]", b"[NH3+]", b"[CH3]", b"[CH2]", b"[OH]", b"[R1]",
             b"[Ph]", b"*", b"[2H]", b"[C]", b"c", b"[Si]", b"[13CH3]", b"[NH2]", b"[OH2+]", b"[C:3]", b"[U+15]", b"[999Og]", b"<unk>", b"", b"[C@@]"]
LONE_PAIR_POOL = [b"N", b"O", b"S", b"[NH]", b"[CH-]", b"[nH]", b"[N-]", b"[OH+]"]
RING_SIZES = [6, 6, 6, 6, 5, 5, 5, 3, 4, 7, 8]
SIDE_TYPES = [1] * 10 + [2, 2, 3, 5, 6, 0, 4, 7]


def kekule_molecule(rng, max_atoms=40):
    """a small molecule of 1..max_atoms atoms: up to four rings of 3..8 atoms with alternating double bonds, alone, fused at a bond
    or joined by a bond, then side atoms of every class on bonds of every type; bond records sorted by (i, j), no pair twice"""
    syms, bonds, has_double = [], {}, set()

    def atom(pool):
        syms.append(pool[int(rng.integers(0, len(pool)))])
        return len(syms) - 1

    def bond(i, j, ty):
        key = (min(i, j), max(i, j))
        if i != j and key not in bonds:
            bonds[key] = ty
            if ty == 2:
                has_double.update(key)

    for _ in range(int(rng.integers(0, 5))):
        size = RING_SIZES[int(rng.integers(0, len(RING_SIZES)))]
        if len(syms) + size > max_atoms:
            break
        old = list(bonds)
        if old and rng.random() < 0.5:                        # fused at a bond
            i, j = old[int(rng.integers(0, len(old)))]
            ring = [i] + [atom(RING_POOL) for _ in range(size - 2)] + [j]
        else:
            ring = [atom(RING_POOL) for _ in range(size)]
            if size == 5 and rng.random() < 0.8:              # the atom that the alternation leaves without a double bond
                syms[ring[-1]] = LONE_PAIR_POOL[int(rng.integers(0, len(LONE_PAIR_POOL)))]
            if len(ring) < len(syms) and rng.random() < 0.7:  # joined by a bond to what is there
                bond(ring[0], int(rng.integers(0, ring[0])), 1)
        alternate = rng.random() < 0.85
        for k in range(len(ring)):
            i, j = ring[k], ring[(k + 1) % len(ring)]
            double = alternate and i not in has_double and j not in has_double and rng.random() < 0.97
            bond(i, j, 2 if double else 1)
    if not syms:
        atom(SIDE_POOL)
    for _ in range(int(rng.integers(0, 8))):
        if len(syms) >= max_atoms:
            break
        to = int(rng.integers(0, len(syms)))
        bond(atom(SIDE_POOL), to, SIDE_TYPES[int(rng.integers(0, len(SIDE_TYPES)))])
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (len(syms), 2))]
    return syms, xy, [(i, j, ty, ty if ty < 5 else 11 - ty) for (i, j), ty in sorted(bonds.items())]


def dense_molecule(rng, n=30):
    """a near-complete bond graph, as the synthetic checkpoint predicts them: no atom is a candidate"""
    syms = [RING_POOL[int(k)] for k in rng.integers(0, len(RING_POOL), n)]
    bonds = [(i, j, int(rng.integers(1, 3)), 1) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.9]
    return syms, [(int(x), int(y)) for x, y in rng.integers(0, 64, (n, 2))], bonds


def kekule_batch(rng, n, dense=0):
    return [kekule_molecule(rng) for _ in range(n)] + [dense_molecule(rng) for _ in range(dense)]


def test_the_generator_reaches_every_outcome():
    out = N.pack(*M.build_tables(kekule_batch(np.random.default_rng(5), 300, dense=3)), tables=TABLES)
    flags, notes = out["mols"]["flags"], out["atom_notes"]
    assert (flags & N.AROMATIZED).astype(bool).sum() > 40 and (flags & N.UNBRACKETED).astype(bool).sum() > 40 and (flags == 0).sum() > 40
    assert (notes & 64).any() and (notes & 32).any() and (notes & 16).sum() > 200
    assert not (flags[-3:] & N.AROMATIZED).any()
    assert {b"[nH]", b"o", b"s", b"n", b"c"} <= {out["text"][int(m["text0"]) + int(a["sym0"]):][:int(a["sym_len"])]
                                                         for m in out["mols"] for a in out["atoms"][int(m["atom0"]):int(m["atom0"]) + int(m["n_atoms"])]}


def test_twice_is_once_on_generated_molecules():
    """idempotence: the oracle on its own output changes nothing, on 300 molecules of the generators of the canonical and the
    expansion tests and on 300 of the Kekule generator"""
    mols = T.generated_set(100) + E.generated_set(100) + H.random_batch(np.random.default_rng(11), 100) + kekule_batch(np.random.default_rng(12), 300, 2)
    once = N.pack(*M.build_tables(mols), tables=TABLES)
    twice = N.pack(once["mols"], once["atoms"], once["bonds"], once["text"], tables=TABLES)
    assert not (once["mols"]["flags"] & N.REFUSED).any()
    for b, (p, q) in enumerate(zip(X.molecules(once), X.molecules(twice))):
        assert p == q, (b, mols[b], p, q)
    assert twice["text"] == once["text"] and same_records(twice["atoms"], once["atoms"]) and same_records(twice["bonds"], once["bonds"])
    assert not (twice["mols"]["flags"] & (N.AROMATIZED | N.UNBRACKETED)).any()
    kept = (twice["atom_notes"] & 64) == 0                    # a new unbracketed c is copied the second time: its H is not counted again
    assert (twice["atom_notes"] & 15)[kept].tolist() == (once["atom_notes"] & 15)[kept].tolist()
    assert ((once["atom_notes"] & 16) != 0)[~kept].sum() > 200 and not (twice["atom_notes"] & (16 | 32)).any()
    # counts and order never change, and every record field that is not the pass's own travels
    t = M.build_tables(mols)
    assert once["mols"]["n_atoms"].tolist() == t[0]["n_atoms"].tolist() and once["mols"]["n_bonds"].tolist() == t[0]["n_bonds"].tolist()
    for name in ("index", "x_bin", "y_bin", "score"):
        assert once["atoms"][name].tolist() == t[1][name].tolist()
    assert once["bonds"]["i"].tolist() == t[2]["i"].tolist() and once["bonds"]["j"].tolist() == t[2]["j"].tolist()


def test_refusals_and_the_truncated_bit():
    ok = ([b"C", b"[CH3]"], [(0, 0), (1, 1)], [(0, 1, 1, 1)])
    big = ([b"C"] * 1000, [(0, 0)] * 1000, [])
    mols, atoms, bonds, text = M.build_tables([ok, big, ok, ([b"C", b"C"], [(0, 0)] * 2, [(0, 2, 1, 1)]), ([], [], [])])
    mols["flags"][0] = mols["flags"][1] = 1 | 2 | 4
    mols["overall_score"] = [0.5, 0.25, 0.125, 1.0, 2.0]
    out = N.pack(mols, atoms, bonds, text, tables=TABLES)
    assert out["mols"]["flags"].tolist() == [1 | N.UNBRACKETED, 1 | N.REFUSED, N.UNBRACKETED, N.REFUSED, 0]
    assert out["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 0] and out["mols"]["atom0"].tolist() == [0, 2, 2, 4, 4]
    assert out["mols"]["overall_score"].tolist() == [0.5, 0.25, 0.125, 1.0, 2.0] and out["text"] == b"CCCC"
    cut = N.pack(mols, atoms, bonds, text, tables=TABLES, n_text_bytes=len(text) - 1)
    assert cut["mols"]["flags"].tolist()[2:] == [N.UNBRACKETED, N.REFUSED, N.REFUSED]    # the empty molecule begins behind the cut too
    cut = N.pack(mols, atoms, bonds, text, tables=TABLES, n_atom_records=len(atoms) - 1)
    assert cut["mols"]["flags"].tolist()[2:] == [N.UNBRACKETED, N.REFUSED, N.REFUSED]
