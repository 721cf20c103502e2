"""CPU: the fragment library (molnextr_amd/vocab/fragments.json, molnextr_amd/fragments.py) and the oracle of mnx_expand_pack
(tests/expand_ref.py): the library parses and says what a chemist means by each name (a list written by hand below, not derived
from the JSON), the product's reader and the oracle's agree, three expanded molecules written out by hand, the properties of the
expansion on random molecules, and the point of it all: a label and the drawn-out group get the same canonical string."""
from collections import Counter

import numpy as np
import pytest

import canon_ref as K
import expand_ref as X
import molfile_ref as M
import packed_tables as P
import stereo_ref as T
from molnextr_amd import chem, fragments as F

# name(s) -> (heavy atoms per element, attachment element, sum of the orders of the non-aromatic bonds, aromatic bonds,
# non-zero charges); written from the structures, not from the JSON
BY_HAND = {
    "Me": ("C", "C", 0, 0, ()), "Et": ("C2", "C", 1, 0, ()), "Pr nPr n-Pr": ("C3", "C", 2, 0, ()), "iPr i-Pr": ("C3", "C", 2, 0, ()),
    "Bu nBu n-Bu": ("C4", "C", 3, 0, ()), "iBu i-Bu": ("C4", "C", 3, 0, ()), "tBu t-Bu": ("C4", "C", 3, 0, ()),
    "Ph": ("C6", "C", 0, 6, ()), "Bn": ("C7", "C", 1, 6, ()), "Bz": ("C7 O", "C", 3, 6, ()), "Ac": ("C2 O", "C", 3, 0, ()),
    "Boc": ("C5 O2", "C", 7, 0, ()), "Cbz": ("C8 O2", "C", 5, 6, ()), "Fmoc": ("C15 O2", "C", 8, 12, ()),
    "Ts Tos": ("C7 O2 S", "S", 6, 6, ()), "Ms": ("C O2 S", "S", 5, 0, ()), "Tf": ("C F3 O2 S", "S", 8, 0, ()),
    "TMS": ("C3 Si", "Si", 3, 0, ()), "TBS": ("C6 Si", "Si", 6, 0, ()), "TIPS": ("C9 Si", "Si", 9, 0, ()),
    "Piv": ("C5 O", "C", 6, 0, ()), "Cy": ("C6", "C", 6, 0, ()), "Allyl": ("C3", "C", 3, 0, ()), "Tol pTol": ("C7", "C", 1, 6, ()),
    "PMB": ("C8 O", "C", 3, 6, ()), "CF3 F3C": ("C F3", "C", 3, 0, ()), "CCl3": ("C Cl3", "C", 3, 0, ()), "CN NC": ("C N", "C", 3, 0, ()),
    "NO2 O2N": ("N O2", "N", 3, 0, (-1, 1)), "CHO OHC": ("C O", "C", 2, 0, ()), "CO2H COOH HO2C": ("C O2", "C", 3, 0, ()),
    "CO2Me MeO2C": ("C2 O2", "C", 4, 0, ()), "CO2Et COOEt EtO2C": ("C3 O2", "C", 5, 0, ()), "CO2tBu": ("C5 O2", "C", 7, 0, ()),
    "OMe MeO OCH3 CH3O H3CO": ("C O", "O", 1, 0, ()), "OEt EtO": ("C2 O", "O", 2, 0, ()), "OiPr iPrO": ("C3 O", "O", 3, 0, ()),
    "OtBu": ("C4 O", "O", 4, 0, ()), "OAc": ("C2 O2", "O", 4, 0, ()), "OBn": ("C7 O", "O", 2, 6, ()), "OBz": ("C7 O2", "O", 4, 6, ()),
    "OPh": ("C6 O", "O", 1, 6, ()), "OMs": ("C O3 S", "O", 6, 0, ()), "OTf": ("C F3 O3 S", "O", 9, 0, ()),
    "OTBS": ("C6 O Si", "O", 7, 0, ()), "OTMS": ("C3 O Si", "O", 4, 0, ()), "OCF3": ("C F3 O", "O", 4, 0, ()),
    "NMe2 Me2N": ("C2 N", "N", 2, 0, ()), "NHAc": ("C2 N O", "N", 4, 0, ()), "NHBoc": ("C5 N O2", "N", 8, 0, ()),
    "NHTs": ("C7 N O2 S", "N", 7, 6, ()), "SMe MeS SCH3": ("C S", "S", 1, 0, ()), "SPh": ("C6 S", "S", 1, 6, ()),
    "SO2Me": ("C O2 S", "S", 5, 0, ()), "SO2Ph": ("C6 O2 S", "S", 5, 6, ()), "SO3H": ("O3 S", "S", 5, 0, ()),
    "N3": ("N3", "N", 4, 0, (-1, 1)), "C6F5": ("C6 F5", "C", 5, 6, ()), "B(OH)2": ("B O2", "B", 2, 0, ()),
}
REQUIRED = ("Me Et Pr nPr n-Pr iPr i-Pr Bu nBu n-Bu iBu i-Bu tBu t-Bu Ph Bn Bz Ac Boc Cbz Fmoc Ts Tos Ms Tf TMS TBS TIPS Piv Cy Allyl "
            "Tol pTol PMB CF3 F3C CCl3 CN NC NO2 O2N CHO OHC CO2H COOH HO2C CO2Me MeO2C CO2Et COOEt EtO2C CO2tBu OMe MeO OCH3 CH3O "
            "H3CO OEt EtO OiPr iPrO OtBu OAc OBn OBz OPh OMs OTf OTBS OTMS OCF3 NMe2 Me2N NHAc NHBoc NHTs SMe MeS SCH3 SPh SO2Me "
            "SO2Ph SO3H N3 C6F5 B(OH)2").split()
NOT_CERTAIN = ("Tcs", "TBZ", "SP", "17Napdh", "OAlI", "SiR2", "SiR23", "OSiR2", "OSiR23", "H3", "(H)")


@pytest.fixture(scope="module")
def table():
    return F.load()


@pytest.fixture(scope="module")
def tables():
    return M.name_tables()


@pytest.fixture(scope="module")
def library(tables):
    return X.library(tables=tables)


def test_every_entry_parses_and_is_an_abbreviation_of_parsed_atoms(table, tables):
    assert set(REQUIRED) <= set(table)
    for name, smiles in table.items():
        assert name in chem.ABBREVIATIONS and tables[name.encode("utf-8")] == 2, name
        symbols, bonds = F.parse(smiles, name)
        assert 1 <= len(symbols) <= 32
        for s in symbols:
            a = M.interpret(s.encode(), tables)
            assert not a["pseudo"] and a["symbol"] != "R" and len(s) <= 8, (name, s)
    assert not set(NOT_CERTAIN) & set(table)


def test_the_hand_written_list_covers_the_required_names():
    listed = [n for names in BY_HAND for n in names.split()]
    assert sorted(listed) == sorted(REQUIRED) and len(set(listed)) == len(listed)


def describe(symbols, bonds, tables):
    atoms = [M.interpret(s, tables) for s in symbols]
    count = Counter(a["symbol"] for a in atoms)
    formula = " ".join(el + (str(k) if k > 1 else "") for el, k in sorted(count.items()))
    return (formula, atoms[0]["symbol"], sum(ty for _, _, ty in bonds if ty != 4), sum(ty == 4 for _, _, ty in bonds),
            tuple(sorted(a["charge"] for a in atoms if a["charge"])))


@pytest.mark.parametrize("names", sorted(BY_HAND))
def test_table_content_against_the_list_written_by_hand(names, library, tables):
    first = None
    for name in names.split():
        symbols, bonds = library[name.encode()]
        assert describe(symbols, bonds, tables) == BY_HAND[names], name
        assert all(a["h"] == 0 for a in (M.interpret(s, tables) for s in symbols)), "hydrogens are implicit"
        first = first or (symbols, bonds)
        assert (symbols, bonds) == first, f"{name} is a synonym of {names.split()[0]}"
        # one connected piece (none of the required names is an ionic pair)
        seen, todo = {0}, [0]
        while todo:
            a = todo.pop()
            for i, j, _ in bonds:
                for x, y in ((i, j), (j, i)):
                    if x == a and y not in seen:
                        seen.add(y)
                        todo.append(y)
        assert len(seen) == len(symbols)


def test_product_reader_and_oracle_reader_give_identical_tables(table, library):
    for name, smiles in table.items():
        symbols, bonds = F.parse(smiles, name)
        assert ([s.encode() for s in symbols], bonds) == library[name.encode("utf-8")], name
    mols, atoms, bonds, text, frag_of_name = F.fragment_tables()
    from molnextr_amd.engine import symbol_tables
    raw, offsets, kinds, n = symbol_tables()
    assert len(frag_of_name) == n and frag_of_name.dtype == np.int32
    for k in range(n):
        name, f = raw[offsets[k]:offsets[k + 1]], int(frag_of_name[k])
        assert (f >= 0) == (name in library and kinds[k] == 2), name
        if f >= 0:
            m = mols[f]
            A, B, t0 = atoms[m["atom0"]:m["atom0"] + m["n_atoms"]], bonds[m["bond0"]:m["bond0"] + m["n_bonds"]], int(m["text0"])
            got = ([text[t0 + a["sym0"]:t0 + a["sym0"] + a["sym_len"]] for a in A],
                   [(int(b["i"]), int(b["j"]), int(b["type"])) for b in B])
            assert got == library[name] and all(b["rev"] == b["type"] for b in B), name


@pytest.mark.parametrize("bad", ["", "C" * 33, "C%10CC%10", "C/C=C/C", "[C@H](C)N", "C1CC", "C(C", "CC)", "C=", "=C", "C:C", "C~C", "*",
                                 "[Ac]", "[H]", "X", "C0CC0", "[12345C]", "C..C", "C.", "[CH3:1]"])
def test_strings_outside_the_grammar_raise_in_both_readers(bad, tables):
    with pytest.raises(ValueError):
        F.parse(bad)
    with pytest.raises(ValueError):
        X.read_fragment(bad, tables)


def expanded(molecules, library, tables):
    t = M.build_tables(molecules)
    return X.pack(*t, frags=library, tables=tables)


def test_three_small_molecules_written_out_by_hand(library, tables):
    one = ([b"C", b"[OMe]"], [(10, 20), (30, 40)], [(0, 1, 1, 1)])
    two = ([b"C", b"[Ac]", b"N"], [(1, 2), (3, 4), (5, 6)], [(0, 1, 1, 1), (1, 2, 2, 2)])
    both = ([b"OMe", b"[Et]"], [(7, 8), (9, 10)], [(0, 1, 1, 1)])
    r = expanded([one, two, both], library, tables)
    assert r["text"] == b"COC" + b"CCNOC" + b"OCCC"
    assert r["mols"].tolist() == [(0, 3, 0, 2, 0, 3, 2, 0, 0.0), (3, 5, 2, 4, 3, 5, 2, 0, 0.0), (8, 4, 6, 3, 8, 4, 2, 0, 0.0)]
    assert r["atoms"].tolist() == [
        (0, 1, 0, 10, 20, 0.0), (1, 1, 1, 30, 40, 0.0), (2, 1, 1, 30, 40, 0.0),
        (0, 1, 0, 1, 2, 0.0), (1, 1, 1, 3, 4, 0.0), (2, 1, 2, 5, 6, 0.0), (3, 1, 1, 3, 4, 0.0), (4, 1, 1, 3, 4, 0.0),
        (0, 1, 0, 7, 8, 0.0), (1, 1, 1, 9, 10, 0.0), (2, 1, 0, 7, 8, 0.0), (3, 1, 1, 9, 10, 0.0)]
    assert r["bonds"].tolist() == [
        (0, 1, 1, 1, 0.0), (1, 2, 1, 1, 0.0),
        (0, 1, 1, 1, 0.0), (1, 2, 2, 2, 0.0), (1, 3, 2, 2, 0.0), (1, 4, 1, 1, 0.0),
        (0, 1, 1, 1, 0.0), (0, 2, 1, 1, 0.0), (1, 3, 1, 1, 0.0)]
    assert r["origin"].tolist() == [0, 1, 1, 0, 1, 2, 1, 1, 0, 1, 0, 1]
    assert r["totals"] == (12, 9, 12)


def test_scores_and_flags_travel(library, tables):
    mols, atoms, bonds, text = M.build_tables([([b"[R1]", b"[tBu]", b"[Tcs]", b"*"], [(1, 1)] * 4, [(0, 1, 5, 6), (1, 2, 1, 1)])])
    atoms["score"], bonds["score"], mols["overall_score"], mols["flags"] = [0.1, 0.2, 0.3, 0.4], [0.5, 0.6], 0.7, 1
    atoms["index"] = [11, 12, 13, 14]
    r = X.pack(mols, atoms, bonds, text, frags=library, tables=tables)
    assert r["mols"]["flags"].tolist() == [1 | X.EXPANDED | X.LABEL_LEFT] and r["mols"]["overall_score"].tolist() == [0.7]
    assert r["atoms"]["score"].tolist() == [0.1, 0.2, 0.3, 0.4, 0.2, 0.2, 0.2] and r["atoms"]["index"].tolist() == [11, 12, 13, 14, 12, 12, 12]
    assert r["bonds"].tolist() == [(0, 1, 5, 6, 0.5), (1, 2, 1, 1, 0.6), (1, 4, 1, 1, 0.2), (1, 5, 1, 1, 0.2), (1, 6, 1, 1, 0.2)]
    only_star = X.pack(*M.build_tables([([b"*", b"[*]", b"C"], [(0, 0)] * 3, [])]), frags=library, tables=tables)
    assert only_star["mols"]["flags"].tolist() == [0], "a parsed '*' is no label"


LABELS = [b"[Ph]", b"Ph", b"OMe", b"[tBu]", b"[CO2Et]", b"[NO2]", b"[Fmoc]", b"[Boc]", b"[N3]", b"[Tcs]", b"[OTf]"]


def random_batch(rng, n, pool=None, max_atoms=24):
    """random molecules of P.POOL plus labels, bond records in the documented order (i ascending, then j), no pair twice"""
    pool = pool or P.POOL + LABELS * 2
    out = []
    for _ in range(n):
        na = int(rng.integers(0, max_atoms))
        syms, xy, bonds = P.random_molecule(rng, na, int(rng.integers(0, na + 4)), pool)
        seen = {}
        for i, j, ty, rv in bonds:
            seen.setdefault((i, j), (i, j, ty, rv))
        out.append((syms, xy, sorted(seen.values())))
    return out


def test_properties_on_random_molecules(library, tables):
    rng = np.random.default_rng(2024)
    batch = random_batch(rng, 300)
    t = M.build_tables(batch)
    r = X.pack(*t, frags=library, tables=tables)
    again = X.pack(r["mols"], r["atoms"], r["bonds"], r["text"], frags=library, tables=tables)
    n_expanded = 0
    for b, ((syms, xy, bonds), (s2, xy2, b2)) in enumerate(zip(batch, X.molecules(r))):
        sizes = [len(f[0]) if f else 1 for f in (X.fragment_of(s, library, tables) for s in syms)]
        assert len(s2) == len(syms) + sum(m - 1 for m in sizes)
        assert not int(r["mols"][b]["flags"]) & X.REFUSED
        n_expanded += bool(int(r["mols"][b]["flags"]) & X.EXPANDED)
        it = iter(b2)
        assert all(any(x == old for x in it) for old in bonds), "the input's bonds survive unchanged, as a subsequence"
        assert [x[:2] for x in b2] == sorted(x[:2] for x in b2) and all(i < j < len(s2) for i, j, _, _ in b2)
        assert len({x[:2] for x in b2}) == len(b2)
        a0 = int(r["mols"][b]["atom0"])
        origin = r["origin"][a0:a0 + len(s2)].tolist()
        assert origin[:len(syms)] == list(range(len(syms)))
        assert origin[len(syms):] == [a for a, m in enumerate(sizes) for _ in range(m - 1)]
        assert all(xy2[k] == xy[o] for k, o in enumerate(origin))
        assert not any(X.fragment_of(s, library, tables) for s in s2)
    assert 150 < n_expanded < 300
    for key in ("atoms", "bonds", "mols"):
        a, c = r[key].copy(), again[key].copy()
        if key == "mols":
            a["flags"] &= ~np.uint32(X.EXPANDED)           # nothing is left to replace the second time
        assert a.tolist() == c.tolist(), key
    assert again["text"] == r["text"] and again["origin"].tolist() == [k for m in r["mols"] for k in range(int(m["n_atoms"]))]


def test_refusals(library, tables):
    ok = ([b"C", b"[OMe]"], [(1, 1), (2, 2)], [(0, 1, 1, 1)])
    unsorted = ([b"C", b"[OMe]", b"N"], [(1, 1)] * 3, [(1, 2, 1, 1), (0, 1, 1, 1)])
    big = ([b"C"] * 2048, [(0, 0)] * 2048, [])
    fits = ([b"[Ph]"] * 2047, [(0, 0)] * 2047, [])
    mols, atoms, bonds, text = M.build_tables([ok, unsorted, big, fits, ok])
    r = X.pack(mols, atoms, bonds, text, frags=library, tables=tables)
    assert [int(f) & X.REFUSED for f in r["mols"]["flags"]] == [0, 8, 8, 0, 0]
    assert r["mols"]["n_atoms"].tolist() == [3, 0, 0, 2047 * 6, 3] and r["mols"]["n_bonds"].tolist() == [2, 0, 0, 2047 * 6, 2]
    short = X.pack(mols, atoms, bonds, text, frags=library, tables=tables, n_atom_records=len(atoms) - 1)
    assert [int(f) & X.REFUSED for f in short["mols"]["flags"]] == [0, 8, 8, 0, 8]


# ---- the user-visible point: a label on one drawing and the drawn-out group on another get the same canonical string ----
CORE = ([b"Cl", b"C", b"C", b"O", b"N"], [(0, 1, 1, 1), (1, 2, 1, 1), (2, 3, 2, 2), (2, 4, 1, 1)])       # ClCC(=O)N-, the group at N
DRAWN_OUT = {
    "Ph": ([b"c"] * 6, [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 4, 4), (4, 5, 4), (0, 5, 4)]),
    "OMe": ([b"O", b"C"], [(0, 1, 1)]),
    "tBu": ([b"C"] * 4, [(0, 1, 1), (0, 2, 1), (0, 3, 1)]),
    "CO2Et": ([b"C", b"O", b"O", b"C", b"C"], [(0, 1, 2), (0, 2, 1), (2, 3, 1), (3, 4, 1)]),
    "NO2": ([b"[N+]", b"O", b"[O-]"], [(0, 1, 2), (0, 2, 1)]),
}


def label_and_drawn_out(name, rng):
    """(the core with the label at its N, the same molecule drawn out atom by atom: distinct coordinates, shuffled numbering)"""
    core_syms, core_bonds = CORE
    n = len(core_syms)
    labelled = (core_syms + [b"[" + name.encode() + b"]"], [(int(x), int(y)) for x, y in rng.integers(0, 64, (n + 1, 2))],
                core_bonds + [(n - 1, n, 1, 1)])
    gsyms, gbonds = DRAWN_OUT[name]
    syms = core_syms + gsyms
    bonds = core_bonds + [(n - 1, n, 1, 1)] + [(n + i, n + j, ty, ty) for i, j, ty in gbonds]
    cells = rng.permutation(64 * 64)[:len(syms)]
    drawn = T.renumber((syms, [(int(c) % 64, int(c) // 64) for c in cells], bonds), [int(p) for p in rng.permutation(len(syms))], rng)
    return labelled, (drawn[0], drawn[1], sorted(drawn[2]))


@pytest.mark.parametrize("name", sorted(DRAWN_OUT))
def test_a_label_and_the_drawn_out_group_get_the_same_canonical_string(name, library, tables):
    rng = np.random.default_rng(sum(name.encode()))
    labelled, drawn = label_and_drawn_out(name, rng)
    r = expanded([labelled, drawn], library, tables)
    assert r["mols"]["flags"].tolist() == [X.EXPANDED, 0]
    c = K.pack(r["mols"], r["atoms"], r["bonds"], r["text"], 0, tables)
    a, b = (c["out"][x["text0"]:x["text0"] + x["len"]] for x in c["recs"])
    assert a == b and len(a) > 0 and b"*" not in a, (a, b)
    unexpanded = K.pack(*M.build_tables([labelled, drawn]), 0, tables)
    assert b"*" in unexpanded["out"], "without the pass the label is a hole in the string"
