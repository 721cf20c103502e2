"""CPU: the oracle of mnx_smiles_pack (tests/smiles_ref.py) against strings written out by hand, its reader against its writer
over random graphs, the ring-number rules at their limit, every flag; and the binding of the new call."""
import ctypes
import os
import re

import numpy as np
import pytest

import molfile_ref as M
import smiles_ref as S
from molnextr_amd import engine
from molnextr_amd.model import predict_pipeline
from packed_tables import POOL, path


def ring(first, n, cls):
    """bonds of a ring over atoms first .. first + n - 1"""
    return [(first + k, first + k + 1, cls, cls) for k in range(n - 1)] + [(first, first + n - 1, cls, cls)]


CUBE = [(0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]

# name: (symbols, bonds (i, j, type, rev), the string, flags) — each string worked out by hand from the rules of the header
HAND = {
    "benzene": ([b"c"] * 6, ring(0, 6, 4), "c1ccccc1", 0),
    "acetic acid": ([b"C", b"C", b"O", b"O"], [(0, 1, 1, 1), (1, 2, 2, 2), (1, 3, 1, 1)], "CC(=O)O", 0),
    "biphenyl": ([b"c"] * 12, ring(0, 6, 4) + ring(6, 6, 4) + [(5, 6, 1, 1)], "c1ccccc1-c1ccccc1", 0),
    "naphthalene": ([b"c"] * 10, path(10, 4) + [(0, 9, 4, 4), (3, 8, 4, 4)], "c1ccc2ccccc2c1", 0),
    "spiro": ([b"C"] * 5, [(0, 1, 1, 1), (1, 2, 1, 1), (0, 2, 1, 1), (0, 3, 1, 1), (3, 4, 1, 1), (0, 4, 1, 1)], "C12(CC1)CC2", 0),
    # the walk is 0 1 2 3 7 4 5 6: atom 7 takes number 1 again, atom 6 closes 4 (to atom 2) in front of 1 (to atom 7)
    "cubane": ([b"C"] * 8, [(i, j, 1, 1) for i, j in CUBE], "C12C3C4C1C1C2C3C41", 0),
    "salt": ([b"[Na+]", b"[Cl-]"], [], "[Na+].[Cl-]", 0),
    "chiral mark dropped": ([b"N", b"[C@@H]", b"C", b"O"], [(0, 1, 1, 1), (1, 2, 6, 0), (1, 3, 1, 1)], "N[CH](C)O", S.FLAG_WEDGES),
    "numbered R-group": ([b"C", b"[R1]"], [(0, 1, 1, 1)], "C[1*]", S.FLAG_PSEUDO),
    "abbreviation": ([b"C", b"[OMe]"], [(0, 1, 1, 1)], "C*", S.FLAG_PSEUDO),
    "aromatic bond to C": ([b"c", b"C"], [(0, 1, 4, 4)], "c:C", 0),
    "unknown class": ([b"C", b"C", b"N"], [(0, 1, 7, 0), (1, 2, 3, 3)], "C~C#N", S.FLAG_UNKNOWN),
    "bracket atoms": ([b"[N++]", b"[C:12]", b"[nH]", b"[13CH3-]", b"[se]", b"[*+]", b"[U+15]", b"[2H]", b"Cl", b"*"], path(10),
                      "[N+2][C][nH][13CH3-][se][*+][U+15][2H]Cl*", 0),
    "branches": ([b"C", b"C", b"C", b"C", b"C", b"C"], [(0, 1, 1, 1), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 2, 2), (3, 5, 1, 1)], "CC(C)(CC)=C", 0),
}


def one(name):
    syms, bonds = HAND[name][:2]
    return M.build_tables([(syms, [(0, 0)] * len(syms), bonds)])


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_equals_hand_written_string(name):
    syms, bonds, want, flags = HAND[name]
    got = S.pack(*one(name))
    assert got["out"].decode() == want and got["recs"]["flags"][0] == flags and got["recs"]["len"][0] == len(want) == got["total"]
    assert got["recs"]["n_rings"][0] == len(bonds) - len(syms) + want.count(".") + 1
    atoms, read_bonds = S.read(want)
    assert len(atoms) == len(syms) and len(read_bonds) == len(bonds)


def test_hand_written_details():
    assert S.pack(*one("cubane"))["order"].tolist() == [0, 1, 2, 3, 5, 6, 7, 4] and S.pack(*one("cubane"))["recs"]["n_rings"][0] == 5
    assert S.read("c1ccccc1-c1ccccc1")[1][(5, 6)] == "-"          # the bond between biphenyl's rings is written
    assert S.read("C12C3C4C1C1C2C3C41")[1] == {tuple(sorted((a, b))): "" for a, b in
                                               [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (0, 3), (0, 5), (1, 6), (2, 7), (4, 7)]}
    all_of_them = S.pack(*M.build_tables([([], [], [])] + [(HAND[k][0], [(0, 0)] * len(HAND[k][0]), HAND[k][1]) for k in sorted(HAND)]))
    assert all_of_them["out"].decode() == "".join(HAND[k][2] for k in sorted(HAND))
    assert all_of_them["recs"]["len"][0] == 0 and all_of_them["recs"]["flags"][0] == 0          # the empty molecule


def test_a_freed_ring_number_comes_back():
    """three fused squares along the path 0 .. 7: number 1 is closed at atom 3 and allotted again at atom 4"""
    text = S.smiles([b"C"] * 8, path(8) + [(0, 3, 1, 1), (2, 5, 1, 1), (4, 7, 1, 1)])[0]
    assert text == "C1CC2C1C1C2CC1"


def test_a_number_closed_at_an_atom_is_not_reused_at_that_atom():
    """two triangles that meet at atom 2: it closes 1 and opens a ring of its own, which must take 2"""
    text = S.smiles([b"C"] * 5, [(0, 1, 1, 1), (1, 2, 1, 1), (0, 2, 1, 1), (2, 3, 1, 1), (3, 4, 1, 1), (2, 4, 1, 1)])[0]
    assert text == "C1CC12CC2"


def complete(n):
    return [b"C"] * n, [(i, j, 1, 1) for i in range(n) for j in range(i + 1, n)]


def fan(r):
    """a path 0 .. r + 1 whose atom 0 is also bonded to atoms 2 .. r + 1: atom 0 opens r ring numbers at once"""
    return [b"C"] * (r + 2), path(r + 2) + [(0, k, 1, 1) for k in range(2, r + 2)]


def numbers_in_use(text):
    """the most ring numbers open behind any atom of a written string (numbers closed at an atom still count there)"""
    open_now, most = set(), 0
    for atom in re.findall(r"(?:\[[^\]]*\]|[A-Za-z*])((?:[-=#:~]?(?:%\d\d|\d))*)", text):
        closing = set()
        for r in re.findall(r"%\d\d|\d", atom):
            r = int(r.lstrip("%"))
            (closing if r in open_now else open_now).add(r)
        most = max(most, len(open_now))
        open_now -= closing
    return most


def test_percent_numbers_and_the_limit_of_99():
    """A complete graph walks as a path, and by the release rule it holds (k + 1)(n - k) - 3 numbers at position k (k >= 1): the
    oracle finds K19 inside the limit, with 97 numbers, and refuses K20, which would need 107."""
    need = lambda n: max((k + 1) * (n - k) - 3 for k in range(1, n - 1))               # noqa: E731
    assert need(19) == 97 and need(20) == 107
    text, order, flags, n_rings = S.smiles(*complete(19))
    assert flags == 0 and n_rings == 19 * 18 // 2 - 19 + 1 and order == list(range(19)) and "(" not in text
    assert numbers_in_use(text) == 97 and "%97" in text and "%98" not in text
    atoms, bonds = S.read(text)
    assert len(atoms) == 19 and sorted(bonds) == [(i, j) for i in range(19) for j in range(i + 1, 19)]
    assert S.smiles(*complete(20)) == (None, None, S.FLAG_RINGS, 20 * 19 // 2 - 20 + 1)
    text, _, flags, n_rings = S.smiles(*fan(99))                                         # exactly 99: written
    assert flags == 0 and n_rings == 99 and text.startswith("C123456789%10%11") and text.endswith("C%97C%98C%99") and numbers_in_use(text) == 99
    assert len(S.read(text)[1]) == 100 + 99
    assert S.smiles(*fan(100)) == (None, None, S.FLAG_RINGS, 100)                        # 100: refused


def random_graph(rng, n_atoms, n_bonds, pool=POOL):
    """a graph without loops or repeated pairs, bond records in random order, classes 0 .. 7"""
    syms = [pool[k] for k in rng.integers(0, len(pool), n_atoms)]
    pairs = set()
    for _ in range(n_bonds if n_atoms >= 2 else 0):
        i, j = sorted(int(v) for v in rng.choice(n_atoms, 2, replace=False))
        pairs.add((i, j))
    pairs = [sorted(pairs)[k] for k in rng.permutation(len(pairs))]
    return syms, [(0, 0)] * n_atoms, [(i, j, int(rng.integers(0, 8)), int(rng.integers(0, 7))) for i, j in pairs]


def components(n, bonds):
    root = list(range(n))

    def find(a):
        while root[a] != a:
            a = root[a]
        return a
    for b in bonds:
        root[find(b[0])] = find(b[1])
    return len({find(a) for a in range(n)})


def test_round_trip_over_random_graphs():
    """read(out), mapped through `order`, gives back every atom's text and every bond's pair and class; ring digits and n_rings"""
    rng = np.random.default_rng(21)
    tables = M.name_tables()
    graphs = [random_graph(rng, int(n), int(rng.integers(0, n + 8))) for n in rng.integers(0, 61, 300)]
    got = S.pack(*M.build_tables(graphs))
    assert not (got["recs"]["flags"] & (S.FLAG_TOO_LARGE | S.FLAG_BEYOND | S.FLAG_DUPLICATE | S.FLAG_RINGS)).any()
    seen = set()
    for (syms, _, bonds), rec, m in zip(graphs, got["recs"], M.build_tables(graphs)[0]):
        text = got["out"][rec["text0"]:rec["text0"] + rec["len"]].decode("ascii")
        order = got["order"][m["atom0"]:m["atom0"] + m["n_atoms"]].tolist()
        atoms, read_bonds = S.read(text)
        assert sorted(order) == list(range(len(syms))) and len(atoms) == len(syms) and len(read_bonds) == len(bonds)
        want = [S.atom_text(s, tables) for s in syms]
        assert [atoms[order[k]] for k in range(len(syms))] == [w[0] for w in want]
        for i, j, ty, _ in bonds:
            symbol = read_bonds[tuple(sorted((order[i], order[j])))]
            both = want[i][1] and want[j][1]
            if symbol == "":                                   # the implicit rule, inverted
                symbol = ":" if both else "-"
            assert symbol == {1: "-", 5: "-", 6: "-", 2: "=", 3: "#", 4: ":"}.get(ty, "~"), (text, i, j, ty)
            seen.add((symbol, both))
        plain = re.sub(r"\[[^\]]*\]", "", text)
        assert len(re.findall(r"%\d\d|\d", plain)) == 2 * rec["n_rings"]
        assert rec["n_rings"] == len(bonds) - len(syms) + components(len(syms), bonds)
        assert text.count(".") == components(len(syms), bonds) - 1 if syms else text == ""
        assert bool(rec["flags"] & S.FLAG_WEDGES) == any(b[2] in (5, 6) for b in bonds)
        assert bool(rec["flags"] & S.FLAG_UNKNOWN) == any(b[2] in (0, 7) for b in bonds)
        assert bool(rec["flags"] & S.FLAG_PSEUDO) == any(w[2] for w in want)
    assert len(seen) == 10 and got["recs"]["n_rings"].max() > 5          # every symbol between aromatic and other atoms


def test_reader_refuses_what_the_writer_never_emits():
    for bad in ("C1CC", "C(C", "CC)", "C=", "=C", "C..C", "C.", "C%1C", "C[Xx]", "C/C=C/C", "C[C@H](N)O", "C0CC0", "C11", "C==C", "C(=)C",
                "C1CC=1", "(C)C", "C.1C"):
        with pytest.raises(ValueError):
            S.read(bad)
    assert S.read("") == ([], {})


def test_every_flag():
    c = lambda n: ([b"C"] * n, [(0, 0)] * n)                                             # noqa: E731
    mols = [c(3) + ([(0, 1, 1, 1), (1, 2, 1, 1), (0, 1, 2, 2)],),          # 0 the pair 0 1 in two records
            c(3) + ([(0, 1, 1, 1), (2, 2, 1, 1)],),                         # 1 a bond from an atom to itself
            c(1000) + ([(0, 1, 1, 1)],),                                    # 2 1000 atoms
            c(3) + ([(0, 1, 7, 1), (1, 2, 0, 1)],),                         # 3 unknown classes
            c(3) + ([(0, 1, 1, 1), (1, 3, 1, 1)],),                         # 4 a bond to an atom the molecule does not have
            ([b"C", b"[R1]", b"C"], [(0, 0)] * 3, [(0, 1, 5, 0), (1, 2, 1, 1), (0, 2, 1, 1), (2, 0, 1, 1)]),      # 5 duplicate, reversed
            c(2) + ([(0, 1, 1, 1)],)]                                       # 6 intact behind them
    tables = M.build_tables(mols)
    tables[0]["flags"][6] = 1
    got = S.pack(*tables)
    assert got["recs"]["flags"].tolist() == [S.FLAG_DUPLICATE, S.FLAG_BEYOND, S.FLAG_TOO_LARGE, S.FLAG_UNKNOWN, S.FLAG_BEYOND,
                                             S.FLAG_DUPLICATE | S.FLAG_PSEUDO, S.FLAG_TRUNCATED]
    assert got["recs"]["len"].tolist() == [0, 0, 0, 5, 0, 0, 2] and got["out"] == b"C~C~CCC" and got["recs"]["text0"].tolist() == [0, 0, 0, 0, 5, 5, 5]
    assert got["recs"]["n_rings"].tolist() == [1, 0, 0, 0, 0, 2, 0]
    a0 = tables[0]["atom0"]
    assert (got["order"][:a0[3]] == S.NO_POSITION).all() and got["order"][a0[3]:a0[4]].tolist() == [0, 1, 2]
    assert (got["order"][a0[4]:a0[6]] == S.NO_POSITION).all() and got["order"][a0[6]:].tolist() == [0, 1]
    mols, atoms, bonds, text = M.build_tables([c(2) + ([(0, 1, 1, 1)],), c(3) + ([(0, 1, 2, 2)],)])
    for kw in ({"n_atom_records": len(atoms) - 1}, {"n_bond_records": 1}, {"n_text_bytes": len(text) - 1}):
        cut = S.pack(mols, atoms, bonds, text, order_fill=0x7F7F, **kw)                 # the second molecule reaches beyond
        assert cut["recs"]["flags"].tolist() == [0, S.FLAG_BEYOND] and cut["out"] == b"CC" and cut["recs"]["n_rings"].tolist() == [0, 0]
        assert cut["order"].tolist() == [0, 1] + [S.NO_POSITION] * (len(cut["order"]) - 2)
    atoms["sym_len"][3] = 9                                                              # a symbol behind the text
    assert S.pack(mols, atoms, bonds, text)["recs"]["flags"].tolist() == [0, S.FLAG_BEYOND]


def test_library_and_binding_carry_the_new_call():
    lib = engine.load_library()
    assert "mnx_smiles_pack" in engine.SYMBOLS and hasattr(lib, "mnx_smiles_pack") and len(lib.mnx_smiles_pack.argtypes) == 15
    assert ctypes.sizeof(engine.MnxSmiles) == engine.SMILES_DTYPE.itemsize == 16
    assert [f[0] for f in engine.MnxSmiles._fields_] == list(engine.SMILES_DTYPE.names) == ["text0", "len", "flags", "n_rings"]
    assert lib.mnx_smiles_pack(None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, None) == -1
    assert (engine.SMILES_TOO_LARGE, engine.SMILES_BEYOND_TABLES, engine.SMILES_PSEUDO_ATOM, engine.SMILES_TRUNCATED,
            engine.SMILES_DUPLICATE_BOND, engine.SMILES_RING_NUMBERS, engine.SMILES_WEDGES_DROPPED, engine.SMILES_UNKNOWN_BOND) == (
        S.FLAG_TOO_LARGE, S.FLAG_BEYOND, S.FLAG_PSEUDO, S.FLAG_TRUNCATED, S.FLAG_DUPLICATE, S.FLAG_RINGS, S.FLAG_WEDGES, S.FLAG_UNKNOWN)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    for name, bit in (("TOO_LARGE", 1), ("BEYOND_TABLES", 2), ("PSEUDO_ATOM", 4), ("TRUNCATED", 8), ("DUPLICATE_BOND", 16),
                      ("RING_NUMBERS", 32), ("WEDGES_DROPPED", 64), ("UNKNOWN_BOND", 128)):
        assert f"#define MNX_SMILES_{name} {bit}u\n" in hdr and getattr(engine, "SMILES_" + name) == bit


def test_smiles_needs_packed():
    with pytest.raises(ValueError, match="packed"):
        predict_pipeline(None, None, smiles=True)
