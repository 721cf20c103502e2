"""CPU: the rule of mnx_molfile_read as the oracle of tests/molfile_read_ref.py implements it — the header's examples against tables
typed out by hand; the exact round trip through the writer's oracle (molfile_ref.molfile) on named molecules and on 2000 seeded
drawn molecules; every refusal with its line; the features of files written elsewhere; fit mode; and tools/molread_host.cpp — the
kernel's own field parsers and speller (csrc/molfile_fields.h) — under the host compiler's sanitizers against the oracle.

Reading is the inverse of the writer on what a drawing holds, NOT a projection on arbitrary tables: a plain C at which a wedge
begins comes back as [C@H], a wedge between two centres changes its owner, [nH] comes back as n. None of that is tested here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import molfile_read_ref as R
import molfile_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = M.name_tables()
DEN = 63


# ------------------------------------------------------------------------------------------------------ files typed by hand
def atom_line(sym=b"C", x=0.0, y=0.0, mass=0, code=0, v=0):
    return b"%10.4f%10.4f%10.4f %-3s%2d%3d  0  0  0%3d  0  0  0  0  0  0" % (x, y, 0.0, sym, mass, code, v)


def bond_line(a1, a2, ty=1, st=0):
    return b"%3d%3d%3d%3d" % (a1, a2, ty, st)


def molfile(atoms=(), bonds=(), props=(), counts=None, end=True, eol=b"\n"):
    counts = counts if counts is not None else b"%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (len(atoms), len(bonds))
    lines = [b"", b"  hand", b"", counts] + list(atoms) + list(bonds) + list(props) + ([b"M  END"] if end else [])
    return eol.join(lines) + eol


def read(data, **kw):
    return R.read(data, den=DEN, **kw)


def symbols(data, **kw):
    return read(data, **kw)["symbols"]


def refusal(data):
    with pytest.raises(R.Refused) as e:
        read(data)
    return e.value.flag, e.value.err_line


def test_the_header_examples():
    co = molfile([atom_line(b"C", 1.0, 2.0), atom_line(b"O")], [bond_line(1, 2)])
    got = read(co)
    # x: (2 * 10000 * 63 + 100000) // 200000 = 6; y: 63 - (2 * 20000 * 63 + 100000) // 200000 = 63 - 13
    assert got == {"symbols": [b"C", b"O"], "bins": [(6, 50), (0, 63)], "bonds": [(0, 1, 1, 1)], "flags": 0, "n_marked": 0}
    packed = R.pack([co, b""])
    assert packed["text"] == b"CO" and packed["totals"] == (2, 1, 2) and packed["mols"]["n_atoms"].tolist() == [2, 0]
    assert packed["atoms"]["sym0"].tolist() == [0, 1] and packed["atoms"]["index"].tolist() == [0, 1] and not packed["recs"]["flags"].any()
    back = read(molfile([atom_line(b"C"), atom_line(b"O")], [bond_line(2, 1, 1, 1)]))
    assert back["bonds"] == [(0, 1, 6, 5)] and back["symbols"] == [b"C", b"O"] and back["n_marked"] == 0      # the wedge begins at O
    fwd = read(molfile([atom_line(b"C"), atom_line(b"O")], [bond_line(1, 2, 1, 6)]))
    assert fwd["bonds"] == [(0, 1, 6, 5)] and fwd["symbols"] == [b"C", b"O"] and fwd["n_marked"] == 0 and fwd["flags"] == 0   # H would be 3
    mark = read(molfile([atom_line(b"C"), atom_line(b"O"), atom_line(b"N"), atom_line(b"F")], [bond_line(1, 2, 1, 6), bond_line(3, 1), bond_line(1, 4)]))
    assert mark["symbols"] == [b"[C@H]", b"O", b"N", b"F"] and mark["n_marked"] == 1 and mark["flags"] == R.H_DEFAULT
    assert mark["bonds"] == [(0, 1, 6, 5), (0, 2, 1, 1), (0, 3, 1, 1)]
    assert symbols(molfile([atom_line(b"N", v=4)], props=[b"M  CHG  1   1   1"])) == [b"[NH4+]"]
    assert read(b"") == {"symbols": [], "bins": [], "bonds": [], "flags": 0, "n_marked": 0}


# ---------------------------------------------------------------------------------------- the round trip through the writer
def roundtrip(mol, sx=M.DEFAULT_SCALE, sy=M.DEFAULT_SCALE):
    syms, xy, bonds = mol
    data, _ = M.molfile(syms, xy, bonds, sx, sy, DEN, TABLES)
    got = R.read(data, sx, sy, DEN, False)
    assert got["symbols"] == list(syms), (syms, got["symbols"], data)
    assert got["bins"] == [tuple(p) for p in xy], (xy, got["bins"])
    assert got["bonds"] == sorted(bonds), (bonds, got["bonds"])
    assert not got["flags"] & (R.CLAMPED | R.STEREO_EITHER | R.IGNORED)
    return got


def grid(n):
    return [(7 * k % 64, 11 * k % 64) for k in range(n)]


def ring(n, ty=4):
    return [(k, k + 1, ty, ty) for k in range(n - 1)] + [(0, n - 1, ty, ty)]


NAMED = {
    "alanine, the wedge from the lower atom": ([b"C", b"[C@H]", b"N", b"C", b"O", b"O"], [(0, 1, 1, 1), (1, 2, 5, 6), (1, 3, 1, 1), (3, 4, 2, 2), (3, 5, 1, 1)]),
    "alanine, the wedge from the higher atom": ([b"N", b"C", b"[C@H]", b"C", b"O", b"O"], [(0, 2, 5, 6), (1, 2, 1, 1), (2, 3, 1, 1), (3, 4, 2, 2), (3, 5, 1, 1)]),
    "four halogens, two wedges": ([b"F", b"Cl", b"[C@]", b"Br", b"I"], [(0, 2, 6, 5), (1, 2, 1, 1), (2, 3, 5, 6), (2, 4, 1, 1)]),
    "benzene": ([b"c"] * 6, ring(6)),
    "pyridine": ([b"n"] + [b"c"] * 5, ring(6)),
    "selenophene": ([b"[se]"] + [b"c"] * 4, ring(5)),
    "acetate": ([b"C", b"C", b"O", b"[O-]"], [(0, 1, 1, 1), (1, 2, 2, 2), (1, 3, 1, 1)]),
    "ammonium chloride": ([b"[NH4+]", b"[Cl-]"], []),
    "labelled methanol": ([b"[13CH3]", b"O"], [(0, 1, 1, 1)]),
    "labels": ([b"[Ph]", b"[OMe]", b"[R1]", b"[R12]", b"*", b"[Xx]", b"C"], [(k, 6, 1, 1) for k in range(6)]),
    "bracket atoms": ([b"[Fe+3]", b"[Si]", b"[2H]", b"[H]", b"[U+15]", b"[C-15]", b"[999Og]"], []),
    "nitrile, alkyne, nitro": ([b"N", b"C", b"C", b"C", b"[N+]", b"O", b"[O-]"], [(0, 1, 3, 3), (1, 2, 1, 1), (2, 3, 3, 3), (3, 4, 1, 1), (4, 5, 2, 2), (4, 6, 1, 1)]),
    "sulfone, phosphate": ([b"C", b"S", b"O", b"O", b"C", b"P", b"O", b"O", b"O", b"[O-]"],
                           [(0, 1, 1, 1), (1, 2, 2, 2), (1, 3, 2, 2), (1, 4, 1, 1), (4, 5, 1, 1), (5, 6, 2, 2), (5, 7, 1, 1), (5, 8, 1, 1), (5, 9, 1, 1)]),
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_molecules_come_back_exactly(name):
    syms, bonds = NAMED[name]
    got = roundtrip((syms, grid(len(syms)), bonds), 150000, 64)
    assert got["n_marked"] == sum(s in M.CHIRAL_CARBONS for s in syms)


UPPER = [b"C", b"C", b"C", b"N", b"O", b"S", b"P", b"F", b"Cl", b"Br", b"I", b"B", b"*", b"[Si]", b"[Na+]", b"[O-]", b"[N+]", b"[13C]", b"[2H]",
         b"[NH3+]", b"[CH2]", b"[Ph]", b"[OMe]", b"[R1]", b"[R12]", b"[Xx]", b"[Fe+2]", b"[S-2]", b"[15NH2]", b"[*+]"]
LOWER = [b"c", b"c", b"c", b"n", b"o", b"s", b"p", b"b", b"[se]", b"[as]", b"[n+]", b"[o+]"]


def drawn_molecule(rng):
    """A drawing as the issue defines it: a tree plus ring closures, 1..40 atoms, degree <= 4; lower-case atoms on class-4 bonds
    among themselves only; wedges from [C@H] (three single bonds) or [C@] (four) to a neighbour that is no centre"""
    n = int(rng.integers(1, 41))
    degree, pairs = [0] * n, []
    for k in range(1, n):
        free = [p for p in range(k) if degree[p] < 4]
        if not free:
            break
        p = free[int(rng.integers(0, len(free)))]
        pairs.append((p, k))
        degree[p] += 1
        degree[k] += 1
    n = 1 + len(pairs) if len(pairs) < n - 1 else n
    for _ in range(int(rng.integers(0, 4))):
        i, j = sorted(int(v) for v in rng.integers(0, n, 2))
        if i != j and (i, j) not in pairs and degree[i] < 4 and degree[j] < 4:
            pairs.append((i, j))
            degree[i] += 1
            degree[j] += 1
    wants_lower = rng.random(n) < 0.35
    types = {}
    for i, j in pairs:
        types[(i, j)] = 4 if wants_lower[i] and wants_lower[j] else int(rng.choice([1, 1, 1, 1, 1, 2, 2, 3]))
    is_lower = [any(t == 4 and k in p for p, t in types.items()) for k in range(n)]
    syms = [LOWER[int(rng.integers(0, len(LOWER)))] if is_lower[k] else UPPER[int(rng.integers(0, len(UPPER)))] for k in range(n)]
    nbrs = {k: [(p, q) for p, q in pairs if k in (p, q)] for k in range(n)}
    blocked, centre = set(), set()
    classes = {p: (t, t) for p, t in types.items()}
    for k in range(n):
        mine = nbrs[k]
        if k in blocked or is_lower[k] or len(mine) not in (3, 4) or any(types[p] != 1 for p in mine) or rng.random() < 0.5:
            continue
        others = [p for p in mine if (p[0] if p[1] == k else p[1]) not in centre]
        if not others:
            continue
        centre.add(k)
        syms[k] = b"[C@H]" if len(mine) == 3 else b"[C@]"
        for p in [others[int(z)] for z in rng.choice(len(others), min(len(others), int(rng.integers(1, 3))), replace=False)]:
            cls = int(rng.choice([5, 6]))
            classes[p] = (cls, 11 - cls) if p[0] == k else (11 - cls, cls)
            blocked.add(p[0] if p[1] == k else p[1])
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (n, 2))]
    return syms, xy, [(i, j) + classes[(i, j)] for i, j in pairs]


def test_2000_drawn_molecules_come_back_exactly():
    rng = np.random.default_rng(2000)
    centres = aromatic = 0
    for _ in range(2000):
        mol = drawn_molecule(rng)
        sx, sy = (int(v) for v in rng.integers(64, 10000001, 2))
        got = roundtrip(mol, sx, sy)
        centres += got["n_marked"]
        aromatic += sum(b[2] == 4 for b in mol[2])
        assert got["n_marked"] == sum(s in M.CHIRAL_CARBONS for s in mol[0])
    assert centres > 300 and aromatic > 1500, (centres, aromatic)


# --------------------------------------------------------------------------------------------------------------- refusals
C2 = [atom_line(b"C"), atom_line(b"O")]
C3 = C2 + [atom_line(b"N")]
REFUSALS = {
    "V3000": (molfile(counts=b"  0  0  0  0  0  0  0  0  0  0999 V3000"), R.SYNTAX, 4),
    "counts are no number": (molfile(counts=b"  x  0"), R.SYNTAX, 4),
    "an inner blank in a count": (molfile(counts=b"1 2  0"), R.SYNTAX, 4),
    "a negative count": (molfile(counts=b" -1  0"), R.SYNTAX, 4),
    "no M  END": (molfile(C2, end=False), R.SYNTAX, 7),
    "two lines": (b"a\nb\n", R.SYNTAX, 3),
    "M  END as line 2": (b"a\nM  END\nc\nd\ne\n", R.SYNTAX, 3),
    "M  END as the counts line": (b"a\nb\nc\nM  END\n", R.SYNTAX, 4),
    "empty lines only": (b"\n" * 5, R.SYNTAX, 6),
    "an atom line of 30 bytes": (molfile([atom_line(b"C"), atom_line(b"C")[:30]]), R.SYNTAX, 6),
    "two dots in x": (molfile([b"   1.0.000" + atom_line(b"C")[10:]]), R.SYNTAX, 5),
    "a blank x": (molfile([b" " * 10 + atom_line(b"C")[10:]]), R.SYNTAX, 5),
    "a blank behind y": (molfile([atom_line(b"C")[:10] + b"   1.000  " + atom_line(b"C")[20:]]), R.SYNTAX, 5),
    "charge code 8": (molfile([atom_line(b"C", code=8)]), R.SYNTAX, 5),
    "valence 16": (molfile([atom_line(b"C", v=16)]), R.SYNTAX, 5),
    "valence -1": (molfile([atom_line(b"C", v=-1)]), R.SYNTAX, 5),
    "a mass difference that is no number": (molfile([atom_line(b"C")[:34] + b" x" + atom_line(b"C")[36:]]), R.SYNTAX, 5),
    "a missing atom line": (molfile(C2, counts=b"  3  0"), R.SYNTAX, 7),
    "a missing bond line": (molfile(C2, [bond_line(1, 2)], counts=b"  2  2"), R.SYNTAX, 8),
    "bond from atom 0": (molfile(C2, [bond_line(0, 2)]), R.SYNTAX, 7),
    "bond beyond the atoms": (molfile(C2, [bond_line(1, 3)]), R.SYNTAX, 7),
    "bond to itself": (molfile(C2, [bond_line(2, 2)]), R.SYNTAX, 7),
    "bond type 0": (molfile(C2, [bond_line(1, 2, 0)]), R.SYNTAX, 7),
    "bond type 9": (molfile(C2, [bond_line(1, 2, 9)]), R.SYNTAX, 7),
    "a query bond": (molfile(C2, [bond_line(1, 2, 5)]), R.QUERY, 7),
    "query type 8": (molfile(C3, [bond_line(1, 2), bond_line(2, 3, 8)]), R.QUERY, 9),
    "stereo 2": (molfile(C2, [bond_line(1, 2, 1, 2)]), R.SYNTAX, 7),
    "a wedge on a double bond": (molfile(C2, [bond_line(1, 2, 2, 1)]), R.SYNTAX, 7),
    "stereo 3 on a single bond": (molfile(C2, [bond_line(1, 2, 1, 3)]), R.SYNTAX, 7),
    "stereo 4 on a double bond": (molfile(C2, [bond_line(1, 2, 2, 4)]), R.SYNTAX, 7),
    "a wedge on a query bond": (molfile(C2, [bond_line(1, 2, 5, 1)]), R.SYNTAX, 7),
    "the same pair twice": (molfile(C3, [bond_line(1, 2), bond_line(2, 3), bond_line(1, 2, 2)]), R.SYNTAX, 10),
    "the same pair the other way round": (molfile(C3, [bond_line(1, 2), bond_line(2, 1)]), R.SYNTAX, 9),
    "alias of atom 0": (molfile(C2, props=[b"A    0", b"x"]), R.SYNTAX, 7),
    "alias beyond the atoms": (molfile(C2, props=[b"A    3", b"x"]), R.SYNTAX, 7),
    "alias of 71 bytes": (molfile(C2, props=[b"A    1", b"x" * 71]), R.SYNTAX, 8),
    "alias without a line": (molfile(C2, props=[b"M  ISO  1   1  13", b"A    1"]), R.SYNTAX, 8),
    "CHG count 0": (molfile(C2, props=[b"M  CHG  0"]), R.SYNTAX, 7),
    "CHG count 9": (molfile(C2, props=[b"M  CHG  9" + b"   1   1" * 9]), R.SYNTAX, 7),
    "CHG atom 0": (molfile(C2, props=[b"M  CHG  1   0   1"]), R.SYNTAX, 7),
    "CHG 16": (molfile(C2, props=[b"M  CHG  1   1  16"]), R.SYNTAX, 7),
    "ISO -1": (molfile(C2, props=[b"M  ISO  1   1  -1"]), R.SYNTAX, 7),
    "RGP atom beyond": (molfile(C2, props=[b"M  CHG  1   1   1", b"M  RGP  1   3   1"]), R.SYNTAX, 8),
    "QUERY in front of SYNTAX": (molfile(C3, [bond_line(1, 2, 6), bond_line(2, 3, 9)]), R.QUERY, 8),
    "SYNTAX in front of QUERY": (molfile(C3, [bond_line(1, 2, 9), bond_line(2, 3, 6)]), R.SYNTAX, 8),
    "SYNTAX and QUERY on one line": (molfile(C3, [bond_line(1, 2), bond_line(1, 2, 7)]), R.SYNTAX, 9),
    "an atom line and a property": (molfile([atom_line(b"C", code=9), atom_line(b"C")], props=[b"M  CHG  0"]), R.SYNTAX, 5),
    "262145 bytes": (b"x" * 100 + b"\n" + b"y" * 262044, R.TOO_LARGE, 0),
    "8193 lines": (b"\n" * 8193, R.TOO_LARGE, 0),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_with_its_line(name):
    data, flag, line = REFUSALS[name]
    assert refusal(data) == (flag, line)
    packed = R.pack([molfile(C2), data, molfile(C2)])
    assert packed["recs"]["flags"].tolist() == [0, flag, 0] and packed["recs"]["err_line"].tolist() == [0, line, 0]
    assert packed["mols"]["n_atoms"].tolist() == [2, 0, 2] and packed["mols"]["atom0"].tolist() == [0, 2, 2]


def test_the_limits_themselves_are_admitted():
    assert read(b"\n" * 8187 + molfile())["symbols"] == []                          # "M  END" is line 8192
    assert refusal(b"\n" * 8188 + molfile(end=False)) == (R.SYNTAX, 8193)           # 8192 lines, none of them "M  END"
    assert refusal(b"\n" * 8188 + molfile()) == (R.TOO_LARGE, 0)                    # "M  END" is line 8193
    body = molfile(C2)
    assert len(read(body + b"x" * (262144 - len(body)))["symbols"]) == 2


# ------------------------------------------------------------------------------------------------ files written elsewhere
FOREIGN = {
    "CRLF": (molfile(C2, [bond_line(1, 2, 2)], eol=b"\r\n"), [b"C", b"O"], 0),
    "atom lines of 34 bytes": (molfile([atom_line(b"Cl")[:34], atom_line(b"C")[:31]]), [b"Cl", b"*"], 0),
    "atom-block charges": (molfile([atom_line(b"N", code=3), atom_line(b"O", code=5), atom_line(b"Fe", code=1), atom_line(b"C", code=4)]),
                           [b"[NH4+]", b"[OH-]", b"[Fe+3]", b"C"], R.H_DEFAULT | R.IGNORED),
    "the M CHG reset": (molfile([atom_line(b"N", code=3), atom_line(b"O", code=5)], props=[b"M  CHG  1   2   1"]), [b"N", b"[OH3+]"], R.H_DEFAULT),
    "D and T": (molfile([atom_line(b"D"), atom_line(b"T"), atom_line(b"D")], props=[b"M  ISO  1   3   1"]), [b"[2H]", b"[3H]", b"[1H]"], R.H_DEFAULT),
    "a label in the symbol column": (molfile([atom_line(b"Ph"), atom_line(b"Xyz"), atom_line(b"c")]), [b"[Ph]", b"[Xyz]", b"[c]"], R.LABEL),
    "v = 15": (molfile([atom_line(b"C", v=15), atom_line(b"N", v=15)], [bond_line(1, 2)]), [b"[C]", b"[N]"], 0),
    "the later entry wins": (molfile(C3, props=[b"M  CHG  2   1   1   1  -1", b"M  CHG  1   2   2", b"M  CHG  1   2   0", b"A    3", b"first",
                                                  b"A    3", b"second"]), [b"[CH3-]", b"O", b"[second]"], R.H_DEFAULT | R.LABEL),
    "an alias that looks like a property": (molfile(C2, props=[b"A    1", b"A    2", b"A    2", b"M  CHG  1   1   1"]), [b"[A    2]", b"[M  CHG  1   1   1]"], R.LABEL),
    "an empty alias": (molfile(C2, props=[b"A    1", b"Me", b"A    1", b""]), [b"C", b"O"], 0),
    "control bytes in an alias": (molfile(C2, props=[b"A    2", b"a\x01\x7f\xc5\x95"]), [b"C", b"[a??\xc5\x95]"], R.LABEL),
    "either stereo": (molfile(C3, [bond_line(1, 2, 1, 4), bond_line(2, 3, 2, 3)]), [b"C", b"O", b"N"], R.STEREO_EITHER),
    "skipped lines": (molfile(C2, props=[b"M  STY  1   1 SUP", b"G    1", b"", b"V    1 x"]), [b"C", b"O"], R.IGNORED),
    "a mass difference": (molfile([atom_line(b"C", mass=1)]), [b"C"], R.IGNORED),
    "text behind M  END": (molfile(C2) + b">  <NAME>\nwhatever  9  9\n\n$$$$\nA    9\n", [b"C", b"O"], 0),
    "no newline at the end": (molfile(C2)[:-1], [b"C", b"O"], 0),
    "an R group": (molfile([atom_line(b"R#"), atom_line(b"R#"), atom_line(b"R")], props=[b"M  RGP  1   1  12"]), [b"[R12]", b"*", b"*"], R.LABEL),
    "H above 9": (molfile([atom_line(b"C", v=14)]), [b"[CH9]"], 0),
    "an isotope and a charge of two": (molfile([atom_line(b"O")], props=[b"M  ISO  1   1  18", b"M  CHG  1   1  -2"]), [b"[18O-2]"], R.H_DEFAULT),
}
# one H_DEFAULT case per row of the table: (symbol, charge, bonds to plain carbons as bond types) -> the spelling with an isotope
H_ROWS = [(b"B", 0, [1], b"[11BH2]"), (b"C", 0, [2], b"[11CH2]"), (b"N", 0, [1], b"[11NH2]"), (b"N", 0, [2, 2], b"[11NH]"), (b"O", 0, [1], b"[11OH]"),
          (b"P", 0, [2, 1, 1], b"[11PH]"), (b"P", 0, [2, 2, 1], b"[11P]"), (b"P", 0, [], b"[11PH3]"), (b"S", 0, [1], b"[11SH]"), (b"S", 0, [2, 1], b"[11SH]"), (b"S", 0, [2, 2, 1], b"[11SH]"),
          (b"S", 0, [2, 2, 2, 1], b"[11S]"), (b"F", 0, [], b"[11FH]"), (b"Cl", 0, [], b"[11ClH]"), (b"Br", 0, [1], b"[11Br]"), (b"I", 0, [], b"[11IH]"),
          (b"N", 1, [1], b"[11NH3+]"), (b"P", 1, [], b"[11PH4+]"), (b"O", 1, [1], b"[11OH2+]"), (b"S", 1, [], b"[11SH3+]"), (b"C", 1, [1], b"[11CH2+]"),
          (b"C", -1, [], b"[11CH3-]"), (b"N", -1, [], b"[11NH2-]"), (b"O", -1, [], b"[11OH-]"), (b"S", -1, [1], b"[11S-]"), (b"B", -1, [], b"[11BH4-]"),
          (b"Si", 0, [], b"[11Si]"), (b"N", 2, [], b"[11N+2]")]


@pytest.mark.parametrize("name", sorted(FOREIGN))
def test_files_written_elsewhere(name):
    data, want, flags = FOREIGN[name]
    got = read(data)
    assert got["symbols"] == want and got["flags"] == flags


def h_row_file(sym, charge, types):
    atoms = [atom_line(sym)] + [atom_line(b"C")] * len(types)
    props = [b"M  ISO  1   1  11"] + ([b"M  CHG  1   1%4d" % charge] if charge else [])
    return molfile(atoms, [bond_line(1, k + 2, t) for k, t in enumerate(types)], props)


@pytest.mark.parametrize("row", H_ROWS, ids=lambda r: r[3].decode())
def test_default_hydrogens_row_by_row(row):
    sym, charge, types, want = row
    got = read(h_row_file(sym, charge, types))
    assert got["symbols"][0] == want and got["flags"] == R.H_DEFAULT


def test_bins_are_clamped_without_fit_and_the_writer_is_inverted():
    got = read(molfile([atom_line(b"C", -0.5, 0.0), atom_line(b"C", 11.0, 10.0), atom_line(b"C", 10.0, -1.0)]))
    assert got["bins"] == [(0, 63), (63, 0), (63, 63)] and got["flags"] == R.CLAMPED
    for s in (64, 65, 999, 100000, 10000000):
        for xb in (0, 1, 31, 62, 63):
            ux, uy = M.units(xb, 63 - xb, s, s, DEN)
            assert read(molfile([atom_line(b"C", ux / 10000, uy / 10000)]), sx=s, sy=s)["bins"] == [(xb, 63 - xb)]


# --------------------------------------------------------------------------------------------------------------------- fit
FIT = {
    "negative coordinates": ([(-2.0, -1.0), (0.0, 1.0), (2.0, -1.0)], [(0, 63), (32, 31), (63, 63)]),
    "equal spans": ([(0.0, 0.0), (1.5, 1.5), (0.75, 0.3)], [(0, 63), (63, 0), (32, 50)]),
    "one atom": ([(3.25, -7.5)], [(0, 63)]),
    "a wide molecule": ([(0.0, 0.0), (10.0, 1.0), (5.0, 0.5)], [(0, 63), (63, 57), (32, 60)]),
    "a tall molecule": ([(0.0, 0.0), (1.0, 10.0), (0.5, 5.0)], [(0, 63), (6, 0), (3, 31)]),
}


@pytest.mark.parametrize("name", sorted(FIT))
def test_fit(name):
    xy, want = FIT[name]
    got = read(molfile([atom_line(b"C", x, y) for x, y in xy]), fit=True)
    assert got["bins"] == want and not got["flags"] & R.CLAMPED


# -------------------------------------------------------------------------------- the kernel's serial code under the sanitizers
def all_inputs():
    """every file of this module with the way it is read: (data, fit, sx, sy)"""
    out = [(d, False, 100000, 100000) for d, _, _ in REFUSALS.values()] + [(d, False, 100000, 100000) for d, _, _ in FOREIGN.values()]
    out += [(h_row_file(s, q, t), False, 100000, 100000) for s, q, t, _ in H_ROWS]
    out += [(molfile([atom_line(b"C", x, y) for x, y in xy]), True, 100000, 100000) for xy, _ in FIT.values()]
    out += [(M.molfile(s, grid(len(s)), b, 150000, 64, DEN, TABLES)[0], False, 150000, 64) for s, b in NAMED.values()]
    rng = np.random.default_rng(7)
    for _ in range(200):
        sx, sy = (int(v) for v in rng.integers(64, 10000001, 2))
        out.append((M.molfile(*drawn_molecule(rng), sx, sy, DEN, TABLES)[0], False, sx, sy))
    out += [(b"", False, 1, 1), (molfile([atom_line(b"C", 99999.9999, -9999.0)] * 3), True, 1, 1), (molfile([atom_line(b"C", 99999.9999, 5.0)]), False, 1, 10000000)]
    return out


def expected_output(data, fit, sx, sy):
    try:
        got = R.read(data, sx, sy, DEN, fit)
    except R.Refused as e:
        return ["%d %d 0 0 0" % (e.flag, e.err_line)]
    lines = ["%d 0 %d %d %d" % (got["flags"], got["n_marked"], len(got["symbols"]), len(got["bonds"]))]
    lines += ["%d %d %s" % (x, y, s.hex()) for s, (x, y) in zip(got["symbols"], got["bins"])]
    return lines + ["%d %d %d %d" % b for b in got["bonds"]]


def test_the_fields_header_under_the_sanitizers(tmp_path):
    """tools/molread_host.cpp — a sequential reader around csrc/molfile_fields.h — built with -fsanitize=address,undefined and run
    once, as a plain executable, over every input of this file: its tables are the oracle's and the sanitizers report nothing (a
    report ends the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "molread_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "molread_host.cpp"), "-o", exe], check=True)
    cases = all_inputs()
    text = b"%d\n" % len(cases) + b"".join(b"%d %d %d %d %d\n" % (fit, sx, sy, DEN, len(d)) + d + b"\n" for d, fit, sx, sy in cases)
    run = subprocess.run([exe], input=text, capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.decode().split("\n")
    at = 0
    for k, case in enumerate(cases):
        want = expected_output(*case)
        assert got[at:at + len(want)] == want, (k, case[0][:300], got[at:at + 3], want[:3])
        at += len(want)
    assert got[at:] == [""]


# ------------------------------------------------------------------------------------------------- the header and the engine
def test_the_header_declares_the_call_and_the_library_exports_it():
    from molnextr_amd import engine
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    assert "int mnx_molfile_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n," in hdr
    for name in ("SYNTAX 1u", "TOO_LARGE 2u", "BEYOND 8u", "QUERY 16u", "STEREO_EITHER 32u", "H_DEFAULT 64u", "CLAMPED 128u", "IGNORED 256u", "LABEL 512u"):
        assert "#define MNX_MOLREAD_" + name in hdr
    assert "#define MNX_ABI_VERSION 7" in hdr
    assert engine.MOLREAD_DTYPE == R.MOLREAD_DTYPE and engine.MOLREAD_DTYPE.itemsize == 16 and engine.MOLREAD_REFUSED == R.REFUSED
    if not os.path.exists(engine.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = engine.load_library()
    assert "mnx_molfile_read" in engine.SYMBOLS and hasattr(lib, "mnx_molfile_read") and len(lib.mnx_molfile_read.argtypes) == 17
    assert lib.mnx_molfile_read(None, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None) == -1


def test_split_sdf():
    from molnextr_amd.model import split_sdf
    a, b = molfile(C2), molfile(C3, eol=b"\r\n")
    assert split_sdf(a + b">  <ID>\n1\n\n$$$$\n" + b + b"$$$$\r\n" + a) == [a + b">  <ID>\n1\n\n", b, a]
    assert split_sdf(a) == [a] and split_sdf(b"") == [] and split_sdf(a + b"$$$$\n") == [a] and split_sdf(a + b"$$$$") == [a]
    assert split_sdf((a + b"$$$$\n").decode()) == [a]
    assert [R.read(x)["symbols"] for x in split_sdf(a + b"$$$$\n" + b)] == [[b"C", b"O"], [b"C", b"O", b"N"]]
