"""CPU: the oracle of mnx_smiles_pack_canonical (tests/canon_ref.py) against the rule's own consequences — the strings that pin
the rule (the header's examples and the two drawings of its known limit), ranks that are permutations, symmetry classes that
every automorphism respects, bytes that survive renumbering and redrawing, strings that read back to the molecule, the strip
invariants among the four sets of marks — and the binding of the new call."""
from itertools import permutations

import numpy as np
import pytest

import canon_ref as K
import ez_ref as E
import smiles_ref as S
import stereo_ref as T


def cycle(n, ty=1, first=0):
    return [(first + k, first + k + 1, ty, ty) for k in range(n - 1)] + [(first, first + n - 1, ty, ty)]


HEXAGON = [(20, 0), (30, 5), (30, 15), (20, 20), (10, 15), (10, 5)]
CHAIN3 = [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 1, 1)]
ALANINE = ([b"N", b"[C@H]", b"C", b"C", b"O", b"O"], [(10, 20), (20, 20), (25, 11), (25, 29), (20, 38), (35, 29)],
           [(0, 1, 1, 1), (1, 2, 5, 6), (1, 3, 1, 1), (3, 4, 2, 2), (3, 5, 1, 1)])
DIFLUORO = ([b"F", b"C", b"C", b"F"], [(0, 20), (10, 10), (20, 10), (30, 0)], CHAIN3)
NAPHTHALENE = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (4, 6), (6, 7), (7, 8), (8, 9), (5, 9)]
CUBE = [(0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (5, 6), (6, 7), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
SMALL_RINGS = [(50, 0), (60, 0), (55, 8), (80, 0), (90, 0), (85, 8)]
THREE_RINGS = cycle(6) + cycle(3, first=6) + cycle(3, first=9)
TIE = K.FLAG_TIE
TABLES = K.M.name_tables()
# name: (molecule, {marks: string}, flags of marks 0 [, ranks, classes])
PINNED = {
    "ethanol": (([b"O", b"C", b"C"], [(0, 0), (10, 0), (20, 0)], [(0, 1, 1, 1), (1, 2, 1, 1)]), {0: "CCO", 3: "CCO"}, 0, [2, 1, 0], [2, 1, 0]),
    "acetate": (([b"[O-]", b"C", b"O", b"C"], [(0, 0), (10, 0), (20, 0), (10, 10)], [(0, 1, 1, 1), (1, 2, 2, 2), (1, 3, 1, 1)]),
                {0: "CC(=O)[O-]", 3: "CC(=O)[O-]"}, 0),
    "alanine": (ALANINE, {0: "C[CH](C(O)=O)N", 1: "C[C@@H](C(O)=O)N", 3: "C[C@@H](C(O)=O)N"}, S.FLAG_WEDGES),
    "difluoroethene": (DIFLUORO, {0: "C(=CF)F", 2: "C(=C\\F)/F", 3: "C(=C\\F)/F"}, TIE, [2, 0, 1, 3], [2, 0, 0, 2]),
    "toluene": (([b"c"] * 6 + [b"C"], HEXAGON + [(40, 20)], cycle(6, 4) + [(2, 6, 1, 1)]), {0: "Cc1ccccc1", 3: "Cc1ccccc1"}, TIE),
    "benzene": (([b"c"] * 6, HEXAGON, cycle(6, 4)), {0: "c1ccccc1"}, TIE),
    "naphthalene": (([b"c"] * 10, [(k * 7 % 31, k * 11 % 29) for k in range(10)], [(i, j, 4, 4) for i, j in NAPHTHALENE]),
                    {0: "c1ccc2ccccc2c1"}, TIE),
    "neopentane": (([b"C"] * 5, [(10, 10), (0, 10), (20, 10), (10, 0), (10, 20)], [(0, k, 1, 1) for k in range(1, 5)]), {0: "CC(C)(C)C"}, TIE),
    "cubane": (([b"C"] * 8, [(0, 0), (10, 0), (10, 10), (0, 10), (3, 3), (13, 3), (13, 13), (3, 13)], [(i, j, 1, 1) for i, j in CUBE]),
               {0: "C12C3C4C1C1C2C3C41"}, TIE),
    # the known limit: no symmetry exchanges an atom of the six-ring with one of a three-ring, yet refinement gives all twelve
    # one class, and the drawing decides which ring is written first
    "limit, six-ring drawn first": (([b"C"] * 12, HEXAGON + SMALL_RINGS, THREE_RINGS), {0: "C1CCCCC1.C1CC1.C1CC1"}, TIE, None, [0] * 12),
    "limit, six-ring drawn last": (([b"C"] * 12, [(x + 100, y) for x, y in HEXAGON] + SMALL_RINGS, THREE_RINGS),
                                   {0: "C1CC1.C1CC1.C1CCCCC1"}, TIE, None, [0] * 12),
}


@pytest.fixture(scope="module")
def molecules():
    """the first 100 molecules of each generated set of the two marks' tests"""
    return T.generated_set(100) + E.generated_set(100)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_strings(name):
    mol, strings, flags, *more = PINNED[name]
    for marks, want in strings.items():
        text, pos, f, n_rings, rank, sym_class = K.smiles(*mol, marks)
        assert text == want and sorted(pos) == list(range(len(mol[0]))), (marks, text)
        assert f & (K.FLAG_TIE | K.FLAG_TIE_INDEX) == flags & K.FLAG_TIE and (marks or f == flags)
        if more and more[0]:
            assert rank == more[0]
        if more:
            assert sym_class == more[1]


def test_a_tie_between_two_atoms_on_one_bin_is_decided_by_the_index():
    on_one_bin = (DIFLUORO[0], [(0, 20), (10, 10), (10, 10), (30, 0)], CHAIN3)
    text, pos, flags, _, rank, sym_class = K.smiles(*on_one_bin)
    assert flags & K.FLAG_TIE and flags & K.FLAG_TIE_INDEX and rank == [2, 0, 1, 3]
    beside = (DIFLUORO[0], [(0, 20), (10, 10), (20, 10), (0, 20)], CHAIN3)      # the fluorines on one bin: once the carbons' tie is
    assert K.smiles(*beside)[2] & (K.FLAG_TIE | K.FLAG_TIE_INDEX) == K.FLAG_TIE  # broken, refinement tells them apart
    methyls = ([b"C"] * 5, [(10, 10), (0, 10), (20, 10), (20, 10), (10, 20)], [(0, k, 1, 1) for k in range(1, 5)])
    assert K.smiles(*methyls)[2] & K.FLAG_TIE_INDEX                             # the last two of the four tie on one bin
    assert not K.smiles(*DIFLUORO)[2] & K.FLAG_TIE_INDEX


def test_ranks_are_a_permutation_and_classes_coarsen_them(molecules):
    ties = 0
    for mol in molecules:
        rank, sym_class, flags = K.ranks(*mol)
        n = len(mol[0])
        assert sorted(rank) == list(range(n))
        assert bool(flags & K.FLAG_TIE) == (len(set(sym_class)) < n)
        for v in set(sym_class):                              # a class of k atoms with rank v takes the ranks v .. v+k-1
            members = [a for a in range(n) if sym_class[a] == v]
            assert sorted(rank[a] for a in members) == list(range(v, v + len(members)))
        ties += bool(flags & K.FLAG_TIE)
    assert 20 <= ties <= len(molecules) - 20                  # both kinds in numbers: at least a tenth of the molecules each


def small_graphs():
    """labelled graphs of at most 7 atoms: the symmetric ones by name, then random ones over two atom texts and two bond classes"""
    out = [([b"C"] * n, cycle(n)) for n in range(3, 8)]
    out += [([b"C"] * n, [(0, k, 1, 1) for k in range(1, n)]) for n in range(2, 8)]                     # stars
    out += [([b"C"] * n, [(k, k + 1, 1, 1) for k in range(n - 1)]) for n in range(1, 8)]                # chains
    out.append(([b"C"] * 6, cycle(3) + cycle(3, first=3) + [(k, k + 3, 1, 1) for k in range(3)]))        # prism
    out.append(([b"C"] * 4, [(i, j, 1, 1) for i in range(4) for j in range(i + 1, 4)]))                 # K4
    out.append(([b"C"] * 6, cycle(3) + cycle(3, first=3)))                                              # two triangles
    out.append(([b"C"] * 7, cycle(4) + cycle(3, first=4)))                                              # the limit's small cousin
    out.append(([b"c", b"c", b"c", b"c", b"c", b"c", b"N"], cycle(6, 4) + [(0, 6, 1, 1)]))
    out.append(([b"C", b"C", b"C", b"C", b"O", b"O"], cycle(4) + [(0, 4, 2, 2), (2, 5, 2, 2)]))
    rng = np.random.default_rng(7)
    for _ in range(60):
        n = int(rng.integers(3, 8))
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.35]
        out.append(([(b"C", b"C", b"N")[int(rng.integers(3))] for _ in range(n)], [(i, j, *[(1, 1, 2)[int(rng.integers(3))]] * 2) for i, j in pairs]))
    return out


def test_every_automorphism_maps_each_class_onto_itself():
    """brute force over all permutations of the atoms: one that keeps every atom's text and every bond with its class is an
    automorphism of the labelled bond graph, and it may move an atom only inside its symmetry class"""
    moved = 0
    for symbols, bonds in small_graphs():
        n = len(symbols)
        xy = [(3 * a, 5 * a % 7) for a in range(n)]
        rank, sym_class, _ = K.ranks(symbols, xy, bonds)
        assert sorted(rank) == list(range(n))
        have = {frozenset(b[:2]): K.BOND_CLASS[b[2]] for b in bonds}
        for p in permutations(range(n)):
            if any(symbols[p[a]] != symbols[a] for a in range(n)):
                continue
            if all(have.get(frozenset((p[i], p[j]))) == c for (i, j), c in ((tuple(k), c) for k, c in have.items())):
                assert all(sym_class[p[a]] == sym_class[a] for a in range(n)), (symbols, bonds, p)
                moved += any(p[a] != a for a in range(n))
    assert moved > 1000


def renumbered(mol, rng):
    return T.renumber(mol, [int(p) for p in rng.permutation(len(mol[0]))], rng)


def test_the_same_drawing_in_any_numbering_gives_the_same_bytes(molecules):
    """5 renumberings (atoms permuted, bond records reordered and their ends swapped) of each molecule, marks 0..3: identical
    bytes and flags whenever no tie was decided by the atom index; at most 5 % of the molecules may have that bit and be left out"""
    rng = np.random.default_rng(71)
    left_out = 0
    for mol in molecules:
        want = {marks: K.smiles(*mol, marks) for marks in range(4)}
        if want[0][2] & K.FLAG_TIE_INDEX:
            left_out += 1
            continue
        for _ in range(5):
            other = renumbered(mol, rng)
            for marks in range(4):
                got = K.smiles(*other, marks)
                assert got[0] == want[marks][0] and got[2:4] == want[marks][2:4], (marks, got[0], want[marks][0])
    assert left_out <= len(molecules) // 20


def test_redrawn_and_renumbered_molecules_give_the_same_unmarked_bytes(molecules):
    """3 copies of each molecule on new random coordinates and in a new numbering: the marks == 0 bytes are identical, no molecule
    left out (the generated sets hold none of the known limit's graphs: where atoms tie, a symmetry exchanges them)"""
    rng = np.random.default_rng(72)
    differ = 0
    for mol in molecules:
        want = K.smiles(*mol)[0]
        for _ in range(3):
            differ += K.smiles(*renumbered(K.redraw(mol, rng), rng))[0] != want
    assert differ == 0


def test_every_string_reads_back_to_the_molecule(molecules):
    """through `order`: atom a of the input is the atom at written position order[a], with its text, and the bonds between the
    written positions are the input's bonds with their symbols"""
    for mol in molecules + [PINNED[k][0] for k in sorted(PINNED)]:
        symbols, xy, bonds = mol
        text, pos = K.smiles(*mol)[:2]
        if text is None:
            continue
        atoms, read = S.read(text)
        assert len(atoms) == len(symbols) and sorted(pos) == list(range(len(symbols)))
        info = [S.atom_text(s, TABLES) for s in symbols]
        assert all(atoms[pos[a]] == info[a][0] for a in range(len(symbols)))
        want = {(min(pos[i], pos[j]), max(pos[i], pos[j])): S.bond_text(ty, info[i][1] and info[j][1]) for i, j, ty, _ in bonds}
        assert read == want


def test_strip_invariants_among_the_canonical_strings(molecules):
    for mol in molecules:
        got = {marks: K.smiles(*mol, marks) for marks in range(4)}
        if got[0][0] is None:
            continue
        assert E.strip(got[2][0]) == got[0][0] and E.strip(got[3][0]) == got[1][0]
        assert got[3][0].replace("@", "") == got[2][0] and got[1][0].replace("@", "") == got[0][0]
        assert all(got[m][1] == got[0][1] and got[m][3:] == got[0][3:] for m in (1, 2, 3))        # order, n_rings, ranks, classes


def test_pack_refuses_where_the_writer_does():
    import molfile_ref as M
    dup = (DIFLUORO[0], DIFLUORO[1], CHAIN3 + [(2, 1, 1, 1)])
    many = ([b"C"] * 102, [(k, 0) for k in range(102)], [(0, k, 1, 1) for k in range(1, 102)] + [(k, k + 1, 1, 1) for k in range(1, 101)])
    tables = M.build_tables([DIFLUORO, dup, many, ([], [], [])])
    ref = K.pack(*tables)
    assert ref["recs"]["flags"].tolist() == [K.FLAG_TIE, S.FLAG_DUPLICATE, S.FLAG_RINGS | K.FLAG_TIE, 0]
    assert ref["rank"][:4].tolist() == [2, 0, 1, 3] and ref["sym_class"][:4].tolist() == [2, 0, 0, 2]
    assert set(ref["rank"][4:8].tolist()) == set(ref["sym_class"][4:8].tolist()) == set(ref["order"][4:8].tolist()) == {K.NO_RANK}
    assert sorted(ref["rank"][8:].tolist()) == list(range(102)) and set(ref["order"][8:].tolist()) == {S.NO_POSITION}
    assert ref["out"] == b"C(=CF)F" and ref["recs"]["len"].tolist() == [7, 0, 0, 0]


def test_library_and_binding_carry_the_new_call():
    import inspect
    from molnextr_amd import engine, model
    assert "mnx_smiles_pack_canonical" in engine.SYMBOLS
    assert (engine.SMILES_CANON_TIE, engine.SMILES_CANON_TIE_INDEX) == (K.FLAG_TIE, K.FLAG_TIE_INDEX) == (8192, 16384)
    assert inspect.signature(engine.Engine.smiles_pack).parameters["canonical"].default is False
    assert inspect.signature(model.predict_pipeline).parameters["canonical"].default is False
    assert inspect.signature(model.molnextr.__init__).parameters["graph_canonical"].default is False
    with pytest.raises(ValueError, match="canonical=True needs smiles=True"):
        model.predict_pipeline(None, None, packed=True, canonical=True)
    # unpack_graphs carries the two arrays
    import molfile_ref as M
    mols, atoms, bonds, text = M.build_tables([DIFLUORO, DIFLUORO])
    rank, cls = np.array([2, 0, 1, 3] + [0xFFFF] * 4, np.uint16), np.array([2, 0, 0, 2] + [0xFFFF] * 4, np.uint16)
    preds = model.unpack_graphs(mols, atoms, bonds, text, rank=rank, sym_class=cls)
    assert preds[0]["canonical_rank"] == [2, 0, 1, 3] and preds[0]["symmetry_class"] == [2, 0, 0, 2]
    assert preds[1]["canonical_rank"] is None and preds[1]["symmetry_class"] is None
    assert "canonical_rank" not in model.unpack_graphs(mols, atoms, bonds, text)[0]
