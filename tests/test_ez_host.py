"""CPU: the oracle of mnx_smiles_pack_marks (tests/ez_ref.py) against the strings that pin the rule of '/' and '\\', its reader
(cis or trans from the string by the OpenSMILES wording, from the drawing through angles) against its writer over generated
molecules and under renumbering, what the generated set covers, every case of the three flags, the strip invariants against the
oracles of the two older calls; and the binding of the new call."""
import ctypes
import os

import numpy as np
import pytest

import ez_ref as E
import molfile_ref as M
import smiles_ref as S
import stereo_ref as T
from molnextr_amd import engine
from molnextr_amd.model import predict_pipeline

DIFLUORO = [b"F", b"C", b"C", b"F"]
CHAIN3 = [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 1, 1)]
RING = [(0, 10), (10, 10), (20, 0), (30, 0), (40, 10), (30, 20), (20, 20), (0, 0)]

# name: (symbols, (x_bin, y_bin), bonds (i, j, type, rev), the string, flags) — the table of the rule (include/molnextr_hip.h)
PINNED = {
    "trans": (DIFLUORO, [(0, 20), (10, 10), (20, 10), (30, 0)], CHAIN3, "F/C=C/F", E.FLAG_EZ),
    "cis": (DIFLUORO, [(0, 20), (10, 10), (20, 10), (30, 20)], CHAIN3, "F/C=C\\F", E.FLAG_EZ),
    "conjugated": ([b"C"] * 6, [(0, 20), (10, 10), (20, 20), (30, 10), (40, 20), (50, 10)],
                   [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 1, 1), (3, 4, 2, 2), (4, 5, 1, 1)], "C/C=C/C=C/C", E.FLAG_EZ),
    "exocyclic": ([b"C"] * 7 + [b"F"], RING, [(0, 1, 2, 2), (1, 2, 1, 1), (2, 3, 1, 1), (3, 4, 1, 1), (4, 5, 1, 1), (5, 6, 1, 1), (1, 6, 1, 1),
                                               (0, 7, 1, 1)], "C(=C1/CCCCC1)/F", E.FLAG_EZ),
}
ZIGZAG = [(0, 20), (10, 10), (20, 20), (30, 10), (40, 20), (50, 10), (60, 20), (70, 10)]
TRIENE = [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 1, 1), (3, 4, 2, 2), (4, 5, 1, 1), (5, 6, 2, 2), (6, 7, 1, 1)]

# name: (molecule, the string of marks == 2, its flags)
FLAG_CASES = {
    # a symmetric double bond is marked like any other: no symmetry check
    "no symmetry check": (([b"F", b"C", b"F", b"C", b"F", b"F"], [(0, 20), (10, 10), (0, 0), (20, 10), (30, 0), (30, 20)],
                           [(0, 1, 1, 1), (1, 2, 1, 1), (1, 3, 2, 2), (3, 4, 1, 1), (3, 5, 1, 1)]), "F/C(/F)=C(/F)\\F", E.FLAG_EZ),
    # a substituent on the line of the double bond: unresolved, bit 11 alone
    "zero side": ((DIFLUORO, [(0, 10), (10, 10), (20, 10), (30, 0)], CHAIN3), "FC=CF", E.FLAG_EZ_UNRESOLVED),
    # two substituents of one end on one side: unresolved
    "same side": (([b"F", b"C", b"C", b"F", b"Cl"], [(0, 20), (10, 10), (20, 10), (30, 0), (32, 2)], CHAIN3 + [(2, 4, 1, 1)]),
                  "FC=C(F)Cl", E.FLAG_EZ_UNRESOLVED),
    # an end without a substituent, three further bonds, a triple bond beside it, a pseudo-atom end: no candidates, no bits
    "bare end": (([b"F", b"C", b"C"], [(0, 20), (10, 10), (20, 10)], CHAIN3[:2]), "FC=C", 0),
    "a bond that is not single": (([b"N", b"C", b"C", b"F"], [(0, 20), (10, 10), (20, 10), (30, 0)], [(0, 1, 3, 3)] + CHAIN3[1:]), "N#C=CF", 0),
    "pseudo-atom end": (([b"F", b"R", b"C", b"F"], [(0, 20), (10, 10), (20, 10), (30, 0)], CHAIN3), "F*=CF", S.FLAG_PSEUDO),
    # wedges count as single bonds: the candidate resolves, the wedge itself is dropped (bit 6)
    "wedge substituent": ((DIFLUORO, [(0, 20), (10, 10), (20, 10), (30, 0)], [(0, 1, 5, 6)] + CHAIN3[1:]), "F/C=C/F", E.FLAG_EZ | S.FLAG_WEDGES),
    # a double bond on a cycle is left alone, its neighbours too
    "on a cycle": (([b"C"] * 4, [(0, 0), (10, 0), (10, 10), (0, 10)], [(0, 1, 2, 2), (1, 2, 1, 1), (2, 3, 1, 1), (0, 3, 1, 1)]), "C1=CCC1", 0),
    # the middle double bond of a triene does not resolve (its end 3 has a second substituent on the same side): the outer two
    # are marked, a reader would read the middle one too: bits 10, 11, 12
    "implied": (([b"C"] * 9, ZIGZAG + [(22, 24)], TRIENE + [(3, 8, 1, 1)]), "C/C=C/C(=C/C=C/C)C", E.FLAG_EZ | E.FLAG_EZ_UNRESOLVED | E.FLAG_EZ_IMPLIED),
    # one resolves, one does not, nothing implied: bits 10 and 11
    "resolved beside unresolved": (([b"C"] * 6, ZIGZAG[:4] + [(40, 10), (50, 10)], TRIENE[:5]), "C/C=C/C=CC", E.FLAG_EZ | E.FLAG_EZ_UNRESOLVED),
    # between aromatic atoms the symbol replaces the '-'
    "aromatic ends": (([b"c", b"c", b"c", b"c"], [(0, 20), (10, 10), (20, 10), (30, 0)], CHAIN3), "c/c=c/c", E.FLAG_EZ),
    # refused (the pair 1 2 twice): no bit of the three
    "refused": ((DIFLUORO, PINNED["trans"][1], CHAIN3 + [(2, 1, 1, 1)]), "", S.FLAG_DUPLICATE),
}


@pytest.fixture(scope="module")
def generated():
    mols = E.generated_set()
    return mols, [E.smiles(*m, 2) for m in mols], [E.smiles(*m, 3) for m in mols]


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_strings(name):
    syms, xy, bonds, want, flags = PINNED[name]
    for marks in (2, 3):
        got = E.pack(*M.build_tables([(syms, xy, bonds)]), marks)
        assert got["out"].decode() == want and got["recs"]["flags"][0] == flags and got["recs"]["len"][0] == len(want)
    plain = S.pack(*M.build_tables([(syms, xy, bonds)]))
    assert E.strip(want) == want.replace("/", "").replace("\\", "") == plain["out"].decode() and got["order"].tolist() == plain["order"].tolist()
    text, pos, _, _, what = E.smiles(syms, xy, bonds)
    back = E.read_back(text, pos, xy)
    assert sorted(map(sorted, back)) == sorted(sorted(k) for k, c in what["candidates"].items() if c["resolved"]) and back
    for pairs in back.values():
        assert all(cis == drawn for _, _, cis, drawn in pairs)


def test_the_two_difluoroethenes_read_as_trans_and_cis():
    assert E.configurations("F/C=C/F") == {(1, 2): {(0, 3): False}} and E.configurations("F/C=C\\F") == {(1, 2): {(0, 3): True}}
    assert E.configurations("F\\C=C\\F") == {(1, 2): {(0, 3): False}} and E.configurations("C(\\F)=C/F") == {(0, 2): {(1, 3): False}}
    assert E.configurations("C(=C1/CCCCC1)/F") == {(0, 1): {(7, 2): True}} and E.configurations("FC=C/F") == {}
    assert E.configurations("F/C(\\Cl)=C/F") == {(1, 3): None}             # both substituents of one end below it


@pytest.mark.parametrize("name", sorted(FLAG_CASES))
def test_flag_cases(name):
    mol, want, flags = FLAG_CASES[name]
    got = E.pack(*M.build_tables([mol]), 2)
    assert got["out"].decode() == want and got["recs"]["flags"][0] == flags, (name, got["out"], got["recs"])
    assert (got["recs"]["len"][0] == 0) == (name == "refused")
    for marks, ref in ((0, S.pack), (1, T.pack)):        # without the double-bond bit: the older calls, none of the three bits
        old = E.pack(*M.build_tables([mol]), marks)
        assert old["out"] == ref(*M.build_tables([mol]))["out"] and not old["recs"]["flags"][0] & 0x1C00
        assert old["recs"].tobytes() == ref(*M.build_tables([mol]))["recs"].tobytes()


def test_reader_agrees_with_writer_over_generated_molecules(generated):
    """every resolved candidate is read back as a marked double bond whose cis / trans is the drawing's, for every pair of its
    directed substituents; a marked double bond that is no resolved candidate appears exactly where bit 12 says so; no ring
    bond is directed (read() refuses one)"""
    marked = pairs_seen = 0
    for (syms, xy, bonds), (text, pos, flags, n_rings, what), _ in zip(*generated):
        if text is None:
            continue
        back = E.read_back(text, pos, xy)
        resolved = {frozenset(k) for k, c in what["candidates"].items() if c["resolved"]}
        assert resolved <= set(back), (text, resolved - set(back))
        assert bool(flags & E.FLAG_EZ_IMPLIED) == bool(set(back) - resolved), text
        assert bool(flags & E.FLAG_EZ) == ("/" in text or "\\" in text) == bool(what["directed"])
        assert bool(flags & E.FLAG_EZ_UNRESOLVED) == any(not c["resolved"] for c in what["candidates"].values())
        for bond in resolved:
            assert back[bond] is not None, (text, bond)
            for x, y, cis, drawn in back[bond]:
                assert drawn is not None and cis == drawn, (text, bond, x, y)
                pairs_seen += 1
            marked += 1
    assert marked > 700 and pairs_seen > marked


def test_generated_set_covers_the_ground(generated):
    mols = generated[0]
    c = E.coverage(mols)
    print(c)
    assert len(mols) == 300 and all(6 <= len(m[0]) <= 60 for m in mols)
    for k, v in c.items():
        assert v >= 20, (k, c)
    assert c["/"] >= 300 and c["\\"] >= 300 and c["resolved"] >= 500
    assert sum(g[0] is None for g in generated[1]) == 0


def test_renumbering_keeps_every_configuration(generated):
    """20 random renumberings of every molecule: the same double bonds resolve, and each one's configuration as the reader takes
    it from the string alone, carried over to the lowest-numbered substituent of each end of the original numbering, is
    unchanged. (Which double bonds are merely IMPLIED depends on which bonds of a cycle the walk makes ring bonds: bit 12.)"""
    rng = np.random.default_rng(32)
    checked = 0
    for (syms, xy, bonds), (text, pos, _, _, what), _ in zip(*generated):
        resolved = {frozenset(k) for k, c in what["candidates"].items() if c["resolved"]}
        first = {bond: E.named(bonds, bond, pairs) for bond, pairs in E.read_back(text, pos, xy).items() if bond in resolved}
        for _ in range(20):
            perm = [int(p) for p in rng.permutation(len(syms))]
            inverse = {p: a for a, p in enumerate(perm)}
            s2, xy2, b2 = T.renumber((syms, xy, bonds), perm, rng)
            t2, pos2, _, _, w2 = E.smiles(s2, xy2, b2)
            again = {frozenset(inverse[u] for u in k) for k, c in w2["candidates"].items() if c["resolved"]}
            assert again == resolved, (text, t2)
            for bond, pairs in E.read_back(t2, pos2, xy2).items():
                here = frozenset(inverse[u] for u in bond)
                if here in resolved:
                    moved = [(inverse[x], inverse[y], cis) for x, y, cis, _ in pairs]
                    assert E.named(bonds, here, moved) == first[here], (text, t2, here)
                    checked += 1
    assert checked > 10000


def test_strip_invariants_against_the_older_oracles(generated):
    """without '/' and '\\' (E.strip: a '-' they replaced between aromatic atoms put back) marks == 2 is the plain writer and
    marks == 3 the stereo writer, without '@' marks == 3 is marks == 2; order, n_rings and flag bits 0-9 are theirs"""
    strip = E.strip
    for (syms, xy, bonds), two, three in zip(*generated):
        plain, stereo = S.smiles(syms, bonds), T.smiles(syms, xy, bonds)
        assert (strip(two[0]), two[1], two[2] & 0x3FF, two[3]) == plain
        assert (strip(three[0]), three[1], three[2] & 0x3FF, three[3]) == stereo[:4]
        assert three[0].replace("@", "") == two[0] and (two[2] & 0x1C00) == (three[2] & 0x1C00)
        assert len(S.read(strip(two[0]))[0]) == len(syms)
    assert sum("@" in g[0] for g in generated[2]) > 50


def test_library_and_binding_carry_the_new_call():
    lib = engine.load_library()
    assert "mnx_smiles_pack_marks" in engine.SYMBOLS and hasattr(lib, "mnx_smiles_pack_marks")
    args = lib.mnx_smiles_pack_marks.argtypes
    assert list(args[:14]) == list(lib.mnx_smiles_pack.argtypes[:14]) and args[14] is ctypes.c_uint32 and len(args) == 16
    assert lib.mnx_smiles_pack_marks(None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 3, None) == -1
    assert lib.mnx_abi_version() == engine.ABI_VERSION == 7
    assert (engine.SMILES_EZ, engine.SMILES_EZ_UNRESOLVED, engine.SMILES_EZ_IMPLIED) == (1024, 2048, 4096) == \
        (E.FLAG_EZ, E.FLAG_EZ_UNRESOLVED, E.FLAG_EZ_IMPLIED)
    assert (engine.SMILES_MARK_TETRAHEDRAL, engine.SMILES_MARK_DOUBLE_BOND) == (1, 2)
    assert not engine.SMILES_REFUSED & 0x1C00
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    for line in ("#define MNX_SMILES_MARK_TETRAHEDRAL 1u\n", "#define MNX_SMILES_MARK_DOUBLE_BOND 2u\n", "#define MNX_SMILES_EZ 1024u\n",
                 "#define MNX_SMILES_EZ_UNRESOLVED 2048u\n", "#define MNX_SMILES_EZ_IMPLIED 4096u\n",
                 "int mnx_smiles_pack_marks(mnx_engine* h, const mnx_mol* mols, int32_t n,", "uint32_t* totals, uint32_t marks,"):
        assert line in hdr, line
    for _, _, _, want, _ in PINNED.values():                 # the header states the rule with its examples
        assert want in hdr, want


def test_double_bonds_need_smiles():
    with pytest.raises(ValueError, match="smiles=True"):
        predict_pipeline(None, None, packed=True, double_bonds=True)
    with pytest.raises(ValueError, match="packed"):
        predict_pipeline(None, None, smiles=True, double_bonds=True)
