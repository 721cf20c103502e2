"""CPU: the oracle of mnx_smiles_pack_symmetric (tests/symmetry_ref.py) against the rule's own consequences — the pinned strings
of the header in both drawings, the seven invariants over generated molecules, what those molecules cover, the molecules all
of whose candidates are symmetric under redrawing and renumbering — and the binding of the new call."""
import numpy as np
import pytest

import canon_ref as K
import ez_ref as E
import smiles_ref as S
import stereo_ref as T
import symmetry_ref as Y
import test_canon_host as H

SYM, TIE, WEDGES, STEREO, UNRESOLVED = Y.FLAG_SYM, K.FLAG_TIE, S.FLAG_WEDGES, T.FLAG_STEREO, T.FLAG_UNRESOLVED
EZ, EZ_UNRESOLVED, EZ_IMPLIED = E.FLAG_EZ, E.FLAG_EZ_UNRESOLVED, E.FLAG_EZ_IMPLIED


def mirrored(mol, span, axis=1):
    """the drawing with y (axis 1) or x (axis 0) replaced by span - it"""
    return mol[0], [(span - x, y) if axis == 0 else (x, span - y) for x, y in mol[1]], mol[2]


RING6 = [(0, 1, 1, 1), (1, 2, 1, 1), (2, 3, 1, 1), (3, 4, 1, 1), (4, 5, 1, 1), (0, 5, 1, 1), (0, 6, 5, 6)]
CYCLOHEXANE = ([b"[C@H]", b"C", b"C", b"[C@H]", b"C", b"C", b"C", b"C"],
               [(10, 20), (15, 11), (25, 11), (30, 20), (25, 29), (15, 29), (0, 20), (40, 20)])
# name: (molecule, marks, the mirror (span, axis) or None, canonical strings (drawing, mirrored), the new call's string for both or
#        per drawing, flag bits set, flag bits clear)
PINNED = {
    "2-fluoropropane": (([b"F", b"[C@H]", b"C", b"C"], [(20, 30), (20, 20), (11, 15), (29, 15)], [(0, 1, 6, 5), (1, 2, 1, 1), (1, 3, 1, 1)]),
                        3, (40, 1), ("C[C@@H](C)F", "C[C@H](C)F"), "C[CH](C)F", SYM | WEDGES, STEREO | UNRESOLVED),
    "3-chloro-3-fluoropentane": (([b"F", b"[C@@]", b"Cl", b"C", b"C", b"C", b"C"], [(20, 30), (20, 20), (20, 10), (11, 25), (29, 25), (3, 20), (37, 20)],
                                  [(0, 1, 6, 5), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 1, 1), (3, 5, 1, 1), (4, 6, 1, 1)]),
                                 3, (40, 1), ("CC[C@@](CC)(Cl)F", "CC[C@](CC)(Cl)F"), "CC[C](CC)(Cl)F", SYM | WEDGES, STEREO | UNRESOLVED),
    "1,1-dimethylcyclopropane": (([b"[C@]", b"C", b"C", b"C", b"C"], [(20, 20), (30, 26), (30, 14), (10, 14), (10, 26)],
                                  [(0, 1, 1, 1), (0, 2, 1, 1), (1, 2, 1, 1), (0, 3, 5, 6), (0, 4, 1, 1)]),
                                 3, (40, 1), ("C[C@@]1(C)CC1", "C[C@]1(C)CC1"), "C[C]1(C)CC1", SYM | WEDGES, STEREO | UNRESOLVED),
    "alanine": (H.ALANINE, 3, (45, 0), ("C[C@@H](C(O)=O)N", "C[C@H](C(O)=O)N"), ("C[C@@H](C(O)=O)N", "C[C@H](C(O)=O)N"), STEREO, SYM | WEDGES),
    "cis-1,4-dimethylcyclohexane": ((*CYCLOHEXANE, RING6 + [(3, 7, 5, 6)]), 3, None, ("C[C@H]1CC[C@@H](C)CC1",), "C[C@H]1CC[C@@H](C)CC1", STEREO, SYM),
    "trans-1,4-dimethylcyclohexane": ((*CYCLOHEXANE, RING6 + [(3, 7, 6, 5)]), 3, None, ("C[C@H]1CC[C@H](C)CC1",), "C[C@H]1CC[C@H](C)CC1", STEREO, SYM),
    "(CH3)2C=CHF": (([b"C", b"C", b"C", b"C", b"F"], [(0, 0), (0, 20), (10, 10), (20, 10), (30, 0)], [(0, 2, 1, 1), (1, 2, 1, 1), (2, 3, 2, 2), (3, 4, 1, 1)]),
                    2, (20, 1), ("C/C(/C)=C\\F", "C/C(/C)=C/F"), "CC(C)=CF", SYM, EZ | EZ_UNRESOLVED | EZ_IMPLIED),
    "tetrafluoroethene": (([b"F", b"F", b"C", b"C", b"F", b"F"], [(0, 0), (0, 20), (10, 10), (20, 10), (30, 0), (30, 20)],
                           [(0, 2, 1, 1), (1, 2, 1, 1), (2, 3, 2, 2), (3, 4, 1, 1), (3, 5, 1, 1)]),
                          2, None, ("C(=C(/F)\\F)(/F)\\F",), "C(=C(F)F)(F)F", SYM, EZ | EZ_UNRESOLVED | EZ_IMPLIED),
    "a diene with a symmetric end": (([b"C"] * 7, [(0, 20), (10, 10), (20, 20), (30, 10), (40, 20), (50, 20), (40, 30)],
                                      [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 1, 1), (3, 4, 2, 2), (4, 5, 1, 1), (4, 6, 1, 1)]),
                                     2, None, ("C/C=C/C=C(\\C)/C",), "C/C=C/C=C(C)C", SYM | EZ, EZ_IMPLIED | EZ_UNRESOLVED),
    "difluoroethene": (H.DIFLUORO, 3, None, ("C(=C\\F)/F",), "C(=C\\F)/F", EZ, SYM),
}


@pytest.fixture(scope="module")
def molecules():
    """the generated molecules of test_canon_host.py, then this rule's own"""
    return T.generated_set(100) + E.generated_set(100) + Y.generated_set()


@pytest.fixture(scope="module")
def written(molecules):
    """per molecule and set of marks: (the new call, mnx_smiles_pack_canonical)"""
    return [{marks: (Y.smiles(*mol, marks), K.smiles(*mol, marks)) for marks in range(4)} for mol in molecules]


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_strings_in_both_drawings(name):
    mol, marks, mirror, before, after, set_bits, clear_bits = PINNED[name]
    drawings = [mol] + ([mirrored(mol, *mirror)] if mirror else [])
    after = (after,) * len(drawings) if isinstance(after, str) else after
    for k, drawing in enumerate(drawings):
        assert K.smiles(*drawing, marks)[0] == before[k], (k, K.smiles(*drawing, marks)[0])
        text, pos, flags, n_rings, rank, sym_class, bits, what = Y.smiles(*drawing, marks)
        assert text == after[k], (k, text)
        assert flags & set_bits == set_bits and not flags & clear_bits, (k, flags)
        assert sorted(pos) == sorted(rank) == list(range(len(mol[0])))
        assert bool(flags & SYM) == any(b & (Y.ATOM_SYM | Y.ATOM_EZ_SYM) for b in bits)
    if mirror and isinstance(PINNED[name][4], str):
        assert before[0] != before[1]                        # where the canonical call gives two strings, the new call gives one


def test_pinned_atom_marks():
    mol = PINNED["2-fluoropropane"][0]
    assert Y.smiles(*mol, 3)[6] == [0, Y.ATOM_SYM, 0, 0] and Y.smiles(*mol, 2)[6] == [0] * 4
    assert Y.smiles(*H.ALANINE, 3)[6] == [0, Y.ATOM_CCW, 0, 0, 0, 0]
    assert Y.smiles(*PINNED["a diene with a symmetric end"][0], 2)[6] == [0, 8, 8, 16, 16, 0, 0]
    assert Y.smiles(*PINNED["tetrafluoroethene"][0], 3)[6] == [0, 0, 16, 16, 0, 0]
    assert Y.smiles(*H.DIFLUORO, 3)[6] == [0, 8, 8, 0] and Y.smiles(*H.DIFLUORO, 1)[6] == [0] * 4


def marks_at(text, pos):
    """the '@' / '@@' of a written string per atom"""
    tokens = E.read(text)[0]
    return [tokens[p].count("@") for p in pos]


def test_invariants(molecules, written):
    """the invariants 1-6 of the header over every generated molecule and every set of marks"""
    fired = 0
    for mol, by_marks in zip(molecules, written):
        for marks in range(4):
            new, old = by_marks[marks]
            assert new[1] == old[1] and new[3:6] == old[3:6], "1: order, n_rings, rank, sym_class"
            assert new[2] & Y.KEPT_BITS == old[2] & Y.KEPT_BITS, "1: flag bits 0-5, 7, 13, 14"
            if new[0] is None:
                assert old[0] is None and new[6] is None and not new[2] & SYM
                continue
            assert E.strip(new[0].replace("@", "")) == by_marks[0][1][0], "2: the strip invariant"
            if not new[2] & SYM:
                assert new[0] == old[0] and new[2] == old[2], "3: bit 15 clear: the canonical call's bytes and flags"
            else:
                assert new[2] & TIE, "4: bit 13 clear implies bit 15 clear"
                fired += 1
            if marks == 0:
                assert new[0] == old[0] and new[2] == old[2] and new[6] == [0] * len(mol[0]), "5"
            now, then = marks_at(new[0], new[1]), marks_at(old[0], old[1])
            assert now == [0 if b & Y.ATOM_SYM else t for b, t in zip(new[6], then)], "6: every mark but the dropped ones, unchanged"
            assert [b & 3 for b in new[6]] == now
    assert fired > 100


def test_the_generated_molecules_cover_the_rule(molecules):
    c = Y.coverage(molecules)
    for key in ("dropped centre", "dropped bond", "kept and dropped", "ring pair kept", "pseudo off", "flip changed", "all symmetric",
                "wedge at dropped centre"):
        assert c[key] >= 1, (key, c)
    own = Y.coverage(Y.generated_set())
    assert own["dropped centre"] >= 10 and own["dropped bond"] >= 10 and own["kept centre"] >= 10 and own["kept bond"] >= 10, own


def test_the_rule_is_off_with_a_pseudo_atom(molecules, written):
    off = 0
    for mol, by_marks in zip(molecules, written):
        new, old = by_marks[3]
        if new[0] is not None and new[7]["pseudo"]:
            assert new[0] == old[0] and new[2] == old[2] and not new[2] & SYM
            off += bool(Y.smiles(*mol, 3, even_with_pseudo=True)[2] & SYM)
    assert off >= 1


def renumbered(mol, rng):
    return T.renumber(mol, [int(p) for p in rng.permutation(len(mol[0]))], rng)


def test_molecules_whose_candidates_are_all_symmetric(molecules, written):
    """every candidate dropped: the new call with marks 3 writes the marks == 0 canonical bytes, and it goes on doing so when the
    molecule is drawn anew and renumbered — identical new bytes wherever the marks == 0 canonical bytes are identical"""
    rng = np.random.default_rng(91)
    seen = same = 0
    for mol, by_marks in zip(molecules, written):
        new = by_marks[3][0]
        verdicts = [] if new[0] is None else list(new[7]["centres"].values()) + list(new[7]["bonds"].values())
        if not verdicts or any(v != "dropped" for v in verdicts):
            continue
        seen += 1
        assert new[0] == by_marks[0][1][0] and not new[2] & (STEREO | UNRESOLVED | EZ | EZ_UNRESOLVED | EZ_IMPLIED)
        for _ in range(3):
            other = renumbered(K.redraw(mol, rng), rng)
            if K.smiles(*other, 0)[0] == by_marks[0][1][0]:
                same += 1
                assert Y.smiles(*other, 3)[0] == new[0]
    assert seen >= 10 and same >= 2 * seen


def test_the_same_drawing_in_any_numbering_gives_the_same_bytes(molecules, written):
    rng = np.random.default_rng(92)
    for mol, by_marks in zip(molecules[200::2], written[200::2]):
        if by_marks[0][0][2] & K.FLAG_TIE_INDEX:
            continue
        other = renumbered(mol, rng)
        for marks in (1, 2, 3):
            got = Y.smiles(*other, marks)
            assert got[0] == by_marks[marks][0][0] and got[2:4] == by_marks[marks][0][2:4], marks


def test_pack_carries_the_atom_marks_and_refuses_where_the_writer_does():
    import molfile_ref as M
    dup = (H.DIFLUORO[0], H.DIFLUORO[1], H.CHAIN3 + [(2, 1, 1, 1)])
    many = ([b"C"] * 102, [(k, 0) for k in range(102)], [(0, k, 1, 1) for k in range(1, 102)] + [(k, k + 1, 1, 1) for k in range(1, 101)])
    tables = M.build_tables([PINNED["2-fluoropropane"][0], dup, many, ([], [], []), H.DIFLUORO])
    ref = Y.pack(*tables, 3)
    assert ref["recs"]["flags"].tolist() == [SYM | TIE | WEDGES, S.FLAG_DUPLICATE, S.FLAG_RINGS | TIE, 0, EZ | TIE]
    assert ref["atom_marks"].dtype == np.uint8 and ref["atom_marks"][:4].tolist() == [0, 4, 0, 0]
    assert set(ref["atom_marks"][4:110].tolist()) == {Y.NO_MARKS} and ref["atom_marks"][110:].tolist() == [0, 8, 8, 0]
    assert set(ref["rank"][4:8].tolist()) == {K.NO_RANK} and sorted(ref["rank"][8:110].tolist()) == list(range(102))
    assert ref["out"] == b"C[CH](C)FC(=C\\F)/F"
    short = Y.pack(*tables, 3, n_atom_records=112, marks_fill=0x7F)
    assert short["recs"]["flags"][4] == S.FLAG_BEYOND and short["atom_marks"][110:].tolist() == [Y.NO_MARKS] * 2


def test_library_and_binding_carry_the_new_call():
    import inspect
    import re
    from pathlib import Path
    from molnextr_amd import engine, model
    assert "mnx_smiles_pack_symmetric" in engine.SYMBOLS and engine.ABI_VERSION == 7
    assert engine.SMILES_SYM_DROPPED == SYM == 1 << 15
    assert (engine.ATOM_MARK_CW, engine.ATOM_MARK_CCW, engine.ATOM_MARK_SYM, engine.ATOM_EZ, engine.ATOM_EZ_SYM) == (1, 2, 4, 8, 16)
    header = (Path(__file__).resolve().parents[1] / "include" / "molnextr_hip.h").read_text()
    assert re.search(r"int mnx_smiles_pack_symmetric\(", header) and "#define MNX_SMILES_SYM_DROPPED 32768u" in header
    for fn, name in ((engine.Engine.smiles_pack, "symmetry"), (model.predict_pipeline, "symmetry"), (model.molnextr.__init__, "graph_symmetry")):
        assert inspect.signature(fn).parameters[name].default is False
    with pytest.raises(ValueError, match="symmetry=True needs canonical=True"):
        engine.Engine.smiles_pack(None, None, symmetry=True)
    for args in ({"smiles": True}, {}):
        with pytest.raises(ValueError, match="symmetry=True needs smiles=True and canonical=True"):
            model.predict_pipeline(None, None, packed=True, symmetry=True, **args)
