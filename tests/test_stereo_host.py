"""CPU: the oracle of mnx_smiles_pack_stereo (tests/stereo_ref.py) against the strings that pin the rule and its sign, its reader
(handedness from the drawing by the OpenSMILES wording, no determinant) against its writer over generated molecules and under
renumbering, what the generated set covers, every case of the three stereo flags; and the binding of the new call."""
import ctypes
import os

import numpy as np
import pytest

import molfile_ref as M
import smiles_ref as S
import stereo_ref as T
from molnextr_amd import engine
from molnextr_amd.model import predict_pipeline

HALIDE = [(20, 30), (20, 20), (20, 10), (11, 25), (29, 25)]
ALANINE = ([b"N", b"[C@H]", b"C", b"C", b"O", b"O"], [(10, 20), (20, 20), (25, 11), (25, 29), (20, 38), (35, 29)])
ACID = [(3, 4, 2, 2), (3, 5, 1, 1)]

# name: (symbols, (x_bin, y_bin), bonds (i, j, type, rev), the string, flags) — the table of the rule (include/molnextr_hip.h)
PINNED = {
    "1": ([b"F", b"[C@@]", b"Cl", b"Br", b"I"], HALIDE, [(0, 1, 6, 5), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 1, 1)], "F[C@](Cl)(Br)I", T.FLAG_STEREO),
    "1b": ([b"[C@@]", b"F", b"Cl", b"Br", b"I"], [HALIDE[k] for k in (1, 0, 2, 3, 4)],
           [(0, 1, 5, 6), (0, 2, 1, 1), (0, 3, 1, 1), (0, 4, 1, 1)], "[C@](F)(Cl)(Br)I", T.FLAG_STEREO),
    "2": (*ALANINE, [(0, 1, 1, 1), (1, 2, 5, 6), (1, 3, 1, 1)] + ACID, "N[C@@H](C)C(=O)O", T.FLAG_STEREO),
    "2b": ([ALANINE[0][k] for k in (1, 0, 2, 3, 4, 5)], [ALANINE[1][k] for k in (1, 0, 2, 3, 4, 5)],
           [(0, 1, 1, 1), (0, 2, 5, 6), (0, 3, 1, 1)] + ACID, "[C@H](N)(C)C(=O)O", T.FLAG_STEREO),
    "2c": (*ALANINE, [(0, 1, 1, 1), (1, 2, 6, 5), (1, 3, 1, 1)] + ACID, "N[C@H](C)C(=O)O", T.FLAG_STEREO),
    "3": ([b"[C@H]", b"C", b"C", b"F"], [(20, 20), (30, 26), (30, 14), (10, 20)], [(0, 1, 1, 1), (0, 2, 1, 1), (1, 2, 1, 1), (0, 3, 5, 6)],
          "[C@H]1(CC1)F", T.FLAG_STEREO),
    "3b": ([b"C", b"C", b"[C@H]", b"F"], [(30, 26), (30, 14), (20, 20), (10, 20)], [(0, 1, 1, 1), (0, 2, 1, 1), (1, 2, 1, 1), (2, 3, 5, 6)],
           "C1C[C@@H]1F", T.FLAG_STEREO),
    "4": ([b"F", b"[C@@]", b"Cl", b"Br", b"I"], HALIDE, [(0, 1, 1, 1), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 1, 1)], "F[C](Cl)(Br)I", 0),
    "4b": ([b"F", b"[C@@]", b"Cl", b"Br", b"I"], HALIDE[:3] + [(20, 25), (20, 5)], [(0, 1, 6, 5), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 1, 1)],
           "F[C](Cl)(Br)I", S.FLAG_WEDGES | T.FLAG_UNRESOLVED),
}
PAIRS = {"1": ("1b", (1, 0, 2, 3, 4)), "2": ("2b", (1, 0, 2, 3, 4, 5)), "3b": ("3", (1, 2, 0, 3))}     # name: (the other numbering, perm)


@pytest.fixture(scope="module")
def generated():
    mols = T.generated_set()
    return mols, [T.smiles(*m) for m in mols]


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_strings(name):
    syms, xy, bonds, want, flags = PINNED[name]
    got = T.pack(*M.build_tables([(syms, xy, bonds)]))
    assert got["out"].decode() == want and got["recs"]["flags"][0] == flags and got["recs"]["len"][0] == len(want)
    plain = S.pack(*M.build_tables([(syms, xy, bonds)]))
    assert want.replace("@", "") == plain["out"].decode() and got["order"].tolist() == plain["order"].tolist()
    text, pos, _, _, centre = T.smiles(syms, xy, bonds)
    for c, (mark, hand, order) in T.read_back(text, pos, xy, bonds).items():          # the drawing, read without the rule
        assert mark == hand == centre[c]["mark"] and order == centre[c]["order"], (name, c, mark, hand, order)
    assert ("@" in want) == bool(T.read_back(text, pos, xy, bonds))


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_one_drawing_numbered_two_ways_names_one_configuration(name):
    other, perm = PAIRS[name]
    a, b = T.smiles(*PINNED[name][:3]), T.smiles(*PINNED[other][:3])
    (ca, ra), = a[4].items()
    (cb, rb), = b[4].items()
    assert cb == perm[ca] and ra["mark"] and rb["mark"]
    moved = [k if k == "H" else perm[k] for k in ra["order"]]
    assert (ra["mark"] == rb["mark"]) == (T.parity(moved, rb["order"]) == 0)


def test_handedness_reads_the_opensmiles_wording():
    """seen from the first point the other three run anticlockwise: '@'; a swap of two and the mirror image flip it, a rotation
    of the three does not"""
    pts = [(0, 0, 1), (1, 0, 0), (-0.5, 0.87, 0), (-0.5, -0.87, 0)]                     # seen from +z: x axis, 120 deg, 240 deg
    assert T.handedness(pts) == "@" and T.handedness([pts[0], pts[2], pts[1], pts[3]]) == "@@"
    assert T.handedness([(x, y, -z) for x, y, z in pts]) == "@@" and T.handedness([pts[0], pts[2], pts[3], pts[1]]) == "@"
    assert T.handedness([(3, 4, 30), (41, 40, 0), (39.5, 40.87, 0), (39.5, 39.13, 0)]) == "@"      # far off the axis of sight


def test_reader_agrees_with_writer_over_generated_molecules(generated):
    """the handedness read from string and drawing equals the mark at EVERY marked atom; every unmarked marked-carbon symbol is
    one the rule leaves out; removing the marks gives the plain writer's string, order, n_rings and other flags"""
    marks = 0
    for (syms, xy, bonds), (text, pos, flags, n_rings, centre) in zip(*generated):
        back = T.read_back(text, pos, xy, bonds)
        assert sorted(back) == sorted(c for c, r in centre.items() if r["mark"])
        for c, (mark, hand, order) in back.items():
            assert mark == hand == centre[c]["mark"] and order == centre[c]["order"], (text, c, mark, hand, order)
            marks += 1
        for c, r in centre.items():
            if not r["mark"]:
                h = syms[c] in T.WITH_H
                degree = sum(c in b[:2] for b in bonds)
                single = all(b[2] in (1, 5, 6) for b in bonds if c in b[:2])
                assert not r["wedge"] or degree + h != 4 or not single or r["d"] == 0, (text, c, r)
        plain = S.smiles(syms, bonds)
        assert (text.replace("@", ""), pos, n_rings) == (plain[0], plain[1], plain[3]) and ((flags ^ plain[2]) & 0xBF) == 0
        atoms, read_bonds = S.read(text.replace("@", ""))
        assert len(atoms) == len(syms) and len(read_bonds) == len(bonds)
        assert bool(flags & S.FLAG_WEDGES) == any(b[2] in (5, 6) and not centre.get(b[0], {}).get("mark") and
                                                  not centre.get(b[1], {}).get("mark") for b in bonds)
    assert marks > 1000


def test_generated_set_covers_the_ground(generated):
    mols = generated[0]
    c = T.coverage(mols)
    print(c)
    assert all(10 <= len(m[0]) <= 60 for m in mols) and len(mols) == 300
    assert all(max(sum(a in b[:2] for b in m[2]) for a in range(len(m[0]))) <= 4 for m in mols)
    assert all(0 <= v <= 63 for m in mols for p in m[1] for v in p)
    assert c["@"] >= 100 and c["@@"] >= 100
    for k in ("root", "H0", "H1", "four", "ring1", "ring2", "dash", "two wedges"):
        assert c[k] >= 20, (k, c)
    assert c["unresolved"] <= 0.05 * c["candidates"], c
    texts = [g[0] for g in generated[1]]
    assert sum("." in t for t in texts) > 30 and sum("1" in t for t in texts) > 100 and sum("=" in t for t in texts) > 100


def test_renumbering_keeps_every_configuration(generated):
    """20 random renumberings of every molecule: the same atoms are marked, and two strings' marks at a centre are equal exactly
    when one string's neighbour order (read from the string) is an even permutation of the other's"""
    rng = np.random.default_rng(22)
    flipped = kept = 0
    for (syms, xy, bonds), (text, pos, _, _, _) in zip(*generated):
        first = T.read_back(text, pos, xy, bonds)
        for _ in range(20):
            perm = [int(p) for p in rng.permutation(len(syms))]
            s2, xy2, b2 = T.renumber((syms, xy, bonds), perm, rng)
            t2, pos2, _, _, _ = T.smiles(s2, xy2, b2)
            second = T.read_back(t2, pos2, xy2, b2)
            assert sorted(second) == sorted(perm[c] for c in first), (text, t2)
            for c, (mark, hand, order) in first.items():
                mark2, hand2, order2 = second[perm[c]]
                assert mark2 == hand2
                odd = T.parity([k if k == "H" else perm[k] for k in order], order2)
                assert (mark == mark2) == (odd == 0), (text, t2, c, order, order2)
                flipped += odd
                kept += 1 - odd
    assert flipped > 1000 and kept > 1000


FLAG_CASES = {
    # a mark: bit 8; the wedge has a marked end: no bit 6
    "marked": (PINNED["1"][:3], T.FLAG_STEREO),
    # a wedge between plain atoms beside the marked centre: bits 6 and 8
    "marked, another wedge dropped": ((PINNED["2"][0], PINNED["2"][1], PINNED["2"][2][:3] + [(3, 4, 2, 2), (3, 5, 5, 6)]), T.FLAG_STEREO | S.FLAG_WEDGES),
    # no marked-carbon symbol at either end: bit 6 alone, as in the plain call
    "no marked carbon": (([b"C", b"C", b"N"], [(0, 0), (9, 0), (9, 9)], [(0, 1, 5, 6), (1, 2, 1, 1)]), S.FLAG_WEDGES),
    # the wedge begins at the other end (the centre sees class 1): not a candidate and not unresolved, bit 6
    "wedge seen from the other end only": ((PINNED["1"][0], HALIDE, [(0, 1, 5, 1)] + PINNED["1"][2][1:]), S.FLAG_WEDGES),
    # three neighbours at [C@@] (needs four): bits 6 and 9
    "neighbour count": ((PINNED["1"][0][:4], HALIDE[:4], PINNED["1"][2][:3]), S.FLAG_WEDGES | T.FLAG_UNRESOLVED),
    # a double bond at the centre: bits 6 and 9
    "a bond that is not single": ((PINNED["1"][0], HALIDE, PINNED["1"][2][:3] + [(1, 4, 2, 2)]), S.FLAG_WEDGES | T.FLAG_UNRESOLVED),
    # d == 0: bits 6 and 9
    "flat": (PINNED["4b"][:3], S.FLAG_WEDGES | T.FLAG_UNRESOLVED),
    # one centre resolves, one does not, and the unresolved one's wedge ends at the marked one: bits 8 and 9, no bit 6
    "unresolved beside a mark": (([b"F", b"[C@@]", b"Cl", b"Br", b"[C@H]"], HALIDE, [(0, 1, 6, 5), (1, 2, 1, 1), (1, 3, 1, 1), (1, 4, 6, 5)]),
                                 T.FLAG_STEREO | T.FLAG_UNRESOLVED),
    # the marked symbol without any wedge: nothing
    "no wedge": (PINNED["4"][:3], 0),
    # refused (the pair 1 2 twice): no stereo bit
    "refused": ((PINNED["1"][0], HALIDE, PINNED["1"][2] + [(2, 1, 1, 1)]), S.FLAG_DUPLICATE),
}


@pytest.mark.parametrize("name", sorted(FLAG_CASES))
def test_flag_cases(name):
    mol, flags = FLAG_CASES[name]
    got = T.pack(*M.build_tables([mol]))
    assert got["recs"]["flags"][0] == flags, (name, got["out"], got["recs"])
    assert ("@" in got["out"].decode()) == bool(flags & T.FLAG_STEREO) and (got["recs"]["len"][0] == 0) == (name == "refused")


def test_library_and_binding_carry_the_new_call():
    lib = engine.load_library()
    assert "mnx_smiles_pack_stereo" in engine.SYMBOLS and hasattr(lib, "mnx_smiles_pack_stereo")
    assert lib.mnx_smiles_pack_stereo.argtypes == lib.mnx_smiles_pack.argtypes and len(lib.mnx_smiles_pack_stereo.argtypes) == 15
    assert lib.mnx_smiles_pack_stereo(None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, None) == -1
    assert lib.mnx_abi_version() == engine.ABI_VERSION == 7
    assert (engine.SMILES_STEREO, engine.SMILES_STEREO_UNRESOLVED) == (T.FLAG_STEREO, T.FLAG_UNRESOLVED) == (256, 512)
    assert not engine.SMILES_REFUSED & (engine.SMILES_STEREO | engine.SMILES_STEREO_UNRESOLVED)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    assert "#define MNX_SMILES_STEREO 256u\n" in hdr and "#define MNX_SMILES_STEREO_UNRESOLVED 512u\n" in hdr
    assert "int mnx_smiles_pack_stereo(mnx_engine* h, const mnx_mol* mols, int32_t n," in hdr
    for _, _, _, want, _ in (PINNED[k] for k in ("1", "2", "2c", "3")):                 # the header states the rule with its examples
        assert want in hdr, want
    assert ctypes.sizeof(engine.MnxSmiles) == 16


def test_stereo_needs_smiles():
    with pytest.raises(ValueError, match="smiles=True"):
        predict_pipeline(None, None, packed=True, stereo=True)
    with pytest.raises(ValueError, match="packed"):
        predict_pipeline(None, None, smiles=True, stereo=True)
