"""CPU: the rule of mnx_smiles_read as the oracle of tests/smiles_read_ref.py implements it — the header's examples against tables
written out by hand, every refusal with its err_pos, agreement with smiles_ref.read on what the writer emits, and the two
properties the reader exists for: write -> read -> write is a fixed point, and the canonical string survives the loss of the
drawing. Plus: the library exports the call, the binding carries it, evaluate's parser knows --graph_match."""
import ctypes
import os

import numpy as np
import pytest

import canon_ref as K
import molfile_ref as M
import smiles_read_ref as R
import smiles_ref as S
from molnextr_amd import engine, evaluate

TABLES = M.name_tables()
RING6 = [(0, 1, 4), (0, 5, 4), (1, 2, 4), (2, 3, 4), (3, 4, 4), (4, 5, 4)]
TRIANGLE = [(0, 1, 1), (0, 2, 1), (1, 2, 1)]

# string -> (atom spans, bonds, flags, n_rings), each written out by hand after the header's rule
HAND = {
    b"CCO": ([(0, 1), (1, 1), (2, 1)], [(0, 1, 1), (1, 2, 1)], 0, 0),
    b"CC(=O)[O-]": ([(0, 1), (1, 1), (4, 1), (6, 4)], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], 0, 0),
    b"c1ccccc1": ([(0, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1)], RING6, 0, 1),
    b"c1ccccc1-c1ccccc1": ([(0, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (9, 1), (11, 1), (12, 1), (13, 1), (14, 1), (15, 1)],
                           RING6 + [(5, 6, 1), (6, 7, 4), (6, 11, 4), (7, 8, 4), (8, 9, 4), (9, 10, 4), (10, 11, 4)], 0, 2),
    b"C1CC1.C1CC1": ([(0, 1), (2, 1), (3, 1), (6, 1), (8, 1), (9, 1)], TRIANGLE + [(3, 4, 1), (3, 5, 1), (4, 5, 1)], 0, 2),
    b"C%12CC%12": ([(0, 1), (4, 1), (5, 1)], TRIANGLE, 0, 1),
    b"C=1CC1": ([(0, 1), (3, 1), (4, 1)], [(0, 1, 1), (0, 2, 2), (1, 2, 1)], 0, 1),
    b"C1CC=1": ([(0, 1), (2, 1), (3, 1)], [(0, 1, 1), (0, 2, 2), (1, 2, 1)], 0, 1),
    b"F/C=C/F": ([(0, 1), (2, 1), (4, 1), (6, 1)], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], R.STEREO_DROPPED, 0),
    b"[13CH3][C@@H](N)C(=O)O": ([(0, 7), (7, 6), (14, 1), (16, 1), (19, 1), (21, 1)],
                                [(0, 1, 1), (1, 2, 1), (1, 3, 1), (3, 4, 2), (3, 5, 1)], R.STEREO_DROPPED, 0),
    b"C(C)(C)(C)C": ([(0, 1), (2, 1), (5, 1), (8, 1), (10, 1)], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)], 0, 0),
    b"[Ph]C": ([(0, 4), (4, 1)], [(0, 1, 1)], 0, 0),
    b"Cl": ([(0, 2)], [], 0, 0),
    b"ClC": ([(0, 2), (2, 1)], [(0, 1, 1)], 0, 0),
    b"C0CC0": ([(0, 1), (2, 1), (3, 1)], TRIANGLE, 0, 1),
}

# string -> err_pos of MNX_READ_SYNTAX, one line per rule of the header
SYNTAX = {
    b"CxC": 1, b"C~C": 1, b"C$C": 1, b"Cr": 1, b"l": 0, b"C\xc5\x95": 1, b"C C": 1,          # an illegal byte
    b"C[N": 1, b"[C[N]": 0, b"C[]C": 1, b"C]C": 1, b"C[N]]": 4,                                 # brackets
    b"C=": 1, b"C==C": 1, b"C=(O)": 1, b"C=)": 1, b"C=.C": 1, b"C(=)C": 2,                       # a bond symbol that leads nowhere
    b"=C": 0, b"C.=C": 1, b"1CC1": 0, b"(C)C": 0, b")C": 0, b".C": 0,                           # no atom in front
    b"C()": 2, b"C((C))": 2, b"C(1CC1)": 2, b"C(=1CC1)": 3, b"C(.C)": 2,
    b"C(C.C)": 3, b"C.": 1, b"C..C": 1, b"C.(C)": 1,                                            # the dot
    b"CC)": 2, b"C(C": 1, b"C(C(C": 1, b"C(C(C)": 1, b"C(C))(": 4,                              # parentheses
    b"C%1C": 1, b"C%": 1, b"C%1": 1, b"C%%12": 1,                                               # '%' without two digits
    b"C1CC": 1, b"C%12CC": 1, b"C1CC1C1": 6, b"C12CC1": 2,                                      # a ring number never closed
    b"C=1CC#1": 6, b"C/1CC\\1": 6, b"C-1CC/1": 6,                                               # conflicting symbols
    b"C11": 2, b"C%011": 4,                                                                     # onto its own atom
    b"C1C1": 3, b"C12CCC12": 7, b"C(C1)1": 5,                                                   # onto a pair that has a bond
    b"C(C$C)": 3, b"C(C$C": 1, b"C1C$C": 1, b"C1C$C1": 3,                                       # each error stands for itself
}


def fields(got, b=0):
    m, r = got["mols"][b], got["recs"][b]
    a0, b0 = int(m["atom0"]), int(m["bond0"])
    atoms = got["atoms"][a0:a0 + int(m["n_atoms"])]
    bonds = got["bonds"][b0:b0 + int(m["n_bonds"])]
    return atoms, bonds, m, r


@pytest.mark.parametrize("text", sorted(HAND))
def test_header_examples_against_hand_written_tables(text):
    spans, bonds, flags, n_rings = HAND[text]
    got = R.pack([b"C", text, b"N"])                       # between two others: offsets of the tables
    atoms, brecs, m, r = fields(got, 1)
    assert (int(m["atom0"]), int(m["bond0"]), int(m["text0"]), int(m["smiles_len"])) == (1, 0, 1, len(text))
    assert got["text"] == b"C" + text + b"N" and int(m["flags"]) == 0 and float(m["overall_score"]) == 0.0
    assert [(int(a["sym0"]), int(a["sym_len"])) for a in atoms] == spans
    assert atoms["index"].tolist() == list(range(len(spans))) and not atoms["x_bin"].any() and not atoms["y_bin"].any() and not atoms["score"].any()
    assert [(int(x["i"]), int(x["j"]), int(x["type"])) for x in brecs] == bonds
    assert brecs["rev"].tolist() == brecs["type"].tolist() and not brecs["score"].any()
    assert (int(r["flags"]), int(r["err_pos"]), int(r["n_rings"]), int(r["reserved"])) == (flags, 0, n_rings, 0)


def test_further_details_of_the_rule():
    lower = lambda s: [t for _, _, t in R.read(s)[1]]                                # noqa: E731
    assert lower(b"[nH]c") == [4] and lower(b"[13cH]c") == [4] and lower(b"[se]c") == [4] and lower(b"[2*]c") == [1]
    assert lower(b"cC") == [1] and lower(b"c:C") == [4] and lower(b"c-c") == [1] and lower(b"c*") == [1] and lower(b"[Nh]c") == [1]
    assert R.read(b"C(C)1CC1")[1] == [(0, 1, 1), (0, 2, 1), (0, 3, 1), (2, 3, 1)]    # a ring number behind ')': the atom in front of '('
    assert R.read(b"C1.C1")[1:] == ([(0, 1, 1)], 0, 1)                               # a ring bond across a dot: n_rings counts it
    assert R.read(b"C=1CC=1")[1] == [(0, 1, 1), (0, 2, 2), (1, 2, 1)]                # the same symbol at both ends
    assert R.read(b"C1CC1C1CC1")[3] == 2 and R.read(b"C%01CC1")[3] == 1              # a number comes back; 01 is 1
    assert R.read(b"CBr")[0] == [(0, 1), (1, 2)] and R.read(b"CBC")[0] == [(0, 1), (1, 1), (2, 1)]
    assert R.read(b"[C@](F)(Cl)(Br)I")[2] == R.STEREO_DROPPED and R.read(b"C[a@b]")[2] == R.STEREO_DROPPED
    assert R.read(b"[\x01\xff (.=%]C")[0] == [(0, 9), (9, 1)]                        # a bracket atom's bytes are not looked at


@pytest.mark.parametrize("text", sorted(SYNTAX))
def test_every_syntax_refusal_with_its_position(text):
    got = R.pack([b"CC", text, b"CC"])
    assert got["recs"]["flags"].tolist() == [0, R.SYNTAX, 0] and int(got["recs"]["err_pos"][1]) == SYNTAX[text]
    m = got["mols"][1]
    assert (int(m["n_atoms"]), int(m["n_bonds"]), int(m["smiles_len"]), int(m["flags"])) == (0, 0, 0, 0)
    assert got["text"] == b"CCCC" and got["totals"] == (4, 2, 4) and got["mols"]["atom0"].tolist() == [0, 2, 2]


def test_size_refusals_and_offsets_beyond_the_bytes():
    thousand_bonds = b"C12" + b"C" * 996 + b"C1C2"                                   # 999 atoms, 998 + 2 bonds
    got = R.pack([b"C" * 4096, b"C" * 4097, b"CC" * 499 + b"C", b"C" * 1000, thousand_bonds, b"C1" + b"C" * 997 + b"C1",
                  b"$" + b"C" * 1000, b"C" * 998 + b"$"])
    assert got["recs"]["flags"].tolist() == [R.TOO_LARGE, R.TOO_LARGE, 0, R.TOO_LARGE, R.TOO_LARGE, 0, R.TOO_LARGE, R.SYNTAX]
    assert got["recs"]["err_pos"].tolist() == [0, 0, 0, 0, 0, 0, 0, 998]
    assert got["mols"]["n_atoms"].tolist() == [0, 0, 999, 0, 0, 999, 0, 0] and got["mols"]["n_bonds"].tolist() == [0, 0, 998, 0, 0, 999, 0, 0]
    arena = b"CCOCN"
    got = R.pack(None, arena=arena, offsets=[0, 2, 1, 3, 6, 6], n_bytes=5)           # descending, then beyond n_bytes
    assert got["recs"]["flags"].tolist() == [0, R.BEYOND, 0, R.BEYOND, R.BEYOND] and got["text"] == b"CCCO"
    assert R.pack(None, arena=arena, offsets=[0, 5], n_bytes=4)["recs"]["flags"].tolist() == [R.BEYOND]


def random_molecule(rng, n_atoms):
    """a drawing: 1 .. 14 atoms in one to three components, each a random tree with up to three ring bonds; bond classes 1 - 5;
    aromatic, bracket and pseudo atoms; random coordinate bins. No numbered R-group: the writers spell [R1] as [1*] and read the
    symbol [1*] as a plain '*', so such an atom is no fixed point of the writers themselves."""
    pool = [b"C", b"C", b"C", b"N", b"O", b"c", b"c", b"n", b"s", b"Cl", b"Br", b"[nH]", b"[O-]", b"[NH3+]", b"[13C]", b"[C@@H]", b"[C@]",
            b"[Ac]", b"[OMe]", b"Ph", b"*", b"[2H]", b"[se]", b"[Fe+3]"]
    syms = [pool[k] for k in rng.integers(0, len(pool), n_atoms)]
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (n_atoms, 2))]
    cuts = sorted(set(int(c) for c in rng.integers(1, n_atoms + 1, int(rng.integers(0, 3)))) | {n_atoms})
    pairs, lo = set(), 0
    for hi in cuts:
        for a in range(lo + 1, hi):
            pairs.add((int(rng.integers(lo, a)), a))
        for _ in range(int(rng.integers(0, 4)) if hi - lo >= 3 else 0):
            i, j = sorted(int(v) for v in rng.choice(np.arange(lo, hi), 2, replace=False))
            pairs.add((i, j))
        lo = hi
    order = [sorted(pairs)[k] for k in rng.permutation(len(pairs))]
    types = rng.integers(1, 6, len(order))                 # rev = type, as mnx_graph_pack's symmetric bond classes give them
    return syms, xy, [(i, j, int(t), int(t)) for (i, j), t in zip(order, types)]


@pytest.fixture(scope="module")
def drawings():
    rng = np.random.default_rng(11)
    mols = [random_molecule(rng, int(n)) for n in rng.integers(1, 15, 1200)]
    return mols, M.build_tables(mols)


def strings(recs, out):
    return [bytes(out[int(r["text0"]):int(r["text0"]) + int(r["len"])]) for r in recs]


def test_agreement_with_the_writers_own_reader_on_emitted_strings(drawings):
    """on what mnx_smiles_pack emits, this reader and smiles_ref.read see the same atoms and the same bonds"""
    mols, tables = drawings
    written = S.pack(*tables, tables=TABLES)
    assert not (written["recs"]["flags"] & 0x33).any()
    n_ring_bonds = 0
    for text in strings(written["recs"], written["out"]):
        atoms, bonds, flags, n_rings = R.read(text)
        want_atoms, want_bonds = S.read(text.decode("ascii"))
        assert [text[p:p + ln].decode() for p, ln in atoms] == want_atoms and flags == 0
        lower = [R.lower_case(text[p:p + ln]) for p, ln in atoms]
        want = sorted((i, j, {"-": 1, "=": 2, "#": 3, ":": 4}[sym] if sym else 4 if lower[i] and lower[j] else 1) for (i, j), sym in want_bonds.items())
        assert bonds == want
        n_ring_bonds += n_rings
    assert n_ring_bonds > 500


def test_write_read_write_is_a_fixed_point(drawings):
    """the string of mnx_smiles_pack, read and written again, is the same bytes: 1200 of 1200"""
    mols, tables = drawings
    first = S.pack(*tables, tables=TABLES)
    texts = strings(first["recs"], first["out"])
    back = R.pack(texts)
    assert not back["recs"]["flags"].any() and back["recs"]["n_rings"].tolist() == first["recs"]["n_rings"].tolist()
    second = S.pack(back["mols"], back["atoms"], back["bonds"], back["text"], tables=TABLES)
    different = [(a, b) for a, b in zip(texts, strings(second["recs"], second["out"])) if a != b]
    assert not different, (len(different), different[:3])
    assert len(set(texts)) > 1000 and sum(b"." in t for t in texts) > 100 and sum(b"%" in t or b"1" in t for t in texts) > 300


def test_the_canonical_string_survives_the_loss_of_the_drawing(drawings):
    """marks == 0: the canonical string of a drawing and of its re-read copy (every coordinate 0, atoms in written order) are equal:
    1200 of 1200, ties among them"""
    mols, tables = drawings
    first = K.pack(*tables, 0, TABLES)
    texts = strings(first["recs"], first["out"])
    back = R.pack(texts)
    assert not back["recs"]["flags"].any()
    second = K.pack(back["mols"], back["atoms"], back["bonds"], back["text"], 0, TABLES)
    different = [(a, b) for a, b in zip(texts, strings(second["recs"], second["out"])) if a != b]
    assert not different, (len(different), different[:3])
    assert ((first["recs"]["flags"] & K.FLAG_TIE) != 0).sum() > 50
    # and from the plain writer's string, which numbers the atoms differently
    plain = S.pack(*tables, tables=TABLES)
    back = R.pack(strings(plain["recs"], plain["out"]))
    third = K.pack(back["mols"], back["atoms"], back["bonds"], back["text"], 0, TABLES)
    different = [(a, b) for a, b in zip(texts, strings(third["recs"], third["out"])) if a != b]
    assert not different, (len(different), different[:3])


def test_library_and_binding_carry_the_new_call():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    assert "int mnx_smiles_read(mnx_engine* h, const char* bytes, uint32_t n_bytes, const uint32_t* offsets, int32_t n," in hdr
    assert "#define MNX_ABI_VERSION 7\n" in hdr
    for name, bit in (("SYNTAX", 1), ("TOO_LARGE", 2), ("STEREO_DROPPED", 4), ("BEYOND", 8)):
        assert f"#define MNX_READ_{name} {bit}u\n" in hdr and getattr(engine, "READ_" + name) == bit == getattr(R, name)
    lib = engine.load_library()
    assert "mnx_smiles_read" in engine.SYMBOLS and hasattr(lib, "mnx_smiles_read") and len(lib.mnx_smiles_read.argtypes) == 15
    assert engine.READ_DTYPE == R.READ_DTYPE and engine.READ_DTYPE.itemsize == 16
    assert lib.mnx_smiles_read(None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None) == -1


def test_evaluate_parser_accepts_graph_match():
    ap = evaluate.build_parser()
    base = ["--test_file", "real/acs.csv", "--load_path", "synthetic"]
    assert ap.parse_args(base).graph_match is False
    assert ap.parse_args(base + ["--graph_match"]).graph_match is True
    assert "NOT the reference's RDKit" in " ".join(ap.format_help().split())
