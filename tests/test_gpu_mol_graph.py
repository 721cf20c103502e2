"""GPU (-m gpu): the neighbour lists that mnx_smiles_pack, mnx_smiles_pack_canonical (marks 0 and 3), mnx_smiles_pack_symmetric and
mnx_fingerprint_pack all begin with (csrc/mol_graph.h), at the smallest molecules at which building them can go wrong: the SAME
tiny tables through every one of the five calls, each result against its oracle (smiles_ref, canon_ref, symmetry_ref,
fingerprint_ref; byte for byte and word for word, no tolerances), and every malformed molecule between two good ones whose
outputs must be what they are alone. Nothing here depends on how the lists are built: the file passes on a library from before
mol_graph.h as it does on one with it.

What other files already assert and this one does not repeat: for mnx_smiles_pack alone a bond to no atom, a bond from an atom
to itself (test_gpu_smiles.py::test_records_beyond_the_tables), a pair twice in either direction and a list of 300 entries
(::test_duplicate_pairs_and_unknown_classes), a list of 998 (::test_deepest_stack_widest_branching_and_the_size_limit); for the
canonical call a duplicate, the empty molecule, 1 .. 999 atoms and the ring of 999 at marks 0 (test_gpu_canon.py::
test_refused_and_special_molecules_alone_and_in_one_batch, ::test_sizes_at_which_the_loops_take_another_turn,
::test_the_two_molecules_that_rank_longest: the ring runs here at marks 3 only); for the fingerprint j == n_atoms, i == j, a pair
given as (0,1),(1,0) and 0, 1 and 2 atoms (test_gpu_fingerprint.py::test_refusals_leave_the_other_molecules_alone,
::test_hand_made_molecules_one_by_one_and_together). New here: every case through all five calls on one set of tables,
i == n_atoms, (0,1),(0,1) for the ranks and the fingerprint, a duplicate with a pseudo-atom for the writers, atoms without bonds, a
list longer than the workgroup for the ranks and the fingerprint, and 1998 of the 2048 slots for the walk and the fingerprint."""
import pytest

import canon_ref as K
import fingerprint_ref as F
import smiles_ref as S
import symmetry_ref as Y
import test_fingerprint_host as FH
import test_gpu_fingerprint as G
from molnextr_amd.engine import FP_REFUSED, SMILES_REFUSED
from packed_tables import FILL, WORD_FILL, Tables, call_text, compare_text, dev, device_texts, eng, mol  # noqa: F401

pytestmark = pytest.mark.gpu


def text_pass(fn, oracle, marks=None):
    """a writer of text as (oracle of the tables, check of the device's result against it -> that result)"""
    def check(eng, t, ref):
        got = call_text(fn, eng, t, ref["total"], **({} if marks is None else {"marks": marks}))
        compare_text(got, ref, fn)
        return got
    return (lambda t: oracle(t.mols, t.atoms, t.bonds, t.text)), check


def fingerprint_check(eng, t, ref):
    G.check(eng, t, ref)
    return G.run(eng, t)


# name -> (oracle(t), check(eng, t, ref) -> the device's result)
PASSES = {
    "smiles": text_pass("mnx_smiles_pack", lambda *a: S.pack(*a, order_fill=WORD_FILL)),
    "canonical0": text_pass("mnx_smiles_pack_canonical", lambda *a: K.pack(*a, 0, order_fill=WORD_FILL), 0),
    "canonical3": text_pass("mnx_smiles_pack_canonical", lambda *a: K.pack(*a, 3, order_fill=WORD_FILL), 3),
    "symmetric3": text_pass("mnx_smiles_pack_symmetric", lambda *a: Y.pack(*a, 3, order_fill=WORD_FILL, marks_fill=FILL), 3),
    "fingerprint": ((lambda t: F.pack(t.mols, t.atoms, t.bonds, t.text, tables=FH.TABLES)), fingerprint_check),
}

# a ring with a branch, a double bond and a wedge: every stage of the writers has something to do
OK = mol([b"C", b"N", b"C", b"O", b"Cl"], [(0, 1, 1, 1), (1, 2, 1, 1), (0, 2, 1, 1), (2, 3, 2, 2), (0, 4, 5, 1)])
CNO, TWO = [b"C", b"N", b"O"], [(0, 1, 1, 1), (1, 2, 1, 1)]
MALFORMED = {
    "j == n_atoms": mol(CNO, [(0, 1, 1, 1), (1, 3, 1, 1)]),
    "i == n_atoms": mol(CNO, [(0, 1, 1, 1), (3, 1, 1, 1)]),
    "i == j": mol(CNO, [(0, 1, 1, 1), (2, 2, 1, 1)]),
    "(0,1),(0,1)": mol(CNO, TWO + [(0, 1, 1, 1)]),
    "(0,1),(1,0)": mol(CNO, TWO + [(1, 0, 2, 2)]),
    "duplicate and pseudo-atom": mol([b"C", b"R", b"O"], TWO + [(1, 0, 1, 1)]),
}
SMALL = [mol(CNO), mol([b"C"]), mol([])]                  # atoms and no bonds, one atom, the empty molecule
STAR = mol([b"C"] + [b"N", b"O"] * 150, [(0, k, 1, 1) for k in range(1, 301)])
RING = ([b"C"] * 999, [(k // 40, k % 40) for k in range(999)], [(k, k + 1, 1, 1) for k in range(998)] + [(0, 998, 1, 1)])


def per_molecule(t, got):
    """what a call left for each molecule, as comparable values: of a writer its string, flags, n_rings and its atoms' slices of
    order, rank, sym_class and atom_marks; of the fingerprint its record and its 64 words"""
    if isinstance(got, G.FpResult):
        return [(got.recs[b].tobytes(), got.bits[b].tobytes()) for b in range(t.n)]
    strings, out = device_texts(got.recs, got.out), []
    for b, m in enumerate(t.mols):
        a0, a1 = int(m["atom0"]), int(m["atom0"]) + int(m["n_atoms"])
        per_atom = [getattr(got, f)[a0:a1].tolist() for f in ("order", "rank", "sym_class", "atom_marks") if getattr(got, f) is not None]
        out.append((strings[b], int(got.recs["flags"][b]), int(got.recs["n_rings"][b]), per_atom))
    return out


@pytest.fixture(scope="module")
def batches(dev):
    """the three sets of tables and, filled as the tests ask, each pass's oracle result for them: computed once"""
    malformed = [OK]
    for bad in MALFORMED.values():
        malformed += [bad, OK]
    sets = {"alone": [OK], "malformed": malformed + SMALL + [OK], "star": [OK, STAR, OK], "ring": [OK, RING, OK]}
    tables, refs = {k: Tables(dev, v) for k, v in sets.items()}, {}

    def get(which, name):
        if (which, name) not in refs:
            refs[which, name] = PASSES[name][0](tables[which])
        return tables[which], refs[which, name]
    return get


def run_set(eng, batches, which, name):
    """the set `which` through the pass `name`: checked against its oracle, and every OK molecule in it holds what OK holds alone"""
    t, ref = batches(which, name)
    got = per_molecule(t, PASSES[name][1](eng, t, ref))
    t1, ref1 = batches("alone", name)
    alone = per_molecule(t1, PASSES[name][1](eng, t1, ref1))[0]
    refused = FP_REFUSED if name == "fingerprint" else SMILES_REFUSED
    flags = (ref["fp"] if name == "fingerprint" else ref["recs"])["flags"]
    assert not int(flags[0]) & refused, "the good molecule is written"
    for b in range(t.n):
        if t.mols["n_atoms"][b] == 5 and t.mols["n_bonds"][b] == 5:
            assert got[b] == alone, f"{name}: the good molecule at {b} differs from what it gives alone: {got[b]} != {alone}"
    return t, ref, flags, refused


@pytest.mark.parametrize("name", list(PASSES))
def test_malformed_and_smallest_molecules_between_good_ones(eng, batches, name):
    t, ref, flags, refused = run_set(eng, batches, "malformed", name)
    is_refused = [bool(int(f) & refused) for f in flags]
    assert is_refused == [False, True] * 6 + [False] * 5, (name, flags.tolist())
    if name == "fingerprint":                              # a bad symbol before a bad record before a duplicate: one bit for the last two
        assert flags[1:12:2].tolist() == [F.BAD_BOND] * 5 + [F.PSEUDO | F.BAD_BOND] and flags[13:16].tolist() == [0, 0, 0]
        assert ref["fp"]["n_bits"][13] > 2 and ref["fp"]["n_bits"][14:16].tolist() == [2, 0] and not ref["bits"][1:12:2].any()
    else:                                                  # a duplicate still counts its rings; the ranks leave no tie bit behind
        assert flags[1:12:2].tolist() == [S.FLAG_BEYOND] * 3 + [S.FLAG_DUPLICATE] * 2 + [S.FLAG_DUPLICATE | S.FLAG_PSEUDO]
        assert ref["recs"]["n_rings"][1:12:2].tolist() == [0, 0, 0, 1, 1, 1] and ref["recs"]["len"][1:12:2].tolist() == [0] * 6
        strings = [ref["out"][r["text0"]:r["text0"] + r["len"]].decode() for r in ref["recs"][13:16]]
        assert [s.replace("N", "C").replace("O", "C") for s in strings] == ["C.C.C", "C", ""]


@pytest.mark.parametrize("name", list(PASSES))
def test_one_list_longer_than_the_workgroup(eng, batches, name):
    """an atom of degree 300: its list takes more than one turn of the 256 threads in the duplicate test and in every sort"""
    t, ref, flags, refused = run_set(eng, batches, "star", name)
    assert not int(flags[1]) & refused
    if name == "fingerprint":
        assert ref["fp"]["max_paths"][1] == 300            # a leaf's bond, then each of the 299 other leaves
    else:
        assert ref["recs"]["len"][1] == 301 + 2 * 299      # 301 atoms, 299 branches


@pytest.mark.parametrize("name", ["smiles", "canonical3", "symmetric3", "fingerprint"])
def test_a_ring_of_999_fills_1998_of_the_2048_slots(eng, batches, name):
    """999 atoms and 999 bonds: the last quad of the degree scan holds atoms 996 .. 998, and off[1024] is 1998"""
    t, ref, flags, refused = run_set(eng, batches, "ring", name)
    assert not int(flags[1]) & refused
    if name == "fingerprint":
        assert ref["fp"]["max_paths"][1] == 7 and ref["fp"]["n_bits"][1] > 0
    else:
        assert ref["recs"]["len"][1] == 1001 and ref["recs"]["n_rings"][1] == 1
