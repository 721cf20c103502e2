"""CPU: the oracle of mnx_main_pack (tests/main_ref.py) on molecules written out by hand with their expected tables written out by
hand — the component with the most atoms stays, among equals the one with the lowest atom, as the reference's
_keep_main_molecule (GetMolFrags, np.argmax) —, what travels with a kept record, the refusals, and engine.py's names against the
header. tests/test_gpu_main.py runs the device against the same cases."""
import os
import re

import numpy as np
import pytest

import main_ref as X
import molfile_ref as M
from molnextr_amd import engine
from packed_tables import mol, path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT, TIE, REFUSED = 1 << 18, 1 << 19, 1 << 20

# name, the molecule (atom k lies at bin (3k % 64, 5k % 64) and has index k), and what is left of it: (n_atoms, n_bonds, smiles_len,
# flags), atoms [(sym0, sym_len, index, x_bin, y_bin)], bonds [(i, j, type, rev)], text, origin
CASES = [
    ("zero atoms", mol([]),
     (0, 0, 0, 0), [], [], b"", []),
    ("one atom", mol([b"C"]),
     (1, 0, 1, 0), [(0, 1, 0, 0, 0)], [], b"C", [0]),
    ("one component", mol([b"C", b"N", b"O"], path(3)),
     (3, 2, 3, 0), [(0, 1, 0, 0, 0), (1, 1, 1, 3, 5), (2, 1, 2, 6, 10)], [(0, 1, 1, 1), (1, 2, 1, 1)], b"CNO", [0, 1, 2]),
    ("2 + 3: the second stays, renumbered", mol([b"C", b"Cl", b"N", b"[NH3+]", b"O"], [(0, 1, 1, 1), (2, 3, 2, 2), (3, 4, 1, 5)]),
     (3, 2, 8, KEPT), [(0, 1, 2, 6, 10), (1, 6, 3, 9, 15), (7, 1, 4, 12, 20)], [(0, 1, 2, 2), (1, 2, 1, 5)], b"N[NH3+]O", [2, 3, 4]),
    ("2 + 2: the first stays, a tie", mol([b"C", b"N", b"O", b"Cl"], [(0, 1, 1, 1), (2, 3, 1, 1)]),
     (2, 1, 2, KEPT | TIE), [(0, 1, 0, 0, 0), (1, 1, 1, 3, 5)], [(0, 1, 1, 1)], b"CN", [0, 1]),
    ("1 + 3 + 2: the middle stays", mol([b"[Na+]", b"C", b"C", b"O", b"Br", b"I"], [(1, 2, 1, 1), (2, 3, 2, 2), (4, 5, 1, 1)]),
     (3, 2, 3, KEPT), [(0, 1, 1, 3, 5), (1, 1, 2, 6, 10), (2, 1, 3, 9, 15)], [(0, 1, 1, 1), (1, 2, 2, 2)], b"CCO", [1, 2, 3]),
    ("only isolated atoms: atom 0 stays, a tie", mol([b"Cl", b"C", b"N"]),
     (1, 0, 2, KEPT | TIE), [(0, 2, 0, 0, 0)], [], b"Cl", [0]),
    ("a self bond joins nothing and stays a record", mol([b"C", b"N", b"O", b"S"], [(0, 0, 1, 1), (1, 2, 1, 1), (2, 2, 3, 3)]),
     (2, 2, 2, KEPT), [(0, 1, 1, 3, 5), (1, 1, 2, 6, 10)], [(0, 1, 1, 1), (1, 1, 3, 3)], b"NO", [1, 2]),
    ("the same pair three times counts two atoms", mol([b"C", b"N", b"O", b"S", b"P"],
                                                      [(0, 1, 1, 1), (0, 1, 2, 2), (1, 0, 1, 1), (2, 3, 1, 1), (3, 4, 1, 1)]),
     (3, 2, 3, KEPT), [(0, 1, 2, 6, 10), (1, 1, 3, 9, 15), (2, 1, 4, 12, 20)], [(0, 1, 1, 1), (1, 2, 1, 1)], b"OSP", [2, 3, 4]),
    ("the same pair twice in the kept component", mol([b"C", b"N", b"O"], [(1, 2, 1, 1), (1, 2, 2, 5)]),
     (2, 2, 2, KEPT), [(0, 1, 1, 3, 5), (1, 1, 2, 6, 10)], [(0, 1, 1, 1), (0, 1, 2, 5)], b"NO", [1, 2]),
    ("unsorted records keep their order", mol([b"C", b"N", b"O", b"S", b"P"], [(3, 4, 1, 1), (0, 1, 1, 1), (4, 2, 2, 2)]),
     (3, 2, 3, KEPT), [(0, 1, 2, 6, 10), (1, 1, 3, 9, 15), (2, 1, 4, 12, 20)], [(1, 2, 1, 1), (2, 0, 2, 2)], b"OSP", [2, 3, 4]),
]
MOLECULES = [c[1] for c in CASES]


def as_lists(ref):
    """an oracle's result as plain tuples: mols, atoms, bonds (scores apart)"""
    return ([tuple(int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len", "flags", "reserved")) for m in ref["mols"]],
            [tuple(int(a[k]) for k in ("sym0", "sym_len", "index", "x_bin", "y_bin")) for a in ref["atoms"]],
            [tuple(int(b[k]) for k in ("i", "j", "type", "rev")) for b in ref["bonds"]])


@pytest.mark.parametrize("name,molecule,counts,atoms,bonds,text,origin", CASES, ids=[c[0] for c in CASES])
def test_one_molecule(name, molecule, counts, atoms, bonds, text, origin):
    ref = X.pack(*M.build_tables([molecule]))
    got_mols, got_atoms, got_bonds = as_lists(ref)
    n_atoms, n_bonds, smiles_len, flags = counts
    assert got_mols == [(0, n_atoms, 0, n_bonds, 0, smiles_len, flags, 0)]
    assert got_atoms == atoms and got_bonds == bonds
    assert ref["text"] == text and ref["origin"].tolist() == origin and ref["origin"].dtype == np.uint16
    assert ref["totals"] == (n_atoms, n_bonds, smiles_len)


def test_all_molecules_in_one_table():
    ref = X.pack(*M.build_tables(MOLECULES))
    got_mols, got_atoms, got_bonds = as_lists(ref)
    a0 = b0 = t0 = 0
    for got, (name, _, (n_atoms, n_bonds, smiles_len, flags), atoms, bonds, text, origin) in zip(got_mols, CASES):
        assert got == (a0, n_atoms, b0, n_bonds, t0, smiles_len, flags, 0), name
        assert got_atoms[a0:a0 + n_atoms] == atoms and got_bonds[b0:b0 + n_bonds] == bonds, name
        assert ref["text"][t0:t0 + smiles_len] == text and ref["origin"][a0:a0 + n_atoms].tolist() == origin, name
        a0, b0, t0 = a0 + n_atoms, b0 + n_bonds, t0 + smiles_len
    assert ref["totals"] == (a0, b0, t0) == (len(ref["atoms"]), len(ref["bonds"]), len(ref["text"]))


def test_scores_indices_and_bit_0_travel_and_other_bits_do_not():
    mols, atoms, bonds, text = M.build_tables(MOLECULES)
    rng = np.random.default_rng(5)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"] = rng.integers(0, 500, len(atoms))
    mols["flags"] = rng.integers(0, 2, len(mols)) | 2 | 16 | 1 << 10 | 1 << 20       # bits of other passes, and a stale refusal
    ref = X.pack(mols, atoms, bonds, text)
    plain = X.pack(*M.build_tables(MOLECULES))
    assert (ref["mols"]["flags"] == (plain["mols"]["flags"] | (mols["flags"] & 1))).all()
    assert (ref["mols"]["overall_score"] == mols["overall_score"]).all()
    for m_in, m_out in zip(mols, ref["mols"]):
        a_in, a_out = atoms[int(m_in["atom0"]):][:int(m_in["n_atoms"])], ref["atoms"][int(m_out["atom0"]):][:int(m_out["n_atoms"])]
        origin = ref["origin"][int(m_out["atom0"]):][:int(m_out["n_atoms"])]
        assert (a_out["score"] == a_in["score"][origin]).all() and (a_out["index"] == a_in["index"][origin]).all()
    k = 3                                                                          # 2 + 3: its second and third bond stay
    b_in, b_out = bonds[int(mols["bond0"][k]):][:3], ref["bonds"][int(ref["mols"]["bond0"][k]):][:2]
    assert b_out["score"].tolist() == b_in["score"][1:].tolist()


def test_refusals_leave_empty_molecules_and_the_others_alone():
    ok = mol([b"C", b"N", b"O"], [(1, 2, 1, 1)])
    tables = M.build_tables([ok, mol([b"C", b"N"], [(0, 2, 1, 1)]), ok, mol([b"C"] * 2048), mol([b"C"] * 2047), ok])
    ref = X.pack(*tables)
    assert ref["mols"]["flags"].tolist() == [KEPT, REFUSED, KEPT, REFUSED, KEPT | TIE, KEPT]
    assert ref["mols"]["n_atoms"].tolist() == [2, 0, 2, 0, 1, 2] and ref["mols"]["atom0"].tolist() == [0, 2, 2, 4, 4, 5]
    assert ref["origin"].tolist() == [1, 2, 1, 2, 0, 1, 2]
    mols, atoms, bonds, text = tables
    for cut in ({"n_atom_records": len(atoms) - 1}, {"n_bond_records": len(bonds) - 1}, {"n_text_bytes": len(text) - 1}):
        assert X.pack(*tables, **cut)["mols"]["flags"].tolist() == [KEPT, REFUSED, KEPT, REFUSED, KEPT | TIE, REFUSED]
    atoms = atoms.copy()
    atoms["sym0"][1] = 60000                                                       # a symbol beyond the text
    assert X.pack(mols, atoms, bonds, text)["mols"]["flags"].tolist() == [REFUSED, REFUSED, KEPT, REFUSED, KEPT | TIE, KEPT]


def test_the_first_of_the_largest_is_np_argmax_over_components_listed_by_their_lowest_atom():
    """the rule in the reference's own words, on random graphs: GetMolFrags lists components by their lowest atom"""
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(2, 30))
        pairs = [tuple(int(v) for v in rng.integers(0, n, 2)) for _ in range(int(rng.integers(0, n)))]
        keep, flags = X.main_component(n, pairs)
        adjacent = {a: {a} for a in range(n)}
        for i, j in pairs:
            adjacent[i].add(j)
            adjacent[j].add(i)
        frags, seen = [], set()
        for a in range(n):                                                         # ascending lowest atom
            if a not in seen:
                frag, todo = set(), [a]
                while todo:
                    x = todo.pop()
                    if x not in frag:
                        frag.add(x)
                        todo += adjacent[x] - frag
                frags.append(sorted(frag))
                seen |= frag
        sizes = [len(f) for f in frags]
        main = frags[int(np.argmax(sizes))]
        assert [a for a in range(n) if keep[a]] == main
        assert flags == (0 if len(frags) == 1 else KEPT | (TIE if sizes.count(max(sizes)) > 1 else 0))


def test_engine_names_match_the_header():
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    assert "mnx_main_pack" in engine.SYMBOLS and re.search(r"\bint mnx_main_pack\s*\(", hdr)
    defines = {k: int(v) for k, v in re.findall(r"#define (MNX_MOL_MAIN_[A-Z]+) (\d+)u", hdr)}
    assert defines == {"MNX_MOL_MAIN_KEPT": engine.MOL_MAIN_KEPT, "MNX_MOL_MAIN_TIE": engine.MOL_MAIN_TIE,
                       "MNX_MOL_MAIN_REFUSED": engine.MOL_MAIN_REFUSED}
    assert (engine.MOL_MAIN_KEPT, engine.MOL_MAIN_TIE, engine.MOL_MAIN_REFUSED) == (KEPT, TIE, REFUSED) == (X.KEPT, X.TIE, X.REFUSED)
    every = {k: int(v) for k, v in re.findall(r"#define (MNX_MOL_[A-Z_]+) (\d+)u", hdr) if not k.endswith("_STEPS")}
    values = list(every.values())
    assert len(set(values)) == len(values) and all(v & (v - 1) == 0 for v in values), every      # one bit each, no bit twice
    # the argument list is mnx_expand_pack's, exactly
    args = {fn: re.sub(r"\s+", " ", re.search(r"\bint " + fn + r"\s*\(([^;]*)\);", hdr).group(1)) for fn in ("mnx_main_pack", "mnx_expand_pack")}
    assert args["mnx_main_pack"] == args["mnx_expand_pack"]
