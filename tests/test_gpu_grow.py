"""GPU (-m gpu): what mnx_formula_pack and mnx_expand_pack share behind their rules (grow_pass.h) — the five scans over the atoms,
the splice of a label's bonds into its row, the appended records and their capped stores — at the smallest shapes that can break
it: one table of three molecules through both passes and through the chain formula -> expand, against tests/formula_ref.py and
tests/expand_ref.py byte for byte, guard bytes included. The molecules: 17 atoms (two threads' worth of 8, plus one) with a formula
label and a table label on either side of a thread boundary of the scan and a label at the last atom; no label that either pass
replaces; labels with own-row bonds in front of and behind them, and rows that move. Each capacity in turn ends inside the first
molecule's appended records."""
import pytest

import expand_ref as X
import formula_ref as F
import molfile_ref as M
import test_formula_host as FH
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_EXPANDED, MOL_FORMULA_EXPANDED, MOL_LABEL_LEFT
from packed_tables import Tables, call_tables, clean, compare_tables, dev, eng, mol, path, same_mols  # noqa: F401
from test_gpu_formula import run as formula

pytestmark = pytest.mark.gpu
PER = 8                                   # GR_PER of grow_pass.h: neighbouring atoms per thread
OWN = 2 * PER + 1                         # atoms of the first molecule
FIRST = [b"C"] * OWN
FIRST[PER - 1], FIRST[PER], FIRST[OWN - 1] = b"[CH2CH3]", b"[OMe]", b"[N(CH3)2]"
MOLECULES = [mol(FIRST, path(7) + [(6, 7, 1, 1), (6, 8, 1, 1), (6, 9, 1, 1)] + path(8, first=9)),
             mol([b"C", b"N", b"O", b"[R1]"], path(4)),
             mol([b"C", b"[COOCH3]", b"C", b"[Ph]", b"[CH2Ph]", b"N"], [(0, 1, 1, 1), (0, 2, 1, 1), (2, 3, 1, 1), (2, 4, 1, 1), (2, 5, 1, 1)])]


def expand(eng, t, caps, **over):
    return call_tables("mnx_expand_pack", eng, t, caps, **over)


# per pass: the oracle, one call on the device, the atom of the first molecule whose label it replaces next to the thread boundary
PASSES = {"formula": (F, formula, PER - 1), "expand": (X, expand, PER)}


@pytest.fixture(scope="module")
def table(dev):
    return Tables(dev, MOLECULES)


def reference(name, arrays):
    return PASSES[name][0].pack(*arrays, frags=FH.FRAGS, tables=FH.TABLES)


def arrays_of(ref):
    return ref["mols"], ref["atoms"], ref["bonds"], ref["text"]


def test_the_references_accept_the_three_molecules():
    arrays = M.build_tables(MOLECULES)
    assert arrays[0]["n_atoms"].tolist() == [OWN, 4, 6] and arrays[0]["n_bonds"].tolist() == [16, 3, 5]
    f, x = reference("formula", arrays), reference("expand", arrays)
    assert f["mols"]["flags"].tolist() == [MOL_FORMULA_EXPANDED, 0, MOL_FORMULA_EXPANDED]
    assert f["mols"]["n_atoms"].tolist() == [20, 4, 10] and tuple(f["totals"]) == (34, 31, 47)
    assert x["mols"]["flags"].tolist() == [MOL_EXPANDED | MOL_LABEL_LEFT, MOL_LABEL_LEFT, MOL_EXPANDED | MOL_LABEL_LEFT]
    assert x["mols"]["n_atoms"].tolist() == [18, 4, 11] and tuple(x["totals"]) == (33, 31, 64)
    fx = reference("expand", arrays_of(f))
    assert fx["mols"]["flags"].tolist() == [MOL_EXPANDED, MOL_LABEL_LEFT, MOL_EXPANDED]
    assert fx["mols"]["n_atoms"].tolist() == [21, 4, 20] and tuple(fx["totals"]) == (45, 44, 48)


@pytest.mark.parametrize("name", sorted(PASSES))
def test_three_molecules_at_exact_capacities(eng, table, name):
    ref = reference(name, (table.mols, table.atoms, table.bonds, table.text))
    compare_tables(PASSES[name][1](eng, table, ref["totals"]), ref, "origin")


def test_the_chain_formula_then_expand_on_the_device(eng, table):
    f = reference("formula", (table.mols, table.atoms, table.bonds, table.text))
    got = formula(eng, table, f["totals"])
    compare_tables(got, f, "origin")
    grown = Tables(table.dev, arrays=(got.mols, got.atoms.view(ATOM_DTYPE), got.bonds.view(BOND_DTYPE), got.text.tobytes()))
    fx = reference("expand", arrays_of(f))
    compare_tables(expand(eng, grown, fx["totals"]), fx, "origin")


def short_capacities(ref, label):
    """per capacity, the one that ends inside the appended records of the first molecule (atom0 = bond0 = text0 = 0): its own atoms
    plus one; one record behind the bonds spliced in behind row `label`; one byte into the first appended symbol"""
    m, bonds = ref["mols"][0], ref["bonds"]
    spliced = [k for k in range(int(m["n_bonds"])) if bonds["i"][k] == label and bonds["j"][k] >= OWN]
    assert spliced and spliced == list(range(spliced[0], spliced[-1] + 1)) and spliced[-1] + 2 < int(m["n_bonds"])
    assert int(bonds["i"][spliced[-1] + 1]) > label and int(bonds["j"][spliced[-1] + 1]) < OWN          # an own bond, moved back
    return {"atoms": OWN + 1, "bonds": spliced[-1] + 2, "text": int(ref["atoms"]["sym0"][OWN]) + 1}


@pytest.mark.parametrize("which", ("atoms", "bonds", "text"))
@pytest.mark.parametrize("name", sorted(PASSES))
def test_a_capacity_ends_inside_the_appended_records(eng, table, name, which):
    ref = reference(name, (table.mols, table.atoms, table.bonds, table.text))
    full = list(ref["totals"])
    caps = list(full)
    k = ("atoms", "bonds", "text").index(which)
    caps[k] = short_capacities(ref, PASSES[name][2])[which]
    assert 0 < caps[k] < full[k]
    got = PASSES[name][1](eng, table, caps)                                        # the harness checks the bytes behind every capacity
    assert got.rc == 0 and got.totals.tolist() == full + [1]
    same_mols(got.mols, ref["mols"])
    sizes = (caps[0] * ATOM_DTYPE.itemsize, caps[1] * BOND_DTYPE.itemsize, caps[2], caps[0] * 2)
    exact = (clean(ref["atoms"]), clean(ref["bonds"]), ref["text"], ref["origin"].tobytes())
    for part, have, want, size in zip(("atoms", "bonds", "text", "origin"), (got.atoms, got.bonds, got.text, got.side), exact, sizes):
        assert have.size == size and have.tobytes() == want[:size], part
