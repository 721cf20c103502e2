"""GPU (-m gpu): what mnx_normalize_pack and mnx_kekulize_pack share behind their rules (respell_pass.h) — a new symbol packed into
8 + 4 bytes of registers and its capped store — at the smallest shapes that can break it: one table of three molecules through
both passes, against tests/normalize_ref.py and tests/kekulize_ref.py byte for byte, guard bytes included. The molecules: atoms
whose new symbol has the speller's 12 bytes, one more of them than a whole number of threads holds; copied atoms only; respelled
and copied atoms mixed, with the text capacity ending behind byte 8 of a respelled 12-byte symbol."""
import numpy as np
import pytest

import kekulize_ref as Q
import molfile_ref as M
import normalize_ref as N
import test_normalize_host as H
from molnextr_amd.engine import MOL_KEKULIZE_REFUSED, MOL_KEKULIZED, MOL_NORMALIZE_REFUSED, MOL_UNBRACKETED, NOTE_COPIED, NOTE_KEKULIZED
from packed_tables import Tables, clean, compare_tables, dev, eng, mol, same_mols  # noqa: F401
from test_gpu_kekulize import run as kekulize
from test_gpu_normalize import run as normalize

pytestmark = pytest.mark.gpu
PER = 4                                   # RS_PER of respell_pass.h: neighbouring atoms per thread
LONG = b"[123ClH2+10]"                    # isotope >= 100, two letters, H2, a charge of two digits: normalize spells it again
LONG_AROMATIC = b"[123seH2+10]"           # the same on an aromatic atom that takes no double bond: kekulize spells [123SeH2+10]
RING = [(0, 1, 4, 4), (1, 2, 4, 4), (2, 3, 4, 4), (3, 4, 4, 4), (0, 4, 4, 4)]

MOLECULES = [mol([LONG] * (PER * 3 + 1)),                                          # the last thread holds one atom
             mol([b"[R1]", b"R", b"*", b"[Ph]", b"[R12]"], [(0, 1, 1, 1), (2, 3, 1, 1)]),
             mol([b"[R1]", LONG, b"c", b"c", b"c", b"c", LONG_AROMATIC, b"[CH4]", b"[Ph]"],
                 [(0, 1, 1, 1)] + [(i + 2, j + 2, ty, rv) for i, j, ty, rv in RING])]
# per pass: the oracle, one call on the device, the refusal's flag, which atoms' notes say that the symbol was spelled again
PASSES = {"normalize": (N, normalize, MOL_NORMALIZE_REFUSED, lambda notes: (notes & NOTE_COPIED) == 0),
          "kekulize": (Q, kekulize, MOL_KEKULIZE_REFUSED, lambda notes: (notes & NOTE_KEKULIZED) != 0)}


@pytest.fixture(scope="module")
def table(dev):
    return Tables(dev, MOLECULES)


def reference(name, arrays):
    """the oracle's tables, checked on the CPU for what the test relies on: no molecule refused, every atom of the first molecule 12
    bytes long, the second all copied, the third mixed; and the text offset of byte 9 of a respelled 12-byte symbol in the third"""
    oracle, _, refused, respelled = PASSES[name]
    ref = oracle.pack(*arrays, tables=H.TABLES)
    assert not (ref["mols"]["flags"] & refused).any() and ref["mols"]["n_atoms"].tolist() == [len(m[0]) for m in MOLECULES]
    first, second, third = (slice(int(m["atom0"]), int(m["atom0"]) + int(m["n_atoms"])) for m in ref["mols"])
    assert (ref["atoms"]["sym_len"][first] == 12).all()
    new = respelled(ref["atom_notes"])
    assert not new[second].any() and new[third].any() and not new[third].all()
    long_new = [a for a in range(third.start, third.stop) if new[a] and ref["atoms"]["sym_len"][a] == 12]
    assert long_new, "no respelled symbol of 12 bytes in the mixed molecule"
    return ref, int(ref["mols"]["text0"][2]) + int(ref["atoms"]["sym0"][long_new[0]]) + 9


def test_the_references_accept_the_three_molecules_and_spell_12_bytes():
    arrays = M.build_tables(MOLECULES)
    ref, _ = reference("normalize", arrays)
    assert ref["text"][:12 * (PER * 3 + 1)] == LONG * (PER * 3 + 1) and not (ref["atom_notes"][:PER * 3 + 1] & NOTE_COPIED).any()
    assert ref["mols"]["flags"].tolist() == [0, 0, MOL_UNBRACKETED]                # [CH4] loses its brackets
    ref, _ = reference("kekulize", arrays)
    assert b"[123SeH2+10]" in ref["text"] and ref["mols"]["flags"].tolist() == [0, 0, MOL_KEKULIZED]


@pytest.mark.parametrize("name", sorted(PASSES))
def test_three_molecules_at_exact_capacities(eng, table, name):
    ref, _ = reference(name, (table.mols, table.atoms, table.bonds, table.text))
    compare_tables(PASSES[name][1](eng, table, ref["totals"]), ref, "atom_notes")


@pytest.mark.parametrize("name", sorted(PASSES))
def test_the_text_capacity_ends_inside_the_high_word_of_a_packed_symbol(eng, table, name):
    ref, cap = reference(name, (table.mols, table.atoms, table.bonds, table.text))
    full = list(ref["totals"])
    assert cap < full[2]
    got = PASSES[name][1](eng, table, (full[0], full[1], cap))                     # the harness checks the bytes behind the capacity
    assert got.rc == 0 and got.totals.tolist() == full + [1]
    same_mols(got.mols, ref["mols"])
    assert got.atoms.tobytes() == clean(ref["atoms"]) and got.bonds.tobytes() == clean(ref["bonds"])
    assert got.text.tobytes() == ref["text"][:cap] and np.array_equal(got.side, ref["atom_notes"])
