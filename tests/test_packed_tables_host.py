"""CPU: the comparisons of tests/packed_tables.py, the harness of the GPU tests of the packed-table passes. An oracle's result wrapped
as a device result passes; with one element of any compared field changed, the comparison raises — so no field is compared in name
only. The text side on the pinned molecules of test_symmetry_host through symmetry_ref.pack (every output a writer of text has),
the table side on the hand table of test_normalize_host through normalize_ref.pack."""
import numpy as np
import pytest

import molfile_ref as M
import normalize_ref as N
import symmetry_ref as Y
import test_normalize_host as HN
import test_symmetry_host as HS
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE, SMILES_DTYPE
from packed_tables import (FILL, GUARD, WORD_FILL, TablesResult, TextResult, assert_refused, clean, compare_tables, compare_text,
                           same_results)


def as_bytes(x):
    return np.frombuffer(x if isinstance(x, bytes) else x.tobytes(), np.uint8).copy()


@pytest.fixture(scope="module")
def text_pair():
    """the oracle's dict for the pinned molecules with all marks, and the same as the result of a call at the exact capacity"""
    mols = []
    for name in sorted(HS.PINNED):
        mol, _, mirror = HS.PINNED[name][:3]
        mols += [mol] + ([HS.mirrored(mol, *mirror)] if mirror else [])
    assert max(len(m[0]) for m in mols) <= 8
    ref = Y.pack(*M.build_tables(mols), marks=3)
    got = TextResult(0, ref["recs"].copy(), ref["order"].copy(), ref["rank"].copy(), ref["sym_class"].copy(), ref["atom_marks"].copy(),
                     np.concatenate([as_bytes(ref["out"]), np.full(GUARD, FILL, np.uint8)]), np.array([ref["total"], 0], np.uint32), "")
    return ref, got


@pytest.fixture(scope="module")
def tables_pair():
    strings = sorted(HN.AROMATIC) + HN.NOT_AROMATIC + sorted(HN.BRACKETS)
    ref = N.pack(*HN.tables_of(strings), tables=HN.TABLES)
    got = TablesResult(0, as_bytes(clean(ref["mols"])).view(MOL_DTYPE), as_bytes(clean(ref["atoms"])), as_bytes(clean(ref["bonds"])),
                       as_bytes(ref["text"]), as_bytes(ref["atom_notes"]), np.array(list(ref["totals"]) + [0], np.uint32), "")
    return ref, got


def changed(got, field, index, name=None):
    """a copy of the result with one element of one field changed: its lowest bit flipped, or 1 added to a float"""
    x = getattr(got, field).copy()
    column = x if name is None else x[name]
    column[index] = column[index] + 1 if column.dtype.kind == "f" else column[index] ^ 1
    return got._replace(**{field: x})


def test_compare_text_passes_and_misses_no_field(text_pair):
    ref, got = text_pair
    total = ref["total"]
    assert total > 0 and len(ref["order"]) == len(ref["atom_marks"]) > 0 and got.recs.dtype == SMILES_DTYPE
    compare_text(got, ref, "SMILES")
    broken = [changed(got, "recs", len(got.recs) - 1, name) for name in SMILES_DTYPE.names]
    broken += [changed(got, "out", 0), changed(got, "out", total - 1), changed(got, "out", total), changed(got, "out", total + GUARD - 1)]
    broken += [changed(got, name, k) for name in ("order", "rank", "sym_class", "atom_marks") for k in (0, len(ref["order"]) - 1)]
    broken += [changed(got, "totals", 0), changed(got, "totals", 1), got._replace(rc=-1), got._replace(order=None)]
    for bad in broken:
        with pytest.raises(AssertionError):
            compare_text(bad, ref, "SMILES")
    plain = {k: v for k, v in ref.items() if k not in ("rank", "sym_class", "atom_marks")}     # an oracle of an older call
    compare_text(changed(got, "rank", 0)._replace(atom_marks=None), plain, "SMILES")
    with pytest.raises(AssertionError):
        compare_text(changed(got, "order", 0), plain, "SMILES")


def test_compare_tables_passes_and_misses_no_field(tables_pair):
    ref, got = tables_pair
    compare_tables(got, ref, "atom_notes")
    # mnx_mol has no padding (`reserved` is a field of it); mnx_atom has bytes 12..15 and mnx_bond bytes 6..7, which no field shows
    assert not any(12 <= o < 16 for _, o in (f[:2] for f in ATOM_DTYPE.fields.values())) and ATOM_DTYPE.itemsize == 24
    assert not any(6 <= o < 8 for _, o in (f[:2] for f in BOND_DTYPE.fields.values())) and BOND_DTYPE.itemsize == 16
    broken = [changed(got, "mols", len(got.mols) - 1, name) for name in MOL_DTYPE.names]
    broken += [changed(got, "atoms", len(got.atoms) - 24 + 15), changed(got, "bonds", len(got.bonds) - 16 + 6)]
    broken += [changed(got, name, k) for name in ("atoms", "bonds", "text", "side") for k in (0, len(getattr(got, name)) - 1)]
    broken += [changed(got, "totals", k) for k in range(4)] + [got._replace(rc=-1), got._replace(side=None), got._replace(text=got.text[:-1])]
    for bad in broken:
        with pytest.raises(AssertionError):
            compare_tables(bad, ref, "atom_notes")
    compare_tables(changed(got, "side", 0), ref)               # an entry point without a side output: not compared


def test_assert_refused_sees_one_byte_in_any_output(text_pair, tables_pair):
    message = "mnx_some_pack: null pointer"
    n, na = len(text_pair[1].recs), len(text_pair[1].order)
    text = TextResult(-1, np.full(n * 16, FILL, np.uint8).view(SMILES_DTYPE), *(np.full(na, WORD_FILL, np.uint16) for _ in range(3)),
                      np.full(na, FILL, np.uint8), np.full(100 + GUARD, FILL, np.uint8), np.full(8, FILL, np.uint8).view(np.uint32), message)
    t = tables_pair[1]
    tables = TablesResult(-1, np.full(t.mols.nbytes, FILL, np.uint8).view(MOL_DTYPE), *(np.full(len(x), FILL, np.uint8) for x in t[2:6]),
                          np.full(16, FILL, np.uint8).view(np.uint32), message)
    for got in (text, tables):
        assert_refused(got, message)
        outputs = [f for f in got._fields[1:-1]]
        for field in outputs:
            x = getattr(got, field).copy()
            x.view(np.uint8)[-1] ^= 1
            with pytest.raises(AssertionError):
                assert_refused(got._replace(**{field: x}), message)
            if field != outputs[0]:
                assert_refused(got._replace(**{field: x}), message, outputs[:1])       # only the outputs named
        for bad, expect in ((got._replace(rc=0), message), (got._replace(rc=-2), message), (got, message + "s"), (got._replace(error=""), message)):
            with pytest.raises(AssertionError):
                assert_refused(bad, expect)


def test_same_results_sees_every_field(text_pair, tables_pair):
    for _, got in (text_pair, tables_pair):
        same_results(got, got._replace())
        for field in got._fields[1:-1]:
            x = getattr(got, field).copy()
            x.view(np.uint8)[0] ^= 1
            with pytest.raises(AssertionError):
                same_results(got, got._replace(**{field: x}))
        with pytest.raises(AssertionError):
            same_results(got, got._replace(rc=1))


def test_the_respelling_passes_keep_their_python_signatures_and_c_argument_lists():
    """Engine.normalize_pack and Engine.kekulize_pack as documented, and the argument types of the two library functions in the
    header's count and order: h, the four input tables with their sizes, mols_out, the three arenas with their capacities,
    atom_notes, totals, (max_steps,) stream"""
    import ctypes as C
    import inspect

    from molnextr_amd import engine
    def parameters(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    free = inspect.Parameter.empty
    assert parameters(engine.Engine.normalize_pack) == [("self", free), ("rec", free), ("caps", None), ("keep_device", False)]
    assert parameters(engine.Engine.kekulize_pack) == [("self", free), ("rec", free), ("caps", None), ("keep_device", False), ("max_steps", 0)]
    vp, u32 = C.c_void_p, C.c_uint32
    tables_in = [vp, C.c_int32, vp, u32, vp, u32, vp, u32]
    tables_out = [vp, vp, u32, vp, u32, vp, u32]
    lib = engine.load_library()
    assert list(lib.mnx_normalize_pack.argtypes) == [vp] + tables_in + tables_out + [vp, vp, vp]
    assert list(lib.mnx_kekulize_pack.argtypes) == [vp] + tables_in + tables_out + [vp, vp, u32, vp]
    assert lib.mnx_normalize_pack.restype is C.c_int and lib.mnx_kekulize_pack.restype is C.c_int
