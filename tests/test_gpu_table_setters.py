"""GPU (-m gpu): the kinds that mnx_set_fragments tests frag_of_name against are those of the LAST mnx_set_symbol_tables call — the
library keeps them on the host beside the device's copy (csrc/engine_tables.hip). One engine, three rounds of setter calls and one
expansion against the oracle of tests/expand_ref.py."""
import functools

import numpy as np
import pytest

import expand_ref as X
import molfile_ref as M
from molnextr_amd import fragments as F
from molnextr_amd.engine import MOL_EXPANDED, Engine, symbol_tables
from packed_tables import Tables, assert_refused, call_tables, compare_tables, dev, mol, path  # noqa: F401

pytestmark = pytest.mark.gpu

run = functools.partial(call_tables, "mnx_expand_pack")


def test_set_fragments_sees_the_kinds_of_the_last_symbol_tables(synth_ckpt, dev):
    eng = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        text, offsets, kinds_a, n = symbol_tables()
        fm, fa, fb, ft, fo = F.fragment_tables()
        k = int(np.nonzero(fo == 0)[0][0])                        # name k: an abbreviation, a name of fragment 0
        name = text[offsets[k]:offsets[k + 1]]
        kinds_b = kinds_a.copy()
        kinds_b[k] = 1                                             # tables B: the same names, name k an R-group

        def set_tables(kinds):
            return eng.lib.mnx_set_symbol_tables(eng.h, text, offsets.ctypes.data, kinds.ctypes.data, n)

        def set_fragments():
            return eng.lib.mnx_set_fragments(eng.h, fm.ctypes.data, len(fm), fa.ctypes.data, len(fa), fb.ctypes.data, len(fb), ft, len(ft),
                                             fo.ctypes.data, len(fo))

        t = Tables(dev, [mol([b"C", b"[" + name + b"]"], path(2))])
        assert kinds_a[k] == 2 and set_tables(kinds_a) == 0 and set_fragments() == 0     # A: frag_of_name[k] = 0 is accepted
        assert set_tables(kinds_b) == 0                                                  # B drops the fragments of A ...
        assert_refused(run(eng, t, (64, 64, 64)), "mnx_expand_pack: call mnx_set_fragments first")
        assert set_fragments() == -1                                                     # ... and the same call is refused
        assert eng.lib.mnx_last_error(eng.h).decode() == "mnx_set_fragments: frag_of_name[%d]: only an abbreviation (kind 2) takes a fragment" % k
        assert set_tables(kinds_a) == 0 and set_fragments() == 0                         # A again
        tables = M.name_tables()
        ref = X.pack(t.mols, t.atoms, t.bonds, t.text, frags=X.library(tables=tables), tables=tables)
        assert int(ref["mols"]["flags"][0]) == MOL_EXPANDED and int(ref["mols"]["n_atoms"][0]) == 1 + int(fm["n_atoms"][0])
        compare_tables(run(eng, t, ref["totals"]), ref, "origin")
    finally:
        eng.close()
