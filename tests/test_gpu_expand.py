"""GPU (-m gpu): mnx_set_fragments / mnx_expand_pack — abbreviation labels replaced by their fragments on the device — against the
oracle of tests/expand_ref.py, records field by field and tables byte for byte (no tolerances): the smallest shapes at which the
kernel's scans, searches and loops take another turn, the refusals, the capacity protocol, determinism, the argument errors of
mnx_set_fragments, the chain into the canonical SMILES writer and the molfile writer, the label-versus-drawn-out pairs of the
host test, and one end-to-end run."""
import functools

import numpy as np
import pytest

import canon_ref as K
import expand_ref as X
import molfile_ref as M
import test_expand_host as H
from molnextr_amd import fragments as F
from molnextr_amd import weights as W
from molnextr_amd.engine import MOL_EXPAND_REFUSED, MOL_EXPANDED, MOL_LABEL_LEFT, Engine, symbol_tables
from packed_tables import (UTF2, Tables, _p, assert_refused, call_tables, clean, compare_tables, dev, eng, mol, path, same_mols,  # noqa: F401
                           same_results)

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the writers' end-to-end tests


@pytest.fixture(scope="module")
def tables():
    return M.name_tables()


@pytest.fixture(scope="module")
def library(tables):
    return X.library(tables=tables)


run = functools.partial(call_tables, "mnx_expand_pack")       # run(eng, t, caps, **over); the result's `side` is `origin`


def check(eng, t, library, tables, ref=None):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    ref = ref or X.pack(t.mols, t.atoms, t.bonds, t.text, frags=library, tables=tables)
    compare_tables(run(eng, t, ref["totals"]), ref, "origin")
    return ref


SMALL = [
    mol([b"C", b"N", b"O"], path(3)),                                              # no label
    mol([b"[Ph]"]),                                                                # a label with no bond
    mol([b"C", b"[OMe]"], path(2)),                                                # one bond
    mol([b"[Ph]", b"C", b"N", b"O"], [(0, 1, 1, 1), (0, 2, 2, 2), (0, 3, 5, 6)]),  # three bonds, the label as atom 0
    mol([b"C", b"C", b"[CO2Et]"], path(3)),                                        # the label as the last atom
    mol([b"OMe", b"[Et]"], path(2)),                                               # two labels bonded to each other
    mol([b"[Boc]", b"[Ph]", b"[NO2]", b"[tBu]"], [(0, 1, 1, 1), (0, 3, 1, 1), (1, 2, 1, 1), (2, 3, 1, 1)]),
    mol([]),                                                                       # no atom
    mol([b"[Fmoc]", b"[" + UTF2 + b"]", UTF2, b"[R1]", b"[Tcs]", b"*", b"[Ac]"], [(0, 1, 1, 1), (0, 6, 1, 1), (1, 2, 4, 4), (5, 6, 6, 5)]),
    mol([b"[3,5-[CF3]2C6H3]", b"[2, 4-Cl2C6H3]", b"Ph", b"[Xx]", b""], path(5)),
]


def test_small_molecules_one_by_one_and_together(eng, dev, library, tables):
    for m in SMALL:
        check(eng, Tables(dev, [m]), library, tables)                              # n = 1
    ref = check(eng, Tables(dev, SMALL), library, tables)
    flags = ref["mols"]["flags"].tolist()
    assert flags[:8] == [0, MOL_EXPANDED, MOL_EXPANDED, MOL_EXPANDED, MOL_EXPANDED, MOL_EXPANDED, MOL_EXPANDED, 0]
    assert flags[8] == MOL_EXPANDED | MOL_LABEL_LEFT and flags[9] == MOL_EXPANDED | MOL_LABEL_LEFT
    assert ref["mols"]["n_atoms"].tolist()[:7] == [3, 6, 3, 9, 7, 4, 6 + 5 + 2 + 3 + 4]


def test_scores_indices_and_the_truncated_bit_travel(eng, dev, library, tables):
    mols, atoms, bonds, text = M.build_tables(SMALL)
    rng = np.random.default_rng(1)
    atoms["score"], bonds["score"], mols["overall_score"] = rng.random(len(atoms)), rng.random(len(bonds)), rng.random(len(mols))
    atoms["index"] = rng.integers(0, 500, len(atoms))
    mols["flags"] = rng.integers(0, 2, len(mols))
    check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)), library, tables)


@pytest.fixture(scope="module")
def batch(dev, library, tables):
    """1025 random molecules of every symbol class with labels (one past the scan tile of 1024) and the oracle's expansion"""
    t = Tables(dev, H.random_batch(np.random.default_rng(7), 1025))
    return t, X.pack(t.mols, t.atoms, t.bonds, t.text, frags=library, tables=tables)


def test_1025_random_molecules_and_two_runs_with_identical_bytes(eng, batch, library, tables):
    t, ref = batch
    assert 500 < (ref["mols"]["flags"] & MOL_EXPANDED).astype(bool).sum() and (ref["mols"]["flags"] & MOL_LABEL_LEFT).any()
    check(eng, t, library, tables, ref)
    same_results(run(eng, t, ref["totals"]), run(eng, t, ref["totals"]))


def test_large_molecules_and_refusals(eng, dev, library, tables):
    rng = np.random.default_rng(3)
    pool = [b"C", b"N", b"[Ph]", b"[OMe]", b"[Fmoc]", b"[R1]", b"c"]
    big = [pool[k] for k in rng.integers(0, len(pool), 257)]                       # more than one pass of a 256-thread workgroup
    ring = path(257) + [(0, 256, 1, 1)]
    most = [b"[Ph]", b"C"] * 1023 + [b"[Ph]"]                                      # 2047 atoms: the most that is expanded
    ok = mol([b"C", b"[OMe]"], path(2))
    molecules = [mol(big, sorted(ring)), mol(most, path(2047)), mol([b"C"] * 2048, path(2048)), ok,
                 mol([b"C", b"[OMe]", b"N"], [(1, 2, 1, 1), (0, 1, 1, 1)]),        # bond records not sorted by i
                 mol([b"C", b"[OMe]"], [(0, 2, 1, 1)]), ok]                        # a bond to an atom that is not there
    t = Tables(dev, molecules)
    ref = check(eng, t, library, tables)
    assert [int(f) & MOL_EXPAND_REFUSED for f in ref["mols"]["flags"]] == [0, 0, 8, 0, 8, 8, 0]
    assert ref["mols"]["n_atoms"][1] == 2047 + 1024 * 5 and ref["mols"]["n_atoms"].tolist()[2:] == [0, 3, 0, 0, 3]
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off; a symbol behind the text
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        want = X.pack(t.mols, t.atoms, t.bonds, t.text, frags=library, tables=tables, n_atom_records=cut.get("na"),
                      n_bond_records=cut.get("nb"), n_text_bytes=cut.get("nt"))
        assert int(want["mols"]["flags"][-1]) & MOL_EXPAND_REFUSED
        a = run(eng, t, want["totals"], **cut)
        assert a.rc == 0 and a.totals.tolist() == list(want["totals"]) + [0]
        same_mols(a.mols, want["mols"])
        assert a.atoms.tobytes() == clean(want["atoms"]) and a.bonds.tobytes() == clean(want["bonds"]) and a.text.tobytes() == want["text"]
    mols, atoms, bonds, text = M.build_tables([ok, ok])
    atoms["sym0"][3] = 60000
    check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)), library, tables)


def test_a_fragment_of_32_atoms_set_by_the_caller(eng, dev, tables):
    """a test-only library through mnx_set_fragments: the 32-atom limit, bonds handed over unsorted, a name redefined"""
    own = {"Fmoc": "C1CCCCC1" + "C" * 24 + "(=O)O", "Ph": "N#C", "OMe": "[Si](C)(C)C.Cl"}
    frags = {k.encode(): X.read_fragment(v, tables) for k, v in own.items()}
    assert len(frags[b"Fmoc"][0]) == 32
    fm, fa, fb, ft, fo = F.fragment_tables(own)
    for m in fm:                                                                   # the host sorts a fragment's bonds
        b0, nb = int(m["bond0"]), int(m["n_bonds"])
        fb[b0:b0 + nb] = fb[b0:b0 + nb][::-1]
    eng.set_fragments(fm, fa, fb, ft, fo)
    try:
        t = Tables(dev, SMALL + [mol([b"[Fmoc]"] * 300, path(300)), mol([b"[Ph]", b"[OMe]", b"[Boc]"], path(3))])
        ref = check(eng, t, frags, tables)
        assert ref["mols"]["n_atoms"].tolist()[-2:] == [300 * 32, 2 + 5 + 1] and int(ref["mols"]["flags"][-1]) == MOL_EXPANDED | MOL_LABEL_LEFT
    finally:
        eng._set_fragments()
    check(eng, Tables(dev, SMALL), X.library(tables=tables), tables)               # the project's library again


def test_capacities_exact_and_one_short(eng, batch):
    """each capacity one record or byte short, separately: nothing is written beyond it, what lies in front of it is right, and
    mols_out and totals are complete"""
    t, ref = batch
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8),
             np.frombuffer(ref["text"], np.uint8), ref["origin"].view(np.uint8))
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, t, caps)                                                      # run() checks the FILL bytes behind every capacity
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same_mols(a.mols, ref["mols"])
        for got, want in zip((a.atoms, a.bonds, a.text, a.side), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, t, (0, 0, 0), atoms_out=None, bonds_out=None, text_out=None, origin=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]                           # the sizing call
    same_mols(a.mols, ref["mols"])


def test_engine_expand_pack_sizes_itself(eng, batch):
    t, ref = batch
    rec = {"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}
    for caps in (None, (1, 1, 1)):
        ex = eng.expand_pack(rec, caps=caps)
        same_mols(ex["mols"], ref["mols"])
        assert ex["atoms"].tobytes() == clean(ref["atoms"]) and ex["bonds"].tobytes() == clean(ref["bonds"]) and ex["text"] == ref["text"]
        assert ex["origin"].tolist() == ref["origin"].tolist() and ex["totals"].tolist() == list(ref["totals"]) + [0]


def test_chain_into_the_canonical_writer_and_the_molfile_writer(eng, batch, tables):
    """device expand -> device mnx_smiles_pack_canonical (marks 3) and mnx_molfile_pack on the device's output, against the
    writers' oracles run on the expansion oracle's tables"""
    t, ref = batch
    ex = eng.expand_pack({"mols": t.mols, "atoms": t.atoms, "bonds": t.bonds, "text": t.text}, keep_device=True)
    want = K.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], 3, tables)
    recs, order, data, rank, sym_class = eng.smiles_pack(ex, stereo=True, double_bonds=True, canonical=True)
    assert data == want["out"] and recs.tobytes() == want["recs"].tobytes()
    assert order.tolist() == want["order"].tolist() and rank.tolist() == want["rank"].tolist() and sym_class.tolist() == want["sym_class"].tolist()
    files, data = eng.molfile_pack(ex)
    want = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=tables)
    assert data == want["out"] and files.tobytes() == want["files"].tobytes()


@pytest.mark.parametrize("name", sorted(H.DRAWN_OUT))
def test_a_label_and_the_drawn_out_group_get_the_same_canonical_string(eng, name):
    labelled, drawn = H.label_and_drawn_out(name, np.random.default_rng(sum(name.encode())))
    mols, atoms, bonds, text = M.build_tables([labelled, drawn])
    ex = eng.expand_pack({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text})
    assert ex["mols"]["flags"].tolist() == [MOL_EXPANDED, 0]
    recs, order, data, rank, sym_class = eng.smiles_pack(ex, canonical=True)
    a, b = (data[r["text0"]:r["text0"] + r["len"]] for r in recs)
    assert a == b and len(a) > 0 and b"*" not in a, (a, b)


def fragment_args(eng, **change):
    """the arguments of one mnx_set_fragments call on the project's library, host arrays kept alive by the caller"""
    fm, fa, fb, ft, fo = (x.copy() if isinstance(x, np.ndarray) else x for x in F.fragment_tables())
    keep = {"mols": fm, "atoms": fa, "bonds": fb, "text": ft, "frag_of_name": fo}
    for key, edit in change.items():
        if callable(edit):
            edit(keep[key])
    a = {"h": eng.h, "frags": keep["mols"].ctypes.data, "n_frags": len(fm), "atoms": fa.ctypes.data, "na": len(fa),
         "bonds": fb.ctypes.data, "nb": len(fb), "text": ft, "nt": len(ft), "frag_of_name": fo.ctypes.data, "n_names": len(fo)}
    a.update({k: v for k, v in change.items() if not callable(v)})
    return keep, a


def test_set_fragments_argument_errors(eng, dev, synth_ckpt, library, tables):
    """every refusal returns MNX_ERR_INVALID_ARG with its text, copies nothing and launches nothing: the library set before stays"""
    def refused(expect, **change):
        keep, a = fragment_args(eng, **change)
        assert eng.lib.mnx_set_fragments(*a.values()) == -1
        msg = eng.lib.mnx_last_error(eng.h).decode()
        assert msg.startswith("mnx_set_fragments: ") and expect in msg, msg

    raw, offsets, kinds, n = symbol_tables()
    rgroup = int(np.nonzero(kinds == 1)[0][0])

    def set_field(table, field, value, k=0):
        def edit(a):
            a[field][k] = value
        return {table: edit}

    refused("n_frags outside 0..512", n_frags=513)
    refused("n_frags outside 0..512", n_frags=-1)
    refused("n_names must be the n of mnx_set_symbol_tables", n_names=n - 1)
    for name in ("frags", "atoms", "bonds", "text", "frag_of_name"):
        refused("null pointer", **{name: None})
    refused("atoms; 1 to 32 required", **set_field("mols", "n_atoms", 0))
    refused("atoms; 1 to 32 required", **set_field("mols", "n_atoms", 33))
    refused("end behind a table", **set_field("mols", "atom0", 1 << 30))
    refused("end behind a table", **set_field("mols", "bond0", 1 << 30))
    refused("end behind a table", **set_field("mols", "text0", 1 << 30))
    refused("end behind a table", na=3)
    refused("a symbol has 1 to 8 bytes", **set_field("atoms", "sym_len", 0))
    refused("a symbol has 1 to 8 bytes", **set_field("atoms", "sym_len", 9))
    refused("its symbol ends behind the text", **set_field("atoms", "sym0", 1 << 20))
    fm = F.fragment_tables()[0]
    k = int(fm["bond0"][np.nonzero(fm["n_bonds"] > 1)[0][0]])                      # the first bond of a fragment with two
    refused("i < j < n_atoms required", **set_field("bonds", "i", 31, k))
    refused("i < j < n_atoms required", **set_field("bonds", "j", 32, k))
    refused("type 1 to 4 and rev == type required", **set_field("bonds", "type", 5, k))
    refused("type 1 to 4 and rev == type required", **set_field("bonds", "type", 0, k))
    refused("type 1 to 4 and rev == type required", **set_field("bonds", "rev", 3, k))

    def twice(b):
        b["i"][k + 1], b["j"][k + 1] = b["i"][k], b["j"][k]
    refused("the same pair of atoms in two bonds", bonds=twice)
    refused("outside -1..", frag_of_name=lambda a: a.__setitem__(0, len(fm)))
    refused("outside -1..", frag_of_name=lambda a: a.__setitem__(0, -2))
    refused("only an abbreviation (kind 2) takes a fragment", frag_of_name=lambda a: a.__setitem__(rgroup, 0))
    check(eng, Tables(dev, SMALL), library, tables)                                # the library set at construction still stands

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        keep, a = fragment_args(bare)
        assert bare.lib.mnx_set_fragments(*a.values()) == -1 and b"call mnx_set_symbol_tables first" in bare.lib.mnx_last_error(bare.h)
        t = Tables(dev, SMALL)
        rc = run(bare, t, (1, 1, 1)).rc
        assert rc == -1 and b"mnx_expand_pack: call mnx_set_symbol_tables first" in bare.lib.mnx_last_error(bare.h)
        Engine._set_symbol_tables(bare)
        rc = run(bare, t, (1, 1, 1)).rc
        assert rc == -1 and b"mnx_expand_pack: call mnx_set_fragments first" in bare.lib.mnx_last_error(bare.h)
        keep, a = fragment_args(bare, n_frags=0, frag_of_name=lambda x: x.fill(-1))     # an empty library: nothing expands
        assert bare.lib.mnx_set_fragments(*a.values()) == 0
        check(bare, t, {}, tables)
        Engine._set_fragments(bare)
        check(bare, t, library, tables)
        Engine._set_symbol_tables(bare)                                            # new names drop the fragments
        assert run(bare, t, (1, 1, 1)).rc == -1 and b"call mnx_set_fragments first" in bare.lib.mnx_last_error(bare.h)
    finally:
        bare.close()


def test_expand_pack_argument_errors(eng, dev):
    t = Tables(dev, SMALL)

    def refused(expect, **over):
        assert_refused(run(eng, t, (64, 64, 64), **over), "mnx_expand_pack: " + expect)

    for name in ("mols", "atoms", "bonds", "text", "mols_out", "atoms_out", "bonds_out", "text_out", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, the output tables too, totals 4-byte, origin 2-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2), ("mols_out", 0), ("atoms_out", 1), ("bonds_out", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, totals=_p(t.d[0], 2))
    refused(aligned, origin=_p(t.d[0], 1))


def test_end_to_end_predict_expand_write(eng, dev, synth_ckpt, library, tables, monkeypatch):
    """8 synthetic images: predict_pipeline(expand=True, smiles=True, canonical=True, molfile=True) against the oracles applied to
    the same run's packed tables; without expand the dicts are what they were; then the facade's graph_expand."""
    from molnextr_amd.model import molnextr, predict_pipeline, unpack_graphs
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4))
    ref = X.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], frags=library, tables=tables)
    assert not (ref["mols"]["flags"] & MOL_EXPAND_REFUSED).any()
    smi = K.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], 0, tables)
    mf = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=tables)
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True)
    grown = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True, smiles=True, canonical=True, molfile=True, expand=True)
    before = unpack_graphs(rec["mols"], rec["atoms"], rec["bonds"], rec["text"])
    after = unpack_graphs(ref["mols"], ref["atoms"], ref["bonds"], ref["text"])
    old = K.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], 0, tables)
    for b, (p, g) in enumerate(zip(plain, grown)):
        assert "expanded" not in p and set(g) == set(p) | {"expanded"}
        assert p["chartok_coords"] == g["chartok_coords"] == before[b]["chartok_coords"] and p["bonds"] == g["bonds"] == before[b]["bonds"]
        r, m = old["recs"][b], rec["mols"][b]
        written = not int(r["flags"]) & 0x33
        assert p["graph_smiles"] == (old["out"][r["text0"]:r["text0"] + r["len"]].decode() if written else None)
        r, m, f = smi["recs"][b], ref["mols"][b], mf["files"][b]
        a0, na = int(m["atom0"]), int(m["n_atoms"])
        written = not int(r["flags"]) & 0x33                                       # SMILES_REFUSED
        assert g["graph_smiles"] == (smi["out"][r["text0"]:r["text0"] + r["len"]].decode() if written else None)
        assert g["graph_smiles_order"] == (smi["order"][a0:a0 + na].tolist() if written else None)
        assert g["canonical_rank"] == (None if smi["rank"][a0:a0 + na].tolist().count(K.NO_RANK) else smi["rank"][a0:a0 + na].tolist())
        assert g["molfile"] == (mf["out"][f["text0"]:f["text0"] + f["len"]].decode() if f["len"] else None)
        assert g["expanded"] == {"symbols": after[b]["chartok_coords"]["symbols"], "coords": after[b]["chartok_coords"]["coords"],
                                 "bonds": after[b]["bonds"], "origin": ref["origin"][a0:a0 + na].tolist(), "flags": int(m["flags"])}
    with pytest.raises(ValueError, match="expand=True needs packed=True"):
        predict_pipeline(eng, imgs[:1], expand=True)

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    with pytest.raises(ValueError, match="graph_expand=True needs graph_smiles=True or graph_molfile=True"):
        molnextr("synthetic", dev, graph_expand=True)
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_canonical=True, graph_expand=True)
    try:
        got = m.predict_images(pages, batch_size=4)
        want = predict_pipeline(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, packed=True, smiles=True, canonical=True,
                                expand=True)
        assert [o["predicted_smiles"] for o in got] == [p["graph_smiles"] for p in want]
        assert [o["expanded"] for o in got] == [p["expanded"] for p in want]
        m.graph_expand = False                                                     # the default: the label stays
        assert all("expanded" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()
