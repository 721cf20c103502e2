"""GPU (-m gpu): mnx_molfile_read — V2000 molfiles read into the packed molecule tables on the device — against the oracle of
tests/molfile_read_ref.py, records field by field and tables byte for byte (no tolerances), with guard bytes behind every
capacity: the smallest shapes at which the kernel takes another turn (atoms and bonds around the workgroup of 256 and at the
three-column limit, a newline on each side of the 4096-byte tile, the 8192-line and 262144-byte limits), every refusal, the
capacity protocol, determinism, the argument errors, fit mode, and the chains with the writers on the device."""
import numpy as np
import pytest
import torch

import molfile_read_ref as R
import molfile_ref as M
import packed_tables
import test_molfile_read_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import MOLREAD_DTYPE, MOLREAD_REFUSED, Engine
from packed_tables import Inputs, _p, assert_refused, call_tables, clean, compare_tables, dev, same_results  # noqa: F401
from packed_tables import same_mols as same

pytestmark = pytest.mark.gpu

# the reader's row of the harness: the output side of mnx_smiles_read
packed_tables.TABLE_ARGS.setdefault("mnx_molfile_read", "mols recs atoms atom_cap bonds bond_cap text text_cap totals")
TILE = 4096                                              # the bytes the kernel looks at per round


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):                                    # the reader needs little room for images: an engine of its own
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=8, dtype="fp16x3")
    yield e
    e.close()


def arena_of(files):
    offsets = np.zeros(len(files) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(x) for x in files])
    return b"".join(files), offsets


def run(eng, dev, arena, offs, caps, scale=None, fit=0, tail=8, **over):
    """One mnx_molfile_read call, the arena uploaded with `tail` spare bytes behind it; the result's `side` are the recs' bytes"""
    d_bytes = torch.frombuffer(bytearray(arena) + bytearray(b"\n" * tail), dtype=torch.uint8).to(dev) if len(arena) + tail else None
    d_off = torch.from_numpy(np.asarray(offs, np.uint32).view(np.int32).copy()).to(dev)
    d_scale = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.int32)).to(dev) if isinstance(scale, np.ndarray) else None
    p_scale = _p(d_scale) if d_scale is not None else scale                            # an array, None, or a raw pointer as it is
    head = {"bytes": _p(d_bytes), "n_bytes": len(arena), "offsets": _p(d_off), "n": len(offs) - 1, "scale": p_scale, "fit": fit}
    return call_tables("mnx_molfile_read", eng, Inputs(dev, len(offs) - 1, head), caps, **over)


def recs_of(got):
    return got.side.view(MOLREAD_DTYPE)


def check(eng, dev, files=None, scale=None, fit=False, ref=None, arena=None, offsets=None, n_bytes=None):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    if arena is None:
        arena, offsets = arena_of(files)
    ref = ref or R.pack(files, scale=scale, fit=fit, den=H.DEN, arena=arena, offsets=offsets, n_bytes=n_bytes)
    over = {} if n_bytes is None else {"n_bytes": n_bytes}
    compare_tables(run(eng, dev, arena, offsets, ref["totals"], scale=scale, fit=int(fit), **over), ref, "recs")
    return ref


def pairs(n_atoms, n_bonds):
    """n_bonds different pairs among n_atoms atoms (1-based), neighbours first"""
    out = [(i, i + d) for d in (1, 2, 3) for i in range(1, n_atoms - d + 1)]
    assert len(out) >= n_bonds
    return out[:n_bonds]


def big(n_atoms, n_bonds, props=(), sym=b"C", first_line=b""):
    """a file of n_atoms atoms on a lattice and n_bonds bonds of changing types, wedges among them"""
    atoms = [H.atom_line(sym if k % 7 else b"N", (k % 30) * 0.3, (k // 30) * 0.25) for k in range(n_atoms)]
    bonds = [H.bond_line(j, i, 1, 1) if k % 5 == 0 else H.bond_line(i, j, 1 + k % 3) for k, (i, j) in enumerate(pairs(n_atoms, n_bonds))]
    counts = b"%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (n_atoms, n_bonds)
    return first_line + H.molfile(atoms, bonds[::-1], props, counts=counts)


def test_the_header_examples_one_by_one_and_a_mixed_batch(eng, dev):
    co = H.molfile([H.atom_line(b"C", 1.0, 2.0), H.atom_line(b"O")], [H.bond_line(1, 2)])
    for data in (co, b"", H.molfile(), H.molfile([H.atom_line(b"N", v=4)], props=[b"M  CHG  1   1   1"])):
        check(eng, dev, [data])                                                        # n = 1
    named = [M.molfile(s, H.grid(len(s)), b, tables=H.TABLES)[0] for s, b in H.NAMED.values()]
    ref = check(eng, dev, [b"", co, b""] + named + [b"", big(40, 44), b""])
    assert not (ref["recs"]["flags"] & MOLREAD_REFUSED).any() and ref["mols"]["n_atoms"].tolist()[:3] == [0, 2, 0]
    assert ref["recs"]["n_marked"][3:3 + len(named)].sum() == 3 and ref["mols"]["n_atoms"][-2] == 40


@pytest.mark.parametrize("n_atoms,n_bonds", [(0, 0), (1, 0), (2, 1), (255, 256), (256, 257), (257, 256), (999, 0), (999, 999), (1000, 999), (999, 1000)])
def test_atoms_and_bonds_around_the_workgroup_and_at_the_limit(eng, dev, n_atoms, n_bonds):
    """1000 does not fit its three columns: the counts line then says something else, and the oracle says what"""
    ref = check(eng, dev, [big(3, 2), big(min(n_atoms, 999), min(n_bonds, 999)) if max(n_atoms, n_bonds) < 1000 else
                           big(999, 999).replace(b"999999  0", b"%d%d  0" % (n_atoms, n_bonds), 1), big(2, 1)])
    if max(n_atoms, n_bonds) < 1000:
        assert ref["recs"]["flags"][1] & MOLREAD_REFUSED == 0 and ref["mols"]["n_atoms"][1] == n_atoms and ref["mols"]["n_bonds"][1] == n_bonds
    else:               # "1000999" reads as 100 atoms and 99 bonds (refused at the first line that is no bond), "9991000" as 999 and 100
        assert (ref["recs"]["flags"][1], ref["mols"]["n_bonds"][1]) == ((R.SYNTAX, 0) if n_atoms == 1000 else (R.IGNORED | R.H_DEFAULT, 100))


@pytest.mark.parametrize("at", [255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 16 * TILE - 1, 16 * TILE])
def test_a_newline_on_each_side_of_a_tile_boundary(eng, dev, at):
    """the first line's '\\n' is byte `at`; and the same file cut so that a later '\\n' is the last byte of a tile"""
    a = big(20, 21, first_line=b"x" * at)
    assert a[at:at + 1] == b"\n" and a.count(b"\n", 0, at) == 0
    body = big(300, 300)
    pad = (-len(body)) % TILE                                                          # the file ends with a tile
    ref = check(eng, dev, [a, b"y" * pad + body, b"y" * (pad + 1) + body, a[:-1]])
    assert not (ref["recs"]["flags"] & MOLREAD_REFUSED).any() and ref["mols"]["n_atoms"].tolist() == [20, 300, 300, 20]


def test_long_lines_many_lines_and_the_byte_limit(eng, dev):
    body = big(30, 31)
    full = body + b">  <x>\n" + b"z" * (262144 - len(body) - 7)
    lines = b"\n" * 8187 + H.molfile()                                                 # "M  END" is line 8192
    files = [b"h" * 100000 + body, full, full + b"z", lines, b"\n" + lines, b"\n" * 8188 + H.molfile(end=False), b"\n" * 5, b"\n" * 8193,
             b"\n" * 262144, b"\r\n" * 4000, big(5, 4, props=[b"G  1"] * 8000), big(5, 4, props=[b"G  1"] * 8200)]
    ref = check(eng, dev, files)
    # big()'s wedges mark carbons whose H comes from the table; the blank lines in front of "M  END" are skipped property lines
    assert ref["recs"]["flags"].tolist() == [R.H_DEFAULT, R.H_DEFAULT, R.TOO_LARGE, R.IGNORED, R.TOO_LARGE, R.SYNTAX, R.SYNTAX, R.TOO_LARGE,
                                             R.TOO_LARGE, R.SYNTAX, R.IGNORED | R.H_DEFAULT, R.TOO_LARGE]
    assert ref["recs"]["err_line"].tolist()[5:7] == [8193, 6] and ref["recs"]["err_line"][9] == 4001


def chg_lines(entries, tag=b"CHG"):
    return [b"M  %s%3d" % (tag, len(entries[k:k + 8])) + b"".join(b" %3d %3d" % e for e in entries[k:k + 8]) for k in range(0, len(entries), 8)]


def test_property_lines_of_8_9_and_999_entries_and_atoms_named_twice(eng, dev):
    eight = [(k + 1, (-1) ** k * (k + 1)) for k in range(8)]
    nine = b"M  CHG  9" + b"".join(b" %3d %3d" % (k + 1, 1) for k in range(9))
    every = [(k + 1, k % 31 - 15) for k in range(999)]
    twice = [b"M  CHG  3   2   1   2  -3   2   5", b"M  ISO  2   4  13   5  14", b"M  ISO  2   5  15   4   0", b"M  CHG  1   3   2", b"M  CHG  1   3  -2"]
    iso = chg_lines([(k + 1, 999 - k) for k in range(999)], b"ISO")
    files = [big(10, 9, chg_lines(eight)), big(10, 9, [nine]), big(999, 998, chg_lines(every)), big(10, 9, twice),
             big(999, 998, iso + chg_lines(every[::-1])), big(999, 0, chg_lines([(k + 1, k + 1) for k in range(999)], b"RGP"), sym=b"R#")]
    ref = check(eng, dev, files)
    assert ref["recs"]["flags"].tolist() == [R.H_DEFAULT, R.SYNTAX, R.H_DEFAULT, R.H_DEFAULT, R.H_DEFAULT, R.LABEL]
    assert ref["recs"]["err_line"][1] == 24 and ref["text"].count(b"[R999]") == 1


def test_aliases_at_the_first_and_the_last_atom(eng, dev):
    def alias(atom, text):
        return [b"A  %3d" % atom, text]

    files = [big(999, 998, alias(1, b"a" * 70) + alias(999, b"\x01" + b"b" * 69)), big(999, 998, alias(1, b"ok") + alias(999, b"b" * 71)),
             big(999, 998, [p for k in range(999) for p in alias(k + 1, b"L%d" % k * 9)]), big(3, 2, alias(1, b"A    2") + alias(3, b"")),
             big(999, 998, [p for k in range(999) for p in alias(999 - k, b"A    1")] + alias(1, b"x") + alias(1, b"y"))]
    ref = check(eng, dev, files)
    assert ref["recs"]["flags"].tolist() == [R.LABEL | R.H_DEFAULT, R.SYNTAX, R.LABEL, R.LABEL | R.H_DEFAULT, R.LABEL] and ref["recs"]["err_line"][1] == 5 + 999 + 998 + 3
    assert ref["text"].startswith(b"[" + b"a" * 70 + b"]") and ref["mols"]["smiles_len"][2] > 30000


def test_every_refusal(eng, dev):
    names = sorted(H.REFUSALS)
    files = [H.REFUSALS[k][0] for k in names]
    ref = check(eng, dev, [H.molfile(H.C2)] + files + [H.molfile(H.C3)])
    assert ref["recs"]["flags"].tolist() == [0] + [H.REFUSALS[k][1] for k in names] + [0]
    assert ref["recs"]["err_line"].tolist()[1:-1] == [H.REFUSALS[k][2] for k in names]
    for data in files:                                                                 # and alone, as the only and last file
        check(eng, dev, [data])
    # the same errors far from the first lines: behind 300 atoms and 300 bonds
    far = [big(300, 300).replace(b"M  END", line + b"\nM  END", 1) for line in (b"M  CHG  1 301   1", b"A  301\nx", b"A    1\n" + b"x" * 71, b"M  ISO  0")]
    far += [big(300, 300).replace(b"  2  3  2  0\n", b"  2  3  7  0\n", 1), big(300, 300).replace(b"  2  3  2  0\n", b"  3  4  1  0\n", 1)]
    ref = check(eng, dev, far)
    assert ref["recs"]["flags"].tolist() == [1, 1, 1, 1, 16, 1] and ref["recs"]["err_line"].tolist() == [605, 605, 606, 605, 603, 603]


def test_files_written_elsewhere_and_the_default_hydrogens(eng, dev):
    names = sorted(H.FOREIGN)
    ref = check(eng, dev, [H.FOREIGN[k][0] for k in names] + [H.h_row_file(s, q, t) for s, q, t, _ in H.H_ROWS])
    assert ref["recs"]["flags"].tolist()[:len(names)] == [H.FOREIGN[k][2] for k in names]


def test_offsets_beyond_the_bytes(eng, dev):
    a, b = H.molfile(H.C2), H.molfile(H.C3)
    arena = a + b
    ref = check(eng, dev, arena=arena, offsets=[0, len(a), 5, len(arena), len(arena) + 1, len(arena) + 1], n_bytes=len(arena))
    # file 2 begins in the middle of a line of the first file: read, and refused for what it then says
    assert ref["recs"]["flags"].tolist() == [0, R.BEYOND, R.SYNTAX, R.BEYOND, R.BEYOND] and ref["mols"]["n_atoms"].tolist() == [2, 0, 0, 0, 0]
    ref = check(eng, dev, arena=arena, offsets=[0, len(arena)], n_bytes=len(arena) - 1)
    assert ref["recs"]["flags"].tolist() == [R.BEYOND]
    got = run(eng, dev, a[:-1], [0, len(a) - 1], (2, 1, 2), tail=0)                  # no '\n' at the end and nothing allocated behind it
    assert got.rc == 0 and recs_of(got)["flags"].tolist() == [0] and got.text.tobytes() == b"CO"


@pytest.fixture(scope="module")
def batch():
    """1025 files (one past the scan tile of 1024): the writer's files of drawn molecules at their scales, every tenth one broken"""
    rng = np.random.default_rng(11)
    mols = [H.drawn_molecule(rng) for _ in range(1025)]
    scale = rng.integers(64, 10000001, (1025, 2))
    files = [M.molfile(*m, int(s[0]), int(s[1]), H.DEN, H.TABLES)[0] for m, s in zip(mols, scale)]
    garbage = b"xV-9 \n"
    for k in range(0, len(files), 10):
        t = bytearray(files[k])
        t[int(rng.integers(20, len(t)))] = garbage[int(rng.integers(0, len(garbage)))]
        files[k] = bytes(t)
    return files, scale, R.pack(files, scale=scale, den=H.DEN), mols


def test_1025_files_and_two_runs_with_identical_bytes(eng, dev, batch):
    files, scale, ref, mols = batch
    assert 20 < (ref["recs"]["flags"] & MOLREAD_REFUSED).astype(bool).sum() < 104
    check(eng, dev, files, scale=scale, ref=ref)
    arena, offsets = arena_of(files)
    same_results(run(eng, dev, arena, offsets, ref["totals"], scale=scale), run(eng, dev, arena, offsets, ref["totals"], scale=scale))
    for k in range(1, len(files), 10):                                                 # an unbroken file is its drawing
        m = ref["mols"][k]
        assert ref["text"][m["text0"]:m["text0"] + m["smiles_len"]] == b"".join(mols[k][0])


def test_capacities_one_short_then_exact(eng, dev, batch):
    """each capacity one record or byte short, separately: nothing is written beyond it, what lies in front of it is right, and
    mols, recs and totals are complete; then the sizing call with null tables, then the exact sizes"""
    files, scale, ref, _ = batch
    arena, offsets = arena_of(files)
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8), np.frombuffer(ref["text"], np.uint8))
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, dev, arena, offsets, caps, scale=scale)                           # run() checks the guard bytes
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same(a.mols, ref["mols"])
        same(recs_of(a), ref["recs"])
        for got, want in zip((a.atoms, a.bonds, a.text), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, dev, arena, offsets, (0, 0, 0), scale=scale, atoms=None, bonds=None, text=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]
    same(a.mols, ref["mols"])


def test_engine_molfile_read_sizes_itself(eng, batch):
    files, scale, ref, _ = batch
    for caps in (None, (1, 1, 1)):
        got = eng.molfile_read(files, scale=scale, caps=caps)
        same(got["mols"], ref["mols"])
        same(got["read"], ref["recs"])
        assert got["atoms"].tobytes() == clean(ref["atoms"]) and got["bonds"].tobytes() == clean(ref["bonds"]) and got["text"] == ref["text"]
        assert got["totals"].tolist() == list(ref["totals"]) + [0]
    assert eng.molfile_read([H.molfile(H.C3).decode(), ""])["mols"]["n_atoms"].tolist() == [3, 0]     # str goes in as UTF-8
    with pytest.raises(ValueError):
        eng.molfile_read(files[:2], scale=scale[:2], fit=True)


def test_argument_errors(eng, dev):
    arena, offsets = arena_of([H.molfile(H.C2), H.molfile(H.C3)])
    d_off = torch.from_numpy(offsets.view(np.int32).copy()).to(dev)
    scale = np.full((2, 2), 100000)

    def refused(expect, **kw):
        assert_refused(run(eng, dev, arena, offsets, (16, 16, 16), **kw), "mnx_molfile_read: " + expect)

    for name in ("bytes", "offsets", "mols", "recs", "atoms", "bonds", "text", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    for fit in (2, -1):
        refused("fit must be 0 or 1", fit=fit)
    refused("fit = 1 takes no scale", fit=1, scale=scale)
    aligned = "mols, atoms and bonds must be 8-byte aligned, recs, offsets, scale and totals 4-byte"
    spare = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for name, off in (("mols", 4), ("atoms", 4), ("bonds", 4), ("recs", 2), ("totals", 2), ("scale", 2)):
        refused(aligned, **{name: _p(spare, off)})
    refused(aligned, offsets=_p(d_off, 2))
    assert run(eng, dev, b"", [0, 0], (0, 0, 0), tail=0, atoms=None, bonds=None, text=None).rc == 0     # no bytes at all: nothing may be null-checked
    assert run(eng, dev, arena, offsets, (5, 3, 5), scale=scale).rc == 0 and run(eng, dev, arena, offsets, (5, 3, 5), fit=1).rc == 0


def test_fit_mode_and_clamped_scales(eng, dev, batch):
    files = [H.molfile([H.atom_line(b"C", x, y) for x, y in xy]) for xy, _ in H.FIT.values()] + batch[0][:40]
    files += [H.molfile([H.atom_line(b"C", 99999.9999, -9999.0), H.atom_line(b"O", -9999.9999, 99999.9999), H.atom_line(b"N", 0.00004, 0.00005)])]
    ref = check(eng, dev, files, fit=True)
    assert not (ref["recs"]["flags"] & R.CLAMPED).any() and ref["atoms"]["x_bin"].max() == 63
    n = len(files)
    scale = np.array([[1, 10000000], [0, -5], [20000000, 64], [63, 62]] * n)[:n]       # clamped to 1..10000000; S <= den is no inverse, but a rule
    ref = check(eng, dev, files, scale=scale)
    assert (ref["recs"]["flags"] & R.CLAMPED).any()


def test_write_read_write_on_the_device(eng):
    """256 drawn molecules -> device mnx_molfile_pack(scale) -> device mnx_molfile_read(scale): the tables that went in; and the
    canonical writer with every mark writes the same bytes from both"""
    rng = np.random.default_rng(256)
    drawn = [H.drawn_molecule(rng) for _ in range(256)]
    mols, atoms, bonds, text = M.build_tables([(s, xy, sorted(b)) for s, xy, b in drawn])        # bond records sorted, as graph_pack's
    scale = rng.integers(64, 10000001, (256, 2))
    rec = {"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}
    files, data = eng.molfile_pack(rec, scale=scale)
    assert not files["flags"].astype(int).__and__(3).any()
    back = eng.molfile_read([data[f["text0"]:f["text0"] + f["len"]] for f in files], scale=scale, keep_device=True)
    assert not back["read"]["flags"].__and__(MOLREAD_REFUSED | R.CLAMPED).any() and back["read"]["n_marked"].sum() > 10
    same(back["mols"], mols)
    assert back["atoms"].tobytes() == clean(atoms) and back["bonds"].tobytes() == clean(bonds) and back["text"] == text
    a = eng.smiles_pack(rec, canonical=True, stereo=True, double_bonds=True)
    b = eng.smiles_pack(back, canonical=True, stereo=True, double_bonds=True)
    assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and b"@" in a[2]


def test_the_molfiles_of_a_predict_job_read_back(eng, dev):
    imgs = W.synthetic_images(8, first_index=500).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4), keep_device=True)
    scale = np.array([[100000 + 7777 * k, 100000 - 999 * k] for k in range(8)])
    files, data = eng.molfile_pack(rec, scale=scale)
    texts = [data[f["text0"]:f["text0"] + f["len"]] for f in files]
    assert sum(map(len, texts)) > 1000
    ref = R.pack(texts, scale=scale, den=H.DEN)
    got = eng.molfile_read(texts, scale=scale)
    same(got["mols"], ref["mols"])
    same(got["read"], ref["recs"])
    assert got["atoms"].tobytes() == clean(ref["atoms"]) and got["bonds"].tobytes() == clean(ref["bonds"]) and got["text"] == ref["text"]
    for f, r, m, w in zip(files, got["read"], got["mols"], rec["mols"]):                 # a file that was written and read: the bins it was written from
        if f["len"] and not r["flags"] & MOLREAD_REFUSED:
            a, b = got["atoms"][m["atom0"]:m["atom0"] + m["n_atoms"]], rec["atoms"][w["atom0"]:w["atom0"] + w["n_atoms"]]
            assert a["x_bin"].tolist() == b["x_bin"].tolist() and a["y_bin"].tolist() == b["y_bin"].tolist()


def alanine(wedge):
    """N-C(C)-C(=O)O drawn flat, the methyl on a wedge of the given stereo flag from the centre"""
    atoms = [H.atom_line(b"N", 0.0, 0.0), H.atom_line(b"C", 1.0, 0.5), H.atom_line(b"C", 1.0, 1.5), H.atom_line(b"C", 2.0, 0.0),
             H.atom_line(b"O", 2.0, -1.0), H.atom_line(b"O", 3.0, 0.5)]
    return H.molfile(atoms, [H.bond_line(1, 2), H.bond_line(2, 3, 1, wedge), H.bond_line(2, 4), H.bond_line(4, 5, 2), H.bond_line(4, 6)])


def test_canonical_molfiles_and_the_facade_of_the_model(eng):
    from molnextr_amd.model import canonical_molfiles, canonical_smiles, molfile_fingerprints, smiles_fingerprints, split_sdf
    sdf = alanine(1) + b"$$$$\n" + alanine(6) + b">  <x>\n1\n\n$$$$\n"
    marked = canonical_molfiles(eng, split_sdf(sdf), stereo=True)
    plain = canonical_molfiles(eng, split_sdf(sdf))
    assert marked[0]["smiles"] != marked[1]["smiles"] and "@" in marked[0]["smiles"] and "@" in marked[1]["smiles"]
    assert plain[0]["smiles"] == plain[1]["smiles"] and "@" not in plain[0]["smiles"] and plain[0]["err_line"] == 0
    assert canonical_molfiles(eng, [alanine(0)], normalize=True)[0]["smiles"] == canonical_smiles(eng, ["CC(N)C(=O)O"], normalize=True)[0]["smiles"]
    bad = canonical_molfiles(eng, [alanine(2), b""])
    assert bad[0]["smiles"] is None and bad[0]["read_flags"] == R.SYNTAX and bad[0]["err_line"] == 12 and canonical_molfiles(eng, []) == []
    fp = molfile_fingerprints(eng, [alanine(0), alanine(2)], normalize=True)
    assert fp[0]["fingerprint"] == smiles_fingerprints(eng, ["CC(N)C(=O)O"], normalize=True)[0]["fingerprint"] and fp[1]["fingerprint"] is None
