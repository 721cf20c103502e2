"""GPU (-m gpu): mnx_smiles_read — SMILES text read into the packed molecule tables on the device — against the oracle of
tests/smiles_read_ref.py, records field by field and tables byte for byte (no tolerances), with guard bytes behind every
capacity: the smallest shapes at which the kernel takes another turn (one byte, 255 / 256 / 257 bytes around the workgroup, the
4096-byte and 999-atom limits, deep nesting, every ring number), every refusal, the capacity protocol, determinism, the argument
errors, and the chains into the writers on the device."""
import numpy as np
import pytest
import torch

import molfile_ref as M
import smiles_read_ref as R
import smiles_ref as S
import test_smiles_read_host as H
from molnextr_amd.engine import READ_DTYPE, READ_REFUSED, Engine
from packed_tables import Inputs, _p, assert_refused, call_tables, clean, compare_tables, dev, same_results  # noqa: F401
from packed_tables import same_mols as same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):                                    # the reader needs no room for images: an engine of its own, max_batch 4
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=4, dtype="fp16x3")
    yield e
    e.close()


def arena_of(strings):
    offsets = np.zeros(len(strings) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(x) for x in strings])
    return b"".join(strings), offsets


def run(eng, dev, arena, offs, caps, tail=8, **over):
    """One mnx_smiles_read call, the arena uploaded with `tail` spare bytes behind it; the result's `side` are the recs' bytes"""
    d_bytes = torch.frombuffer(bytearray(arena) + bytearray(b"[" * tail), dtype=torch.uint8).to(dev) if len(arena) + tail else None
    d_off = torch.from_numpy(np.asarray(offs, np.uint32).view(np.int32).copy()).to(dev)
    head = {"bytes": _p(d_bytes), "n_bytes": len(arena), "offsets": _p(d_off), "n": len(offs) - 1}
    return call_tables("mnx_smiles_read", eng, Inputs(dev, len(offs) - 1, head), caps, **over)


def recs_of(got):
    return got.side.view(READ_DTYPE)


def check(eng, dev, strings=None, ref=None, arena=None, offsets=None, n_bytes=None):
    """the device's tables equal the oracle's at the exact capacities, byte for byte; returns the oracle's"""
    if arena is None:
        arena, offsets = arena_of(strings)
    ref = ref or R.pack(strings, arena=arena, offsets=offsets, n_bytes=n_bytes)
    over = {} if n_bytes is None else {"n_bytes": n_bytes}
    compare_tables(run(eng, dev, arena, offsets, ref["totals"], **over), ref, "recs")
    return ref


def test_the_header_examples_one_by_one_and_a_mixed_batch(eng, dev):
    for text in (b"CCO", b"", b"C", b"[13CH3][C@@H](N)C(=O)O"):
        check(eng, dev, [text])                                                    # n = 1
    batch = sorted(H.HAND) + [b"", b"C", b"Cl", b"", b"C" * 300, b"c1ccccc1" * 40, b"N"]
    ref = check(eng, dev, batch)
    assert not (ref["recs"]["flags"] & READ_REFUSED).any() and ref["mols"]["n_atoms"].tolist()[-3:] == [300, 240, 1]


def chain_of(n_bytes):
    """a valid string of exactly n_bytes with branches, rings, bracket atoms and two-byte atoms across every 16-byte boundary"""
    unit = b"C(=O)c1cc[nH]c1Cl[13CH2]%12CBrC%12N"
    s = (unit * (n_bytes // len(unit) + 1))[:n_bytes]
    while True:
        try:
            R.read(s)
            return s
        except R.Refused:
            n = len(s.rstrip(b"C"))
            s = s[:max(n - 1, 0)] + b"C" * (n_bytes - max(n - 1, 0))               # the cut broke a token: plain atoms from there


@pytest.mark.parametrize("n_bytes", [255, 256, 257, 4096])
def test_strings_around_the_workgroup_and_at_the_byte_limit(eng, dev, n_bytes):
    s = chain_of(n_bytes) if n_bytes < 4096 else b"C(C)" * 224 + b"[C@@H2+]" * 400        # 4096 bytes, 848 atoms
    assert len(s) == n_bytes
    ref = check(eng, dev, [b"CC", s, b"O"])
    assert ref["recs"]["flags"][1] & READ_REFUSED == 0 and ref["mols"]["n_atoms"][1] > 60


def test_limits_of_bytes_atoms_and_bonds(eng, dev):
    thousand_bonds = b"C12" + b"C" * 996 + b"C1C2"
    ref = check(eng, dev, [b"C" * 4097, b"CO" * 499 + b"N", b"C" * 1000, b"N", thousand_bonds, b"C1" + b"C" * 997 + b"C1",
                           b"$" + b"C" * 1000, b"C" * 998 + b"$", b"[CH4]" * 819 + b"C", b"C(" * 1000 + b"C" + b")" * 1000])
    assert ref["recs"]["flags"].tolist() == [2, 0, 2, 0, 2, 0, 2, 1, 0, 2]
    assert ref["mols"]["n_atoms"].tolist() == [0, 999, 0, 1, 0, 999, 0, 0, 820, 0]


def test_deep_nesting_and_every_ring_number(eng, dev):
    nest = b"C(" * 200 + b"C" + b")" * 200 + b"N"                                   # a branch nested 200 deep
    reuse = b"C1CC1" * 200                                                          # one number, 200 times
    # all 100 numbers open at one atom (0 as a digit), closed in reverse order behind a spacer atom
    all_open = b"C" + b"".join(b"%%%02d" % r for r in range(100))[3:] + b"0N" + b"".join(b"C%%%02d" % r for r in range(99, -1, -1))
    fan = b"C" + b"".join(b"%d" % r for r in range(1, 10)) + b"".join(b"%%%02d" % r for r in range(10, 100)) + b"N" + \
        b"".join(b"C%%%02d" % r for r in range(1, 100))                             # the writer's most: 99 numbers open at once
    mixed = b"C%99CC%99.C0CC0.C%00CC0.C%01CC1.C9CC%09"
    both = b"C=1CC=1.C=1CC1.C1CC=1.C-1CC1.c1ccc-1.c:1cc1.C/1CC1"                     # a symbol at one end or at both
    ref = check(eng, dev, [nest, reuse, all_open, fan, mixed, both, b"C=1CC#1", b"C(C)1CC1", b"C1.C1"])
    assert ref["recs"]["flags"].tolist() == [0, 0, 0, 0, 0, 4, 1, 0, 0]
    assert ref["recs"]["n_rings"].tolist()[:5] == [0, 200, 100, 99, 5] and ref["mols"]["n_atoms"].tolist()[:4] == [202, 600, 102, 101]


def test_two_byte_atoms_against_one_byte_atoms(eng, dev):
    ref = check(eng, dev, [b"Cl", b"Br", b"ClC", b"BrB", b"CB", b"CCl", b"BC", b"CBr", b"ClBr", b"BrCl", b"C(Cl)Br", b"Cl1CC1Br",
                           b"CN" * 7 + b"CCl" + b"C" * 20, b"C" * 15 + b"Br" + b"C" * 20])     # across a thread's 16 bytes
    assert ref["mols"]["n_atoms"].tolist()[:12] == [1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 4]


def test_every_refusal(eng, dev):
    texts = sorted(H.SYNTAX)
    ref = check(eng, dev, [b"CC"] + texts + [b"OO"])
    assert ref["recs"]["flags"].tolist() == [0] + [R.SYNTAX] * len(texts) + [0]
    assert ref["recs"]["err_pos"].tolist()[1:-1] == [H.SYNTAX[t] for t in texts]
    for t in texts:                                                                 # and alone, as the only and last string
        check(eng, dev, [t])
    # the same errors far from the first bytes: behind 300 bytes of chain, and the late ones around it
    far = [b"C" * 300 + t for t in texts if t[:1] not in b"=1().l["] + [b"C(" + b"C" * 300 + b"$C)", b"C(" + b"C" * 300 + b"$C",
                                                                        b"C1" + b"C" * 300 + b"$C1", b"C1" + b"C" * 300 + b"$C"]
    ref = check(eng, dev, far)
    assert (ref["recs"]["flags"] == R.SYNTAX).all() and ref["recs"]["err_pos"].tolist()[-4:] == [302, 1, 302, 1]


def test_offsets_beyond_the_bytes_and_an_open_bracket_as_the_last_byte(eng, dev):
    arena = b"CCOCN"
    ref = check(eng, dev, arena=arena, offsets=[0, 2, 1, 3, 6, 6], n_bytes=5)
    assert ref["recs"]["flags"].tolist() == [0, R.BEYOND, 0, R.BEYOND, R.BEYOND]
    ref = check(eng, dev, arena=arena, offsets=[0, 5], n_bytes=4)
    assert ref["recs"]["flags"].tolist() == [R.BEYOND]
    # "C[" ends the arena; the bytes behind n_bytes (run() puts "[[[[[[[[" there) are not read
    arena, offsets = arena_of([b"CC", b"C["])
    ref = R.pack([b"CC", b"C["])
    assert ref["recs"]["flags"].tolist() == [0, R.SYNTAX] and ref["recs"]["err_pos"].tolist() == [0, 1]
    check(eng, dev, ref=ref, arena=arena, offsets=offsets)
    a = run(eng, dev, arena, offsets, ref["totals"], tail=0)                         # and with nothing allocated behind it
    assert a.rc == 0 and recs_of(a)["flags"].tolist() == [0, R.SYNTAX]


@pytest.fixture(scope="module")
def batch():
    """1025 strings (one past the scan tile of 1024): the writer's strings of random drawings, every tenth one broken"""
    rng = np.random.default_rng(5)
    mols = [H.random_molecule(rng, int(n)) for n in rng.integers(1, 15, 1025)]
    written = S.pack(*M.build_tables(mols), tables=H.TABLES)
    texts = H.strings(written["recs"], written["out"])
    garbage = b"()[]=#%1.Cc$l\\"
    for k in range(0, len(texts), 10):
        t = bytearray(texts[k] + b"C")
        t[int(rng.integers(0, len(t)))] = garbage[int(rng.integers(0, len(garbage)))]
        texts[k] = bytes(t)
    return texts, R.pack(texts)


def test_1025_strings_and_two_runs_with_identical_bytes(eng, dev, batch):
    texts, ref = batch
    assert 40 < (ref["recs"]["flags"] & R.SYNTAX).astype(bool).sum() < 110
    check(eng, dev, texts, ref)
    arena, offsets = arena_of(texts)
    same_results(run(eng, dev, arena, offsets, ref["totals"]), run(eng, dev, arena, offsets, ref["totals"]))


def test_capacities_one_short_then_exact(eng, dev, batch):
    """each capacity one record or byte short, separately: nothing is written beyond it, what lies in front of it is right, and
    mols, recs and totals are complete; then the sizing call with null tables, then the exact sizes"""
    texts, ref = batch
    arena, offsets = arena_of(texts)
    full = list(ref["totals"])
    exact = (np.frombuffer(clean(ref["atoms"]), np.uint8), np.frombuffer(clean(ref["bonds"]), np.uint8), np.frombuffer(ref["text"], np.uint8))
    for k in range(3):
        caps = list(full)
        caps[k] -= 1
        a = run(eng, dev, arena, offsets, caps)                                          # run() checks the guard bytes
        assert a.rc == 0 and a.totals.tolist() == full + [1]
        same(a.mols, ref["mols"])
        same(recs_of(a), ref["recs"])
        for got, want in zip((a.atoms, a.bonds, a.text), exact):
            assert np.array_equal(got, want[:len(got)])
    a = run(eng, dev, arena, offsets, (0, 0, 0), atoms=None, bonds=None, text=None)
    assert a.rc == 0 and a.totals.tolist() == full + [1]
    same(a.mols, ref["mols"])
    check(eng, dev, texts, ref)


def test_engine_smiles_read_sizes_itself(eng, batch):
    texts, ref = batch
    for caps in (None, (1, 1, 1)):
        got = eng.smiles_read(texts, caps=caps)
        same(got["mols"], ref["mols"])
        same(got["read"], ref["recs"])
        assert got["atoms"].tobytes() == clean(ref["atoms"]) and got["bonds"].tobytes() == clean(ref["bonds"]) and got["text"] == ref["text"]
        assert got["totals"].tolist() == list(ref["totals"]) + [0]
    assert eng.smiles_read(["CCO", ""])["mols"]["n_atoms"].tolist() == [3, 0]          # str goes in as UTF-8


def test_argument_errors(eng, dev):
    arena, offsets = arena_of([b"CCO", b"C1CC1"])
    d_off = torch.from_numpy(offsets.view(np.int32).copy()).to(dev)

    def refused(expect, **over):
        assert_refused(run(eng, dev, arena, offsets, (16, 16, 16), **over), "mnx_smiles_read: " + expect)

    for name in ("bytes", "offsets", "mols", "recs", "atoms", "bonds", "text", "totals"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, recs, offsets and totals 4-byte"
    spare = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for name, off in (("mols", 4), ("atoms", 4), ("bonds", 4), ("recs", 2), ("totals", 2)):
        refused(aligned, **{name: _p(spare, off)})
    refused(aligned, offsets=_p(d_off, 2))
    assert run(eng, dev, b"", [0, 0], (0, 0, 0), tail=0, atoms=None, bonds=None, text=None).rc == 0     # no bytes at all: nothing may be null-checked


def test_write_read_write_on_the_device(eng, batch):
    """device mnx_smiles_pack -> device mnx_smiles_read -> device mnx_smiles_pack: the same bytes"""
    rng = np.random.default_rng(17)
    mols, atoms, bonds, text = M.build_tables([H.random_molecule(rng, int(n)) for n in rng.integers(1, 15, 300)])
    recs, _, data = eng.smiles_pack({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text})
    texts = H.strings(recs, data)
    back = eng.smiles_read(texts, keep_device=True)
    assert not back["read"]["flags"].any() and back["read"]["n_rings"].tolist() == recs["n_rings"].tolist()
    again, _, data2 = eng.smiles_pack(back)
    assert data2 == data and all(again[k].tolist() == recs[k].tolist() for k in ("text0", "len", "n_rings"))


def canonical(eng, strings, expand=False):
    rec = eng.smiles_read(strings, keep_device=True)
    assert not (rec["read"]["flags"] & READ_REFUSED).any()
    if expand:
        rec = eng.expand_pack(rec, keep_device=True)
    recs, _, data, _, _ = eng.smiles_pack(rec, canonical=True)
    return H.strings(recs, data)


def test_one_canonical_string_for_one_graph(eng):
    a = canonical(eng, ["OCC", "CCO", "C(O)C", "Cc1ccccc1", "c1ccccc1C", "c1ccc(C)cc1", "c1cc(ccc1)C", "C1CC1.N", "N.C1CC1"])
    assert a[0] == a[1] == a[2] and a[3] == a[4] == a[5] == a[6] and a[7] == a[8] and len({a[0], a[3], a[7]}) == 3 and all(a)
    b = canonical(eng, ["[Ph]C", "Cc1ccccc1", "C[OMe]", "COC"], expand=True)
    assert b[0] == b[1] == a[3] and b[2] == b[3] and b"*" not in b[0] + b[2]
    assert canonical(eng, ["[Ph]C"])[0] != a[3]                                        # without expansion the label is a '*'


def test_molfile_of_a_read_molecule(eng):
    texts = [b"CC(=O)[O-]", b"c1ccccc1-c1ccccc1", b"[13CH3][C@@H](N)C(=O)O", b"", b"C$"]
    rec = eng.smiles_read(texts, keep_device=True)
    files, data = eng.molfile_pack(rec)
    ref = R.pack(texts)
    want = M.pack(ref["mols"], ref["atoms"], ref["bonds"], ref["text"], tables=H.TABLES)
    assert data == want["out"] and files.tobytes() == want["files"].tobytes() and files["len"][0] > 0
