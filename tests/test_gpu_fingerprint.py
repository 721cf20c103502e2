"""GPU (-m gpu): mnx_fingerprint_pack — the path fingerprint of every packed molecule — and mnx_tanimoto against the oracle of
tests/fingerprint_ref.py, word for word (no tolerances), guard bytes included: the shapes at which the prologue, the split of the
directed bonds over the threads, the depth of the walk and the step limit take another turn, the refusals, determinism, every
argument error, the documented place behind the chain of passes, and one end-to-end run through predict_pipeline, the facade and
evaluate's graded score."""
import collections
import functools
import math

import numpy as np
import pytest

import fingerprint_ref as F
import packed_tables
import test_fingerprint_host as H
from molnextr_amd import weights as W
from molnextr_amd.engine import FP_DTYPE, FP_LIMIT, FP_REFUSED, FP_WORDS, READ_REFUSED, SMILES_REFUSED, Engine
from packed_tables import Tables, _call, _p, _up, assert_refused, dev, eng, mol, random_molecule, same_array, same_mols  # noqa: F401

pytestmark = pytest.mark.gpu

E2E_FIRST_INDEX = 500          # the batch of the writers' end-to-end tests

FpResult = collections.namedtuple("FpResult", "rc recs bits error")
SimResult = collections.namedtuple("SimResult", "rc both either similarity error")


def run(eng, t, sizes=None, max_bonds=0, max_steps=0, **over):
    """one call of mnx_fingerprint_pack on the tables t: its argument list has no counterpart in packed_tables, so this is the
    caller around packed_tables._call — both outputs FILL-filled with GUARD bytes behind them, found untouched"""
    args = {**t.head(sizes), "recs": None, "bits": None, "max_bonds": max_bonds, "max_steps": max_steps}
    nbytes = {"recs": t.n * FP_DTYPE.itemsize, "bits": t.n * FP_WORDS * 4}
    rc, error, host = _call(eng, "mnx_fingerprint_pack", t.dev, args, nbytes, over)
    return FpResult(rc, host["recs"][:nbytes["recs"]].view(FP_DTYPE), host["bits"][:nbytes["bits"]].view(np.uint32).reshape(t.n, FP_WORDS), error)


def similar(eng, dev, rows_a, rows_b, **over):
    """one call of mnx_tanimoto on two arrays [n, 64], the three outputs guarded as above; over: arguments by name, as for run"""
    n = len(rows_a)
    d = [_up(dev, np.ascontiguousarray(x, np.uint32).reshape(n, FP_WORDS)) for x in (rows_a, rows_b)]
    args = {"a": _p(d[0]), "b": _p(d[1]), "n": n, "both": None, "either": None, "similarity": None}
    nbytes = {"both": 4 * n, "either": 4 * n, "similarity": 8 * n}
    rc, error, host = _call(eng, "mnx_tanimoto", dev, args, nbytes, over)
    return SimResult(rc, host["both"][:4 * n].view(np.uint32), host["either"][:4 * n].view(np.uint32), host["similarity"][:8 * n].view(np.float64), error)


def check(eng, t, ref=None, **kw):
    """the device's records and words equal the oracle's; returns the oracle's"""
    ref = ref or F.pack(t.mols, t.atoms, t.bonds, t.text, tables=H.TABLES, **kw)
    got = run(eng, t, **kw)
    assert got.rc == 0, f"rc {got.rc}: {got.error}"
    same_mols(got.recs, ref["fp"], "recs")
    assert got.recs.tobytes() == ref["fp"].tobytes()
    same_array(got.bits.reshape(-1), ref["bits"].reshape(-1), "bits")
    return ref


def ring(n, ty=1, sym=b"C"):
    return mol([sym] * n, [(k, (k + 1) % n, ty, ty) if k + 1 < n else (0, k, ty, ty) for k in range(n)])


def ladder(n):
    """two rails of n atoms and a rung between every pair: 3 n - 2 bonds, every atom on a cycle"""
    syms = [b"N" if k % 7 == 0 else b"C" for k in range(2 * n)]
    return mol(syms, [(k, k + 1, 1, 1) for k in range(n - 1)] + [(n + k, n + k + 1, 1, 1) for k in range(n - 1)] +
               [(k, n + k, 2 if k % 3 == 0 else 1, 1) for k in range(n)])


def test_hand_made_molecules_one_by_one_and_together(eng, dev):
    """0, 1 and 2 atoms, rings of 7 and 8 (the longest path that does and does not fit), a star with 20 leaves, a 12-byte atom
    text, the five bond words with two unknown types and both wedges"""
    star = mol([b"C"] + [b"N", b"O"] * 10, [(0, k, 1, 1) for k in range(1, 21)])
    words = mol([b"C", b"N", b"O", b"S", b"Cl", b"[999OgH2+15]", b"Br", b"I"],
                [(0, 1, 1, 1), (1, 2, 2, 2), (2, 3, 3, 3), (3, 4, 4, 4), (4, 5, 0, 0), (5, 6, 5, 1), (6, 7, 6, 1), (0, 7, 7, 7)])
    molecules = [mol([]), mol([b"C"]), mol([b"C", b"O"], [(0, 1, 1, 1)]), mol([b"C", b"O"], [(0, 1, 2, 2)]), ring(7), ring(8, 4, b"c"), star, words]
    for m in molecules:
        check(eng, Tables(dev, [m]))                                               # n = 1
    ref = check(eng, Tables(dev, molecules))
    assert ref["fp"]["max_paths"].tolist() == [0, 0, 1, 1, 6, 7, 20, 7] and not ref["fp"]["flags"].any()
    assert ref["fp"]["n_bits"].tolist()[:4] == [0, 2, 6, 6] and (ref["bits"][2] != ref["bits"][3]).any()


def test_more_directed_bonds_than_threads(eng, dev):
    """a ladder of 2 x 60 atoms has 178 bonds, 356 directed bonds for 256 threads: a thread walks from several"""
    t = Tables(dev, [ladder(60), mol([b"C"])])
    assert int(t.mols["n_bonds"][0]) == 178
    ref = check(eng, t)
    assert 7 < ref["fp"]["max_paths"][0] < F.DEFAULT_STEPS and 100 < ref["fp"]["n_bits"][0] < 2048


def test_chains_of_999_and_1000_atoms(eng, dev):
    syms = [b"C", b"N", b"O"] * 334
    t = Tables(dev, [H.chain(syms[:999]), H.chain(syms[:1000]), H.chain(syms[:5])])
    ref = check(eng, t)
    assert ref["fp"]["flags"].tolist() == [0, F.TOO_LARGE, 0] and ref["fp"]["max_paths"].tolist() == [7, 0, 4]
    assert ref["bits"][0].any() and not ref["bits"][1].any()


@functools.lru_cache(maxsize=None)
def complete_ref(max_steps):
    mols, atoms, bonds, text = F.M.build_tables([H.complete(8), H.complete(9), H.chain([b"C", b"O"])])
    return (mols, atoms, bonds, text), F.pack(mols, atoms, bonds, text, tables=H.TABLES, max_steps=max_steps)


@pytest.mark.parametrize("max_steps,flags,most", [(0, [0, FP_LIMIT, 0], [1957, F.LIMITED_PATHS, 1]), (8660, [0, 0, 0], [1957, 8660, 1]),
                                                  (8659, [0, FP_LIMIT, 0], [1957, F.LIMITED_PATHS, 1])])
def test_the_step_limit_on_complete_graphs(eng, dev, max_steps, flags, most):
    """K8 is written at the default and K9 is limited; K9 is written at 8660 steps and limited at 8659; the molecule behind a
    limited one is left alone"""
    arrays, ref = complete_ref(max_steps)
    assert ref["fp"]["flags"].tolist() == flags and ref["fp"]["max_paths"].tolist() == most
    check(eng, Tables(dev, arrays=arrays), ref, max_steps=max_steps)


def test_refusals_leave_the_other_molecules_alone(eng, dev):
    ok = mol([b"C", b"[NH3+]", b"O"], [(0, 1, 1, 1), (1, 2, 1, 1)])
    two = [b"C", b"N"]
    molecules = [ok, H.chain([b"C"] * 1000), ok, mol(two, [(0, 2, 1, 1)]), mol(two, [(1, 1, 1, 1)]), mol(two, [(0, 1, 1, 1), (1, 0, 2, 2)]),
                 mol([b"C", b"Ph", b"[Xx]"], [(0, 1, 1, 1), (1, 2, 1, 1)]), mol([b"R", b"N"], [(0, 0, 1, 1)]), H.complete(9), ok]
    mols, atoms, bonds, text = F.M.build_tables(molecules)
    mols["flags"][9] = 1 | 1 << 10                                                 # truncated; the bits of the passes are not copied
    t = Tables(dev, arrays=(mols, atoms, bonds, text))
    ref = check(eng, t)
    assert ref["fp"]["flags"].tolist() == [0, F.TOO_LARGE, 0, F.BAD_BOND, F.BAD_BOND, F.BAD_BOND, F.PSEUDO, F.PSEUDO | F.BAD_BOND, F.LIMIT, F.TRUNCATED]
    assert (ref["bits"][0] == ref["bits"][2]).all() and (ref["bits"][0] == ref["bits"][9]).all() and ref["bits"][0].any()
    # records beyond the tables passed: the last molecule's atoms, bonds or text are cut off
    for cut in ({"na": len(t.atoms) - 1}, {"nb": len(t.bonds) - 1}, {"nt": len(t.text) - 1}):
        sizes = (cut.get("na", len(t.atoms)), cut.get("nb", len(t.bonds)), cut.get("nt", len(t.text)))
        want = F.pack(t.mols, t.atoms, t.bonds, t.text, tables=H.TABLES, n_atom_records=sizes[0], n_bond_records=sizes[1], n_text_bytes=sizes[2])
        assert int(want["fp"]["flags"][-1]) == F.TRUNCATED | F.BEYOND and want["fp"]["flags"].tolist()[:-1] == ref["fp"]["flags"].tolist()[:-1]
        got = run(eng, t, sizes=sizes)
        assert got.rc == 0 and got.recs.tobytes() == want["fp"].tobytes() and (got.bits == want["bits"]).all()
    mols, atoms, bonds, text = F.M.build_tables([ok, ok])
    atoms["sym0"][4] = 60000                                                       # a symbol beyond the text
    ref = check(eng, Tables(dev, arrays=(mols, atoms, bonds, text)))
    assert ref["fp"]["flags"].tolist() == [0, F.BEYOND]


@pytest.fixture(scope="module")
def batch(dev):
    """64 random molecules of 0 to 40 atoms of every symbol class with about half as many bonds as atoms"""
    rng = np.random.default_rng(64)
    molecules = []
    for _ in range(64):
        na = int(rng.integers(0, 41))
        molecules.append(random_molecule(rng, na, na // 2 + int(rng.integers(0, 3))))
    return Tables(dev, molecules)


@pytest.mark.parametrize("max_bonds", [1, 3, 7])
def test_64_random_molecules_and_two_runs_with_identical_words(eng, batch, max_bonds):
    ref = check(eng, batch, max_bonds=max_bonds)
    flags = ref["fp"]["flags"]
    assert ((flags & FP_REFUSED) == 0).sum() >= 32 and ((flags & F.PSEUDO) != 0).sum() >= 16
    a, b = run(eng, batch, max_bonds=max_bonds), run(eng, batch, max_bonds=max_bonds)
    assert a.rc == b.rc == 0 and a.recs.tobytes() == b.recs.tobytes() and a.bits.tobytes() == b.bits.tobytes()
    if max_bonds == 7:
        assert (check(eng, batch, ref, max_bonds=0)["bits"] == ref["bits"]).all()  # 0 means 7


def test_engine_methods(eng, batch):
    ref = F.pack(batch.mols, batch.atoms, batch.bonds, batch.text, tables=H.TABLES, max_bonds=3)
    rec = {"mols": batch.mols, "atoms": batch.atoms, "bonds": batch.bonds, "text": batch.text}
    out = eng.fingerprint_pack(rec, max_bonds=3)
    assert out["fp"].tobytes() == ref["fp"].tobytes() and out["bits"].dtype == np.uint32 and (out["bits"] == ref["bits"]).all()
    kept = eng.fingerprint_pack(rec, max_bonds=3, keep_device=True)
    assert kept["bits"].is_cuda and (kept["bits"].cpu().numpy().view(np.uint32) == ref["bits"]).all()
    turned = np.roll(ref["bits"], 1, axis=0)
    want = F.tanimoto(ref["bits"], turned)
    for a, b in ((kept["bits"], turned), (ref["bits"], turned)):
        got = eng.tanimoto(a, b)
        assert got["both"].tolist() == want["both"].tolist() and got["either"].tolist() == want["either"].tolist()
        assert got["similarity"].tobytes() == want["similarity"].tobytes()
    with pytest.raises(ValueError, match="row with row"):
        eng.tanimoto(ref["bits"], turned[:3])


def test_fingerprint_argument_errors(eng, dev, synth_ckpt):
    t = Tables(dev, H.molecules()[:4])

    def refused(expect, **over):
        assert_refused(run(eng, t, **over), "mnx_fingerprint_pack: " + expect)

    for name in ("mols", "atoms", "bonds", "text", "recs", "bits"):
        refused("null pointer", **{name: None})
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "mols, atoms and bonds must be 8-byte aligned, recs and bits 4-byte"
    for name, k in (("mols", 0), ("atoms", 1), ("bonds", 2)):
        refused(aligned, **{name: _p(t.d[k], 4)})
    refused(aligned, recs=_p(t.d[0], 2))
    refused(aligned, bits=_p(t.d[0], 1))
    refused("max_bonds must be 1 to 7, or 0 for 7", max_bonds=8)
    refused("max_steps must not exceed MNX_FP_MAX_STEPS (1048576)", max_steps=(1 << 20) + 1)
    assert run(eng, t, max_bonds=7, max_steps=1 << 20).rc == 0                     # the largest values are admitted

    class Bare(Engine):                                                            # a fresh handle that was told no tables
        def _set_symbol_tables(self):
            pass

        def _set_fragments(self):
            pass
    bare = Bare(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=2, dec_slots=32)
    try:
        refused("call mnx_set_symbol_tables first", h=bare.h)
        assert eng.lib.mnx_last_error(eng.h).decode() == "mnx_fingerprint_pack: max_steps must not exceed MNX_FP_MAX_STEPS (1048576)"
    finally:
        bare.close()


@pytest.mark.parametrize("n", [1, 65])
def test_tanimoto_rows(eng, dev, n):
    """identical rows, disjoint rows, both rows empty (0.0), and rows of the molecules of the host test; each output null in turn"""
    rng = np.random.default_rng(n)
    real = np.stack([F.words_of(H.bits_of(m)) for m in H.molecules()[:8]])
    a = rng.integers(0, 1 << 32, (n, FP_WORDS), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, (n, FP_WORDS), dtype=np.uint64).astype(np.uint32)
    for r in range(n):
        kind = r % 5 if n > 1 else 4
        if kind == 0:
            b[r] = a[r]                                                            # identical
        elif kind == 1:
            b[r] = ~a[r]                                                           # disjoint
        elif kind == 2:
            a[r] = b[r] = 0                                                        # both empty
        elif kind == 3:
            a[r], b[r] = real[r % 8], real[(r + 1) % 8]
    for x, y in ((a, b), (a, a), (a, ~a), (np.zeros_like(a), np.zeros_like(a))):
        want = F.tanimoto(x, y)
        got = similar(eng, dev, x, y)
        assert got.rc == 0, got.error
        assert got.both.tolist() == want["both"].tolist() and got.either.tolist() == want["either"].tolist()
        assert got.similarity.tobytes() == want["similarity"].tobytes()
    assert want["similarity"].tolist() == [0.0] * n                                # both rows empty
    assert F.tanimoto(a, a)["similarity"].tolist() == [1.0 if r.any() else 0.0 for r in a]
    want = F.tanimoto(a, b)
    for name in ("both", "either", "similarity"):
        got = similar(eng, dev, a, b, **{name: None})
        assert got.rc == 0, got.error
        for other in ("both", "either", "similarity"):
            x = getattr(got, other)
            if other == name:
                assert (x.view(np.uint8) == packed_tables.FILL).all()              # not written
            else:
                assert x.tobytes() == want[other].tobytes()


def test_tanimoto_argument_errors(eng, dev):
    a = np.ones((2, FP_WORDS), np.uint32)
    skew = _up(dev, np.zeros(64, np.uint8))

    def refused(expect, **over):
        assert_refused(similar(eng, dev, a, a, **over), "mnx_tanimoto: " + expect)

    refused("null pointer", a=None)
    refused("null pointer", b=None)
    refused("both, either and similarity are all null", both=None, either=None, similarity=None)
    for n in (0, -1, 65537):
        refused("1 <= n <= 65536 required", n=n)
    aligned = "a, b, both and either must be 4-byte aligned, similarity 8-byte"
    for name, off in (("a", 2), ("b", 1), ("both", 2), ("either", 1), ("similarity", 4)):
        refused(aligned, **{name: _p(skew, off)})


def test_the_place_behind_the_chain(eng):
    """read -> kekulize -> normalize -> fingerprint: the aromatic and the Kekule spelling of benzene get the same words and the
    similarity 1.0; without the passes they do not"""
    rec = eng.smiles_read(["c1ccccc1", "C1=CC=CC=C1"], keep_device=True)
    assert not (rec["read"]["flags"] & READ_REFUSED).any()
    plain = eng.fingerprint_pack(rec)
    assert not plain["fp"]["flags"].any() and (plain["bits"][0] != plain["bits"][1]).any()
    assert eng.tanimoto(plain["bits"][:1], plain["bits"][1:])["similarity"][0] < 1.0
    last = eng.normalize_pack(eng.kekulize_pack(rec, keep_device=True), keep_device=True)
    fp = eng.fingerprint_pack(last, keep_device=True)
    words = fp["bits"].cpu().numpy().view(np.uint32)
    assert not fp["fp"]["flags"].any() and words[0].any() and (words[0] == words[1]).all()
    assert eng.tanimoto(fp["bits"][:1], fp["bits"][1:])["similarity"].tolist() == [1.0]
    want = F.pack(last["mols"], last["atoms"], last["bonds"], last["text"], tables=H.TABLES)
    assert (words == want["bits"]).all() and fp["fp"].tobytes() == want["fp"].tobytes()


def test_end_to_end_predict_fingerprint_facade_and_evaluate(eng, dev, synth_ckpt, monkeypatch):
    """8 synthetic images: predict_fingerprints (predict_pipeline(packed=True) with the fingerprint in every dict) against the calls
    made by hand on the tables of the same prediction; smiles_fingerprints and tanimoto on a caller's strings; the facade's
    graph_fingerprint; evaluate's graph_tanimoto at two bonds against the mean computed by hand. With paths of two bonds P(s) <= 1 + (max_atoms - 2) < 4096 for any graph,
    so nothing hides behind the step limit, however dense the synthetic checkpoint's bond graphs are."""
    from molnextr_amd import evaluate as E
    from molnextr_amd.model import molnextr, predict_fingerprints, predict_pipeline, smiles_fingerprints, tanimoto
    imgs = W.synthetic_images(8, first_index=E2E_FIRST_INDEX).to(dev)
    rec = eng.graph_pack(eng.predict(imgs, ref_batch=4), keep_device=True)
    by_hand = eng.fingerprint_pack(rec)
    oracle = F.pack(rec["mols"], rec["atoms"], rec["bonds"], rec["text"], tables=H.TABLES)
    assert by_hand["fp"].tobytes() == oracle["fp"].tobytes() and (by_hand["bits"] == oracle["bits"]).all()
    plain = predict_pipeline(eng, imgs, ref_batch_size=4, packed=True)
    got = predict_fingerprints(eng, imgs, ref_batch_size=4)
    for p, g, r, words in zip(plain, got, by_hand["fp"], by_hand["bits"]):
        assert "fingerprint" not in p and set(g) == set(p) | {"fingerprint"}
        assert g["fingerprint"] == (None if int(r["flags"]) & (FP_REFUSED | FP_LIMIT) else words.tobytes())
        assert g["fingerprint"] is None or len(g["fingerprint"]) == 256
    with pytest.raises(ValueError, match="predict_fingerprints needs packed=True: the paths are walked in the packed tables"):
        predict_fingerprints(eng, imgs[:1], packed=False)

    items = smiles_fingerprints(eng, ["c1ccccc1", "C1=CC=CC=C1", "C1CC", "CC(=O)Oc1ccccc1C(=O)O"], kekulize=True, normalize=True)
    assert items[0]["fingerprint"] == items[1]["fingerprint"] and len(items[0]["fingerprint"]) == 256 and items[0]["fingerprint_flags"] == 0
    assert items[2]["fingerprint"] is None and items[2]["read_flags"] & READ_REFUSED                # an unreadable string
    assert smiles_fingerprints(eng, ["CCCC"], max_bonds=1)[0]["fingerprint"] != smiles_fingerprints(eng, ["CCCC"])[0]["fingerprint"]
    with pytest.raises(TypeError, match="no pass named"):
        smiles_fingerprints(eng, ["C"], aromatize=True)
    strings = ["c1ccccc1", "CC(=O)Oc1ccccc1C(=O)O", "c1ccccc1", "C1CC", "CCO"]
    others = ["C1=CC=CC=C1", "OC(=O)c1ccccc1O", "CCCCCC", "CCO", "CCO"]
    sims = tanimoto(eng, strings, others, kekulize=True, normalize=True)
    assert sims[0] == 1.0 and 0.3 < sims[1] < 1.0 and sims[2] == 0.0 and sims[3] == 0.0 and sims[4] == 1.0, sims
    assert tanimoto(eng, strings[:1], others[:1])[0] < 1.0 and tanimoto(eng, [], []) == []

    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: synth_ckpt)      # the session's copy: no second build
    pages = [W.synthetic_page(c) for c in range(5)]
    m = molnextr("synthetic", dev, max_batch=4, graph_smiles=True, graph_kekulize=True, graph_normalize=True)
    try:
        assert m.graph_fingerprint is False
        m.graph_fingerprint = True                                                 # an attribute: the constructor's list is closed
        out = m.predict_images(pages, batch_size=4)
        want = predict_fingerprints(m.engine, m._transform(pages), m.tokenizer, ref_batch_size=4, smiles=True, stereo=False, kekulize=True,
                                    normalize=True)
        assert all("fingerprint" in o for o in out) and [o["fingerprint"] for o in out] == [p["fingerprint"] for p in want]
        assert m.tanimoto(["CCO"], ["CCO"]) == [1.0]
        m.graph_fingerprint = False                                                # the default: no such key
        assert all("fingerprint" not in o for o in m.predict_images(pages[:2], batch_size=2))
    finally:
        m.engine.close()

    import torch
    from molnextr_amd.shard import MAX_LEN
    kept, n, kmax = {}, 8, eng.max_atoms
    E.run_inference(eng, lambda i: W.synthetic_page(i % 15), n, batch_size=4, keep_records=kept)
    r = torch.from_numpy(kept["records"]).to(torch.device("cuda", 0))
    edges = r[:, 2 + MAX_LEN + kmax:].contiguous().view(torch.uint8)[:, :kmax * kmax].reshape(n, kmax, kmax).contiguous()
    pack = eng.graph_pack({"lengths": r[:, 0].contiguous(), "n_atoms": r[:, 1].contiguous(), "tokens": r[:, 2:2 + MAX_LEN].contiguous(),
                           "atom_idx": r[:, 2 + MAX_LEN:2 + MAX_LEN + kmax].contiguous(), "edges": edges}, keep_device=True)
    recs, _, data, _, _ = eng.smiles_pack(pack, canonical=True)
    own = [None if int(x["flags"]) & SMILES_REFUSED else data[int(x["text0"]):int(x["text0"]) + int(x["len"])].decode() for x in recs]
    gold = [t if t is not None else "C" for t in own]

    def prints(side):
        last = eng.normalize_pack(eng.kekulize_pack(side, keep_device=True), keep_device=True)
        return eng.fingerprint_pack(last, max_bonds=2)
    sides = [prints(pack), prints(eng.smiles_read(gold, keep_device=True))]
    assert not any((s["fp"]["flags"] & FP_LIMIT).any() for s in sides)
    each = F.tanimoto(sides[0]["bits"], sides[1]["bits"])["similarity"].tolist()
    print("written", [t is not None for t in own], "similarity", each)
    scores = E.graph_tanimoto_scores(eng, kept["records"], gold, chunk=4, max_bonds=2)
    assert set(scores) == {"graph_tanimoto", "tanimoto_limited"} and scores == E.graph_tanimoto_scores(eng, kept["records"], gold, max_bonds=2)
    assert scores["graph_tanimoto"] == math.fsum(each) / n and scores["tanimoto_limited"] == 0, (scores, each)
    # a molecule the writers refuse may score 0; one at least is written on both sides and equals its own string read back
    assert any(t is not None and s == 1.0 for t, s in zip(own, each)), (own, each)
    args = E.build_parser().parse_args(["--test_file", "t.csv", "--load_path", "synthetic", "--graph_match", "--graph_tanimoto", "--graph_tanimoto_bonds", "2"])
    assert args.graph_tanimoto and args.graph_tanimoto_bonds == 2
