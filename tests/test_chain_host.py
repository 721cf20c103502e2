"""The chain of passes over the packed tables as Python drives it (molnextr_amd/chain.py), without a GPU: a recording stand-in
engine shows, for every subset of the five flags and every writer, the order of the calls, which record each stage is handed,
where keep_device is set and which keys a prediction carries; the error texts and the signatures are the ones the call sites had
when each spelled the chain out by hand, written here as literals. The order below is written by hand too, not read from the table."""
import inspect
import itertools
import types

import numpy as np
import pytest

import molfile_ref as R
from molnextr_amd import evaluate as E
from molnextr_amd import model as M
from molnextr_amd import weights as W
from molnextr_amd.engine import MOL_FORMULA_LEFT, MOLFILE_DTYPE, READ_DTYPE, SMILES_DTYPE

# option, Engine method, key of a prediction dict, key of canonical_smiles' items — in the documented order of the chain
ORDER = [("formula", "formula_pack", "formula", "formula_flags"), ("expand", "expand_pack", "expanded", None),
         ("keep_main", "main_pack", "main", "main_flags"), ("kekulize", "kekulize_pack", "kekulized", "kekulize_flags"),
         ("normalize", "normalize_pack", "normalized", "normalize_flags")]
SUBSETS = [dict(zip([o[0] for o in ORDER], bits)) for bits in itertools.product((False, True), repeat=5)]
TOK = {"chartok_coords": types.SimpleNamespace(maxx=64)}


def record(symbols, flags=0, **side):
    """one molecule on a path, as packed tables"""
    mols, atoms, bonds, text = R.build_tables([(symbols, [(k, 2 * k) for k in range(len(symbols))],
                                                [(k, k + 1, 1, 1) for k in range(len(symbols) - 1)])])
    mols["flags"] = flags
    return {"mols": mols, "atoms": atoms, "bonds": bonds, "text": text, **side}


def symbols_of(rec):
    return [rec["text"][a["sym0"]:a["sym0"] + a["sym_len"]] for a in rec["atoms"]]


class Recorder:
    """Every method that predict_pipeline's packed tail and canonical_smiles call, each logging (name, the record it was handed,
    keep_device). A growing pass appends one atom that came from the last one, main drops atom 0, a respelling pass keeps them."""
    max_atoms = 160

    def __init__(self):
        self.log = []

    def predict(self, images, **kw):
        return "predicted"

    def graph_pack(self, out, keep_device=False):
        assert out == "predicted"
        self.log.append(("graph_pack", out, keep_device))
        return record([b"C", b"[CH2CH3]"])

    def smiles_read(self, strings, keep_device=False):
        self.log.append(("smiles_read", strings, keep_device))
        return record([b"C", b"[CH2CH3]"], read=np.zeros(1, READ_DTYPE))

    def _grow(self, name, rec, keep_device, flags):
        self.log.append((name, rec, keep_device))
        syms = symbols_of(rec)
        return record(syms + [b"N"], flags, origin=np.array(list(range(len(syms))) + [len(syms) - 1], np.uint16))

    def formula_pack(self, rec, keep_device=False):
        return self._grow("formula_pack", rec, keep_device, MOL_FORMULA_LEFT)

    def expand_pack(self, rec, keep_device=False):
        return self._grow("expand_pack", rec, keep_device, 2)

    def main_pack(self, rec, keep_device=False):
        self.log.append(("main_pack", rec, keep_device))
        syms = symbols_of(rec)
        return record(syms[1:], 1 << 18, origin=np.arange(1, len(syms), dtype=np.uint16))

    def _respell(self, name, rec, keep_device, flags):
        self.log.append((name, rec, keep_device))
        syms = symbols_of(rec)
        return record(syms, flags, atom_notes=np.arange(len(syms), dtype=np.uint8) | 64)

    def kekulize_pack(self, rec, keep_device=False):
        return self._respell("kekulize_pack", rec, keep_device, 128)

    def normalize_pack(self, rec, keep_device=False):
        return self._respell("normalize_pack", rec, keep_device, 16)

    def smiles_pack(self, rec, stereo=False, double_bonds=False, canonical=False, symmetry=False):
        self.log.append(("smiles_pack", rec, None))
        recs = np.zeros(1, SMILES_DTYPE)
        recs["len"] = 2
        na = len(rec["atoms"])
        order = np.arange(na, dtype=np.uint16)
        return (recs, order, b"CC") + ((order + 10, order + 20) if canonical else ())

    def molfile_pack(self, rec, scale=None):
        self.log.append(("molfile_pack", rec, None))
        files = np.zeros(1, MOLFILE_DTYPE)
        files["len"] = 3
        return files, b"mol"


def check_calls(log, first, on, writer):
    """the calls of one run: `first`, the passes of `on` in ORDER, the writer; each stage on the record of the one before it;
    keep_device exactly where a later stage or a writer follows"""
    passes = [o[1] for o in ORDER if on[o[0]]]
    assert [c[0] for c in log[0]] == [first] + passes + ([writer] if writer else [])
    made = log[1]                                              # the records in the order they were returned
    for k, (name, handed, keep) in enumerate(log[0][1:], 1):
        assert handed is made[k - 1], (name, "was not handed the record of the call before it")
    n = 1 + len(passes)
    for k, (name, _, keep) in enumerate(log[0][:n]):
        assert bool(keep) == (k + 1 < n or writer is not None), (name, keep, on, writer)


def logged(eng):
    """wraps the recorder's methods so that the records they return are kept, in order"""
    made = []
    for name in ["graph_pack", "smiles_read"] + [o[1] for o in ORDER]:
        def wrap(*a, _f=getattr(eng, name), **kw):
            made.append(_f(*a, **kw))
            return made[-1]
        setattr(eng, name, wrap)
    return made


@pytest.mark.parametrize("writer", [None, "smiles", "molfile"])
def test_every_subset_of_the_flags_runs_in_order_and_keeps_its_tables_where_they_are_read(writer):
    for on in SUBSETS:
        eng = Recorder()
        made = logged(eng)
        preds = M.predict_pipeline(eng, None, TOK, packed=True, **on, **({writer: True} if writer else {}))
        check_calls((eng.log, made), "graph_pack", on, writer and writer + "_pack")
        assert len(preds) == 1
        p = preds[0]
        want = {"chartok_coords", "bonds"} | {o[2] for o in ORDER if on[o[0]]}
        want |= {"smiles": {"graph_smiles", "graph_smiles_order"}, "molfile": {"molfile"}, None: set()}[writer]
        assert set(p) == want, on
        assert p["chartok_coords"]["symbols"] == ["C", "[CH2CH3]"]                 # the predicted atoms are what they are without a pass
        n = 2
        if on["formula"]:
            assert p["formula"]["origin"] == [0, 1, 1] and p["formula"]["symbols"] == ["C", "[CH2CH3]", "N"]
            assert p["formula"]["replaced"] == [] and p["formula"]["left"] == [1] and p["formula"]["flags"] == MOL_FORMULA_LEFT
            assert set(p["formula"]) == {"symbols", "coords", "bonds", "origin", "flags", "replaced", "left"}
            n += 1
        if on["expand"]:                                                           # composed through formula to the predicted atom
            assert p["expanded"]["origin"] == ([0, 1, 1, 1] if on["formula"] else [0, 1, 1])
            assert set(p["expanded"]) == {"symbols", "coords", "bonds", "origin", "flags"}
            n += 1
        if on["keep_main"]:                                                        # not composed: the molecule the pass received
            assert p["main"]["origin"] == list(range(1, n)) and set(p["main"]) == {"symbols", "coords", "bonds", "origin", "flags"}
            n -= 1
        for key, flags in (("kekulized", 128), ("normalized", 16)):
            if key in p:
                assert p[key] == {"symbols": p[key]["symbols"], "bonds": p[key]["bonds"], "hydrogens": list(range(n)),
                                  "notes": [k | 64 for k in range(n)], "flags": flags} and len(p[key]["symbols"]) == n
        if writer == "smiles":
            assert p["graph_smiles"] == "CC" and p["graph_smiles_order"] == list(range(n))
        if writer == "molfile":
            assert p["molfile"] == "mol"


def test_the_ranks_of_the_tables_the_writer_read_are_attached_once():
    for on in SUBSETS:
        eng = Recorder()
        p, = M.predict_pipeline(eng, None, TOK, packed=True, smiles=True, canonical=True, **on)
        n = 2 + on["formula"] + on["expand"] - on["keep_main"]
        assert p["canonical_rank"] == list(range(10, 10 + n)) and p["symmetry_class"] == list(range(20, 20 + n))
        assert [c[0] for c in eng.log].count("smiles_pack") == 1 and eng.log[-1][0] == "smiles_pack"


def test_canonical_smiles_runs_the_same_chain_and_reports_each_stage_its_flags():
    flags = {"formula_flags": MOL_FORMULA_LEFT, "main_flags": 1 << 18, "kekulize_flags": 128, "normalize_flags": 16}
    for on in SUBSETS:
        eng = Recorder()
        made = logged(eng)
        item, = M.canonical_smiles(eng, ["C[CH2CH3]"], **on)
        check_calls((eng.log, made), "smiles_read", on, "smiles_pack")
        keys = [o[3] for o in ORDER if on[o[0]] and o[3]]
        assert item == {"smiles": "CC", "read_flags": 0, "err_pos": 0, "smiles_flags": 0, **{k: flags[k] for k in keys}}
    assert M.canonical_smiles(Recorder(), []) == []


def test_needs_packed_messages_and_the_one_reported_first():
    texts = {"formula": "formula=True needs packed=True: the labels are replaced in the packed tables",
             "keep_main": "keep_main=True needs packed=True: the atoms are dropped from the packed tables",
             "normalize": "normalize=True needs packed=True: the atoms are respelled in the packed tables",
             "kekulize": "kekulize=True needs packed=True: the aromatic systems are rewritten in the packed tables",
             "expand": "expand=True needs packed=True: the labels are replaced in the packed tables",
             "molfile": "molfile=True needs packed=True: the molfiles are written from the packed tables",
             "smiles": "smiles=True needs packed=True: the graph SMILES are written from the packed tables"}
    for name, text in texts.items():
        with pytest.raises(ValueError) as err:
            M.predict_pipeline(None, None, **{name: True})
        assert str(err.value) == text
    names = list(texts)                                         # the order they were always reported in
    for k in range(len(names)):
        with pytest.raises(ValueError) as err:
            M.predict_pipeline(None, None, **dict.fromkeys(names[k:], True))
        assert str(err.value) == texts[names[k]]


def test_facade_messages_and_the_one_reported_first(monkeypatch):
    monkeypatch.setattr(W, "synthetic_checkpoint", lambda *a, **k: {"encoder": {}, "decoder": {}})
    texts = {"graph_expand": "graph_expand=True needs graph_smiles=True or graph_molfile=True: the expanded molecule is what they write",
             "graph_normalize": "graph_normalize=True needs graph_smiles=True or graph_molfile=True: the normalised molecule is what they write",
             "graph_kekulize": "graph_kekulize=True needs graph_smiles=True or graph_molfile=True: the kekulised molecule is what they write",
             "graph_formula": "graph_formula=True needs graph_smiles=True or graph_molfile=True: the molecule with its formulas replaced is what they write",
             "graph_keep_main": "graph_keep_main=True needs graph_smiles=True or graph_molfile=True: the main molecule is what they write"}
    names = list(texts)
    for k, name in enumerate(names):
        for given in ({name: True}, dict.fromkeys(names[k:], True)):
            with pytest.raises(ValueError) as err:
                M.molnextr("synthetic", **given)
            assert str(err.value) == texts[name]


def test_evaluate_messages(capsys):
    texts = {"--graph_normalize": "--graph_normalize adds a score to --graph_match",
             "--graph_kekulize": "--graph_kekulize adds a score to --graph_match",
             "--graph_formula": "--graph_formula adds a score to --graph_match",
             "--graph_keep_main": "--graph_keep_main adds a score to --graph_match"}
    for flag, text in texts.items():
        with pytest.raises(SystemExit):
            E.main(["--test_file", "t.csv", "--load_path", "synthetic", flag])
        assert capsys.readouterr().err.endswith("error: " + text + "\n")


def test_signatures_are_the_ones_the_call_sites_had():
    def parameters(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    free = inspect.Parameter.empty
    assert parameters(M.predict_pipeline) == [
        ("engine", free), ("images", free), ("tokenizer", None), ("ref_batch_size", 16), ("max_len", None), ("beam_size", 1),
        ("compute_confidence", False), ("labels", None), ("free_run", False), ("packed", False), ("molfile", False),
        ("molfile_scale", None), ("smiles", False), ("stereo", False), ("double_bonds", False), ("canonical", False), ("expand", False),
        ("symmetry", False), ("normalize", False), ("kekulize", False), ("formula", False), ("keep_main", False)]
    assert parameters(M.canonical_smiles) == [("engine", free), ("smiles_list", free), ("expand", False), ("normalize", False),
                                              ("kekulize", False), ("formula", False), ("keep_main", False)]
    assert parameters(M.molnextr.canonical_smiles) == [("self", free)] + parameters(M.canonical_smiles)[1:]
    assert parameters(M.molnextr.__init__) == [
        ("self", free), ("model_path", free), ("device", None), ("max_batch", 32), ("dtype", "fp16x3"), ("device_preprocess", True),
        ("image_format", "fp32"), ("packed_results", False), ("graph_molfile", False), ("graph_smiles", False), ("graph_stereo", False),
        ("graph_double_bonds", False), ("graph_canonical", False), ("graph_expand", False), ("graph_symmetry", False),
        ("graph_normalize", False), ("graph_kekulize", False), ("graph_formula", False), ("graph_keep_main", False)]
    assert parameters(E.graph_match_scores) == [("engine", free), ("records", free), ("gold", free), ("chunk", 512), ("normalize", False),
                                                ("kekulize", False), ("formula", False), ("keep_main", False)]
    for name in ("graph_expand", "graph_normalize", "graph_kekulize", "graph_formula", "graph_keep_main"):
        assert getattr(M.molnextr, name) is False                                  # the class attributes stay


def test_the_facade_passes_a_flag_only_when_it_is_on_and_copies_the_stage_keys(monkeypatch):
    import contextlib
    seen = []

    def fake_pipeline(eng, x, tok, ref_batch_size=16, **kw):
        seen.append(kw)
        return [{"chartok_coords": {"symbols": ["C"], "coords": [[0.0, 0.0]]}, "bonds": [],
                 **{o[2]: {"hydrogens": [3], "origin": [0], "of": o[0]} for o in ORDER if kw.get(o[0])}} for _ in x]

    monkeypatch.setattr(M, "predict_pipeline", fake_pipeline)
    monkeypatch.setattr(M.molnextr, "_side_context", lambda self: contextlib.nullcontext())
    for on in SUBSETS:
        m = M.molnextr.__new__(M.molnextr)
        m.engine = types.SimpleNamespace(max_batch=8, preprocess=lambda images: list(images))
        m.group_images, m.tokenizer, m.device_preprocess, m.graph_smiles = 8, None, True, True
        for name, v in on.items():
            setattr(m, "graph_" + name, v)
        del seen[:]
        out, = m.predict_images([np.zeros((4, 4, 3), np.uint8)], batch_size=1)
        assert seen == [{"packed": True, "smiles": True, "stereo": False, **{k: True for k, v in on.items() if v}}]
        want = {"predicted_smiles", "predicted_molfile"} | {o[2] for o in ORDER if on[o[0]]}
        want |= ({"hydrogens"} if on["normalize"] else set()) | ({"main_atoms"} if on["keep_main"] else set())
        assert set(out) == want
        for o in ORDER:
            if on[o[0]]:
                assert out[o[2]]["of"] == o[0]
        assert out.get("hydrogens", [3]) == [3] and out.get("main_atoms", [0]) == [0]
