"""CPU: confidences on the continuous-batching path — the ABI symbols, the name-length bits of the token classes, and the
facade's routing of predict_images(return_confidence=True) through predict_pipeline with a stub engine. The device side is
tests/test_gpu_confidence.py."""
import contextlib
import types
import warnings

import pytest

from molnextr_amd import engine as E
from molnextr_amd import model as M
from molnextr_amd.engine import MNX_ERR_RANGE, MnxError


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(E.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


def test_confidence_entry_points_are_exported_and_listed(lib):
    for name in ("mnx_predict_confidence", "mnx_confidence"):
        assert name in E.SYMBOLS
        assert hasattr(lib, name)
    assert len(lib.mnx_predict_confidence.argtypes) == 16 and len(lib.mnx_confidence.argtypes) == 13
    assert lib.mnx_abi_version() == E.ABI_VERSION == 7


def test_confidence_rejects_a_null_handle_without_gpu(lib):
    assert lib.mnx_confidence(None, None, None, None, 1, 1, None, None, None, 1, None, None, None) == -1
    assert lib.mnx_predict_confidence(None, None, 1, 1, 1, None, None, None, None, None, 1, None, None, None, None, None) == -1


def test_token_classes_carry_symbol_name_lengths(lib):
    """mnx_set_token_classes flags bits 2-4 = name length - 1: '<unk>' (id 3) spells five characters, every other symbol
    one; bits 0-1 (what the atom scan reads) are unchanged."""
    from molnextr_amd.tokenizer import UNK_ID, CharTokenizer
    seen = {}

    def set_tc(h, flags, n, *ids):
        seen["flags"], seen["n"], seen["ids"] = bytes(flags[:n]), n, ids
        return 0

    fake = types.SimpleNamespace(lib=types.SimpleNamespace(mnx_set_token_classes=set_tc), h=None,
                                 _check=lambda rc, what: None, token_class_flags=E.Engine.token_class_flags)
    E.Engine._set_token_classes(fake)
    tok = CharTokenizer(64)
    flags = seen["flags"]
    assert seen["n"] == tok.offset == len(flags)
    assert UNK_ID == 3 and (flags[3] >> 2) & 7 == 4
    for i, f in enumerate(flags):
        assert f & 1 == (1 if tok.is_symbol(i) else 0) and (f >> 1) & 1 == (1 if tok.is_atom(i) else 0), i
        if i != UNK_ID:
            assert f >> 2 == 0, (i, tok.itos[i])
        if tok.is_symbol(i):
            assert ((f >> 2) & 7) + 1 == len(tok.itos[i]), i


class _StubEngine:
    built = []

    def __init__(self, enc, dec, device=0, max_batch=32, dtype="fp16x3", **kw):
        self.dtype, self.device, self.max_batch, self.closed = dtype, device, max_batch, False
        _StubEngine.built.append(self)

    def close(self):
        self.closed = True

    def preprocess(self, images):
        assert not self.closed
        return list(images)

    def encode(self, x):
        raise AssertionError("the confidence path must not run the per-batch encode")


def _facade(monkeypatch):
    monkeypatch.setattr(M, "Engine", _StubEngine)
    _StubEngine.built = []
    m = M.molnextr.__new__(M.molnextr)
    m._states, m._max_batch = {"encoder": {}, "decoder": {}}, 8
    m.engine = _StubEngine({}, {}, device=0, max_batch=8, dtype="fp16x3")
    m.group_images, m.tokenizer, m.device_preprocess = 4, None, True
    monkeypatch.setattr(M.molnextr, "_side_context", lambda self: contextlib.nullcontext())
    monkeypatch.setattr(M, "decode_batch",
                        lambda *a, **kw: (_ for _ in ()).throw(AssertionError("decode_batch must not be called")))
    return m


def _pred(i, dtype):
    """One predict_pipeline(compute_confidence=True) dict: two atoms, one single bond."""
    c = {"smiles": "CC", "symbols": ["C", "C"], "indices": [3, 6], "coords": [[0.1, 0.2], [0.3, 0.4]],
         "atom_scores": [0.5 + i / 100, 0.25]}
    return {"chartok_coords": c, "edges": [[0, 1], [1, 0]], "edge_scores": [[0.9, 0.75 - i / 100], [0.75 - i / 100, 0.9]],
            "overall_score": 0.125, "id": i, "dtype": dtype}


def test_return_confidence_uses_the_grouped_prefetched_pipeline(monkeypatch):
    m = _facade(monkeypatch)
    calls = []
    # the real _prefetched: group g + 1 is transformed on a helper thread while the engine runs group g
    prefetched = M.molnextr._prefetched
    groups_seen = []

    def spy_prefetched(self, groups):
        groups_seen.append([list(g) for g in groups])
        return prefetched(self, groups)

    monkeypatch.setattr(M.molnextr, "_prefetched", spy_prefetched)

    def fake_pipeline(eng, x, tok, ref_batch_size=16, compute_confidence=False):
        calls.append((list(x), ref_batch_size, compute_confidence))
        return [_pred(i, eng.dtype) for i in x]

    monkeypatch.setattr(M, "predict_pipeline", fake_pipeline)
    out = m.predict_images(list(range(10)), return_atoms_bonds=True, return_confidence=True, batch_size=2)
    assert groups_seen == [[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]]
    assert calls == [([0, 1, 2, 3], 2, True), ([4, 5, 6, 7], 2, True), ([8, 9], 2, True)]
    assert len(out) == 10
    for i, o in enumerate(out):
        assert [a["confidence"] for a in o["atom_sets"]] == [0.5 + i / 100, 0.25]
        assert [(b["endpoints"], b["confidence"]) for b in o["bond_sets"]] == [((0, 1), 0.75 - i / 100)]
    # without confidences the call is the plain one (no compute_confidence keyword at all)
    calls.clear()
    monkeypatch.setattr(M, "predict_pipeline", lambda eng, x, tok, ref_batch_size=16: calls.append(list(x)) or
                        [_pred(i, eng.dtype) for i in x])
    out = m.predict_images(list(range(5)), return_atoms_bonds=True, batch_size=2)
    assert calls == [[0, 1, 2, 3], [4]] and all("confidence" not in a for o in out for a in o["atom_sets"])


def test_return_confidence_restarts_the_whole_call_on_a_range_error(monkeypatch):
    m = _facade(monkeypatch)
    seen = []

    def fake_pipeline(eng, x, tok, ref_batch_size=16, compute_confidence=False):
        assert compute_confidence and not eng.closed
        seen.append((eng.dtype, list(x)))
        if eng.dtype == "fp16x3" and 5 in x:
            raise MnxError("mnx_predict_confidence failed (-6)", code=MNX_ERR_RANGE)
        return [_pred(i, eng.dtype) for i in x]

    monkeypatch.setattr(M, "predict_pipeline", fake_pipeline)
    monkeypatch.setattr(M.molnextr, "_assemble", lambda self, preds, imgs, a, c: preds)
    with pytest.warns(RuntimeWarning, match="bf16x3"):
        out = m.predict_images(list(range(10)), return_atoms_bonds=True, return_confidence=True, batch_size=2)
    assert [p["id"] for p in out] == list(range(10)) and {p["dtype"] for p in out} == {"bf16x3"}
    assert seen == [("fp16x3", [0, 1, 2, 3]), ("fp16x3", [4, 5, 6, 7]),
                    ("bf16x3", [0, 1, 2, 3]), ("bf16x3", [4, 5, 6, 7]), ("bf16x3", [8, 9])]
    assert len(_StubEngine.built) == 2 and _StubEngine.built[0].closed
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.predict_images(list(range(3)), return_confidence=True, batch_size=2)     # the rebuilt engine serves silently


def test_pipeline_refuses_confidences_with_beam_search():
    with pytest.raises(NotImplementedError):
        M.predict_pipeline(None, None, beam_size=3, compute_confidence=True)
