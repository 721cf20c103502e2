"""CPU: reference batches of more than 32 rows through the host layers (model facade, evaluation harness), with stub engines.

The reference numbers positional-encoding rows inside the whole batch, so the batches handed to the engine must be exactly
the caller's: 64 rows for predict_images(batch_size=64) and for the evaluation at --batch_size 32 (main.py:445 loads
batch_size * 2), up to 512."""
import numpy as np
import pytest
import torch

from molnextr_amd import evaluate as E
from molnextr_amd import model as M


class _StubEngine:
    built = []

    def __init__(self, enc, dec, device=0, max_batch=32, dtype="fp16x3", **kw):
        self.dtype, self.device, self.max_batch, self.closed = dtype, device, max_batch, False
        _StubEngine.built.append(self)

    def close(self):
        self.closed = True


def _facade(monkeypatch, seen):
    monkeypatch.setattr(M, "Engine", _StubEngine)
    _StubEngine.built = []
    m = M.molnextr.__new__(M.molnextr)
    m._states, m._max_batch = {"encoder": {}, "decoder": {}}, 32
    m.engine = _StubEngine({}, {}, device=2, max_batch=32, dtype="bf16x3")
    m.group_images, m.tokenizer, m.device_preprocess = 1024, None, False

    def fake_pipeline(eng, x, tok, ref_batch_size=16):
        assert not eng.closed
        seen.append((eng, list(x), ref_batch_size))
        return [{"id": i} for i in x]

    monkeypatch.setattr(M, "predict_pipeline", fake_pipeline)
    monkeypatch.setattr(M.molnextr, "_prefetched", lambda self, groups: iter(groups))
    monkeypatch.setattr(M.molnextr, "_assemble", lambda self, preds, imgs, a, c: preds)
    return m


def test_predict_images_hands_64_row_batches_and_grows_the_engine_once(monkeypatch):
    seen = []
    m = _facade(monkeypatch, seen)
    first = m.engine
    out = m.predict_images(list(range(150)), batch_size=64)
    assert [p["id"] for p in out] == list(range(150))
    assert [(len(x), rb) for _, x, rb in seen] == [(150, 64)]          # one engine call, reference batches of 64 inside it
    assert first.closed and len(_StubEngine.built) == 2
    eng = m.engine
    assert eng.max_batch >= 64 and eng.max_batch % 32 == 0 and eng.dtype == "bf16x3" and eng.device == 2
    m.predict_images(list(range(70)), batch_size=40)                  # fits the grown engine: no second rebuild
    assert len(_StubEngine.built) == 2 and seen[-1][0] is eng and seen[-1][2] == 40
    m.predict_images(list(range(600)), batch_size=512)
    assert len(_StubEngine.built) == 3 and m.engine.max_batch == 512 and seen[-1][2] == 512
    with pytest.raises(ValueError, match="1..512"):
        m.predict_images(list(range(600)), batch_size=513)


def test_predict_pipeline_and_decode_batch_keep_32_where_they_must():
    with pytest.raises(ValueError, match="beam search takes reference batches of at most 32"):
        M.predict_pipeline(None, torch.zeros(40, 3, 8, 8), ref_batch_size=40, beam_size=5)
    with pytest.raises(ValueError, match="predict_pipeline"):
        M.decode_batch(None, torch.zeros(40, 144, 1024), ref_batch_size=40)


class _BigBatchEngine:
    """Stub of the engine's greedy predict with reference batches up to MAX_REF_BATCH rows: records the batches."""
    ROWS_PER_DECODE = 32
    MAX_REF_BATCH = 512
    max_atoms = 8
    torch_device = torch.device("cpu")

    def __init__(self):
        self.batches = []

    def preprocess(self, images, pad_to_square=False):
        return torch.tensor([int(im[0, 0, 0]) * 256 + int(im[0, 0, 1]) for im in images], dtype=torch.int32)

    def predict(self, x, ref_batch=32, max_len=None):
        n = x.shape[0]
        self.batches += [x[i:i + ref_batch].tolist() for i in range(0, n, ref_batch)]
        tokens = torch.zeros(n, 480, dtype=torch.int32)
        tokens[:, 0] = 5 + x % 90
        tokens[:, 1] = 2
        return {"tokens": tokens, "lengths": torch.full((n,), 2, dtype=torch.int32),
                "n_atoms": torch.zeros(n, dtype=torch.int32), "atom_idx": torch.zeros(n, 8, dtype=torch.int32),
                "edges": torch.zeros(n, 8, 8, dtype=torch.uint8)}


def _page(i):
    p = np.zeros((2, 2, 3), np.uint8)
    p[0, 0, 0], p[0, 0, 1] = i // 256, i % 256
    return p


def test_run_inference_hands_64_row_batches_at_the_readme_configuration():
    """README: batch size 32 on one GPU -> the reference loads batches of 64 (main.py:445)."""
    eng = _BigBatchEngine()
    preds = E.run_inference(eng, _page, 150, batch_size=32)
    assert sorted(preds) == list(range(150))
    assert [len(b) for b in eng.batches] == [64, 64, 22]
    assert eng.batches == E.reference_batches(list(range(150)), batch_size=32)
    eng = _BigBatchEngine()
    E.run_inference(eng, _page, 600, batch_size=256)                 # main.py's default --batch_size
    assert [len(b) for b in eng.batches] == [512, 88]


def test_run_inference_refuses_batches_beyond_512():
    with pytest.raises(ValueError, match="batch_size <= 256"):
        E.run_inference(_BigBatchEngine(), _page, 600, batch_size=257)
    with pytest.raises(SystemExit):
        E.main(["--test_file", "x.csv", "--load_path", "synthetic", "--batch_size", "257"])
