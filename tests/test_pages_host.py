"""CPU: the pages-in path (batched transform, gray-byte encoder input) as far as it exists without a device — the host
restatement split into its gray byte and the normalisation, the new C ABI symbols and their argument refusals, and the
facade carrying `image_format` through restarts and the range-fallback rebuild with a stub engine. The device side is
tests/test_gpu_pages.py."""
import ctypes
import json
import os
import re
import warnings

import numpy as np
import pytest

from molnextr_amd import engine
from molnextr_amd import model as M
from molnextr_amd import weights as W
from molnextr_amd.engine import MNX_ERR_RANGE, MnxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged_pages():
    """The page recipe of tests/test_gpu_parity.py::test_device_preprocess_is_bit_identical_to_host_restatement: ragged
    sizes, 1x1, blank, noise, single-channel, ink in the corners."""
    rng = np.random.default_rng(7)
    pages = []
    for (h, w) in [(470, 923), (64, 64), (1, 1), (37, 911), (1500, 2000), (384, 384), (300, 17)]:
        img = np.full((h, w, 3), 255, np.uint8)
        for _ in range(12):       # random coloured strokes, some touching the page border
            y, x = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(1, max(2, h // 3)), rng.integers(1, max(2, w // 3))
            img[y:y + hh, x:x + ww] = rng.integers(0, 256, size=3, dtype=np.uint8)
        pages.append(img)
    pages.append(np.full((50, 70, 3), 255, np.uint8))                       # blank page: no crop, border only
    pages.append(rng.integers(0, 256, size=(200, 333, 3), dtype=np.uint8))  # noise: exercises every weight pair
    pages.append(rng.integers(0, 256, size=(90, 120), dtype=np.uint8))      # single-channel input
    edge = np.full((40, 40, 3), 255, np.uint8); edge[0, 0] = 0; edge[-1, -1] = 254
    pages.append(edge)
    return pages


def golden_pages():
    with open(os.path.join(ROOT, "tests", "golden", "crop_pad.json")) as f:
        cases = json.load(f)["cases"]
    return cases, [W.synthetic_page(c["case"]) for c in cases]


@pytest.mark.parametrize("square", [False, True])
def test_transform_image_is_the_normalised_gray_byte(square):
    from molnextr_amd.preprocess import normalise_gray, transform_image, transform_image_gray
    for p in ragged_pages() + golden_pages()[1]:
        g = transform_image_gray(p, square=square)
        assert g.dtype == np.uint8 and g.shape == (384, 384)
        x = normalise_gray(g)
        assert x.dtype == np.float32 and x.shape == (3, 384, 384)
        assert np.array_equal(x, transform_image(p, square=square)), p.shape


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return engine.load_library()


def test_header_declares_and_library_exports_the_pages_entry_points(lib):
    with open(os.path.join(ROOT, "include", "molnextr_hip.h")) as f:
        hdr = f.read()
    for name in ("mnx_preprocess_batch", "mnx_encode_gray8", "mnx_predict_gray8"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in engine.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"\}\s*mnx_page\s*;", hdr) and re.search(r"#define MNX_PREP_MAX_PAGES (\d+)", hdr)
    assert int(re.search(r"#define MNX_PREP_MAX_PAGES (\d+)", hdr).group(1)) == engine.PREP_MAX_PAGES >= 4096
    assert re.search(r"MNX_IMG_F32 = 0, MNX_IMG_GRAY8 = 1", hdr) and engine.IMAGE_FORMATS == {"fp32": 0, "gray8": 1}
    assert ctypes.sizeof(engine.MnxPage) == 16
    assert engine.MnxPage.offset.offset == 0 and engine.MnxPage.height.offset == 8 and engine.MnxPage.width.offset == 12
    assert lib.mnx_abi_version() == engine.ABI_VERSION == 7


def test_null_handle_is_refused_not_dereferenced(lib):
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mnx_preprocess_batch(None, p, p, 1, 1, 50, 0, None, p, 1, None) == -1
    assert lib.mnx_encode_gray8(None, p, 1, p, None) == -1
    assert lib.mnx_predict_gray8(None, p, 1, 1, 8, p, p, p, p, p, 4, None, None, None, None, None) == -1


class _StubEngine:
    """Records what the facade hands to predict; `preprocess` returns a tagged object, as Engine.preprocess returns the
    tensor of the engine's image format."""
    built = []

    def __init__(self, enc, dec, device=0, max_batch=32, dtype="fp16x3", image_format="fp32", **kw):
        self.dtype, self.device, self.max_batch, self.closed = dtype, device, max_batch, False
        self.image_format = image_format
        _StubEngine.built.append(self)

    def preprocess(self, images):
        return (self.image_format, id(self), list(images))

    def close(self):
        self.closed = True


def test_facade_hands_the_transform_result_to_predict_and_keeps_the_format_across_a_rebuild(monkeypatch):
    import contextlib
    monkeypatch.setattr(M, "Engine", _StubEngine)
    _StubEngine.built = []
    m = M.molnextr.__new__(M.molnextr)
    m._states, m._max_batch, m.image_format = {"encoder": {}, "decoder": {}}, 8, "gray8"
    m.engine = _StubEngine({}, {}, device=1, max_batch=8, dtype="fp16x3", image_format="gray8")
    m.group_images, m.tokenizer, m.device_preprocess = 2, None, True
    monkeypatch.setattr(M.molnextr, "_side_context", lambda self: contextlib.nullcontext())
    monkeypatch.setattr(M.molnextr, "_assemble", lambda self, preds, imgs, a, c: preds)
    seen = []

    def fake_pipeline(eng, x, tok, ref_batch_size=16):
        fmt, made_by, ids = x
        seen.append((eng.dtype, fmt, ids))
        assert fmt == "gray8" and eng.image_format == "gray8"       # what preprocess returned goes straight to predict
        if eng.dtype == "fp16x3" and 2 in ids:
            raise MnxError("mnx_predict_gray8 failed (-6)", code=MNX_ERR_RANGE)
        return [{"id": i, "dtype": eng.dtype} for i in ids]

    monkeypatch.setattr(M, "predict_pipeline", fake_pipeline)
    with pytest.warns(RuntimeWarning, match="bf16x3"):
        out = m.predict_images([0, 1, 2, 3, 4], batch_size=2)
    assert [p["id"] for p in out] == [0, 1, 2, 3, 4] and {p["dtype"] for p in out} == {"bf16x3"}
    assert seen == [("fp16x3", "gray8", [0, 1]), ("fp16x3", "gray8", [2, 3]), ("bf16x3", "gray8", [0, 1]),
                    ("bf16x3", "gray8", [2, 3]), ("bf16x3", "gray8", [4])]
    assert len(_StubEngine.built) == 2 and _StubEngine.built[0].closed
    assert m.engine.image_format == "gray8" and m.engine.dtype == "bf16x3" and m.engine.device == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m._rebuild_engine(max_batch=64)                                # growing the engine keeps the format too
    assert m.engine.image_format == "gray8" and m.engine.max_batch == 64


def test_host_transform_follows_the_format_when_the_device_transform_is_off():
    from molnextr_amd.preprocess import transform_image_gray
    import torch
    m = M.molnextr.__new__(M.molnextr)
    m.device_preprocess, m.input_size, m.device, m.image_format = False, 384, torch.device("cpu"), "gray8"
    page = W.synthetic_page(0)
    x = m._transform([page])
    assert x.dtype == torch.uint8 and tuple(x.shape) == (1, 384, 384)
    assert np.array_equal(x[0].numpy(), transform_image_gray(page))
    assert M.molnextr.image_format == "fp32"                            # the default stays fp32
