"""GPU: predict from raw pages — the batched transform (mnx_preprocess_batch) and the encoder reading gray bytes
(mnx_encode_gray8 / mnx_predict_gray8). Nothing here may round differently from the fp32-image path, so every comparison
with that path is equality (np.array_equal / torch.equal); only the comparison with the CPU oracle carries the project's
feature bound."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from molnextr_amd import weights as W
from test_pages_host import golden_pages, ragged_pages

pytestmark = pytest.mark.gpu

TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    yield e
    e.close()


def _engine_fixed_ticks(synth_ckpt, **kw):
    """An engine whose decode ticks all run the bit-identical fused / mid forms (MNX_DEC_MID_MAX=4096), so that log-probs do
    not depend on the capacity the host happens to pick."""
    from molnextr_amd.engine import Engine
    old = os.environ.get("MNX_DEC_MID_MAX")
    os.environ["MNX_DEC_MID_MAX"] = "4096"
    try:
        return Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3", **kw)
    finally:
        if old is None:
            os.environ.pop("MNX_DEC_MID_MAX", None)
        else:
            os.environ["MNX_DEC_MID_MAX"] = old


def _ink_pages(n, seed=11):
    """n ragged pages with strokes (every one bears ink, sizes 40..400)."""
    rng = np.random.default_rng(seed)
    pages = []
    for _ in range(n):
        h, w = int(rng.integers(40, 400)), int(rng.integers(40, 400))
        img = np.full((h, w, 3), 255, np.uint8)
        for _ in range(int(rng.integers(4, 14))):
            y, x = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(1, max(2, h // 4)), rng.integers(1, max(2, w // 4))
            img[y:y + hh, x:x + ww] = rng.integers(0, 200, size=3, dtype=np.uint8)
        pages.append(img)
    return pages


@pytest.mark.parametrize("square", [False, True])
def test_batched_transform_equals_the_per_image_one_and_the_host(eng, square):
    from molnextr_amd.preprocess import transform_image, transform_image_gray
    pages = ragged_pages()
    ref32 = np.stack([transform_image(p, square=square) for p in pages])
    ref8 = np.stack([transform_image_gray(p, square=square) for p in pages])
    per_image = eng.preprocess(pages, pad_to_square=square).cpu().numpy()
    assert np.array_equal(per_image, ref32)
    b32 = eng.preprocess_batch(pages, pad_to_square=square, out="fp32").cpu().numpy()        # all pages in ONE call
    b8 = eng.preprocess_batch(pages, pad_to_square=square, out="gray8").cpu().numpy()
    assert b32.dtype == np.float32 and b8.dtype == np.uint8
    for i, p in enumerate(pages):
        assert np.array_equal(b32[i], per_image[i]), (i, p.shape)
        assert np.array_equal(b8[i], ref8[i]), (i, p.shape)
    order = np.random.default_rng(3).permutation(len(pages))
    s8 = eng.preprocess_batch([pages[i] for i in order], pad_to_square=square, out="gray8").cpu().numpy()
    s32 = eng.preprocess_batch([pages[i] for i in order], pad_to_square=square, out="fp32").cpu().numpy()
    assert np.array_equal(s8, ref8[order]) and np.array_equal(s32, ref32[order])
    for i in (0, 2, 4, 9):                                                                    # n = 1
        assert np.array_equal(eng.preprocess_batch([pages[i]], pad_to_square=square).cpu().numpy()[0], ref8[i])
    on_dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() if i % 2 else p for i, p in enumerate(pages)]
    assert np.array_equal(eng.preprocess_batch(on_dev, pad_to_square=square).cpu().numpy(), ref8)   # device-resident pages


def test_batched_crop_boxes_vs_reference_golden(eng):
    from molnextr_amd.preprocess import transform_image_gray
    cases, pages = golden_pages()
    for fmt in ("gray8", "fp32"):
        out, crops = eng.preprocess_batch(pages, return_crops=True, out=fmt)
        for c, crop in zip(cases, crops.cpu().numpy()):
            assert crop.tolist() == c["crop"], (fmt, c["case"], crop.tolist(), c["crop"])
    out, _ = eng.preprocess_batch(pages, return_crops=True)
    sq = eng.preprocess_batch(pages, pad_to_square=True).cpu().numpy()
    for c, page in zip(cases, pages):
        assert np.array_equal(out[c["case"]].cpu().numpy(), transform_image_gray(page))
        assert np.array_equal(sq[c["case"]], transform_image_gray(page, square=True))


def test_more_pages_than_one_call_holds_are_chunked_and_the_raw_call_names_its_bound(eng, dev):
    from molnextr_amd.engine import PREP_MAX_PAGES, MnxPage, _ptr
    from molnextr_amd.preprocess import transform_image_gray
    base = [W.synthetic_page(c) for c in (1, 3, 8, 9, 11, 12, 13)] + _ink_pages(4, seed=5)
    want = torch.from_numpy(np.stack([transform_image_gray(p) for p in base])).to(dev)
    n = PREP_MAX_PAGES + 1
    got = eng.preprocess_batch([base[i % len(base)] for i in range(n)])
    idx = torch.arange(n, device=dev) % len(base)
    same = (got == want[idx]).flatten(1).all(1)
    assert bool(same.all()), f"pages {torch.nonzero(~same).flatten()[:8].tolist()} differ from the host result"
    del got
    pages = (MnxPage * n)()
    for i in range(n):
        pages[i].offset, pages[i].height, pages[i].width = 0, 1, 1
    table = torch.frombuffer(bytearray(pages), dtype=torch.uint8).to(dev)
    arena = torch.full((16,), 255, dtype=torch.uint8, device=dev)
    out = torch.empty(16, dtype=torch.uint8, device=dev)          # never written: the call must refuse before it launches
    rc = eng.lib.mnx_preprocess_batch(eng.h, _ptr(arena), _ptr(table), n, 1, 50, 0, None, _ptr(out), 1, None)
    msg = eng.lib.mnx_last_error(eng.h).decode()
    assert rc == -5 and "MNX_PREP_MAX_PAGES" in msg and str(PREP_MAX_PAGES) in msg, (rc, msg)
    rc = eng.lib.mnx_preprocess_batch(eng.h, _ptr(arena), _ptr(table), 1, 1, 50, 0, None, _ptr(out), 7, None)
    assert rc == -1 and "out_format" in eng.lib.mnx_last_error(eng.h).decode()
    rc = eng.lib.mnx_preprocess_batch(eng.h, ctypes.c_void_p(arena.data_ptr() + 4), _ptr(table), 1, 1, 50, 0, None, _ptr(out), 1, None)
    assert rc == -1 and "aligned" in eng.lib.mnx_last_error(eng.h).decode()


def test_arena_addresses_beyond_4_gib(eng, dev):
    """One page at offset 0 and one above 2^32 of a 4 GiB + 64 MiB arena allocated on the device: 32-bit offsets would read
    the wrong page."""
    from molnextr_amd.engine import MnxPage, _ptr
    from molnextr_amd.preprocess import transform_image_gray
    size = (4 << 30) + (64 << 20)
    try:
        arena = torch.empty(size, dtype=torch.uint8, device=dev)
    except (RuntimeError, torch.OutOfMemoryError) as e:
        pytest.skip(f"the device refused a {size} byte allocation: {e}")
    lo, hi = W.synthetic_page(0), W.synthetic_page(5)
    off_hi = (4 << 30) + (32 << 20) + 16
    pages = (MnxPage * 2)()
    pages[0].offset, pages[0].height, pages[0].width = off_hi, hi.shape[0], hi.shape[1]
    pages[1].offset, pages[1].height, pages[1].width = 0, lo.shape[0], lo.shape[1]
    # what a 32-bit offset would alias to holds another page, so that a truncated address cannot pass by luck
    arena[off_hi - (4 << 30):off_hi - (4 << 30) + hi.size] = 255
    arena[off_hi:off_hi + hi.size].copy_(torch.from_numpy(hi.reshape(-1)).to(dev))
    arena[:lo.size].copy_(torch.from_numpy(lo.reshape(-1)).to(dev))
    table = torch.frombuffer(bytearray(pages), dtype=torch.uint8).to(dev)
    out = torch.empty(2, 384, 384, dtype=torch.uint8, device=dev)
    crops = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    rc = eng.lib.mnx_preprocess_batch(eng.h, _ptr(arena), _ptr(table), 2, max(hi.shape[0], lo.shape[0]), 50, 0, _ptr(crops),
                                      _ptr(out), 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.mnx_last_error(eng.h).decode()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), transform_image_gray(hi))
    assert np.array_equal(out[1].cpu().numpy(), transform_image_gray(lo))


def _gray_and_fp32(n, S, dev, seed):
    """n random gray-byte images (white page statistics do not matter to equality) and their normalised fp32 form."""
    from molnextr_amd.preprocess import normalise_gray
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, size=(n, S, S), dtype=np.uint8)
    g[:, : S // 2][g[:, : S // 2] < 200] = 255                        # half a page of mostly white
    x = np.stack([normalise_gray(a) for a in g])
    return torch.from_numpy(g).to(dev), torch.from_numpy(x).to(dev)


@pytest.mark.parametrize("B", [1, 2, 32])
def test_encoder_on_gray_bytes_equals_the_encoder_on_their_fp32_image(eng, dev, B):
    g, x = _gray_and_fp32(B, 384, dev, seed=B)
    tap_g = torch.zeros(B, 96 * 96, 128, device=dev)
    tap_x = torch.zeros_like(tap_g)
    eng.set_tap(0, tap_g)
    fg = eng.encode(g)
    eng.set_tap(0, tap_x)
    fx = eng.encode(x)
    eng.set_tap(-1, None)
    torch.cuda.synchronize()
    assert torch.equal(tap_g, tap_x), f"patch embedding differs: {(tap_g - tap_x).abs().max().item()}"
    assert torch.equal(fg, fx)
    assert torch.isfinite(fg).all()


@pytest.mark.parametrize("dtype", ["fp16x3", "fp32"])
def test_tiny_encoder_on_gray_bytes_equals_fp32_input(dev, dtype):
    from molnextr_amd.engine import Engine
    dec = W.DecoderDims(enc_dim=TINY.num_features)
    ck = W.synthetic_checkpoint(0, enc=TINY, dec=dec)
    e = Engine(ck["encoder"], ck["decoder"], max_batch=2, enc=TINY, dec=dec, dtype=dtype)
    try:
        for B in (1, 2):
            g, x = _gray_and_fp32(B, 96, dev, seed=20 + B)
            tap_g = torch.zeros(B, 24 * 24, 32, device=dev)
            tap_x = torch.zeros_like(tap_g)
            e.set_tap(0, tap_g)
            fg = e.encode(g)
            e.set_tap(0, tap_x)
            fx = e.encode(x)
            e.set_tap(-1, None)
            torch.cuda.synchronize()
            assert torch.equal(tap_g, tap_x) and torch.equal(fg, fx), (dtype, B)
    finally:
        e.close()


def _assert_same_predictions(a, b, conf):
    la = a["lengths"].cpu().numpy()
    assert np.array_equal(la, b["lengths"].cpu().numpy())
    na = a["n_atoms"].cpu().numpy()
    assert np.array_equal(na, b["n_atoms"].cpu().numpy())
    ta, tb = a["tokens"].cpu().numpy(), b["tokens"].cpu().numpy()
    ia, ib = a["atom_idx"].cpu().numpy(), b["atom_idx"].cpu().numpy()
    ea, eb = a["edges"].cpu().numpy(), b["edges"].cpu().numpy()
    for r in range(len(la)):
        k = int(na[r])
        assert np.array_equal(ta[r, :la[r]], tb[r, :la[r]]), r
        assert np.array_equal(ia[r, :k], ib[r, :k]) and np.array_equal(ea[r, :k, :k], eb[r, :k, :k]), r
    if conf:
        lpa, lpb = a["token_logp"].cpu().numpy(), b["token_logp"].cpu().numpy()
        sa, sb = a["atom_scores"].cpu().numpy(), b["atom_scores"].cpu().numpy()
        xa, xb = a["edge_scores"].cpu().numpy(), b["edge_scores"].cpu().numpy()
        assert np.array_equal(a["overall_score"].cpu().numpy(), b["overall_score"].cpu().numpy())
        for r in range(len(la)):
            k = int(na[r])
            assert np.array_equal(lpa[r, :la[r]], lpb[r, :la[r]]), r
            assert np.array_equal(sa[r, :k], sb[r, :k]) and np.array_equal(xa[r, :k, :k], xb[r, :k, :k]), r


@pytest.mark.parametrize("ref_batch", [4, 32])
def test_predict_on_gray_bytes_equals_predict_on_fp32_images(eng, dev, synth_ckpt, ref_batch):
    pages = _ink_pages(72, seed=ref_batch)                       # max_batch 32: three encoder launch groups (32 + 32 + 8)
    g = eng.preprocess_batch(pages, out="gray8")
    x = eng.preprocess_batch(pages, out="fp32")
    # tokens / atoms / bonds in the default configuration
    _assert_same_predictions(eng.predict(g, ref_batch=ref_batch, max_len=96), eng.predict(x, ref_batch=ref_batch, max_len=96),
                             conf=False)
    # log-probs and scores under the bit-identical tick arithmetic
    e = _engine_fixed_ticks(synth_ckpt)
    try:
        _assert_same_predictions(e.predict(g, ref_batch=ref_batch, max_len=96, confidence=True),
                                 e.predict(x, ref_batch=ref_batch, max_len=96, confidence=True), conf=True)
        _assert_same_predictions(e.predict(g, ref_batch=ref_batch, max_len=96), e.predict(x, ref_batch=ref_batch, max_len=96),
                                 conf=False)
    finally:
        e.close()


def test_pages_to_molecules_vs_the_cpu_oracle(eng, dev, synth_ckpt):
    """One reference batch of 8 ink-bearing pages: host transform_image -> CPU oracle (encoder, greedy decode, bond head)
    against device preprocess_batch(gray8) -> predict. Tokens / atoms / bonds equal, features within the 1e-4 of
    tests/test_gpu_pixels.py::test_default_mode_on_images_beyond_the_fixtures_vs_the_oracle."""
    from molnextr_amd.preprocess import transform_image
    from molnextr_amd.tokenizer import get_tokenizer
    from oracle.decoder import greedy_decode
    from oracle.edges import predict_edges
    from oracle.swin import encoder_forward
    pages = [W.synthetic_page(c) for c in (0, 1, 4, 5, 6, 7, 11, 14)]
    img = torch.from_numpy(np.stack([transform_image(p) for p in pages]))
    ref_f = encoder_forward(img, synth_ckpt["encoder"])
    ref = greedy_decode(ref_f, synth_ckpt["decoder"])
    g = eng.preprocess_batch(pages, out="gray8")
    feats = eng.encode(g)
    ferr = (feats.cpu() - ref_f).abs().max().item()
    print(f"feature max|err| vs oracle: {ferr:.3e}")
    assert ferr < 1e-4, ferr
    out = eng.predict(g, ref_batch=8)
    lens, toks = out["lengths"].cpu().numpy(), out["tokens"].cpu().numpy()
    n_atoms, atom_idx, edges = out["n_atoms"].cpu().numpy(), out["atom_idx"].cpu().numpy(), out["edges"].cpu().numpy()
    tok = get_tokenizer()["chartok_coords"]
    for r in range(len(pages)):
        assert toks[r, :lens[r]].tolist() == ref.tokens[r], f"row {r}: tokens differ from the oracle's"
        d = tok.sequence_to_smiles(ref.tokens[r])
        k = len(d["indices"])
        assert int(n_atoms[r]) == k and atom_idx[r, :k].tolist() == list(d["indices"]), r
        e_ref, _ = predict_edges(ref.hidden[r], d["indices"], synth_ckpt["decoder"])
        assert np.array_equal(edges[r, :k, :k], e_ref), f"row {r}: bond classes differ from the oracle's"


def test_facade_in_gray8_format_equals_the_fp32_facade(dev):
    from molnextr_amd.model import molnextr
    pages = [W.synthetic_page(c) for c in range(11)] + [np.full((90, 130, 3), 255, np.uint8)]
    for i, p in enumerate(pages[-1:]):
        p[30:60, 20 + i:100] = 0
    outs = {}
    for fmt in ("fp32", "gray8"):
        m = molnextr("synthetic", dev, max_batch=8, image_format=fmt)
        try:
            assert m.engine.image_format == fmt
            m.group_images = 4                                   # 3 engine calls, the prefetch helper active
            outs[fmt] = m.predict_images(pages, return_atoms_bonds=True, return_confidence=True, batch_size=4)
        finally:
            m.engine.close()
    assert len(outs["fp32"]) == 12 and outs["fp32"] == outs["gray8"]
    m = molnextr("synthetic", dev, max_batch=8, image_format="gray8", device_preprocess=False)
    try:
        m.group_images = 4
        assert m.predict_images(pages, return_atoms_bonds=True, return_confidence=True, batch_size=4) == outs["fp32"]
    finally:
        m.engine.close()


def test_beam_search_refuses_gray_bytes(eng, dev):
    g = torch.full((2, 384, 384), 255, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="beam search takes fp32 images"):
        eng.predict(g, ref_batch=2, beam=2)
