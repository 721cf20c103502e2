"""GPU (-m gpu): the device page transform (csrc/preprocess.hip, prep_resize_body.inc) against the float64 bilinear reference
of tests/prep_ref.py, through both entry points (mnx_preprocess: prep_bbox_kernel + prep_resize_kernel; mnx_preprocess_batch:
the (row, page) box grid + prep_resize_batch_kernel, gray bytes and fp32), at pad 50 and 0, squared and not.

The other tests of the transform hold the device equal to the host restatement; what the two share (tap position, weight
pair, border clamp, gray coefficients, the order of pad and resize) is held here to the operation itself: half-pixel-centre
bilinear interpolation in exact arithmetic, prep_ref.ref_rgb, whose resize tests/test_prep_ref_host.py anchors on
torch.nn.functional.interpolate to 1e-9. The equality with the host is asserted here too, so that a failure tells "the
kernel differs from the host" from "both are wrong".

Bound, per channel: the byte v that the fixed-point resize writes against the exact value r, canvas up to 8290 a side.
  two weights, each rounded to 11 bits, horizontally      255 * 2 * 2^-12 = 0.1245
  the same vertically                                     0.1245
  the >> 4 of the horizontal sums                         2^-7
  the two >> 16 truncations, to quarter units             under 0.5 together
  the final (+ 2) >> 2                                    0.5
  fp32 tap coordinate (half an ulp at 2^13, slope 255)    0.0625 an axis, 0.125
  |v - r| <= 1.38                                         (prep_ref.CHANNEL_BOUND; the host exposes the channels)
Gray adds its own rounding, 0.5, and the 14-bit coefficients against 0.299 / 0.587 / 0.114, 255 * 5e-5: |gray - ref_gray|
<= 1.90; the tests use 2.0 grey levels (prep_ref.GRAY_BOUND).

Bias, on the images without white (pad 0, not squared, box of 17 x 23 at least): the mean of gray - ref_gray lies in
[-0.30, +0.15] (prep_ref.BIAS_WINDOW): the two quarter-unit truncations give at most -0.25, >> 4 gives -0.008, every other
term is symmetric. A dropped + 2 or + 8192 moves the mean by -0.5 and passes the maximum; test_prep_ref_host.py shows that
both leave the window (-0.62 .. -0.63) and that every structural mistake on its list is 20 grey levels away or more.

Normalised output: (float(g) - 255 mean) * (1 / (255 std)), two fp32 operations on fp32 constants: |out - ref| <= 4 * 2^-24 *
max(1, |ref|) against the float64 normalisation of the device's own gray byte.

Measured, host (test_prep_ref_host.py, S = 384 / 96): channel 0.826 / 0.783, gray 1.191 / 1.146, bias -0.120 .. -0.130,
normalised 0.53 of its bound. Measured on an MI355X (printed by these tests, S = 384): gray 1.191, bias -0.120 .. -0.128,
normalised 0.53 of its bound, every byte and every fp32 word equal to the host's; the device does not expose the channels.

The box cases (prep_ref.box_cases) compare crop parameters only, exactly: single ink pixels at the seams of the box kernels'
256-pixel stride, first / last row, one grey level from white in one channel, pages narrower than a wave, one pixel wide or
high, blank, the widest page the library admits; one batch call holds them all beside a 1-row page and the 8190-row page,
so that most (row, page) workgroups leave at once. A page of 70000 columns is wider than the library admits: both entry
points must refuse it before they launch."""
import time

import numpy as np
import pytest
import torch

import prep_ref as R
from test_prep_ref_host import COMBOS, check_gray, check_normalised, measured

pytestmark = pytest.mark.gpu

S = 384
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def eng(synth_ckpt):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from molnextr_amd.engine import Engine
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    assert e.enc.img_size == S and e.image_format == "fp32"
    t = time.perf_counter()
    yield e
    e.close()
    print(f"\ntest_gpu_prep_ref: {time.perf_counter() - t:.1f} s behind the engine, {time.perf_counter() - T0:.1f} s in all")


def _pages():
    return [c.page for c in R.page_cases()]


def _on_device(page):
    return torch.from_numpy(page.copy()).cuda()           # the case pages are read-only


def _gray_byte_of(out32):
    """The gray byte behind a normalised fp32 image, from channel 0 (a grey level is 0.017 there; check_normalised then
    holds all three channels to that byte within a few 1e-7)."""
    g = np.rint(out32[0].astype(np.float64) * (255.0 * R.STD[0]) + 255.0 * R.MEAN[0])
    assert g.min() >= 0 and g.max() <= 255
    return g.astype(np.uint8)


def _check_case(ci, pad, square, gray, out32, crop, entry):
    """One page case of one entry point: the reference first, then the host."""
    from molnextr_amd.preprocess import normalise_gray
    case = R.page_cases()[ci]
    what = (entry, case.name, pad, square)
    m = measured(ci, S, pad, square)
    assert list(crop) == R.crop_params(case.page), (what, list(crop))
    err, bias = check_gray(gray, m.ref_gray, R.is_bias_case(case, pad, square), what)
    q = check_normalised(out32, gray, what) if out32 is not None else 0.0
    assert np.array_equal(gray, m.gray), (what, "inside the bound, yet not the host's bytes")
    if out32 is not None:
        assert np.array_equal(out32, normalise_gray(m.gray)), what
    return err, bias, q


def _report(entry, pad, square, rows):
    biases = [b for (ci, (e, b, q)) in enumerate(rows) if R.is_bias_case(R.page_cases()[ci], pad, square)]
    print(f"device {entry} pad {pad} square {square}: gray {max(e for e, _, _ in rows):.3f} normalised "
          f"{max(q for _, _, q in rows):.2f} of its bound, bias {min(biases, default=0):+.3f} .. {max(biases, default=0):+.3f} "
          f"on {len(biases)} cases")


@pytest.mark.parametrize("pad,square", COMBOS)
def test_per_image_entry_vs_float64(eng, pad, square):
    out, crops = eng.preprocess(_pages(), pad=pad, pad_to_square=square, return_crops=True)
    out, crops = out.cpu().numpy(), crops.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (len(R.page_cases()), 3, S, S)
    rows = [_check_case(ci, pad, square, _gray_byte_of(out[ci]), out[ci], crops[ci], "preprocess")
            for ci in range(len(R.page_cases()))]
    _report("preprocess", pad, square, rows)


@pytest.mark.parametrize("pad,square", COMBOS)
def test_batch_entry_vs_float64(eng, pad, square):
    g8, c8 = eng.preprocess_batch(_pages(), pad=pad, pad_to_square=square, return_crops=True, out="gray8")
    f32, c32 = eng.preprocess_batch(_pages(), pad=pad, pad_to_square=square, return_crops=True, out="fp32")
    g8, c8, f32, c32 = g8.cpu().numpy(), c8.cpu().numpy(), f32.cpu().numpy(), c32.cpu().numpy()
    assert g8.dtype == np.uint8 and g8.shape == (len(R.page_cases()), S, S) and f32.dtype == np.float32
    rows = []
    for ci in range(len(R.page_cases())):
        _check_case(ci, pad, square, g8[ci], None, c8[ci], "batch gray8")
        assert np.array_equal(_gray_byte_of(f32[ci]), g8[ci]), (ci, pad, square)
        rows.append(_check_case(ci, pad, square, g8[ci], f32[ci], c32[ci], "batch fp32"))
    _report("preprocess_batch", pad, square, rows)


def test_pad_reaches_the_kernels(eng):
    """pad is a parameter of both entry points; the reference tests above run at pad 0 and would fail at the default. Said
    once more in the plainest way: a black page keeps no white at pad 0 and a white frame at pad 7."""
    black = np.zeros((20, 20, 3), np.uint8)
    for pad in (0, 7):
        a = eng.preprocess_batch([black], pad=pad).cpu().numpy()[0]
        b = _gray_byte_of(eng.preprocess([black], pad=pad).cpu().numpy()[0])
        assert np.array_equal(a, b)
        assert (a[S // 2, S // 2] == 0) and a[0, 0] == (0 if pad == 0 else 255), (pad, a[0, 0])
        assert np.abs(a - R.ref_gray(black, S, pad, False)).max() <= R.GRAY_BOUND


def _admitted_box_cases():
    return [c for c in R.box_cases() if max(c.page.shape[:2]) <= R.WIDEST]


def test_box_cases_per_image(eng):
    cases = _admitted_box_cases()
    _, crops = eng.preprocess([c.page for c in cases], return_crops=True)
    _, on_dev = eng.preprocess([_on_device(c.page) for c in cases], return_crops=True)
    for c, crop, crop_d in zip(cases, crops.cpu().numpy().tolist(), on_dev.cpu().numpy().tolist()):
        assert crop == R.crop_params(c.page), (c.name, crop)
        assert crop_d == R.crop_params(c.page), (c.name, "device-resident", crop_d)


def test_box_cases_in_one_batch_call_of_mixed_heights(eng):
    from molnextr_amd.preprocess import transform_image_gray
    cases = list(_admitted_box_cases())
    tall_ci = [c.name for c in R.page_cases()].index("8190x40")
    tall = R.page_cases()[tall_ci]
    one_row = R.Page("noise_1_row", np.ascontiguousarray(R.page_cases()[5].page[7:8]), None)      # a row of the 668 x 668 box
    assert one_row.page.shape[0] == 1 and any(c.page.shape[0] == 1 for c in cases)
    cases = cases[:5] + [tall] + cases[5:] + [one_row]
    pages = [c.page for c in cases]
    assert max(p.shape[0] for p in pages) >= 8190 and sorted(p.shape[0] for p in pages)[-2] <= 40
    want = [R.crop_params(p) for p in pages]
    for fmt in ("gray8", "fp32"):
        _, crops = eng.preprocess_batch(pages, return_crops=True, out=fmt)
        assert crops.cpu().numpy().tolist() == want, fmt
    on_dev = [_on_device(p) for p in pages]
    gray, crops = eng.preprocess_batch(on_dev, return_crops=True)
    assert crops.cpu().numpy().tolist() == want, "device-resident"
    mixed = [d if i % 2 else p for i, (d, p) in enumerate(zip(on_dev, pages))]
    gray_m, crops = eng.preprocess_batch(mixed, pad=0, pad_to_square=True, return_crops=True)
    assert crops.cpu().numpy().tolist() == want, "half of the pages device-resident, pad 0, square"
    gray = gray.cpu().numpy()
    for i, c in enumerate(cases):                          # the pixels behind those boxes: the host's
        assert np.array_equal(gray[i], transform_image_gray(c.page)), c.name
        assert np.abs(gray[i] - R.ref_gray(c.page, S, 50, False)).max() <= R.GRAY_BOUND, c.name
    assert np.array_equal(gray_m.cpu().numpy()[5], measured(tall_ci, S, 0, True).gray)


def test_a_page_wider_than_the_library_admits_is_refused(eng):
    from molnextr_amd.engine import MnxError
    wide = next(c for c in R.box_cases() if c.name == "w70000").page
    assert wide.shape[1] > R.WIDEST
    with pytest.raises(MnxError, match="larger than 16384x16384") as ei:
        eng.preprocess([wide])
    assert ei.value.code == -5
    with pytest.raises(ValueError, match="outside 1..16384"):
        eng.preprocess_batch([wide])
    # and the engine goes on working
    small = R.box_cases()[0].page
    _, crops = eng.preprocess_batch([small], return_crops=True)
    assert crops.cpu().numpy().tolist() == [R.crop_params(small)]
