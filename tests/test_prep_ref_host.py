"""CPU: the host page transform (molnextr_amd/preprocess.py) against the float64 bilinear reference of tests/prep_ref.py.

The bounds (prep_ref.CHANNEL_BOUND 1.38, GRAY_BOUND 2.0, BIAS_WINDOW, NORM_BOUND_ULPS) are derived in the docstring of
tests/test_gpu_prep_ref.py, which holds the device to the same reference. Here:

  * the reference's resize is anchored on torch.nn.functional.interpolate (float64, bilinear, align_corners=False) to 1e-9,
    on the materialised canvas of every case whose canvas stays under 4 M pixels;
  * the host transform lies inside the bounds on every case, at pad 50 and 0, squared and not, at S = 384 and 96;
  * the bounds bite: every wrong variant of the transform listed in VARIANTS (one named mistake each, restated here in
    the host's own fixed point, `restated`) is at least ten bounds away on some case, and the two rounding mistakes, which no
    maximum could see, fall out of the bias window.

Measured with the host transform over all cases (printed by the tests): worst channel error 0.826 (S 384) / 0.783 (S 96),
worst gray error 1.191 / 1.146, bias on the cases without white -0.120 .. -0.130, normalised output 0.53 of its bound."""
import functools
from typing import NamedTuple

import numpy as np
import pytest
import torch

import prep_ref as R
from molnextr_amd import preprocess as P

SIZES = (384, 96)
ANCHOR_MAX_PIXELS = 4_000_000
COMBOS = [(pad, sq) for pad in R.PADS for sq in R.SQUARES]


def host_rgb_gray(page, S, pad, square):
    """The host transform up to ToGray at any pad, from the product's own steps (transform_image_gray fixes pad = 50 and is
    held equal to this in test_host_transform_within_the_bounds): (resized uint8 [S,S,3], gray uint8 [S,S])."""
    img = P.crop_white(np.ascontiguousarray(page[..., :3]), pad)
    if square:
        img = P.pad_to_square(img)
    rgb = P.resize_bilinear_u8(img, S)
    return rgb, np.ascontiguousarray(P.to_gray(rgb))


class Measured(NamedTuple):
    rgb: np.ndarray         # host, uint8 [S,S,3]
    gray: np.ndarray        # host, uint8 [S,S]
    ref_gray: np.ndarray    # float64 [S,S]
    channel_err: float      # max |rgb - ref_rgb|


@functools.lru_cache(maxsize=None)
def measured(ci, S, pad, square):
    """Host result and reference of page case ci, computed once per process and shared (read-only) by the tests here and in
    tests/test_gpu_prep_ref.py."""
    page = R.page_cases()[ci].page
    rgb, gray = host_rgb_gray(page, S, pad, square)
    ref = R.ref_rgb(page, S, pad, square)
    ref_gray = R.to_gray(ref)
    for a in (rgb, gray, ref_gray):
        a.setflags(write=False)
    return Measured(rgb, gray, ref_gray, float(np.abs(rgb - ref).max()))


def check_gray(gray, ref_gray, bias_case, what):
    """The 2.0 bound on every pixel and, on an image without white, the bias window. Returns (max error, mean error)."""
    d = gray.astype(np.float64) - ref_gray
    err, bias = float(np.abs(d).max()), float(d.mean())
    assert err <= R.GRAY_BOUND, (what, err)
    if bias_case:
        assert R.BIAS_WINDOW[0] <= bias <= R.BIAS_WINDOW[1], (what, bias)
    return err, bias


def check_normalised(out32, gray, what):
    """fp32 [3,S,S] against the float64 normalisation of its own gray byte. Returns the worst error in units of the bound."""
    ref = R.normalise(gray)
    q = float((np.abs(out32.astype(np.float64) - ref) / R.norm_bound(ref)).max())
    assert q <= 1.0, (what, q)
    return q


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_reference_resize_equals_torch_interpolate_on_the_built_canvas():
    worst, n = 0.0, 0
    for case in R.page_cases():
        for pad, sq in COMBOS:
            if R.canvas_pixels(case, pad, sq) >= ANCHOR_MAX_PIXELS:
                continue
            cv = R.canvas(case.page, pad, sq)
            assert cv.shape[0] * cv.shape[1] == R.canvas_pixels(case, pad, sq)
            x = torch.from_numpy(cv).permute(2, 0, 1)[None].double()
            for S in SIZES:
                want = torch.nn.functional.interpolate(x, size=(S, S), mode="bilinear", align_corners=False, antialias=False)
                err = float(np.abs(want[0].permute(1, 2, 0).numpy() - R.ref_rgb(case.page, S, pad, sq)).max())
                assert err <= 1e-9, (case.name, pad, sq, S, err)
                worst, n = max(worst, err), n + 1
    print(f"reference vs torch interpolate: {n} resizes, worst {worst:.2e}")
    big = {c.name for c in R.page_cases() if R.canvas_pixels(c, 0, False) >= ANCHOR_MAX_PIXELS}
    assert big == {"3000x2200"}, big                      # every other box is anchored at one combination at least


def test_reference_geometry_and_case_pages():
    for case in R.page_cases():
        h, w = case.box
        t, b, l, r = R.ink_box(case.page)
        assert (b - t, r - l) == (h, w), case.name
        assert max(R.crop_params(case.page)) <= 5 and not (case.page[t:b, l:r] == 255).all(axis=2).any(), case.name
    page = R.page_cases()[3].page                          # 17 x 23
    assert R.canvas_geometry(page, 50, False) == (117, 123, 50, 50)
    assert R.canvas_geometry(page, 50, True) == (123, 123, 53, 50)         # 6 // 2 white rows first
    assert R.canvas_geometry(R.page_cases()[1].page, 0, True) == (300, 300, 149, 0)      # 299 // 2 first, 150 after
    cv = R.canvas(R.page_cases()[1].page, 0, True)
    assert (cv[:149] == 255).all() and (cv[149] != 255).any(axis=1).all() and (cv[150:] == 255).all()
    blank = np.full((6, 10, 3), 255, np.uint8)
    assert R.ink_box(blank) == (0, 6, 0, 10) and R.crop_params(blank) == [0, 0, 0, 0]
    assert (R.ref_gray(blank, 8, 3, True) == 255.0).all()


def test_box_cases_on_the_host():
    names = [c.name for c in R.box_cases()]
    assert len(set(names)) == len(names)
    for c in R.box_cases():
        assert list(P.crop_box(c.page)) == R.crop_params(c.page), c.name
    by = {c.name: R.crop_params(c.page) for c in R.box_cases()}
    assert by["w1024_col511_512"] == [1, 1, 511, 511] and by["w70000"] == [1, 0, 69999, 0] and by["blank"] == [0, 0, 0, 0]
    assert by["row_first"] == [0, 39, 20, 29] and by["row_last"] == [39, 0, 20, 29] and by["green_254"] == [4, 4, 5, 5]


# ---- the host transform ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad,square", COMBOS)
def test_host_transform_within_the_bounds(pad, square):
    for S in SIZES:
        worst_c = worst_g = worst_n = 0.0
        biases = []
        for ci, case in enumerate(R.page_cases()):
            m = measured(ci, S, pad, square)
            what = (case.name, S, pad, square)
            assert m.channel_err <= R.CHANNEL_BOUND, (what, m.channel_err)
            bias_case = R.is_bias_case(case, pad, square)
            err, bias = check_gray(m.gray, m.ref_gray, bias_case, what)
            if bias_case:
                biases.append(bias)
            if pad == 50:                                 # the product's entry points
                out = P.transform_image(case.page, S, square)
                assert np.array_equal(out, P.normalise_gray(m.gray)), what
                if R.canvas_pixels(case, pad, square) < ANCHOR_MAX_PIXELS:
                    assert np.array_equal(P.transform_image_gray(case.page, S, square), m.gray), what
            else:
                out = P.normalise_gray(m.gray)
            assert out.dtype == np.float32 and out.shape == (3, S, S)
            worst_n = max(worst_n, check_normalised(out, m.gray, what))
            # and the whole transform against the whole reference: the gray bound carried through the normalisation
            full = R.normalise(m.ref_gray)
            slack = R.GRAY_BOUND / (255.0 * R.STD[:, None, None]) + R.norm_bound(full)
            assert (np.abs(out - full) <= slack).all(), what
            worst_c, worst_g = max(worst_c, m.channel_err), max(worst_g, err)
        print(f"host S {S} pad {pad} square {square}: channel {worst_c:.3f} gray {worst_g:.3f} normalised {worst_n:.2f} of "
              f"its bound, bias {min(biases, default=0):+.3f} .. {max(biases, default=0):+.3f} on {len(biases)} cases")
        assert len(biases) == (8 if pad == 0 and not square else 0)


@pytest.mark.parametrize("square", R.SQUARES)
def test_identity_resize_returns_the_canvas(square):
    ci = [c.name for c in R.page_cases()].index("284x284")
    page = R.page_cases()[ci].page
    cv = R.canvas(page, 50, square)
    assert cv.shape == (384, 384, 3)
    m = measured(ci, 384, 50, square)
    assert np.array_equal(m.rgb, cv) and np.array_equal(m.gray, P.to_gray(cv))
    assert m.channel_err == 0.0
    # the integer gray against 0.299 R + 0.587 G + 0.114 B: its rounding and the 14-bit coefficients, nothing else
    assert np.abs(m.gray - m.ref_gray).max() <= 0.5 + 255 * 5e-5


# ---- the bounds bite -------------------------------------------------------------------------------------------------------
STRUCTURAL = ("no_half_pixel", "align_corners", "weights_swapped", "nearest_tap", "pad_after_resize",
              "square_remainder_first", "square_wrong_axis", "crop_max_off_by_one", "bgr")
ROUNDING = ("no_plus_2", "no_plus_8192")
VARIANTS = STRUCTURAL + ("gray_before_resize",) + ROUNDING


def _taps(n, S, variant):
    """preprocess._linear_coeffs with the named mistake."""
    d = np.arange(S, dtype=np.float64)
    if variant == "no_half_pixel":
        fx = d * (n / S)
    elif variant == "align_corners":
        fx = d * ((n - 1) / (S - 1))
    else:
        fx = (d + 0.5) * (1.0 / (float(S) / float(n))) - 0.5
    fx = fx.astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    frac = (fx - sx.astype(np.float32)).astype(np.float32)
    frac[sx < 0] = 0.0
    sx[sx < 0] = 0
    over = sx >= n - 1
    frac[over] = 0.0
    sx[over] = n - 1
    w0 = np.rint((np.float32(1.0) - frac) * np.float32(2048.0)).astype(np.int64)
    w1 = np.rint(frac * np.float32(2048.0)).astype(np.int64)
    i1 = np.minimum(sx + 1, n - 1)
    if variant == "weights_swapped":
        w0, w1 = w1, w0
    if variant == "nearest_tap":
        sx, w0, w1 = np.where(w1 > w0, i1, sx), np.full_like(w0, 2048), np.zeros_like(w1)
    return sx, i1, w0, w1


def _resize(img, S, variant):
    """preprocess.resize_bilinear_u8 with the named mistake; gathers the S rows before it widens them."""
    h, w, _ = img.shape
    y0, y1, wy0, wy1 = _taps(h, S, variant)
    x0, x1, wx0, wx1 = _taps(w, S, variant)
    a, b = img[y0].astype(np.int64), img[y1].astype(np.int64)
    r0 = a[:, x0] * wx0[None, :, None] + a[:, x1] * wx1[None, :, None]
    r1 = b[:, x0] * wx0[None, :, None] + b[:, x1] * wx1[None, :, None]
    half = 0 if variant == "no_plus_2" else 2
    out = (((wy0[:, None, None] * (r0 >> 4)) >> 16) + ((wy1[:, None, None] * (r1 >> 4)) >> 16) + half) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def _gray(img, variant):
    c = (1868, 9617, 4899) if variant == "bgr" else (4899, 9617, 1868)
    half = 0 if variant == "no_plus_8192" else 8192
    x = img.astype(np.int64)
    return ((x[..., 0] * c[0] + x[..., 1] * c[1] + x[..., 2] * c[2] + half) >> 14).astype(np.uint8)


def _border(img, top, bottom, left, right):
    out = np.full((img.shape[0] + top + bottom, img.shape[1] + left + right, img.shape[2]), 255, np.uint8)
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out


def restated(page, S, pad, square, variant=None):
    """The host transform up to ToGray, restated with one named mistake (None: none, equal to the product bit for bit).
      no_half_pixel           f = d n / S                       align_corners      f = d (n - 1) / (S - 1)
      weights_swapped         the tap takes frac, the neighbour 1 - frac           nearest_tap   the heavier tap alone
      pad_after_resize        the crop is resized to S - 2 pad, the border comes last
      square_remainder_first  diff - diff // 2 white first     square_wrong_axis  the longer side grows
      crop_max_off_by_one     the box ends on its last ink row / column (exclusive)
      bgr                     0.114 R + 0.587 G + 0.299 B      gray_before_resize  ToGray, then Resize of one channel
      no_plus_2               (x) >> 2 for (x + 2) >> 2        no_plus_8192        the gray sum truncated"""
    t, b, l, r = R.ink_box(page)
    if variant == "crop_max_off_by_one":
        b, r = b - 1, r - 1
    img = page[t:b, l:r, :3]
    if variant == "pad_after_resize":
        h, w = img.shape[:2]
        if square and h != w:
            d = abs(h - w)
            img = _border(img, d // 2, d - d // 2, 0, 0) if h <= w else _border(img, 0, 0, d // 2, d - d // 2)
        return _gray(_border(_resize(img, S - 2 * pad, variant), pad, pad, pad, pad), variant)
    img = _border(img, pad, pad, pad, pad)
    if square:
        h, w = img.shape[:2]
        d = abs(h - w)
        p1, p2 = (d - d // 2, d // 2) if variant == "square_remainder_first" else (d // 2, d - d // 2)
        rows = (h > w) if variant == "square_wrong_axis" else (h <= w)
        img = _border(img, p1, p2, 0, 0) if rows else _border(img, 0, 0, p1, p2)
    if variant == "gray_before_resize":
        return _resize(_gray(img, variant)[..., None], S, variant)[..., 0]
    return _gray(_resize(img, S, variant), variant)


def _variant_cases(variant):
    """(case index, pad, square) on which a variant runs: built canvases under 4 M pixels; only where it can differ."""
    for ci, case in enumerate(R.page_cases()):
        for pad, sq in COMBOS:
            if R.canvas_pixels(case, pad, sq) >= ANCHOR_MAX_PIXELS:
                continue
            if variant == "pad_after_resize" and pad == 0:
                continue
            if variant.startswith("square") and not sq:
                continue
            if variant == "crop_max_off_by_one" and min(case.box) == 1:
                continue                                   # nothing would remain of the box
            yield ci, pad, sq


def test_restatement_without_a_mistake_is_the_host_transform():
    for ci, pad, sq in _variant_cases("none"):
        assert np.array_equal(restated(R.page_cases()[ci].page, 384, pad, sq), measured(ci, 384, pad, sq).gray), (ci, pad, sq)


@pytest.mark.parametrize("variant", STRUCTURAL)
def test_each_wrong_structural_variant_exceeds_the_bound_tenfold(variant):
    errs = {}
    for ci, pad, sq in _variant_cases(variant):
        g = restated(R.page_cases()[ci].page, 384, pad, sq, variant)
        e = float(np.abs(g - measured(ci, 384, pad, sq).ref_gray).max())
        name = R.page_cases()[ci].name
        errs[name] = max(errs.get(name, 0.0), e)
    print(f"{variant}: worst gray error per case {({k: round(v, 1) for k, v in errs.items()})}")
    assert max(errs.values()) >= 10 * R.GRAY_BOUND, (variant, errs)


def test_gray_before_resize_differs_by_rounding_only():
    """ToGray and Resize are both linear: which comes first shows in the roundings alone. The variant rounds the gray first
    (0.5 and the coefficients, 0.013) and then resizes one channel (prep_ref.CHANNEL_BOUND): 1.90, inside the gray bound."""
    worst = 0.0
    for ci, pad, sq in _variant_cases("gray_before_resize"):
        g = restated(R.page_cases()[ci].page, 384, pad, sq, "gray_before_resize")
        worst = max(worst, float(np.abs(g - measured(ci, 384, pad, sq).ref_gray).max()))
    print(f"gray_before_resize: worst gray error {worst:.3f}")
    assert worst <= R.GRAY_BOUND, worst


@pytest.mark.parametrize("variant", ROUNDING)
def test_each_wrong_rounding_variant_leaves_the_bias_window(variant):
    biases = {}
    for ci, case in enumerate(R.page_cases()):
        if not R.is_bias_case(case, 0, False) or R.canvas_pixels(case, 0, False) >= ANCHOR_MAX_PIXELS:
            continue
        for S in SIZES:
            ref = measured(ci, S, 0, False).ref_gray
            biases[(case.name, S)] = float((restated(case.page, S, 0, False, variant) - ref).mean())
    print(f"{variant}: bias {min(biases.values()):+.3f} .. {max(biases.values()):+.3f} on {len(biases)} images")
    assert len(biases) >= 12
    for k, v in biases.items():
        assert not (R.BIAS_WINDOW[0] <= v <= R.BIAS_WINDOW[1]), (variant, k, v)
