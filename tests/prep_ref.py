"""A float64 statement of the page transform, independent of molnextr_amd.preprocess (numpy only):

  CropWhite(pad) [-> PadToSquare] -> Resize(S, S) -> ToGray -> Normalize(ImageNet)

as the operation that the fixed-point host / device arithmetic approximates: half-pixel-centre bilinear interpolation in
exact arithmetic on the cropped page behind its white border. The border is never built: `ref_rgb` samples a virtual
canvas through an index function that answers 255 outside the ink box, so a page of 8190 rows costs S^2 taps.
`canvas` does build it, for the tests that hand it to third-party code (tests/test_prep_ref_host.py anchors the resize on
torch.nn.functional.interpolate) and as a second, plainer statement of the geometry.

Also here: the seeded page cases that the host and the GPU tests share (`page_cases`, `box_cases`)."""
import functools
from typing import NamedTuple

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float64)       # IMAGENET_DEFAULT_MEAN / STD
STD = np.array([0.229, 0.224, 0.225], dtype=np.float64)
GRAY = np.array([0.299, 0.587, 0.114], dtype=np.float64)

# ---- the bounds of tests/test_prep_ref_host.py and tests/test_gpu_prep_ref.py (derived in the latter's docstring) -------
CHANNEL_BOUND = 1.38          # |resized channel byte - exact bilinear|
GRAY_BOUND = 2.0              # |gray byte - exact gray|
BIAS_WINDOW = (-0.30, 0.15)   # mean(gray byte - exact gray) over an image without white
NORM_BOUND_ULPS = 4.0         # |fp32 out - ref_normalised(gray byte)| <= 4 * 2^-24 * max(1, |ref|)
PADS = (50, 0)
SQUARES = (False, True)


# ---- geometry ------------------------------------------------------------------------------------------------------------
def ink_box(page: np.ndarray):
    """(top, bottom, left, right), half open: the bounding box of the pixels that differ from 255 in any channel; the whole
    page when it is blank."""
    h, w = page.shape[:2]
    ink = (page[..., :3] != 255).any(axis=2)
    rows, cols = np.flatnonzero(ink.any(axis=1)), np.flatnonzero(ink.any(axis=0))
    if rows.size == 0:
        return 0, h, 0, w
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def crop_params(page: np.ndarray):
    """[crop_top, crop_bottom, crop_left, crop_right]: the rows / columns dropped on each side of the page."""
    h, w = page.shape[:2]
    t, b, l, r = ink_box(page)
    return [t, h - b, l, w - r]


def canvas_geometry(page: np.ndarray, pad: int, square: bool):
    """(Hp, Wp, off_t, off_l): the size of the virtual canvas and where the ink box's first row / column lies in it. pad
    white pixels on every side; with square the shorter side grows to the longer, diff // 2 white first, the rest after."""
    t, b, l, r = ink_box(page)
    hp, wp, off_t, off_l = b - t + 2 * pad, r - l + 2 * pad, pad, pad
    if square:
        diff = abs(hp - wp)
        if hp <= wp:
            off_t, hp = off_t + diff // 2, wp
        else:
            off_l, wp = off_l + diff // 2, hp
    return hp, wp, off_t, off_l


def canvas(page: np.ndarray, pad: int, square: bool) -> np.ndarray:
    """The canvas, built: uint8 [Hp, Wp, 3]. For small cases only."""
    t, b, l, r = ink_box(page)
    hp, wp, off_t, off_l = canvas_geometry(page, pad, square)
    out = np.full((hp, wp, 3), 255, dtype=np.uint8)
    out[off_t:off_t + b - t, off_l:off_l + r - l] = page[t:b, l:r, :3]
    return out


# ---- resize / gray / normalise ----------------------------------------------------------------------------------------------
def axis_taps(n: int, S: int):
    """Half-pixel-centre sampling of an axis of n source pixels at S outputs: (tap, neighbour, fraction), float64."""
    f = np.clip((np.arange(S, dtype=np.float64) + 0.5) * n / S - 0.5, 0.0, n - 1.0)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), f - i0


def ref_rgb(page: np.ndarray, S: int, pad: int, square: bool) -> np.ndarray:
    """float64 [S, S, 3]: exact bilinear resize of the virtual canvas, per channel, before any rounding."""
    t, b, l, r = ink_box(page)
    hp, wp, off_t, off_l = canvas_geometry(page, pad, square)
    hc, wc = b - t, r - l

    def sample(yi, xi):                                   # canvas[yi[:, None], xi[None, :]] without a canvas
        y, x = yi - off_t, xi - off_l
        inside = ((y >= 0) & (y < hc))[:, None] & ((x >= 0) & (x < wc))[None, :]
        v = page[(t + np.clip(y, 0, hc - 1))[:, None], (l + np.clip(x, 0, wc - 1))[None, :], :3].astype(np.float64)
        return np.where(inside[..., None], v, 255.0)

    y0, y1, fy = axis_taps(hp, S)
    x0, x1, fx = axis_taps(wp, S)
    fy, fx = fy[:, None, None], fx[None, :, None]
    upper = (1.0 - fx) * sample(y0, x0) + fx * sample(y0, x1)
    lower = (1.0 - fx) * sample(y1, x0) + fx * sample(y1, x1)
    return (1.0 - fy) * upper + fy * lower


def to_gray(rgb: np.ndarray) -> np.ndarray:
    return np.asarray(rgb, dtype=np.float64) @ GRAY


def ref_gray(page: np.ndarray, S: int, pad: int, square: bool) -> np.ndarray:
    """float64 [S, S]: 0.299 R + 0.587 G + 0.114 B of the exact resize."""
    return to_gray(ref_rgb(page, S, pad, square))


def normalise(gray: np.ndarray) -> np.ndarray:
    """float64 [3, S, S]: (g / 255 - mean) / std of a gray image [S, S] (bytes or real)."""
    g = np.asarray(gray, dtype=np.float64)
    return (g[None] / 255.0 - MEAN[:, None, None]) / STD[:, None, None]


def ref_normalised(page: np.ndarray, S: int, pad: int, square: bool) -> np.ndarray:
    """float64 [3, S, S]: the whole transform without a rounding."""
    return normalise(ref_gray(page, S, pad, square))


def norm_bound(ref: np.ndarray) -> np.ndarray:
    return NORM_BOUND_ULPS * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


# ---- page cases ------------------------------------------------------------------------------------------------------------
NOISE_BOXES = ((1, 1), (1, 300), (300, 1), (17, 23), (284, 284), (668, 668), (257, 511), (1000, 90), (3000, 2200),
               (4100, 333), (8190, 40))


class Page(NamedTuple):
    name: str
    page: np.ndarray       # uint8 [H, W, 3]
    box: tuple             # (h, w) of the ink box for a noise page, None for a box-finder page


def noise_page(h: int, w: int, seed: int = 0) -> np.ndarray:
    """An h x w box of pixels uniform in 0..254 per channel (none is white: the ink box is the box exactly) inside a white
    margin of 0..5 pixels per side."""
    rng = np.random.default_rng([seed, h, w])
    mt, mb, ml, mr = (int(m) for m in rng.integers(0, 6, size=4))
    page = np.full((h + mt + mb, w + ml + mr, 3), 255, dtype=np.uint8)
    page[mt:mt + h, ml:ml + w] = rng.integers(0, 255, size=(h, w, 3), dtype=np.uint8)
    return page


@functools.lru_cache(maxsize=None)
def page_cases():
    """The noise pages, built once per process; treat them as read-only."""
    out = []
    for h, w in NOISE_BOXES:
        p = noise_page(h, w)
        p.setflags(write=False)
        out.append(Page(f"{h}x{w}", p, (h, w)))
    return tuple(out)


def canvas_pixels(case: Page, pad: int, square: bool) -> int:
    hp, wp = case.box[0] + 2 * pad, case.box[1] + 2 * pad
    return max(hp, wp) ** 2 if square else hp * wp


def is_bias_case(case: Page, pad: int, square: bool) -> bool:
    """No white dilutes the mean: pad 0, not squared, a box of 17 x 23 at least."""
    return pad == 0 and not square and case.box[0] >= 17 and case.box[1] >= 17


def _dots(h, w, dots, value=(0, 0, 0)):
    page = np.full((h, w, 3), 255, dtype=np.uint8)
    for y, x in dots:
        page[y, x] = value
    return page


WIDEST = 16384      # the widest / tallest page that mnx_preprocess and mnx_preprocess_batch admit


@functools.lru_cache(maxsize=None)
def box_cases():
    """White pages with single ink pixels where a box kernel can go wrong: at the seams of its 256-pixel stride, on the first
    and the last row, one grey level from white in one channel, pages narrower than a wave, one pixel wide or high, blank.
    'w70000' is wider than the library admits (WIDEST): the host finds its box, the device entry points must refuse it."""
    out = [Page(f"w1024_col{'_'.join(map(str, cols))}", _dots(3, 1024, [(1, c) for c in cols]), None)
           for cols in ((255,), (256,), (257,), (511, 512), (1023,), (0,))]
    out += [Page("w70000", _dots(2, 70000, [(1, 69999)]), None),
            Page("w16384", _dots(2, WIDEST, [(1, WIDEST - 1)]), None),
            Page("row_first", _dots(40, 50, [(0, 20)]), None),
            Page("row_last", _dots(40, 50, [(39, 20)]), None),
            Page("red_254", _dots(9, 11, [(4, 5)], (254, 255, 255)), None),
            Page("green_254", _dots(9, 11, [(4, 5)], (255, 254, 255)), None),
            Page("blue_254", _dots(9, 11, [(4, 5)], (255, 255, 254)), None),
            Page("w63", _dots(5, 63, [(2, 62)]), None),
            Page("w1", _dots(7, 1, [(3, 0)]), None),
            Page("h1", _dots(1, 9, [(0, 4)]), None),
            Page("blank", _dots(6, 10, []), None)]
    for c in out:
        c.page.setflags(write=False)
    return tuple(out)
