#!/usr/bin/env python3
"""Does the pages-in path pay? Times, on one GPU and in one process, the per-image transform against the batched one, the
facade from pages in both image formats, and the patch embedding on fp32 against gray input. Measurement only: nothing here
is part of the product path and no number is asserted.

    python tools/pages_time.py [--part a,b,c] [--pages 1024] [--facade-pages 2048] [--repeats 5] [--out profiles/pages_time.txt]

(a) transform alone, `--pages` pages of three sizes: Engine.preprocess (one mnx_preprocess per page) against
    preprocess_batch(out="fp32") and (out="gray8"); wall time per call (host + device, the call synchronises) and the device
    time between two events around it;
(b) predict_images from `--facade-pages` synthetic pages, batch_size 32, image_format fp32 against gray8: molecules / s;
(c) patch embedding per 512 images from mnx_profile_read (kind 3), fp32 against gray input.
The variants of a part alternate inside every repeat (A B A B ...), the table reports the median and the min .. max spread of
each, and the spread of the fp32 path against itself is the yardstick for "not slower".
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from molnextr_amd import weights as W  # noqa: E402
from molnextr_amd.engine import Engine  # noqa: E402


def stroke_pages(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = []
    for _ in range(16):          # 16 distinct pages, repeated: page content does not change the work
        img = np.full((h, w, 3), 255, np.uint8)
        for _ in range(12):
            y, x = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(1, max(2, h // 4)), rng.integers(1, max(2, w // 4))
            img[y:y + hh, x:x + ww] = rng.integers(0, 200, size=3, dtype=np.uint8)
        base.append(img)
    return [base[i % 16] for i in range(n)]


def fmt(v):
    return f"{statistics.median(v):10.2f} [{min(v):9.2f} .. {max(v):9.2f}]"


def part_a(eng, n, repeats, lines):
    lines.append(f"(a) transform alone, {n} pages per call: pages/s by wall clock | device ms per call (events)   median [min .. max]")
    variants = (("preprocess loop", lambda p: eng.preprocess(p)),
                ("batch fp32", lambda p: eng.preprocess_batch(p, out="fp32")),
                ("batch gray8", lambda p: eng.preprocess_batch(p, out="gray8")))
    for (h, w) in ((300, 400), (1000, 1000), (1500, 2000)):
        pages = stroke_pages(n, h, w)
        rate = {k: [] for k, _ in variants}
        dev_ms = {k: [] for k, _ in variants}
        for k, f in variants:            # warm-up: allocator, staging buffer
            f(pages[:64])
        for _ in range(repeats):
            for k, f in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                out = f(pages)
                b.record()
                torch.cuda.synchronize()
                rate[k].append(n / (time.perf_counter() - t0))
                dev_ms[k].append(a.elapsed_time(b))
                del out
        for k, _ in variants:
            lines.append(f"  {h:5d} x {w:5d}  {k:16s} {fmt(rate[k])} pages/s | {fmt(dev_ms[k])} ms")


def part_b(n, repeats, lines):
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    pages = [W.synthetic_page(i % 15) for i in range(n)]
    lines.append(f"(b) predict_images from {n} synthetic pages, batch_size 32: molecules/s   median [min .. max]")
    ms = {f: molnextr("synthetic", dev, max_batch=32, image_format=f) for f in ("fp32", "gray8")}
    rate = {f: [] for f in ms}
    for f, m in ms.items():
        m.predict_images(pages[:256], batch_size=32)
    for _ in range(repeats):
        for f, m in ms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.predict_images(pages, batch_size=32)
            rate[f].append(n / (time.perf_counter() - t0))
    for f, m in ms.items():
        lines.append(f"  image_format {f:6s} {fmt(rate[f])} molecules/s")
        m.engine.close()


def part_c(eng, repeats, lines):
    from molnextr_amd.preprocess import normalise_gray
    dev = torch.device("cuda", eng.device)
    B = eng.max_batch
    g = np.random.default_rng(0).integers(0, 256, size=(B, 384, 384), dtype=np.uint8)
    x = torch.from_numpy(np.stack([normalise_gray(a) for a in g])).to(dev)
    g = torch.from_numpy(g).to(dev)
    ms = {"fp32": [], "gray8": []}
    for _ in range(3):
        eng.encode(x); eng.encode(g)
    for _ in range(repeats):
        for k, t in (("fp32", x), ("gray8", g)):
            eng.profile(1)
            for _ in range(4):
                eng.encode(t)
            t_ms, _, launches = eng.profile_read("patch_embed")
            eng.profile(0)
            ms[k].append(t_ms / launches * 512 / B)
    lines.append(f"(c) patch embedding, ms per 512 images (HIP events around the launch, {B} images per launch)   median [min .. max]")
    for k in ms:
        lines.append(f"  {k:6s} {fmt(ms[k])} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="a,b,c")
    ap.add_argument("--pages", type=int, default=1024)
    ap.add_argument("--facade-pages", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.part.split(",")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = [f"pages_time: commit {commit or 'unknown'} (+ working tree), {torch.cuda.get_device_name(0)}, repeats {args.repeats}"]
    ck = W.synthetic_checkpoint(0)
    if "a" in parts or "c" in parts:
        eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=32)
        if "a" in parts:
            part_a(eng, args.pages, args.repeats, lines)
        if "c" in parts:
            part_c(eng, args.repeats, lines)
        eng.close()
    if "b" in parts:
        part_b(args.facade_pages, args.repeats, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
