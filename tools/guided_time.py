#!/usr/bin/env python3
"""Molecules/s of predict_coords-shaped work (label-guided decoding, mnx_predict_guided) next to free prediction on the same
images: N synthetic images, reference batches of RB rows; the labels are the images' own free predictions with every
coordinate masked again, so both jobs decode sequences of the same lengths. Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from molnextr_amd import weights as W  # noqa: E402
from molnextr_amd.engine import Engine  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
RB = int(sys.argv[2]) if len(sys.argv) > 2 else 32
ck = W.synthetic_checkpoint(0)
eng = Engine(ck["encoder"], ck["decoder"], max_batch=64)
x = W.synthetic_images(N).cuda()
free = eng.predict(x, ref_batch=RB)
toks, lens = free["tokens"].cpu().numpy(), free["lengths"].cpu().numpy()
x0 = eng.dec.vocab - 128                   # first coordinate bin (64 x-bins, 64 y-bins close the vocabulary)
lab = np.zeros((N, int(lens.max()) + 1), np.int32)
lab[:, 0] = 1
for r, n in enumerate(lens):
    row = toks[r, :n].copy()
    row[row >= x0] = 4                       # every coordinate bin back to '<mask>'
    lab[r, 1:1 + n] = row
lab = torch.from_numpy(lab).cuda()
res = {"images": N, "ref_batch": RB, "mean_len": float(lens.mean())}
for name, fn in (("free", lambda: eng.predict(x, ref_batch=RB)),
                 ("guided", lambda: eng.predict(x, ref_batch=RB, labels=lab, free_run=True))):
    fn()
    best = 1e9
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    res[f"{name}_molecules_per_s"] = round(N / best, 1)
print(json.dumps(res))
eng.close()
