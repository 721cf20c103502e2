#!/usr/bin/env python3
"""Throughput of the confidence path against the plain path and the per-batch path it replaced (run on the GPU box).

    python tools/confidence_throughput.py [--images 640] [--ref-batch 32] [--max-batch 512] [--repeats 3] [--out FILE]

The same seeded synthetic images (weights.synthetic_images, first_index 0), reference batches of --ref-batch (BASELINE
config 2: batch 32), all resident in HBM, go through three paths:
  predict             mnx_predict: Engine.predict, then predict_pipeline's host part (detokenisation, lists)
  predict_confidence  mnx_predict_confidence: Engine.predict(confidence=True), then the host part with confidences
  per_batch           encode + decode_batch(compute_confidence=True), --max-batch images per encode (the confidence path of
                      molnextr.predict_images before it moved onto mnx_predict_confidence)
`molecules_per_s` is end to end, up to the per-image prediction dicts; `engine_molecules_per_s` (first two paths) is the
engine call alone, outputs complete on the device. The host part is the same Python work in all three paths (per_batch
interleaves it with its engine calls, so it has no engine-only figure). Each path is run once to warm up, then the paths
alternate for --repeats rounds; every time is host wall time around work that ends in a device synchronise, with a garbage
collection before (not inside) each timed window. Prints one JSON line per path (median, every repeat, spread =
(max - min) / median) and one line comparing the warm-up outputs: structure = smiles / symbols / indices / coords / bond
classes; confidences where the structures agree."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=640)
    ap.add_argument("--ref-batch", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from molnextr_amd import weights as W
    from molnextr_amd.engine import Engine
    from molnextr_amd.model import decode_batch, predict_pipeline

    if not torch.cuda.is_available():
        raise SystemExit("confidence_throughput.py measures the MI355X path: no HIP device visible")
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=args.max_batch)
    imgs = W.synthetic_images(args.images).to(dev)
    rb = args.ref_batch

    def per_batch(x):
        preds = []
        for i in range(0, x.shape[0], eng.max_batch):
            feats = eng.encode(x[i:i + eng.max_batch].contiguous())
            preds += decode_batch(eng, feats, ref_batch_size=rb, compute_confidence=True)
        return preds

    def engine_only(confidence):
        return lambda x: eng.predict(x, ref_batch=rb, confidence=confidence)

    def end_to_end(confidence):
        return lambda x: predict_pipeline(eng, x, ref_batch_size=rb, compute_confidence=confidence)

    paths = {"predict": (end_to_end(False), engine_only(False)),
             "predict_confidence": (end_to_end(True), engine_only(True)),
             "per_batch": (per_batch, None)}
    outputs = {name: fns[0](imgs) for name, fns in paths.items()}     # warm-up; these outputs are compared below
    for name, fns in paths.items():
        if fns[1] is not None:
            fns[1](imgs)
    times = {(name, level): [] for name, fns in paths.items() for level in (0, 1) if fns[level] is not None}

    def timed(fn):
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(imgs)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        del r
        return t

    for _ in range(args.repeats):
        for name, fns in paths.items():
            for level in (0, 1):
                if fns[level] is not None:
                    times[(name, level)].append(timed(fns[level]))

    def summary(ts):
        rates = [args.images / t for t in ts]
        med = statistics.median(rates)
        return round(med, 1), [round(r, 1) for r in rates], round((max(rates) - min(rates)) / med, 4)

    lines, rate, eng_rate = [], {}, {}
    for name, fns in paths.items():
        med, reps, spread = summary(times[(name, 0)])
        ln = {"run": name, "images": args.images, "ref_batch": rb, "max_batch": args.max_batch,
              "molecules_per_s": med, "repeats_molecules_per_s": reps, "spread": spread}
        rate[name] = med
        if fns[1] is not None:
            med, reps, spread = summary(times[(name, 1)])
            ln.update(engine_molecules_per_s=med, engine_repeats_molecules_per_s=reps, engine_spread=spread)
            eng_rate[name] = med
        lines.append(ln)

    FIELDS = ("smiles", "symbols", "indices", "coords", "edges")

    def structure(p):
        c = p["chartok_coords"]
        return c["smiles"], c["symbols"], c["indices"], c["coords"], p["edges"]

    a, c, b = outputs["predict"], outputs["predict_confidence"], outputs["per_batch"]
    atom_rel = edge_abs = overall_rel = 0.0
    for pc, pb in zip(c, b):
        if structure(pc) != structure(pb):
            continue
        sa, sb = np.array(pc["chartok_coords"]["atom_scores"]), np.array(pb["chartok_coords"]["atom_scores"])
        if sa.size:
            atom_rel = max(atom_rel, float(np.max(np.abs(sa - sb) / np.abs(sb))))
            edge_abs = max(edge_abs, float(np.max(np.abs(np.array(pc["edge_scores"]) - np.array(pb["edge_scores"])))))
        if pb["overall_score"] > 0:
            overall_rel = max(overall_rel, abs(pc["overall_score"] - pb["overall_score"]) / pb["overall_score"])
    lines.append({"run": "comparison", "images": args.images,
                  "confidence_vs_plain_rate": round(rate["predict_confidence"] / rate["predict"], 4),
                  "confidence_vs_plain_engine_rate": round(eng_rate["predict_confidence"] / eng_rate["predict"], 4),
                  "confidence_vs_per_batch_rate": round(rate["predict_confidence"] / rate["per_batch"], 3),
                  "plain_vs_confidence_structure_mismatches": sum(structure(p) != structure(q) for p, q in zip(a, c)),
                  "confidence_vs_per_batch_structure_mismatches": sum(structure(p) != structure(q) for p, q in zip(c, b)),
                  "plain_vs_per_batch_structure_mismatches": sum(structure(p) != structure(q) for p, q in zip(a, b)),
                  "confidence_vs_per_batch_mismatched_fields": sorted({f for p, q in zip(c, b)
                                                                       for f, u, v in zip(FIELDS, structure(p), structure(q))
                                                                       if u != v}),
                  "atom_scores_max_rel": atom_rel, "edge_scores_max_abs": edge_abs, "overall_score_max_rel": overall_rel})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
