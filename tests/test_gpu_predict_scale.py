"""Greedy predict (continuous batching) on engines of more than 1024 slots: every output word of a job that fills every
tile equals what the engine's own lone per-chunk calls give.

What only these sizes reach (tests/predict_scale_ref.py builds the jobs):
  1088 slots  34 tiles: the second pass of dec_begin_kernel's 1024 threads, partial (s < slots); chunk tag 33; tick
              capacity 1088 = min(dec_slots, 1152)
  3072 slots  the benchmark's size: three passes, tags to 95, capacity steps of 128 and 256, self_k / self_v past 4 GiB
  4096 slots  MAX_SLOTS: four passes, tag 127, mem_kv past 4 GiB, every state array at its bound
and with them the gather, the atom scan, the bond head and the confidences reading slots >= 1024.

Two engine forms run ONE arithmetic at every tick capacity, so a crowded job must equal the lone calls bit for bit:
"tile0" (MNX_DEC_TILE=0) runs the eight-launches-per-layer tick of decoder.hip at every capacity — each output element of
dec_linear_kernel is a fixed chain per (row, column), dec_attn_kernel works per (slot, head), the heads per row: none of
them reads the row count —, the kernels of the benchmark's large ticks; "mid" (MNX_DEC_MID_MAX=4096) runs the fused tick up
to 128 rows and its bit-identical mid form beyond, which takes dec_fused.hip to high slots. The default mix of the two
arithmetics is not compared: its capacity follows poll timing, and the two differ by 1e-5.

The expectation comes from lone calls predict(pool batch, ref_batch=rb): one chunk in tile 0, a one-pass scan (asserted
from their trace). Each job's trace (MNX_TRACE, read per call) must show that the regime was reached: every tile live at
once, the scan at dec_slots, capacities that follow predict_impl's rule with the 128 and the 256 step both seen. These are
conditions on the inputs: if one fails, the inputs are to be fixed, not the assertion.

Measured on the MI355X (wall time per case, polls, largest `live`, the (scan, capacity) pairs):
profiles/predict_scale_gpu.json. One JSON line per case is printed, prefixed "predict_scale" (run with -s)."""
import json
import os
import time

import pytest
import torch

import predict_scale_ref as P
from molnextr_amd import weights as W

pytestmark = pytest.mark.gpu

FORMS = {"tile0": ("MNX_DEC_TILE", "0"), "mid": ("MNX_DEC_MID_MAX", "4096")}
CASES = [("tile0", 1088), ("mid", 1088), ("tile0", 3072), ("tile0", 4096), ("mid", 4096)]

_lone = {}          # (form, rb, pool batch, rows) -> result of the lone call (device tensors), shared by the cases of a form


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ckpt():
    return W.synthetic_checkpoint(0, enc=P.TINY, dec=P.DEC)


@pytest.fixture(scope="module")
def pool(dev):
    """The images of the 7 pool batches of 96; image i is a pure function of i, so [:7 * 32] is the pool of 7 batches of 32."""
    return W.synthetic_images(P.K * 96, size=96).to(dev)


def _engine(ckpt, form, dec_slots):
    from molnextr_amd.engine import Engine
    name, value = FORMS[form]
    old = os.environ.get(name)
    os.environ[name] = value            # read once, at mnx_create
    try:
        return Engine(ckpt["encoder"], ckpt["decoder"], device=0, max_batch=512, max_len=480, dtype="fp16x3", enc=P.TINY,
                      dec=P.DEC, dec_slots=dec_slots)
    finally:
        if old is None:
            os.environ.pop(name)
        else:
            os.environ[name] = old


def _traced_predict(eng, x, rb, path):
    """predict(confidence=True) with its MNX_TRACE lines: (result, polls, wall seconds)."""
    if os.path.exists(path):
        os.remove(path)
    os.environ["MNX_TRACE"] = path       # read per call
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.predict(x, ref_batch=rb, confidence=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        os.environ.pop("MNX_TRACE")
    with open(path) as f:
        polls, ends = P.parse_trace(f.read())
    assert len(ends) == 1 and polls, "one predict call leaves its poll lines and one end line"
    return out, polls, wall


def _lone_results(eng, form, pool, n_img, rb, path):
    """The lone calls a job's expectation needs, made on `eng` unless an earlier case of the form made them. A lone call must
    have run in the small regime: one chunk, a one-pass scan, the capacity of its own rows."""
    lone = {}
    for batch, rows in P.lone_calls(n_img, rb):
        key = (form, rb, batch, rows)
        if key not in _lone:
            x = pool[batch * rb:batch * rb + rows].contiguous()
            out, polls, _ = _traced_predict(eng, x, rb, path)
            assert {p["scan"] for p in polls} == {1024}, (key, sorted({p["scan"] for p in polls}))
            assert max(p["rows_cap"] for p in polls) == (rows + 63) // 64 * 64 and max(p["live"] for p in polls) == 1, key
            _lone[key] = out
        lone[batch, rows] = _lone[key]
    return lone


@pytest.mark.parametrize("form,dec_slots", CASES)
def test_crowded_job_equals_lone_calls(form, dec_slots, ckpt, pool, tmp_path):
    path = str(tmp_path / "trace.txt")
    n_tiles = dec_slots // P.ROW_TILE
    allowed = P.allowed_rows_caps(dec_slots)
    eng = _engine(ckpt, form, dec_slots)
    rec = {"form": form, "dec_slots": dec_slots, "workspace_gb": round(eng.workspace_bytes / 1e9, 2)}
    t_case = time.perf_counter()
    try:
        for job, (rb, n_img) in P.job_images(dec_slots).items():
            tiles_per_chunk = rb // P.ROW_TILE
            lone = _lone_results(eng, form, pool, n_img, rb, path)
            want = P.expectation(lone, n_img, rb)
            x = pool[P.job_index(n_img, rb).to(pool.device)].contiguous()
            got, polls, wall = _traced_predict(eng, x, rb, path)
            pairs = sorted({(p["scan"], p["rows_cap"]) for p in polls})
            caps = {c for _, c in pairs}
            steps = set().union(*(allowed.get(c, set()) for c in caps))
            rec[job] = {"ref_batch": rb, "images": n_img, "wall_s": round(wall, 3), "polls": len(polls),
                        "max_live": max(p["live"] for p in polls), "min_free_tiles": min(p["free_tiles"] for p in polls),
                        "max_scan": max(p["scan"] for p in polls), "scan_rows_cap": pairs}
            print("predict_scale", form, dec_slots, job, json.dumps(rec[job]))      # before anything is asserted
            # ---- 1. every word
            P.compare(got, want, rb, f"{form}, {dec_slots} slots, job {job} (ref_batch {rb}, {n_img} images)")
            # ---- 2. the regime was reached
            assert min(p["free_tiles"] for p in polls) == (0 if job == "A" else n_tiles % tiles_per_chunk), rec[job]
            assert min(p["free_tiles"] for p in polls) < tiles_per_chunk
            assert max(p["live"] for p in polls) == n_tiles // tiles_per_chunk, rec[job]
            assert max(p["scan"] for p in polls) == dec_slots, rec[job]
            assert caps <= set(allowed), (sorted(caps - set(allowed)), "capacities outside predict_impl's rule")
            assert all(s >= c and (s % 1024 == 0 or s in (c, dec_slots)) for s, c in pairs), pairs
            if job == "A":
                assert max(caps) == dec_slots, rec[job]         # every slot alive in one tick
            assert 128 in steps, (sorted(caps), "no capacity from the 128 step")
            if dec_slots > 2048:
                assert 256 in steps, (sorted(caps), "no capacity from the 256 step")
        rec["wall_s"] = round(time.perf_counter() - t_case, 3)
    finally:
        eng.close()
    print("predict_scale", json.dumps(rec))
