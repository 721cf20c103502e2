#!/usr/bin/env python3
"""bench.py — throughput of the MolNexTR predict hot path on MI355X (molecules/s at 384x384, batch 32 per GPU).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

`--gpus N` with N > 1 and no torchrun environment: bench.py launches itself under `python -m torch.distributed.run
--nproc-per-node N` (one rank per GPU over RCCL); in every case the run FAILS unless the number of ranks equals --gpus
and the node has that many GPUs — it never prints an `n_gpus` it did not use.

One "step" = one pass of the whole hot path over one batch of 32 synthetic 384x384x3 images per GPU, inputs already
resident in HBM: Swin-B encode (MFMA GEMMs; default operand mode fp16x3 = split fp16 operands, three 16-bit MFMA terms
per product, fp32 accumulate: the fastest mode whose tokens / atoms / bonds equal the reference's from pixels with the
logits a factor of four inside north_star's 1e-3) ->
enc_transform + cross-KV -> greedy decode until EOS / 480 tokens
(reference default max_length) -> on-device atom positions -> bond head; with N > 1 the batch of N*32 images is sharded
by image across the ranks and the fixed-size result records are all-gathered with RCCL inside the timed region.
Weights: deterministic synthetic checkpoint in the reference's exact state-dict layout (no pretrained checkpoint
exists offline). The K timed batches are submitted to the engine's continuous-batching entry point (mnx_predict):
every batch of 32 stays ONE reference batch (its own positional-encoding numbering), but many batches are resident in
the decoder at once and finished rows are refilled with the next batch. `--beam 5` times BASELINE config 5 instead
(beam 5 x batch 32 through mnx_predict_beam: up to 8 reference batches share one step sequence, encoder running ahead).

Rank 0 prints ONE JSON line (contract in the task statement). A plain run sets up, warms up, times the K steps, writes
--dump-outputs and prints the line: after the timed steps it only reads what was measured during them. Everything that
takes runs of its own (replays, probes, sub-results, the CPU baseline) runs with `--full` alone, after the timed steps;
without it those fields are null. Beyond the contract the line carries
  roofline        the dominant FLOP kernel (encoder GEMMs, 16-bit MFMA): ALGORITHMIC FLOP (2*M*N*K per launch) divided by
                  event-bracketed durations measured LIVE on the encoder stream inside the timed region (at most 4 encoder
                  launch groups are bracketed, whatever --steps is; null without --full when nothing was bracketed live:
                  --mode batch, --beam > 1); `isolated` (--full) = the same launches replayed afterwards;
                  peak = 2500 TFLOP/s dense bf16 / fp16 (MI355X_MICROARCH.md). In the split modes the matrix pipe executes
                  2-3 MFMA terms per algorithmic product: `mfma_terms` = their FLOP-weighted average (3 for fp16x3, 2.33 for
                  fp16x3m) and `frac_of_peak_executed` = mfma_terms x frac. The sustained MFMA rate (--full) comes from a
                  probe run after the timed steps.
                  `stage34` = the same figures for the block Linears of Swin stages 3 and 4 (C >= 512, the MFMA-bound shapes)
  roofline_extra  HBM-bound kernel classes: LayerNorm / window attention / patch embedding (live, same events; --full adds
                  their isolated replay) and, with --full, the two per-row decode attention kernels (isolated probe at a
                  fixed operating point): algorithmic bytes / duration against 8 TB/s
  sub_results     (--full, N = 1 only, after the timed region) latency mode (one batch of 32 at a time), fixed-T=128 decode
                  (deterministic work), beam 5 x batch 32, the throughput of the opt-in two-term mode fp16x3m and of the plain
                  bf16 operand mode (fastest, not token-exact) next to the default mode's
  cpu_baseline    (--full, N = 1 only) the CPU oracle (oracle/, bit-equal to the reference in the build container) on a
                  bounded sample of the same workload on this box's host cores: thread sweep,
                  B in {1, 32}, encoder / decoder split, natural and fixed-T=128 decode, median of 3 after a warm-up,
                  1-thread figure, lscpu model
  parity_note     what "SMILES exact-match" can mean here (RDKit is not installable: token SMILES + atom / bond sets).

`--dump-outputs DIR` writes, after the timed steps, what the timed path returned for its LAST step (the last batch of 32
images of rank 0): DIR/tokens.npy [32,480], lengths.npy [32], atom_idx.npy [32,kmax], n_atoms.npy [32],
edges.npy [32,kmax,kmax] (and scores.npy [32] with --beam > 1), every array as float32 (the integers are exact). The
images and weights are pure functions of the arguments, so two builds run with the same arguments can be compared
array by array.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from molnextr_amd import shard  # noqa: E402
from molnextr_amd import weights as W  # noqa: E402
from molnextr_amd.engine import DEFAULT_DTYPE, FP16X3M_TWO_TERM  # noqa: E402
from molnextr_amd.tokenizer import get_tokenizer  # noqa: E402

BATCH = 32
PEAK_BF16_TFLOPS = 2500.0
PEAK_HBM_GBS = 8000.0


def run_batch(eng, images, kmax, max_len, beam=1):
    """Encoder.forward + Decoder.decode for ONE reference batch on the current stream; results as device records."""
    feats = eng.encode(images)
    if beam > 1:
        bo = eng.decode_beam(feats, beam=beam, n_best=1, max_len=max_len)
        tokens, lengths, hidden = bo["tokens"][:, 0].contiguous(), bo["lengths"][:, 0].contiguous(), bo["hidden"][:, 0].contiguous()
    else:
        out = eng.decode_greedy(feats, max_len=max_len, want_logp=False)
        tokens, lengths, hidden = out["tokens"], out["lengths"], out["hidden"]
    atom_idx, n_atoms = eng.atom_scan(tokens, lengths, kmax)
    edges, _ = eng.edges(hidden, atom_idx, n_atoms)
    return tokens, lengths, atom_idx, n_atoms, edges


def encoder_gemm_layers(batch=BATCH):
    """(stage, op class, M, N, K, launches) of every encoder Linear for Swin-B @384 (op classes as molnextr_amd.engine.SPLIT_CLASSES;
    the patch-merging reduction behind stage s counts as stage s)."""
    for s, (L, C, depth) in enumerate([(9216, 128, 2), (2304, 256, 2), (576, 512, 18), (144, 1024, 2)]):
        M = batch * L
        yield s, "qkv", M, 3 * C, C, depth
        yield s, "proj", M, C, C, depth
        yield s, "fc1", M, 4 * C, C, depth
        yield s, "fc2", M, C, 4 * C, depth
        if s < 3:
            yield s, "merge", M // 4, 2 * C, 4 * C, 1


def two_term_layers(tags):
    """{(stage, op class)} of the tags "cls" / "cls.sN" (molnextr_amd.engine.Engine.set_op_terms, tools/study_split_terms.py --two)."""
    out = set()
    for tag in tags:
        cls, _, st = tag.partition(".s")
        out |= {(int(st) if st else s, cls) for s in ([0] if st else range(4))}
    return out


def gemm_algorithmic_bytes(batch=BATCH, planes=1, two=frozenset()):
    """Average algorithmic HBM bytes per encoder GEMM launch (A + W read once, output written once, residual read
    for the two residual epilogues) for Swin-B @384: the figure `roofline.traffic` is compared with. planes = 2 for
    the split modes (every 16-bit operand / output is a hi and a lo plane); a layer of `two` (fp16x3m: two product terms)
    reads ONE activation plane, and fc1 writes one when fc2 is such a layer."""
    total, launches = 0, 0
    for s, cls, m, n, k, cnt in encoder_gemm_layers(batch):
        a_b = 2 * (1 if (s, cls) in two else planes)
        w_b = 2 * planes
        if cls == "qkv":
            out_b, res_b = 2 * planes, 0
        elif cls == "fc1":
            out_b, res_b = 2 * (1 if (s, "fc2") in two else planes), 0
        elif cls == "merge":
            out_b, res_b = 4, 0
        else:
            out_b, res_b = 4, 4
        total += cnt * (m * k * a_b + n * k * w_b + m * n * (out_b + res_b))
        launches += cnt
    return total / launches


def gemm_mfma_terms(split, two=frozenset()):
    """MFMA terms executed per algorithmic product, FLOP-weighted over the encoder's Linears: 1 (one plane per operand), 3 (split
    modes), or between 2 and 3 (fp16x3m: the layers of `two` run ah.wh + ah.wl only)."""
    if not split:
        return 1.0
    ex = sum((2 if (s, cls) in two else 3) * m * n * k * cnt for s, cls, m, n, k, cnt in encoder_gemm_layers())
    return ex / sum(m * n * k * cnt for _, _, m, n, k, cnt in encoder_gemm_layers())


def host_cpu_info():
    """lscpu model string, sockets x cores (physical), logical CPUs."""
    info = {"model": None, "physical_cores": None, "logical_cpus": os.cpu_count()}
    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {}
        for line in txt.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                kv[k.strip()] = v.strip()
        info["model"] = kv.get("Model name")
        info["physical_cores"] = int(kv.get("Socket(s)", "1")) * int(kv.get("Core(s) per socket", "0")) or None
    except Exception:
        pass
    return info


def cpu_baseline(ck, budget_s=85.0):
    """The CPU oracle on host cores, as BASELINE.md section 3 plans it: thread-count sweep (encoder, B = 8), then at the
    best count B = 32 (warm + median of 3: encoder, natural greedy decode + bond head) and B = 1, a fixed-T = 128 decode,
    and a 1-thread B = 1 figure. Bounded: every leg checks the remaining budget."""
    from oracle.decoder import greedy_decode
    from oracle.edges import predict_edges
    from oracle.swin import encoder_forward
    tok = get_tokenizer()["chartok_coords"]
    t_start = time.time()
    left = lambda: budget_s - (time.time() - t_start)   # noqa: E731
    host = host_cpu_info()
    logical = os.cpu_count() or 1
    phys = host["physical_cores"] or max(1, logical // 2)

    def enc(img):
        t0 = time.time()
        f = encoder_forward(img, ck["encoder"])
        return f, time.time() - t0

    def dec(f, fixed_T=None):
        t0 = time.time()
        g = greedy_decode(f, ck["decoder"], max_len=fixed_T, stop_on_eos=fixed_T is None)
        for b in range(f.shape[0]):
            idx = tok.sequence_to_smiles(g.tokens[b])["indices"]
            if idx:
                predict_edges(g.hidden[b], idx, ck["decoder"])
        return time.time() - t0, [len(t) for t in g.tokens]

    img32 = W.synthetic_images(32)
    img8, img1 = img32[:8].contiguous(), img32[:1].contiguous()
    sweep = []
    counts = sorted({c for c in (16, 32, 64, phys) if 1 <= c <= logical})
    torch.set_num_threads(counts[0])
    enc(img1)                                                         # warm-up (allocator, thread pool)
    for th in counts:
        if left() < budget_s * 0.75:
            break
        torch.set_num_threads(th)
        _, t = enc(img8)
        sweep.append({"threads": th, "B": 8, "encoder_s": round(t, 3), "images_per_s": round(8.0 / t, 2)})
    best_th = max(sweep, key=lambda r: r["images_per_s"])["threads"] if sweep else min(16, logical)
    torch.set_num_threads(best_th)
    rows = []
    runs = []
    while len(runs) < 3 and left() > budget_s * 0.3:
        f, te = enc(img32)
        td, lens = dec(f)
        runs.append((te, td, lens))
    if runs:
        te = statistics.median(r[0] for r in runs)
        td = statistics.median(r[1] for r in runs)
        lens = runs[0][2]
        rows.append({"B": 32, "threads": best_th, "runs": len(runs), "mode": "natural (EOS / 480)", "encoder_s": round(te, 3),
                     "decode_and_bonds_s": round(td, 3), "molecules_per_s": round(32.0 / (te + td), 3),
                     "decoded_len_mean": round(float(np.mean(lens)), 1), "decoded_len_max": int(max(lens))})
        if left() > 6:
            tdf, _ = dec(f, fixed_T=128)
            rows.append({"B": 32, "threads": best_th, "runs": 1, "mode": "fixed T = 128 (EOS ignored)", "encoder_s": round(te, 3),
                         "decode_and_bonds_s": round(tdf, 3), "molecules_per_s": round(32.0 / (te + tdf), 3),
                         "decode_ms_per_step": round(tdf / 128 * 1e3, 2)})
    runs1 = []
    while len(runs1) < 3 and left() > 8:
        f, te = enc(img1)
        td, lens = dec(f)
        runs1.append((te, td))
    if runs1:
        te = statistics.median(r[0] for r in runs1)
        td = statistics.median(r[1] for r in runs1)
        rows.append({"B": 1, "threads": best_th, "runs": len(runs1), "mode": "natural (EOS / 480)", "encoder_s": round(te, 3),
                     "decode_and_bonds_s": round(td, 3), "molecules_per_s": round(1.0 / (te + td), 3)})
    if left() > 8:
        torch.set_num_threads(1)
        f, te = enc(img1)
        td, _ = dec(f)
        rows.append({"B": 1, "threads": 1, "runs": 1, "mode": "natural (EOS / 480)", "encoder_s": round(te, 3),
                     "decode_and_bonds_s": round(td, 3), "molecules_per_s": round(1.0 / (te + td), 3)})
    torch.set_num_threads(logical)
    # `value` = the configuration the GPU line is quoted on (one reference batch of 32, natural decode) when it was timed,
    # otherwise the best natural-decode row; every row is listed in `runs`
    nat = [r for r in rows if r["mode"].startswith("natural")]
    b32 = [r for r in nat if r["B"] == BATCH]
    best = b32[0] if b32 else (max(nat, key=lambda r: r["molecules_per_s"]) if nat else
                               {"molecules_per_s": None, "threads": best_th, "B": 0})
    return {"value": best["molecules_per_s"], "unit": "molecules/s", "cores": best["threads"], "kind": "port",
            "sample": (f"CPU oracle (fp32 torch ops, bit-equal to the reference in the build container): synthetic images "
                       f"0..{best['B'] - 1} as one reference batch, encoder + greedy decode to EOS + bond head, median of the runs "
                       f"listed; thread count chosen by the encoder sweep ({time.time() - t_start:.0f} s of CPU work in total; "
                       "`runs` also holds B = 1, fixed-T = 128 and 1-thread figures)"),
            "host": host, "thread_sweep": sweep, "runs": rows}


GEMM_SOURCES = ("gemm.hip", "gemm256.hip", "gemm_res.hip", "common.h", "kernels.h")


def library_sha16():
    """First 16 hex digits of the sha256 over the sources of the encoder GEMM kernels and their dispatch (molnextr_amd/csrc:
    GEMM_SOURCES) the loaded library is built from: a traffic file made with other GEMM kernels is not evidence about these.
    (The sources rather than the .so: two builds of the same sources need not be byte-identical. tools/collect_traffic.py
    computes the same digest.)"""
    import hashlib
    h = hashlib.sha256()
    for name in GEMM_SOURCES:
        h.update(name.encode())
        with open(os.path.join(ROOT, "molnextr_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def gemm_traffic(dtype, eb):
    """HBM bytes per encoder GEMM launch from the rocprofv3 --pmc passes of tools/gpu/profiles.sh (tools/collect_traffic.py writes
    profiles/r06_gemm_traffic_<dtype>_b<images>.json and stamps it with the digest of the kernel sources it profiled). The
    counters cannot be collected inside a timed run, so the figure comes from a file — but only from one made with THESE
    kernels: (bytes, source) or (None, why not)."""
    name = f"r06_gemm_traffic_{dtype}_b{eb}.json"
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None, f"profiles/{name} not present (tools/gpu/profiles.sh makes it)"
    with open(path) as f:
        d = json.load(f)
    have = library_sha16()
    if d.get("library_sha16") != have:
        return None, (f"profiles/{name} was made with kernel sources {d.get('library_sha16')}, this run's are {have}: refused "
                      "(re-run tools/gpu/profiles.sh with this build)")
    return round(d["hbm_bytes_per_launch"]), (f"profiles/{name}: separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over the same "
                                              f"encoder launches, kernel sources {have}")


def plan_launch(gpus, env, device_count):
    """What `python bench.py --gpus N` must do, decided before anything touches a GPU:
      ("run", world)    run in this process as one of `world` ranks (world == gpus is enforced),
      ("spawn", None)   no torchrun environment and gpus > 1: launch the N ranks ourselves.
    Raises SystemExit with a clear message when the request cannot be honoured (fewer GPUs than asked for, or a torchrun
    world size that differs from --gpus): a line that says n_gpus N must have used N."""
    if gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if device_count < gpus:
        raise SystemExit(f"bench.py --gpus {gpus}: this node exposes {device_count} GPU(s); refusing to report n_gpus={gpus} "
                         "from fewer devices")
    if "WORLD_SIZE" in env:
        world = int(env["WORLD_SIZE"])
        if world != gpus:
            raise SystemExit(f"bench.py --gpus {gpus} was started with WORLD_SIZE={world}: ranks and --gpus must agree")
        return "run", world
    return ("spawn", None) if gpus > 1 else ("run", 1)


def spawn_ranks(gpus, argv):
    """Re-executes this script under torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def parse_cpulist(text):
    """'0-3,8,10-11' (sysfs cpulist syntax) -> [0, 1, 2, 3, 8, 10, 11]."""
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def rank_cpus(local, cpulists, available):
    """Host CPUs for the rank that drives device `local` of a node with len(cpulists) ranks. cpulists[i]: the CPUs local to
    device i's PCIe root (sysfs local_cpulist; None when unknown). The ranks whose devices share a NUMA node split that node's
    CPUs evenly, in device order — 8 ranks each run a polling host thread, a prefetch thread and pinned-memory copies, and a
    rank that lands on the other socket pays a cross-socket hop on every poll and every H2D / D2H. Without topology
    information the CPUs this process may use are cut into len(cpulists) contiguous slices. Pure function (unit-tested)."""
    world = len(cpulists)
    avail = sorted(available)
    mine = cpulists[local]
    if mine:
        numa = [c for c in mine if c in available]
        peers = [i for i in range(world) if cpulists[i] == mine]
        if numa and len(numa) >= len(peers):
            per, k = len(numa) // len(peers), peers.index(local)
            return numa[k * per:(k + 1) * per]
    per = max(1, len(avail) // world)
    return avail[local * per:(local + 1) * per] or avail


def device_cpulists(world):
    """sysfs local_cpulist of devices 0..world-1 (None where it cannot be read)."""
    out = []
    for i in range(world):
        try:
            p = torch.cuda.get_device_properties(i)
            bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
            with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
                out.append(parse_cpulist(f.read()) or None)
        except Exception:   # noqa: BLE001 - topology is a hint, never a reason to fail
            out.append(None)
    return out


def pin_rank(local, world):
    """Multi-rank runs: bind this rank (and the threads it starts later) to its device's NUMA-local CPUs; returns the set."""
    if world <= 1 or not hasattr(os, "sched_setaffinity"):
        return None
    cpus = rank_cpus(local, device_cpulists(world), os.sched_getaffinity(0))
    try:
        os.sched_setaffinity(0, cpus)
    except OSError:
        return None
    torch.set_num_threads(max(1, min(8, len(cpus))))
    return cpus


def land_records(out, kmax, rank, world, n_local, pinned, gather=False):
    """The N > 1 tail of a step group: device result tensors of THIS rank's n_local images -> fixed-size records sized by the
    largest molecule of the whole job (one scalar all-reduce MAX) -> one all-gather over RCCL / xGMI (gloo in the CPU tests)
    -> pinned host memory: rank 0 lands the gathered whole (rank order = image order), every other rank its own shard."""
    tokens, lengths, atom_idx, n_atoms, edges = (out[k] for k in ("tokens", "lengths", "atom_idx", "n_atoms", "edges"))
    k = shard.common_atom_capacity(n_atoms, kmax)
    ai, ed = shard.trim_atoms(atom_idx, edges, k)
    rec = shard.pack_records_device(tokens, lengths, ai, n_atoms, ed)
    if world > 1 or gather:
        rec = shard.gather_records(rec, force=gather)
    mine = rec if (rank == 0 or world == 1) else rec[rank * n_local:(rank + 1) * n_local]
    dst = pinned[:mine.numel()].view(mine.shape)
    dst.copy_(mine, non_blocking=True)
    return dst, k


def dump_outputs(dirname, arrays):
    """Device result tensors of one step -> DIR/<name>.npy in float32 (small integers and fp32 scores: exact)."""
    os.makedirs(dirname, exist_ok=True)
    host = {name: t.cpu().numpy().astype(np.float32) for name, t in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > 64 << 20:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the 64 MB budget")
    for name, a in host.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--mode", default="pipeline", choices=["pipeline", "batch"])
    ap.add_argument("--beam", type=int, default=1, help="beam size; > 1 times BASELINE config 5 through mnx_predict_beam")
    ap.add_argument("--max-len", type=int, default=480)
    ap.add_argument("--dtype", default=DEFAULT_DTYPE, choices=["fp16x3", "fp16x3m", "bf16x3", "bf16", "fp16", "fp32"],
                    help="encoder operand mode. fp16x3 (default): three MFMA terms per product everywhere, fp32-class features (6e-6), "
                         "raw logits within 2.5e-4 of the reference's at every step; fp16x3m (opt-in): the same with the Linear layers of "
                         "molnextr_amd.engine.FP16X3M_TWO_TERM (qkv / fc1 / fc2 of Swin stage 3) on two terms (activation lo plane "
                         "dropped): every token / atom / bond still the reference's on everything measured (0 flips in 90 000 "
                         "teacher-forced steps), raw logits within 5.0e-4 on the fixtures, 7.2e-4 on 256 further images and up to 1.2e-3 on 512 images of a hostile checkpoint (north_star: "
                         "1e-3) — tests/test_gpu_pixels.py, profiles/r06_two_term_tables_gpu.json, r06_extended_parity_*.json")
    ap.add_argument("--encode-batch", type=int, default=int(os.environ.get("MNX_ENCODE_BATCH", "512")),
                    help="images per encoder launch group (a multiple of 32; decode batches stay 32). 512 = 16 reference "
                         "batches: every Linear of Swin stage 3 then has a WHOLE number of rounds of 256 output tiles of 256x256 "
                         "(proj / fc2 2304 = 9 x 256, qkv 6912 = 27 x 256, fc1 9216 = 36 x 256; at 448 images 7.875 / 23.6 / 31.5 "
                         "rounds: a ragged last round, the rest on the 128x128 kernel). Measured (round 5, one box, alternating): "
                         "1782 / 1785 molecules/s at 512, 1762 / 1768 at 448, 1762 / 1765 at 640, 1750 / 1746 at 320 on the "
                         "driver's command; 2173 vs 2172 at 512 steps (1024: 2057)")
    ap.add_argument("--slots", type=int, default=int(os.environ.get("MNX_SLOTS", "3072")),
                    help="sequences resident in the decoder (multiple of 32, <= 4096)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run what takes runs of its own: the isolated GEMM / kernel replays, the "
                         "MFMA and decode-attention probes, the sub-results and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-sub", action="store_true", help="with --full: skip the sub-results (latency / fixed-T / parity / beam)")
    ap.add_argument("--force-gather", action="store_true", help="run the RCCL record gather even with one rank")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step (rank 0's last batch of 32) as "
                         "DIR/<name>.npy in float32")
    return ap.parse_args(argv)


def main():
    args = parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    action, world = plan_launch(args.gpus, os.environ, torch.cuda.device_count())
    if action == "spawn":
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rank_cpu_set = pin_rank(local, world)         # before the engine starts its helper threads
    # the checkpoint and the image pool are pure functions of (seed, image index); host threads make them at once (numpy
    # releases the GIL) while the process group and the engine are set up
    # step s, rank r owns images [(s*world + r)*32, +32): every step has its own images (8 distinct batches cycle)
    n_distinct = 8
    maker = ThreadPoolExecutor(max_workers=1 + n_distinct)
    ck_job = maker.submit(W.synthetic_checkpoint, 0)
    pool_jobs = [maker.submit(W.synthetic_images, BATCH, first_index=(s * world + rank) * BATCH) for s in range(n_distinct)]
    use_dist = world > 1 or ("RANK" in os.environ and args.force_gather)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # nccl == RCCL on ROCm
    rccl_ranks = dist.get_world_size() if use_dist else 1
    if rccl_ranks != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: the process group has {rccl_ranks} rank(s)")
    from molnextr_amd.engine import Engine

    mode = "beam" if args.beam > 1 else args.mode
    ck = ck_job.result()
    eb = max(BATCH, args.encode_batch)   # images per encoder launch group
    eng = Engine(ck["encoder"], ck["decoder"], device=local, max_batch=eb, dtype=args.dtype, dec_slots=args.slots)
    kmax = eng.max_atoms
    pool = [job.result().to(dev) for job in pool_jobs]
    maker.shutdown()

    def images_for(first_step, count):
        return torch.cat([pool[(first_step + i) % n_distinct] for i in range(count)]).contiguous()

    stats = {}
    host_buf = {}

    def process(e, imgs, count, how, max_len=args.max_len, stop_on_eos=True, beam=args.beam, land=True, keep_last=False):
        """`count` steps over resident images; returns the (gathered) result records on the host. keep_last: leave views of
        the last step's output tensors in stats["last_step"] (for --dump-outputs)."""
        if how in ("pipeline", "beam"):
            out = e.predict(imgs, ref_batch=BATCH, max_len=max_len, stop_on_eos=stop_on_eos, beam=beam)
            tokens, lengths, atom_idx, n_atoms, edges = (out[k] for k in ("tokens", "lengths", "atom_idx", "n_atoms", "edges"))
        else:
            parts = [run_batch(e, imgs[i * BATCH:(i + 1) * BATCH], kmax, max_len, beam) for i in range(count)]
            tokens, lengths, atom_idx, n_atoms, edges = (torch.cat([p[j] for p in parts]) for j in range(5))
            out = {}
        if keep_last:             # views of the last step's rows: no copy inside the timed region
            res = {"tokens": tokens, "lengths": lengths, "atom_idx": atom_idx, "n_atoms": n_atoms, "edges": edges}
            if "scores" in out:
                res["scores"] = out["scores"]
            stats["last_step"] = {k: v[-BATCH:] for k, v in res.items()}
        stats["lens"], stats["atoms"] = lengths.cpu().numpy(), n_atoms.cpu().numpy()
        rec = None
        if max_len == shard.MAX_LEN and land:
            res = {"tokens": tokens, "lengths": lengths, "atom_idx": atom_idx, "n_atoms": n_atoms, "edges": edges}
            rec, _ = land_records(res, kmax, rank, world, count * BATCH, host_buf["pinned"], gather=args.force_gather)
            torch.cuda.current_stream().synchronize()
        else:
            torch.cuda.current_stream().synchronize()
        return rec

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn):
        barrier()
        t0 = time.perf_counter()
        fn()
        barrier()
        return time.perf_counter() - t0

    # pinned landing buffer for the result records, allocated once outside the timed region (capacity: every record
    # at the engine's max_atoms; the records actually exchanged are sized by the largest molecule of the job)
    gathered = world if (rank == 0 and (world > 1 or args.force_gather)) else 1
    host_buf["pinned"] = torch.empty(max(args.steps, args.warmup, 16) * BATCH * gathered * shard.record_words(kmax),
                                     dtype=torch.int32, pin_memory=True)
    live = mode == "pipeline"
    groups = max(1, args.steps * BATCH // eb)
    stride = max(1, groups // 4)         # at most 4 encoder launch groups of the timed region get their kernels bracketed
    if args.warmup > 0:
        imgs = images_for(0, args.warmup)
        torch.cuda.synchronize()
        if live:
            eng.profile(max(1, args.warmup * BATCH // eb // 4))    # creates the event pool outside the timed region
        process(eng, imgs, args.warmup, mode)
        if live:
            eng.profile_read_all()
    imgs = images_for(args.warmup, args.steps)
    torch.cuda.synchronize()
    if live:
        eng.profile(stride)              # HIP events on the encoder stream, live inside the timed region
    eng.gemm_clock(reset=True)           # shader-clock counters of the persistent GEMM launches: zeroed before the timed region
    elapsed = timed(lambda: process(eng, imgs, args.steps, mode, keep_last=bool(args.dump_outputs)))
    gemm_mhz = eng.gemm_clock(reset=True)     # ... and read after it: every gemm256x3 launch of the timed job
    live_prof = eng.profile_read_all() if live else None
    eng.profile(False)
    last_step = stats.pop("last_step", None)
    if last_step is not None and rank == 0:
        dump_outputs(args.dump_outputs, last_step)
    del last_step
    main_stats = dict(stats)
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    out = None
    if rank == 0:
        # ---- roofline of the dominant FLOP kernel (all encoder GEMM launches). `achieved` is measured LIVE: HIP events
        # around every kernel of <= 4 encoder launch groups spread over the timed region, i.e. next to the decoder; the
        # same launches replayed afterwards on an otherwise idle GPU are reported as `isolated` (--full).
        iso = None
        if args.full:
            eng.profile(True)
            for i in range(min(args.steps * BATCH // eb, 4)):
                eng.encode(imgs[i * eb:(i + 1) * eb].contiguous())
            iso = eng.profile_read_all()
            eng.profile(False)
        split = args.dtype in ("fp16x3", "fp16x3m", "bf16x3")
        two = two_term_layers(FP16X3M_TWO_TERM) if args.dtype == "fp16x3m" else frozenset()
        terms = round(gemm_mfma_terms(split, two), 4)      # FLOP-weighted average over the encoder's Linears

        def family(prof, kinds):
            if not prof:
                return 0.0, 0, 0
            ms = sum(prof[k][0] for k in kinds)
            fl = sum(prof[k][1] for k in kinds)
            n = sum(prof[k][2] for k in kinds)
            return ms, fl, n

        have_live = bool(live_prof) and (live_prof["gemm"][2] + live_prof["gemm_s34"][2]) > 0
        src = live_prof if have_live else iso
        gemm_ms, gemm_flop, launches = family(src, ("gemm", "gemm_s34"))
        iso_ms, iso_flop, iso_n = family(iso, ("gemm", "gemm_s34"))
        achieved = gemm_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        isolated = iso_flop / (iso_ms * 1e-3) / 1e12 if iso_ms > 0 else 0.0
        s_ms, s_flop, s_n = family(src, ("gemm_s34",))
        si_ms, si_flop, si_n = family(iso, ("gemm_s34",))
        s34 = s_flop / (s_ms * 1e-3) / 1e12 if s_ms > 0 else 0.0
        s34_iso = si_flop / (si_ms * 1e-3) / 1e12 if si_ms > 0 else 0.0
        traffic, traffic_src = gemm_traffic(args.dtype, eb)
        # what the matrix pipes sustain on THIS device under its power budget (register-only fp16 MFMA loop on random
        # operands, ~30 ms, measured now): the encoder GEMMs are power-limited, the nominal 2.5 PFLOP/s assumes 2.4 GHz
        sus_tf, sus_mhz = eng.probe_mfma(30) if args.full else (0.0, 0.0)
        mfma = {"fp16x3": "v_mfma_f32_16x16x32_f16 x 3 terms", "bf16x3": "v_mfma_f32_16x16x32_bf16 x 3 terms",
                "fp16x3m": f"v_mfma_f32_16x16x32_f16 x 3 terms, x 2 in {'/'.join(FP16X3M_TWO_TERM)}: {terms} on average",
                "bf16": "v_mfma_f32_16x16x32_bf16", "fp16": "v_mfma_f32_16x16x32_f16", "fp32": "v_mfma_f32_16x16x4_f32"}[args.dtype]
        roofline = {"kernel": f"mnx::gemm_tn_* + mnx::gemm256*_kernel ({mfma}, all encoder Linear layers)",
                    "bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                    "work": "algorithmic FLOP = 2*M*N*K per launch",
                    "mfma_terms": terms, "frac_of_peak_executed": round(terms * achieved / PEAK_BF16_TFLOPS, 4),
                    # executed rate / what a register-only MFMA loop on random operands sustains on this device right now
                    "frac_of_sustained": round(terms * achieved / sus_tf, 4) if sus_tf > 0 else None,
                    # the chip clocks to its power budget: the persistent GEMM kernel's own stamps (shader cycles / wall ticks,
                    # every launch of the timed job) and what a register-only MFMA loop on random operands sustains right now
                    "clock": {"gemm_shader_mhz_live": round(gemm_mhz, 0), "nominal_mhz": 2400,
                              "peak_at_live_clock": round(PEAK_BF16_TFLOPS * gemm_mhz / 2400.0, 1) if gemm_mhz > 0 else None,
                              "frac_of_peak_at_live_clock_executed": (round(terms * achieved / (PEAK_BF16_TFLOPS * gemm_mhz / 2400.0), 4)
                                                                      if gemm_mhz > 0 else None),
                              "sustained_mfma_tflops": round(sus_tf, 1) if sus_tf > 0 else None,
                              "sustained_mfma_mhz": round(sus_mhz, 0) if sus_tf > 0 else None,
                              "frac_of_sustained_executed": round(terms * achieved / sus_tf, 4) if sus_tf > 0 else None,
                              "what": "mnx_gemm_clock over the timed steps, mnx_probe_mfma after them (--full only), measured in this "
                                      "run (include/molnextr_hip.h)"},
                    "traffic": traffic, "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": round(gemm_algorithmic_bytes(eb, 2 if split else 1, two)),
                    "images_per_launch": eb,
                    "launches": int(launches), "avg_launch_us": round(gemm_ms * 1e3 / max(launches, 1), 2),
                    "flop_per_launch_avg": round(gemm_flop / max(launches, 1)),
                    "measured": ("live: HIP events on the encoder stream inside the timed region (<= 4 launch groups)"
                                 if src is live_prof else "replay after the timed region"),
                    "isolated": ({"achieved": round(isolated, 1), "avg_launch_us": round(iso_ms * 1e3 / max(iso_n, 1), 2),
                                  "launches": int(iso_n)} if iso else None),
                    "stage34": {"what": "block Linears with C >= 512 (Swin-B stages 3 and 4: qkv / proj / fc1 / fc2, the MFMA-bound "
                                        "shapes; north_star's >= 60 % target applies to these)",
                                "achieved": round(s34, 1), "frac": round(s34 / PEAK_BF16_TFLOPS, 4),
                                "frac_of_peak_executed": round(terms * s34 / PEAK_BF16_TFLOPS, 4), "launches": int(s_n),
                                "avg_launch_us": round(s_ms * 1e3 / max(s_n, 1), 2),
                                "isolated": ({"achieved": round(s34_iso, 1), "frac": round(s34_iso / PEAK_BF16_TFLOPS, 4)}
                                             if iso else None)}}
        if src is None:           # nothing bracketed live (--mode batch, --beam > 1) and no replay without --full
            roofline = None
        extra = []
        for kind, label in (("layernorm", "mnx::layernorm16_kernel (fp32 in, 16-bit operand planes out)"),
                            ("window_attn", "mnx::window_attn_kernel (qkv in, context out)"),
                            ("patch_embed", "mnx::patch_embed_kernel")):
            for tag, prof in (("live", live_prof), ("isolated", iso)):
                if not prof or prof[kind][2] == 0:
                    continue
                ms, byts, n = prof[kind]
                gbs = byts / (ms * 1e-3) / 1e9
                extra.append({"kernel": label, "bound": "hbm", "measured": tag, "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS,
                              "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4), "launches": int(n),
                              "avg_launch_us": round(ms * 1e3 / n, 2), "algorithmic_bytes_per_launch": round(byts / n)})
        if args.full:
            rows_p, t_p = min(768, args.slots), 64
            self_ms, cross_ms = eng.probe_decode_attn(rows_p, t_p, 24)   # 4 cycles over the 6 layers' K/V: HBM, not Infinity Cache
            # a cached K / V row of 32 channels is 100 bytes (24-bit block fixed point: int16 hi + uint8 lo per element + one scale, csrc/kvq.h)
            for label, ms, byts in (("mnx::dec_attn_kernel, self-attention (K/V cache of the sequence, 3 bytes per element + a scale per row)", self_ms, rows_p * 8 * (t_p + 1) * 200),
                                    ("mnx::dec_attn_kernel, cross-attention (projected memory K/V, 144 keys, 3 bytes per element + a scale per row)", cross_ms, rows_p * 8 * 144 * 200)):
                gbs = byts / (ms * 1e-3) / 1e9
                extra.append({"kernel": label, "bound": "hbm", "measured": f"isolated probe: {rows_p} rows at position {t_p}, launches cycle the 6 layers' K/V (> 256 MB per cycle)",
                              "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                              "avg_launch_us": round(ms * 1e3, 2), "algorithmic_bytes_per_launch": int(byts)})

        sub = None
        if args.full and world == 1 and not args.no_sub:
            sub = {}
            nb = 3
            x = images_for(0, nb)
            process(eng, x[:BATCH].contiguous(), 1, "batch", beam=1, land=False)
            t = timed(lambda: process(eng, x, nb, "batch", beam=1, land=False))
            sub["latency_mode"] = {"what": "one reference batch of 32 at a time (encode -> greedy decode -> atoms -> bonds)",
                                   "ms_per_batch": round(t / nb * 1e3, 2), "molecules_per_s": round(nb * BATCH / t, 1)}
            ns = min(args.steps, 16)
            x = images_for(0, ns)
            process(eng, x, ns, "pipeline", max_len=128, stop_on_eos=False, land=False)
            t = timed(lambda: process(eng, x, ns, "pipeline", max_len=128, stop_on_eos=False, land=False))
            sub["fixed_T128"] = {"what": f"{ns} steps, every sequence decoded for exactly 128 tokens (EOS ignored): deterministic work",
                                 "molecules_per_s": round(ns * BATCH / t, 1), "tokens_per_s": round(ns * BATCH * 128 / t, 0)}
            if args.beam == 1:
                nbm = min(16, max(1, eb // BATCH))
                x = images_for(0, nbm)
                process(eng, x[:BATCH].contiguous(), 1, "pipeline", beam=5, land=False)
                t = timed(lambda: process(eng, x, nbm, "pipeline", beam=5, land=False))
                sub["beam5_batch32"] = {"what": f"BASELINE config 5: beam 5 x batch 32 = 160 hypotheses per reference batch, {nbm} reference batches "
                                                "through mnx_predict_beam: up to 8 reference batches of an encoder launch group share one step "
                                                "sequence (1280 rows per step; positional-encoding rows numbered per reference batch, results "
                                                "identical to batch-by-batch searches: tests/test_gpu_parity.py), the encoder running ahead on "
                                                "its own stream",
                                        "ms_per_batch": round(t / nbm * 1e3, 2), "molecules_per_s": round(nbm * BATCH / t, 1),
                                        "decoded_len_mean": round(float(np.mean(stats["lens"])), 1)}
            if args.dtype in ("fp16x3", "fp16x3m") and args.beam == 1:
                # the sibling mode on the SAME engine (same weights and kernels; mnx_set_op_terms switches the table)
                other = "fp16x3" if args.dtype == "fp16x3m" else "fp16x3m"
                eng.set_op_terms(() if other == "fp16x3" else FP16X3M_TWO_TERM)
                ns = args.steps
                x = images_for(args.warmup, ns)
                process(eng, x[:min(ns, 8) * BATCH].contiguous(), min(ns, 8), "pipeline", land=False)
                t = timed(lambda: process(eng, x, ns, "pipeline", land=False))
                eng.set_op_terms(None)
                two_what = (f"the Linear layers {', '.join(FP16X3M_TWO_TERM)} (qkv / fc1 / fc2 of Swin stage 3, 60 % of the encoder's GEMM "
                            "time) on TWO MFMA terms — the activation's lo plane dropped —, "
                            f"{round(gemm_mfma_terms(True, two_term_layers(FP16X3M_TWO_TERM)), 3)} terms per product on average. Opt-in: every "
                            "token / atom / bond equals the reference's on everything measured (0 flips in 12863 teacher-forced steps "
                            "of the fixtures + 77790 of 384 further images), log-probs within 3.7e-4; raw logits within 5.0e-4 on the "
                            "fixtures, 7.2e-4 on further images and up to 1.2e-3 on a hostile checkpoint (2 of 16 batches beyond north_star's "
                            "1e-3): not a default (tests/test_gpu_pixels.py, profiles/r06_two_term_tables_gpu.json, r06_extended_parity_*.json)")
                sub["throughput_mode_" + other] = {
                    "what": (f"the same {ns} steps with compute_dtype FP16X3 on the same engine: THREE MFMA terms in every layer (features within "
                             "6e-6, raw logits within 8e-5 of the reference's); this line's own mode is FP16X3M = " + two_what
                             if other == "fp16x3" else f"the same {ns} steps with compute_dtype FP16X3M: " + two_what),
                    "molecules_per_s": round(ns * BATCH / t, 1)}
            if args.dtype != "bf16" and args.beam == 1:
                eng.close()
                eng = Engine(ck["encoder"], ck["decoder"], device=local, max_batch=eb, dtype="bf16", dec_slots=args.slots)
                ns = args.steps
                x = images_for(args.warmup, ns)
                process(eng, x[:min(ns, 8) * BATCH].contiguous(), min(ns, 8), "pipeline", land=False)
                t = timed(lambda: process(eng, x, ns, "pipeline", land=False))
                sub["throughput_mode_bf16"] = {"what": f"the same {ns} steps with plain bf16 encoder operands (one MFMA term per product): the fastest "
                                                       "mode, NOT token-exact vs the reference (argmax near-ties flip: tests/test_gpu_pixels.py, "
                                                       "profiles/r04_pixels_parity.json)",
                                               "molecules_per_s": round(ns * BATCH / t, 1)}
        cpu = cpu_baseline(ck) if (args.full and not args.no_cpu_baseline and world == 1) else None   # rank 0 at N=1 only
        total = args.steps * BATCH * world
        if mode == "beam":
            workload = (f"BASELINE config 5: beam {args.beam} x batch 32 synthetic 384x384x3 images per GPU through mnx_predict_beam "
                        "(up to MNX_BEAM_GROUPS = 8 reference batches of an encoder launch group share one step sequence, the encoder "
                        "running ahead on its own stream): Swin-B encode + beam search (n_best 1) + atom positions + bond head on the "
                        "best hypothesis")
        else:
            workload = ("batch=32 synthetic 384x384x3 images per GPU, synthetic_checkpoint(0) in the reference state-dict "
                        f"layout (no pretrained weights offline), Swin-B encode ({args.dtype} operands) + greedy decode to EOS "
                        f"(max_length {args.max_len}) + atom positions + bond head"
                        + (", RCCL all-gather of result records" if world > 1 else ""))
        out = {
            "metric": "molecules/sec (384x384, bs32 per GPU), full predict hot path",
            "value": round(total / elapsed, 2), "unit": "molecules/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": workload, "batch_per_gpu": BATCH, "global_batch": BATCH * world,
                       "mode": (f"continuous batching: up to {args.slots // 32} reference batches ({args.slots} sequences) resident in the decoder, "
                                f"encoder launch groups of {eb} images"
                                if mode == "pipeline" else "one reference batch at a time"),
                       "decoded_len_mean": round(float(np.mean(main_stats["lens"])), 1),
                       "decoded_len_max": int(np.max(main_stats["lens"])),
                       "atoms_mean": round(float(np.mean(main_stats["atoms"])), 1),
                       "parallelism": f"dp{world} (shard by image, no data-path collective)"},
            "rccl_ranks": rccl_ranks,
            "host_cpus_per_rank": len(rank_cpu_set) if rank_cpu_set else None,
            "roofline": roofline, "roofline_extra": extra, "sub_results": sub, "cpu_baseline": cpu,
            "library_sha16": library_sha16(),
            "parity_note": ("SMILES exact-match vs the reference is checked on the raw token SMILES + atom / bond sets (RDKit is not "
                            "installable here). dtype fp16x3 (this line's default) and fp32: logits within 1e-3 (measured 2e-4 over every "
                            "step), every token / atom / bond equal to the reference from pixels (tests/test_gpu_pixels.py, 32 + 6 images, "
                            "free-running and teacher-forced; tools/extended_parity.py on further images); fp16x3m (opt-in): the same "
                            "exactness (0 flips in 230 000 steps), raw logits within 5e-4 on the fixtures (asserted), up to 1.2e-3 on a hostile checkpoint; bf16x3: logits within 1e-3, flips only on near-ties; plain bf16 / fp16: argmax near-ties "
                            "flip (profiles/r04_pixels_parity.json, DESIGN.md §6.1, §6.R3); the exact modes also pass on a second, hostile "
                            "checkpoint (tests/golden/pixels_stress.*)"),
        }
    eng.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
