"""Device time of mnx_tanimoto_search beside the only route to the same answer without it (DESIGN.md section 6.30,
profiles/nearest_time.txt):

    python tools/nearest_time.py [--repeats 7] [--out profiles/nearest_time.txt]

Libraries of 65 536 and of 1 048 576 rows of random words with about 384 of 2048 bits set (the drug-like median is about 400), 1, 64
and 1024 queries of the same kind, k = 8. Device time between two events around the call's launches, the calls of one library
alternating inside every repeat, median [min .. max] after 3 warm-up rounds; rows, outputs and the scratch stay on the device.
  mnx_tanimoto_search   one call
  pairs + topk          for the 65 536-row library only, what a caller had before: per query its row gathered against every
                        library row (65 536 copies of 256 bytes), one mnx_tanimoto call of 65 536 pairs, the similarities kept
                        as a row of a [nq, nl] matrix; then one torch.topk over the matrix. Checked first: the same indices as
                        the search wherever a query's first k + 1 similarities are all different.
Reported beside the times: pairs per second, and library bytes read per second — the library's size times the number of query
tiles, since every tile of NEAREST_QUERY_TILE queries reads the library once — to set against the 6.0-6.3 TB/s an HBM sweep reaches
on this chip. A record, not a gate: the call is opt-in and off the default path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from molnextr_amd import abi                  # noqa: E402
from molnextr_amd import engine as E          # noqa: E402
from molnextr_amd import weights as W         # noqa: E402
from pages_time import fmt                    # noqa: E402

K = 8
PAIRS_PER_CALL = 65536


def random_rows(n, gen, dev):
    a, b, c, d = (torch.randint(-(1 << 31), 1 << 31, (n, abi.FP_WORDS), dtype=torch.int64, generator=gen, device=dev).to(torch.int32) for _ in range(4))
    return ((a & b) & ~(c & d)).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = E.Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    gen = torch.Generator(device=dev)
    gen.manual_seed(30)
    queries = random_rows(1024, gen, dev)
    lines = [f"nearest_time: {torch.cuda.get_device_name(0)}, repeats {args.repeats}, k {K}, query tile {abi.NEAREST_QUERY_TILE}, "
             f"slab {abi.NEAREST_SLAB_ROWS} rows, at most {abi.NEAREST_MAX_LISTS} lists"]
    for nl in (65536, 1048576):
        library = random_rows(nl, gen, dev)
        bits = int(np.median(np.unpackbits(library[:1024].cpu().numpy().view(np.uint8), axis=1).sum(axis=1)))
        lines.append(f"library of {nl} rows ({nl * 256 / 1e6:.1f} MB), bits set per row median {bits}")
        lines.append("  device us between two events around the launches, the calls alternating   median [min .. max]")
        baseline = nl == PAIRS_PER_CALL
        for nq in (1, 64, 1024):
            q = queries[:nq]
            count = torch.empty(nq, dtype=torch.int32, device=dev)
            index, both, either = (torch.empty((nq, K), dtype=torch.int32, device=dev) for _ in range(3))
            similarity = torch.empty((nq, K), dtype=torch.float64, device=dev)
            work_bytes = int(eng.lib.mnx_tanimoto_search_work_bytes(nq, nl, K))
            work = torch.empty(work_bytes // 8, dtype=torch.int64, device=dev)
            matrix = torch.empty((nq, nl), dtype=torch.float64, device=dev) if baseline else None
            top = {}

            def search():
                return eng.lib.mnx_tanimoto_search(eng.h, ptr(q), nq, ptr(library), nl, K, 0.0, 0, ptr(count), ptr(index), ptr(both), ptr(either),
                                                   ptr(similarity), ptr(work), work_bytes, stream())

            def pairs_topk():
                for i in range(nq):
                    gathered = q[i].expand(nl, abi.FP_WORDS).contiguous()
                    rc = eng.lib.mnx_tanimoto(eng.h, ptr(gathered), ptr(library), nl, None, None, ptr(matrix[i]), stream())
                    if rc:
                        return rc
                top["values"], top["indices"] = torch.topk(matrix, K + 1, dim=1)
                return 0

            calls = {"mnx_tanimoto_search": search, **({"pairs + topk": pairs_topk} if baseline else {})}
            us = {name: [] for name in calls}
            for i in range(args.repeats + 3):
                for name, call in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    rc = call()
                    b.record()
                    torch.cuda.synchronize()
                    assert rc == 0, (name, eng.lib.mnx_last_error(eng.h))
                    if i >= 3:
                        us[name].append(a.elapsed_time(b) * 1000.0)
            if baseline:        # the same indices wherever the first k + 1 similarities of a query are all different
                values, indices = top["values"].cpu().numpy(), top["indices"].cpu().numpy()
                untied = [r for r in range(nq) if len(set(values[r].tolist())) == K + 1]
                found = index.cpu().numpy().view(np.uint32)
                assert all(found[r].tolist() == indices[r, :K].tolist() for r in untied), "the two routes disagree without a tie"
                assert all(similarity.cpu().numpy()[r].tolist() == values[r, :K].tolist() for r in range(nq)), "the two routes' similarities differ"
                agree = f"; same indices in all {len(untied)} of {nq} queries without a tie"
            tiles = -(-nq // abi.NEAREST_QUERY_TILE)
            t = statistics.median(us["mnx_tanimoto_search"]) * 1e-6
            lines.append(f"  nq {nq:4d}  mnx_tanimoto_search {fmt(us['mnx_tanimoto_search'])} us   {nq * nl / t / 1e9:8.2f} G pairs/s   "
                         f"library read {tiles} x: {tiles * nl * 256 / t / 1e12:6.3f} TB/s")
            if baseline:
                tb = statistics.median(us["pairs + topk"]) * 1e-6
                lines.append(f"           pairs + topk        {fmt(us['pairs + topk'])} us   {nq * nl / tb / 1e9:8.2f} G pairs/s   "
                             f"search / pairs + topk, median {t / tb:.4f}{agree}")
        del library
    eng.close()
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
