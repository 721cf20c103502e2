"""Device time of mnx_substructure_match beside mnx_fingerprint_pack on the same tables (profiles/match_time.txt):

    python tools/match_time.py [--repeats 7] [--out profiles/match_time.txt]

1024 hand-made molecules of drug-like size (tools/pages_time.druglike_records). One call each, device time between two events around
the call's launch, the calls alternating inside every repeat, median [min .. max] after 3 warm-up rounds; the tables stay on the
device and every output buffer has its exact size:
  one query        an aromatic six-ring with a carbon on it, 7 atoms, against the 1024 tables (1024 pairs)
  item by item     molecule i against molecule i + 1 (1024 pairs; a whole molecule as the query: nearly all are refuted)
  itself           molecule i against itself (1024 pairs; the identity is found)
  mnx_fingerprint_pack on the 1024 tables
A record, not a gate: the calls are opt-in and off the default path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from molnextr_amd import engine as E          # noqa: E402
from molnextr_amd import weights as W         # noqa: E402
from pages_time import druglike_records, fmt  # noqa: E402


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
    n = 1024
    rec = dict(zip(("mols", "atoms", "bonds", "text"), druglike_records(n)))
    query = eng.smiles_read(["Cc1ccccc1"], keep_device=True)
    t_tables, t_args = eng._packed_tables(rec)
    q_tables, q_args = eng._packed_tables(query)
    ids = np.arange(n)
    lists = {"one query": (q_args, np.stack([np.zeros(n, np.int64), ids], 1)), "item by item": (t_args, np.stack([ids, (ids + 1) % n], 1)),
             "itself": (t_args, np.stack([ids, ids], 1))}
    pairs_d = {k: torch.from_numpy(p.astype(np.int32)).to(dev) for k, (_, p) in lists.items()}
    recs_d = torch.empty(n * E.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    maps_d = torch.empty((n, E.MATCH_MAX_QUERY), dtype=torch.int16, device=dev)
    fp_d, bits_d = torch.empty(n * 16, dtype=torch.uint8, device=dev), torch.empty((n, E.FP_WORDS), dtype=torch.int32, device=dev)

    def match(k):
        return eng.lib.mnx_substructure_match(eng.h, *lists[k][0], *t_args, ptr(pairs_d[k]), n, ptr(recs_d), ptr(maps_d), 1, 0, stream())

    calls = {"mnx_substructure_match, " + k: (lambda k=k: match(k)) for k in lists}
    calls["mnx_fingerprint_pack"] = lambda: eng.lib.mnx_fingerprint_pack(eng.h, *t_args, ptr(fp_d), ptr(bits_d), 0, 0, stream())
    us, seen = {k: [] for k in calls}, {}
    for i in range(args.repeats + 3):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            rc = call()
            b.record()
            torch.cuda.synchronize()
            assert rc == 0, (k, eng.lib.mnx_last_error(eng.h))
            if i >= 3:
                us[k].append(a.elapsed_time(b) * 1000.0)
            if k.startswith("mnx_substructure_match"):
                seen[k] = recs_d.cpu().numpy().view(E.MATCH_DTYPE).copy()
    lines = [f"match_time: {torch.cuda.get_device_name(0)}, repeats {args.repeats}",
             f"one call over {n} hand-made molecules of drug-like size: {len(rec['atoms'])} atoms, {len(rec['bonds'])} bonds; the query "
             f"Cc1ccccc1 has {int(query['mols']['n_atoms'][0])} atoms",
             "  device us between two events around the launch, the four alternating   median [min .. max]"]
    for k in us:
        lines.append(f"  {k:38s} {fmt(us[k])} us")
        if k in seen:
            m = seen[k]
            lines.append(f"  {'':38s} matched {int((m['n_matches'] > 0).sum())}, limited {int((m['flags'] & E.MATCH_LIMIT != 0).sum())}, refused "
                         f"{int((m['flags'] & E.MATCH_REFUSED != 0).sum())}, steps median {int(np.median(m['steps']))} max {int(m['steps'].max())}")
    lines.append(f"  one query / fingerprint, median {statistics.median(us['mnx_substructure_match, one query']) / statistics.median(us['mnx_fingerprint_pack']):.2f}")
    eng.close()
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
