#!/usr/bin/env python3
"""Does the pages-in path pay? Times, on one GPU and in one process, the per-image transform against the batched one, the
facade from pages in both image formats, and the patch embedding on fp32 against gray input. Measurement only: nothing here
is part of the product path and no number is asserted.

    python tools/pages_time.py [--part a,b,c] [--pages 1024] [--facade-pages 2048] [--repeats 5] [--out profiles/pages_time.txt]

(a) transform alone, `--pages` pages of three sizes: Engine.preprocess (one mnx_preprocess per page) against
    preprocess_batch(out="fp32") and (out="gray8"); wall time per call (host + device, the call synchronises) and the device
    time between two events around it;
(b) predict_images from `--facade-pages` synthetic pages, batch_size 32, image_format fp32 against gray8: molecules / s;
    then (gray8) the dense result path against the packed one (molnextr(packed_results=True): mnx_graph_pack), each with and
    without return_confidence, with the result bytes per image that cross to the host in each; `--pack-out FILE` writes that
    table to a file of its own, and `--pack-only N` runs N mnx_graph_pack calls over 1024 images alone (for a kernel trace);
(c) patch embedding per 512 images from mnx_profile_read (kind 3), fp32 against gray input;
(m) (only when asked for: --part m) molfiles written on the device: one mnx_molfile_pack call over the packed tables of 1024
    images between two events, and predict_images from `--facade-pages` pages with molnextr(graph_molfile=True) against the
    packed facade without it; `--molfile-out FILE` writes the table to a file of its own.
(s) (only when asked for: --part s) graph SMILES written on the device: one mnx_smiles_pack call over the packed tables of 1024
    images between two events, alternating with one mnx_molfile_pack and one mnx_smiles_pack_stereo call over the same tables,
    then mnx_smiles_pack_marks with marks 0, 1, 2 and 3 alternating with the two older SMILES calls in a pass of their own,
    then mnx_smiles_pack_canonical with each set of marks alternating with mnx_smiles_pack_marks in a pass of their own,
    then mnx_smiles_pack_symmetric with each set of marks alternating with mnx_smiles_pack_canonical in a pass of their own
    (also on the drug-like molecules with every third candidate centre a gem-dimethyl carbon, so that the rule fires),
    with how many molecules were written and how many refused per flag; `--smiles-out FILE` writes the table to a file of its
    own.
(x) (only when asked for: --part x) abbreviation expansion on the device: mnx_expand_pack alone, against mnx_graph_pack on the
    same molecules (both are count / scan / fill passes over the same records), and mnx_expand_pack followed by
    mnx_smiles_pack_canonical against the canonical writer on the unexpanded tables — on the synthetic checkpoint's predictions
    (near-complete graphs), on hand-made molecules of drug-like size, and on those with a label at every ninth atom;
    `--expand-out FILE` writes the table to a file of its own.
(r) (only when asked for: --part r) SMILES read on the device: one mnx_smiles_read call over the strings of 1024 hand-made
    molecules of drug-like size against the one mnx_smiles_pack call that writes those strings, then the worst strings the
    reader admits, each alone in a call; `--read-out FILE` writes the table to a file of its own.
(v) (only when asked for: --part v) molfile read on the device: one mnx_molfile_read call over the V2000 molfiles of 1024 hand-made
    molecules of drug-like size against the one mnx_molfile_pack call that writes those files and against mnx_smiles_read on the
    same molecules' SMILES, then the worst files the reader admits, each alone in a call; `--molread-out FILE` writes the table
    to a file of its own.
(f) (only when asked for: --part f) condensed formulas on the device: mnx_formula_pack alone, against mnx_expand_pack on the same
    tables (the same frame: count, scan, fill, one workgroup per molecule), on the drug-like tables of part x and on those with a
    condensed formula in the place of every label; at the default step limit and at a limit of one step, where every search ends
    at its first placement: what the two differ by is the serial search lane
(n) (only when asked for: --part n) normalisation on the device: mnx_normalize_pack alone, against mnx_expand_pack on the same
    input tables (the same shape of pass), and followed by mnx_smiles_pack_canonical against the canonical writer on the tables
    as they came — on the synthetic checkpoint's predictions (near-complete graphs), on hand-made molecules of drug-like size
    with aromatic rings, and on those with the rings in Kekule form; and mnx_kekulize_pack, the inverse pass, on the same tables
    at the default step limit and at a limit of one step; `--normalize-out FILE` writes the table to a file of its own.
(k) (only when asked for: --part k) the main molecule on the device: mnx_main_pack alone, against mnx_expand_pack on the same
    tables (the neighbouring pass of the same three-launch shape), on the drug-like tables of part x and on those with every fifth
    bond record taken out, so that most molecules fall apart; `--main-out FILE` writes the table to a file of its own.
(p) (only when asked for: --part p) path fingerprints on the device: one mnx_fingerprint_pack call (one launch) against one
    mnx_smiles_pack_canonical call (four launches) on the same drug-like tables, at paths of up to 7 bonds and of up to 2, then
    one mnx_tanimoto call over the rows against their neighbours; `--fingerprint-out FILE` writes the table to a file of its own.
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


def result_bytes(m, pages, conf):
    """Result bytes per image copied to the host by predict_pipeline for one group of pages: dense (tokens, lengths, n_atoms,
    edges [, the score matrices cut to the group's largest atom count]) and packed (the records and the 16 bytes of totals)."""
    out = m.engine.predict(m._transform(pages), ref_batch=32, confidence=conf)
    n, T = out["tokens"].shape
    k = m.engine.max_atoms
    dense = n * (4 * T + 4 + 4 + k * k)
    full = dense + n * 8 * (k * k + k + 1)
    if conf:
        k_hi = int(out["n_atoms"].max())
        dense += n * 8 * (k_hi * k_hi + k_hi + 1)
    rec = m.engine.graph_pack(out)
    packed = 16 + rec["mols"].nbytes + rec["atoms"].nbytes + rec["bonds"].nbytes + len(rec["text"])
    return dense / n, (full if conf else dense) / n, packed / n


def part_b_packed(n, repeats, lines):
    """The facade's result side: dense against packed, alternating inside every repeat; the dense facade is the baseline."""
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    pages = [W.synthetic_page(i % 15) for i in range(n)]
    ms = {"dense": molnextr("synthetic", dev, max_batch=32, image_format="gray8"),
          "packed": molnextr("synthetic", dev, max_batch=32, image_format="gray8", packed_results=True)}
    variants = [(k, c) for c in (False, True) for k in ms]
    rate = {v: [] for v in variants}
    for k, c in variants:
        ms[k].predict_images(pages[:256], return_atoms_bonds=True, return_confidence=c, batch_size=32)
    for _ in range(repeats):
        for k, c in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms[k].predict_images(pages, return_atoms_bonds=True, return_confidence=c, batch_size=32)
            rate[(k, c)].append(n / (time.perf_counter() - t0))
    lines.append(f"(b2) predict_images(return_atoms_bonds=True) from {n} synthetic pages, batch_size 32, image_format gray8: "
                 "molecules/s   median [min .. max] | result bytes per image copied to the host")
    for c in (False, True):
        dense_b, full_b, packed_b = result_bytes(ms["dense"], pages[:1024], c)
        for k in ms:
            note = (f"{dense_b:9.0f} B ({full_b:.0f} B before the k_hi slice)" if k == "dense" else
                    f"{packed_b:9.0f} B (40 + 24 x atoms + 16 x bonds + text)")
            lines.append(f"  {k:6s} return_confidence={str(c):5s} {fmt(rate[(k, c)])} molecules/s | {note}")
    for c in (False, True):
        d, p = rate[("dense", c)], rate[("packed", c)]
        verdict = ("packed is faster than dense beyond the dense path's own spread" if min(p) > max(d) else
                   "packed is slower than dense beyond the dense path's own spread" if max(p) < min(d) else
                   "packed and dense overlap: no difference beyond the dense path's own spread")
        lines.append(f"  return_confidence={str(c):5s}: packed / dense median {statistics.median(p) / statistics.median(d):.3f} - {verdict}")
    for m in ms.values():
        m.engine.close()


def pack_only(calls):
    """`calls` mnx_graph_pack calls over the dense outputs of 1024 images with confidences, and nothing else on the GPU
    afterwards: run under a kernel trace, the three graph_* kernels of one call add up to its device time."""
    from molnextr_amd.model import molnextr
    m = molnextr("synthetic", torch.device("cuda", 0), max_batch=32, image_format="gray8")
    out = m.engine.predict(m._transform([W.synthetic_page(i % 15) for i in range(1024)]), ref_batch=32, confidence=True)
    for _ in range(calls):
        rec = m.engine.graph_pack(out)
    print(f"pack_only: {calls} calls over 1024 images, totals {rec['totals'].tolist()}")
    m.engine.close()


def part_m(n, repeats, lines):
    """Molfiles from the device: the three launches of one mnx_molfile_pack call over 1024 images between two events (the
    tables stay on the device, the output buffer has the exact size), then the facade with and without graph_molfile."""
    import ctypes as C
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    pages = [W.synthetic_page(i % 15) for i in range(n)]
    ms = {"packed": molnextr("synthetic", dev, max_batch=32, image_format="gray8", packed_results=True),
          "packed + molfile": molnextr("synthetic", dev, max_batch=32, image_format="gray8", graph_molfile=True)}
    eng = ms["packed"].engine
    rec = eng.graph_pack(eng.predict(ms["packed"]._transform(pages[:1024]), ref_batch=32), keep_device=True)
    files, data = eng.molfile_pack(rec)
    mols, atoms, bonds, text = rec["device"]
    na, nb, nt = (int(v) for v in rec["totals"][:3])
    files_d = torch.empty(len(files) * 16, dtype=torch.uint8, device=dev)
    out_d = torch.empty(len(data), dtype=torch.uint8, device=dev)
    totals_d = torch.empty(2, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    ms_call = []
    for i in range(repeats + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rc = eng.lib.mnx_molfile_pack(eng.h, ptr(mols), len(files), ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, None, ptr(files_d),
                                      ptr(out_d), len(data), ptr(totals_d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        b.record()
        torch.cuda.synchronize()
        assert rc == 0 and out_d.cpu().numpy().tobytes() == data
        if i >= 3:
            ms_call.append(a.elapsed_time(b) * 1000.0)
    lines.append(f"(m) one mnx_molfile_pack call over the packed tables of {len(files)} images ({na} atoms, {nb} bonds -> {len(data)} "
                 f"bytes of molfiles, {int((files['len'] == 0).sum())} molecules without one): device us between two events around "
                 "its three launches   median [min .. max]")
    lines.append(f"  mnx_molfile_pack {fmt(ms_call)} us")
    rate = {k: [] for k in ms}
    for m in ms.values():
        m.predict_images(pages[:256], batch_size=32)
    for _ in range(repeats):
        for k, m in ms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.predict_images(pages, batch_size=32)
            rate[k].append(n / (time.perf_counter() - t0))
    lines.append(f"    predict_images from {n} synthetic pages, batch_size 32, image_format gray8: molecules/s   median [min .. max]")
    for k in ms:
        lines.append(f"  {k:16s} {fmt(rate[k])} molecules/s")
    p, q = rate["packed"], rate["packed + molfile"]
    verdict = ("slower with molfiles beyond the packed facade's own spread" if max(q) < min(p) else
               "faster with molfiles beyond the packed facade's own spread" if min(q) > max(p) else
               "the two overlap: no difference beyond the packed facade's own spread")
    lines.append(f"  with molfiles / without, median {statistics.median(q) / statistics.median(p):.3f} - {verdict}")
    for m in ms.values():
        m.engine.close()


LABELS = (b"[OMe]", b"[Ph]", b"[tBu]", b"[CO2Et]", b"[NO2]", b"[Boc]")


def druglike_records(n_mols, seed=0, centres=False, labels=False, gem=False, kekule=False):
    """Packed records of n_mols hand-made molecules of drug-like size: a chain of 20 .. 40 atoms, every seventh atom starting
    an aromatic six-ring, a few hetero atoms and double bonds (about 1.1 bonds per atom) — (mols, atoms, bonds, text).
    centres: every [C@@H] of the chain also carries a methyl on a wedge or a dash that begins at it, and its chain bonds are
    single: a candidate centre of mnx_smiles_pack_stereo (the molecules are the same otherwise). labels: every ninth atom that is a
    plain 'C' becomes an abbreviation label of mnx_expand_pack, the six of LABELS in turn, or of the tuple passed as `labels`
    (the same molecules otherwise). gem
    (with centres): every third centre is a [C@@] with a second methyl — a gem-dimethyl carbon, which mnx_smiles_pack_symmetric
    drops — and every bond record carries its class in `rev` too, as mnx_graph_pack writes it (the older sets leave 0 there, so
    a bond whose ends the ranks swap is written '~' and no centre beside it is a candidate). kekule: the six-rings are drawn in
    Kekule form — upper-case atoms, double and single bonds in turn — for mnx_normalize_pack to perceive (the same molecules
    otherwise)."""
    from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE
    rng = np.random.default_rng(seed)
    mols = np.zeros(n_mols, MOL_DTYPE)
    A, B, text = [], [], bytearray()
    for b in range(n_mols):
        n = int(rng.integers(20, 41))
        syms, bonds = [b"C"] * n, {}
        for k in range(n - 1):
            bonds[(k, k + 1)] = 2 if rng.integers(0, 8) == 0 else 1
        for r in range(0, n - 5, 7):
            for k in range(r, r + 6):
                syms[k] = b"n" if rng.integers(0, 6) == 0 else b"c"
                bonds[(k, k + 1) if k < r + 5 else (r, r + 5)] = 4
        for k in range(n):
            if syms[k] == b"C" and rng.integers(0, 4) == 0:
                syms[k] = (b"N", b"O", b"[C@@H]", b"Cl")[int(rng.integers(0, 4))]
        if labels:
            for k in range(8, n, 9):
                if syms[k] == b"C":
                    syms[k] = (LABELS if labels is True else labels)[k // 9 % len(LABELS)]
        if kekule:
            for r in range(0, n - 5, 7):
                for k in range(r, r + 6):
                    syms[k] = syms[k].upper()
                    bonds[(k, k + 1) if k < r + 5 else (r, r + 5)] = 2 - (k - r) % 2
        xy = [(k % 64, k // 2 % 64) for k in range(n)]
        rev = {}
        if centres:
            for k in [k for k in range(n) if syms[k] == b"[C@@H]"]:
                for pair in ((k - 1, k), (k, k + 1)):
                    if pair in bonds:
                        bonds[pair] = 1
                bonds[(k, len(syms))] = 5 + k % 2
                rev[(k, len(syms))] = 6 - k % 2
                syms.append(b"C")
                xy.append((xy[k][0], (xy[k][1] + 3) % 64))
                if gem and k % 3 == 0:
                    syms[k] = b"[C@@]"
                    bonds[(k, len(syms))] = 1
                    syms.append(b"C")
                    xy.append(((xy[k][0] + 3) % 64, xy[k][1]))
        own = b"".join(syms)
        mols[b] = (len(A), len(syms), len(B), len(bonds), len(text), len(own), 0, 0, 0.0)
        off = 0
        for k, sym in enumerate(syms):
            A.append((off, len(sym), k, xy[k][0], xy[k][1], 0.0))
            off += len(sym)
        B += [(i, j, ty, rev.get((i, j), ty if gem else 0), 0.0) for (i, j), ty in sorted(bonds.items())]
        text += own
    return mols, np.array(A, ATOM_DTYPE), np.array(B, BOND_DTYPE), bytes(text)


def longest_ranking_records():
    """The two molecules on which the ranks of mnx_smiles_pack_canonical take longest, one molecule each: 999 identical isolated
    atoms (998 ties, each followed by one round) and a ring of 999 (two ties, about a thousand rounds) — [(name, records)]."""
    from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE
    out = []
    for name, pairs in (("999 identical isolated atoms", []), ("a ring of 999 atoms", [(k, k + 1) for k in range(998)] + [(0, 998)])):
        mols = np.zeros(1, MOL_DTYPE)
        mols[0] = (0, 999, 0, len(pairs), 0, 999, 0, 0, 0.0)
        atoms = np.array([(k, 1, k, k // 40, k % 40, 0.0) for k in range(999)], ATOM_DTYPE)
        bonds = np.array([(i, j, 1, 1, 0.0) for i, j in pairs], BOND_DTYPE).reshape(-1)
        out.append((name, {"mols": mols, "atoms": atoms, "bonds": bonds, "text": b"C" * 999}))
    return out


def part_s(repeats, lines):
    """Graph SMILES from the device: the three launches of one mnx_smiles_pack call over 1024 molecules between two events, next
    to mnx_molfile_pack and mnx_smiles_pack_stereo over the same tables (the tables stay on the device, the output buffers have
    the exact size) — on the synthetic checkpoint's predictions, on hand-made molecules of drug-like size, and on those with
    candidate centres."""
    import ctypes as C
    from molnextr_amd import engine as E
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    m = molnextr("synthetic", dev, max_batch=32, image_format="gray8", packed_results=True)
    eng = m.engine
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731

    def measure(rec, what):
        files, mol_data = eng.molfile_pack(rec)
        recs, order, data = eng.smiles_pack(rec)
        st_recs, _, st_data = eng.smiles_pack(rec, stereo=True)
        mols, atoms, bonds, text = rec["device"]
        n, na, nb, nt = len(recs), len(rec["atoms"]), len(rec["bonds"]), len(rec["text"])
        recs_d = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        order_d = torch.empty(max(na, 1), dtype=torch.int16, device=dev)
        out_d = {"mnx_smiles_pack": torch.empty(max(len(data), 1), dtype=torch.uint8, device=dev),
                 "mnx_molfile_pack": torch.empty(max(len(mol_data), 1), dtype=torch.uint8, device=dev),
                 "mnx_smiles_pack_stereo": torch.empty(max(len(st_data), 1), dtype=torch.uint8, device=dev)}
        totals_d = torch.empty(2, dtype=torch.int32, device=dev)
        calls = {"mnx_smiles_pack": lambda: eng.lib.mnx_smiles_pack(eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt,
                                                                    ptr(recs_d), ptr(order_d), ptr(out_d["mnx_smiles_pack"]), len(data),
                                                                    ptr(totals_d), stream()),
                 "mnx_molfile_pack": lambda: eng.lib.mnx_molfile_pack(eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, None,
                                                                      ptr(recs_d), ptr(out_d["mnx_molfile_pack"]), len(mol_data),
                                                                      ptr(totals_d), stream()),
                 "mnx_smiles_pack_stereo": lambda: eng.lib.mnx_smiles_pack_stereo(
                     eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, ptr(recs_d), ptr(order_d),
                     ptr(out_d["mnx_smiles_pack_stereo"]), len(st_data), ptr(totals_d), stream())}
        want = {"mnx_smiles_pack": data, "mnx_molfile_pack": mol_data, "mnx_smiles_pack_stereo": st_data}
        ez = {2: eng.smiles_pack(rec, double_bonds=True), 3: eng.smiles_pack(rec, stereo=True, double_bonds=True)}
        for marks, text_of in ((0, data), (1, st_data), (2, ez[2][2]), (3, ez[3][2])):       # mnx_smiles_pack_marks, every set of marks
            k = f"marks {marks}"
            out_d[k], want[k] = torch.empty(max(len(text_of), 1), dtype=torch.uint8, device=dev), text_of
            calls[k] = lambda marks=marks, k=k: eng.lib.mnx_smiles_pack_marks(
                eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, ptr(recs_d), ptr(order_d), ptr(out_d[k]), len(want[k]),
                ptr(totals_d), marks, stream())

        canon = hasattr(eng.lib, "mnx_smiles_pack_canonical")        # absent from a build of before the call existed
        if canon:                                                     # mnx_smiles_pack_canonical, every set of marks
            rank_d, class_d = torch.empty_like(order_d), torch.empty_like(order_d)
            cn = {marks: eng.smiles_pack(rec, stereo=bool(marks & 1), double_bonds=bool(marks & 2), canonical=True) for marks in range(4)}
            for marks in range(4):
                k = f"canonical {marks}"
                out_d[k], want[k] = torch.empty(max(len(cn[marks][2]), 1), dtype=torch.uint8, device=dev), cn[marks][2]
                calls[k] = lambda marks=marks, k=k: eng.lib.mnx_smiles_pack_canonical(
                    eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, ptr(recs_d), ptr(order_d), ptr(rank_d),
                    ptr(class_d), ptr(out_d[k]), len(want[k]), ptr(totals_d), marks, stream())

        sym = hasattr(eng.lib, "mnx_smiles_pack_symmetric")        # absent from a build of before the call existed
        if sym:                                                     # mnx_smiles_pack_symmetric, every set of marks
            marks_d = torch.empty(max(na, 1), dtype=torch.uint8, device=dev)
            sy = {marks: eng.smiles_pack(rec, stereo=bool(marks & 1), double_bonds=bool(marks & 2), canonical=True, symmetry=True)
                  for marks in range(4)}
            for marks in range(4):
                k = f"symmetric {marks}"
                out_d[k], want[k] = torch.empty(max(len(sy[marks][2]), 1), dtype=torch.uint8, device=dev), sy[marks][2]
                calls[k] = lambda marks=marks, k=k: eng.lib.mnx_smiles_pack_symmetric(
                    eng.h, ptr(mols), n, ptr(atoms), na, ptr(bonds), nb, ptr(text), nt, ptr(recs_d), ptr(order_d), ptr(rank_d),
                    ptr(class_d), ptr(marks_d), ptr(out_d[k]), len(want[k]), ptr(totals_d), marks, stream())

        def alternate(names):
            us = {k: [] for k in names}
            for i in range(repeats + 3):
                for k in names:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    rc = calls[k]()
                    b.record()
                    torch.cuda.synchronize()
                    assert rc == 0 and out_d[k][:len(want[k])].cpu().numpy().tobytes() == want[k]
                    if i >= 3:
                        us[k].append(a.elapsed_time(b) * 1000.0)
            return us

        us = alternate(("mnx_smiles_pack", "mnx_molfile_pack"))              # the plain pair, measured as before the stereo call existed
        pair = alternate(("mnx_smiles_pack", "mnx_smiles_pack_stereo"))      # then stereo against plain, in a pass of their own
        like0 = alternate(("marks 0", "mnx_molfile_pack"))                   # marks 0 and 1 measured the way the older calls are above
        like1 = alternate(("mnx_smiles_pack", "marks 1"))
        six = alternate(("mnx_smiles_pack", "mnx_smiles_pack_stereo", "marks 0", "marks 1", "marks 2", "marks 3"))   # and every set of marks
        eight = alternate(tuple(f"{c} {marks}" for marks in range(4) for c in ("marks", "canonical"))) if canon else None
        again = alternate(tuple(f"{c} {marks}" for marks in range(4) for c in ("canonical", "symmetric"))) if sym else None
        refused = (recs["flags"] & E.SMILES_REFUSED) != 0
        lines.append(f"(s) one call over the packed tables of {n} {what} ({na} atoms, {nb} bonds): device us between two events around "
                     "its three launches, the two calls alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:17s} {fmt(us[k])} us   -> {len(want[k])} bytes")
        lines.append("  stereo against plain, the two alternating in a pass of their own:")
        for k in pair:
            lines.append(f"  {k:22s} {fmt(pair[k])} us   -> {len(want[k])} bytes")
        lines.append(f"  stereo / plain, median {statistics.median(pair['mnx_smiles_pack_stereo']) / statistics.median(pair['mnx_smiles_pack']):.3f}; "
                     f"marks written: {st_data.count(b'@') - st_data.count(b'@@')} in {int((st_recs['flags'] & E.SMILES_STEREO != 0).sum())} "
                     f"molecules, unresolved in {int((st_recs['flags'] & E.SMILES_STEREO_UNRESOLVED != 0).sum())}, wedges still dropped in "
                     f"{int((st_recs['flags'] & E.SMILES_WEDGES_DROPPED != 0).sum())}")
        lines.append("  mnx_smiles_pack_marks, marks 0 alternating with mnx_molfile_pack and marks 1 with mnx_smiles_pack, as the older calls above:")
        lines.append(f"  {'marks 0':22s} {fmt(like0['marks 0'])} us   -> {len(want['marks 0'])} bytes")
        lines.append(f"  {'marks 1':22s} {fmt(like1['marks 1'])} us   -> {len(want['marks 1'])} bytes")
        lines.append("  mnx_smiles_pack_marks with every set of marks against the two older calls, the six alternating in a pass of their own:")
        for k in six:
            lines.append(f"  {k:22s} {fmt(six[k])} us   -> {len(want[k])} bytes")
        base = {2: statistics.median(six["mnx_smiles_pack"]), 3: statistics.median(six["mnx_smiles_pack_stereo"])}
        f2 = ez[2][0]["flags"]
        lines.append(f"  marks 2 / plain, median {statistics.median(six['marks 2']) / base[2]:.3f}; marks 3 / stereo, median "
                     f"{statistics.median(six['marks 3']) / base[3]:.3f}; '/' and '\\' written: {ez[2][2].count(b'/') + ez[2][2].count(bytes([92]))} in "
                     f"{int((f2 & E.SMILES_EZ != 0).sum())} molecules, a candidate unresolved in {int((f2 & E.SMILES_EZ_UNRESOLVED != 0).sum())}, "
                     f"a configuration implied in {int((f2 & E.SMILES_EZ_IMPLIED != 0).sum())}")
        if canon:
            lines.append("  mnx_smiles_pack_canonical (four launches) against mnx_smiles_pack_marks with the same marks, the eight alternating "
                         "in a pass of their own:")
            for k in eight:
                lines.append(f"  {k:22s} {fmt(eight[k])} us   -> {len(want[k])} bytes")
            ratios = []
            for marks in range(4):
                base_us = statistics.median(eight[f"marks {marks}"])
                r = [v / base_us for v in eight[f"canonical {marks}"]]
                ratios.append(f"marks {marks}: {statistics.median(r):.2f} [{min(r):.2f} .. {max(r):.2f}]")
            fc = cn[0][0]["flags"]
            lines.append("  canonical / marks, each run over the median of marks   median [min .. max]: " + "; ".join(ratios))
            lines.append(f"  a tie broken in {int((fc & E.SMILES_CANON_TIE != 0).sum())} molecules, one by the atom index alone in "
                         f"{int((fc & E.SMILES_CANON_TIE_INDEX != 0).sum())}; strings that differ from the uncanonical ones: "
                         f"{sum(cn[0][2][a:a + l] != data[b:b + l2] for a, l, b, l2 in zip(cn[0][0]['text0'].tolist(), cn[0][0]['len'].tolist(), recs['text0'].tolist(), recs['len'].tolist()))}")
        if sym:
            lines.append("  mnx_smiles_pack_symmetric against mnx_smiles_pack_canonical with the same marks (four launches each), the eight "
                         "alternating in a pass of their own:")
            for k in again:
                lines.append(f"  {k:22s} {fmt(again[k])} us   -> {len(want[k])} bytes")
            med = {k: statistics.median(v) for k, v in again.items()}
            spread = max(max(v) - min(v) for v in again.values())
            f3, bits = sy[3][0]["flags"], sy[3][5]
            lines.append(f"  symmetric - canonical, medians: " + "; ".join(f"marks {q}: {med[f'symmetric {q}'] - med[f'canonical {q}']:+.2f} us" for q in range(4)))
            lines.append(f"  the low pass at marks 1: symmetric 1 - canonical 1 = {med['symmetric 1'] - med['canonical 1']:+.2f} us against "
                         f"canonical 3 - canonical 1 = {med['canonical 3'] - med['canonical 1']:+.2f} us; the widest min .. max of the pass: {spread:.2f} us")
            lines.append(f"  marks 3: a mark dropped in {int((f3 & E.SMILES_SYM_DROPPED != 0).sum())} molecules ({int((bits == E.ATOM_MARK_SYM).sum())} centres, "
                         f"{int(((bits != E.ATOM_MARKS_NONE) & (bits & E.ATOM_EZ_SYM != 0)).sum()) // 2} double bonds), kept: "
                         f"{int(((bits != E.ATOM_MARKS_NONE) & (bits & 3 != 0)).sum())} centres, "
                         f"{int(((bits != E.ATOM_MARKS_NONE) & (bits & E.ATOM_EZ != 0)).sum()) // 2} double bonds; the rule is off (a pseudo-atom) in "
                         f"{int((f3 & E.SMILES_PSEUDO_ATOM != 0).sum())} molecules")
        lines.append(f"  graph SMILES written for {int((~refused).sum())} of {n} molecules ({int(((~refused) & (recs['len'] == 0)).sum())} of "
                     f"them empty), refused {int(refused.sum())}; ring bonds per molecule: median {int(np.median(recs['n_rings']))}, max "
                     f"{int(recs['n_rings'].max())}; molfiles refused: {int((files['len'] == 0).sum())}")
        for name in ("TOO_LARGE", "BEYOND_TABLES", "PSEUDO_ATOM", "TRUNCATED", "DUPLICATE_BOND", "RING_NUMBERS", "WEDGES_DROPPED", "UNKNOWN_BOND"):
            lines.append(f"    flag {name:15s} {int((recs['flags'] & getattr(E, 'SMILES_' + name) != 0).sum()):5d} molecules")
        sizes = sorted(int(k) for k in rec["mols"]["n_atoms"][~refused])
        if sizes:
            lines.append(f"    atoms of the written molecules: median {int(np.median(sizes))}, max {sizes[-1]}; the first string: "
                         f"{data[recs['text0'][~refused][0]:][:recs['len'][~refused][0]].decode()[:120]}")

    pages = [W.synthetic_page(i % 15) for i in range(1024)]
    measure(eng.graph_pack(eng.predict(m._transform(pages), ref_batch=32), keep_device=True), "images of the synthetic checkpoint")
    mols, atoms, bonds, text = druglike_records(1024)
    up = lambda a: torch.frombuffer(bytearray(a if isinstance(a, bytes) else a.tobytes()) + bytearray(8), dtype=torch.uint8).to(dev)   # noqa: E731
    measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text, "device": (up(mols), up(atoms), up(bonds), up(text))},
            "hand-made molecules of drug-like size")
    mols, atoms, bonds, text = druglike_records(1024, centres=True)
    measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text, "device": (up(mols), up(atoms), up(bonds), up(text))},
            "hand-made molecules of drug-like size with candidate centres")
    if hasattr(eng.lib, "mnx_smiles_pack_symmetric"):
        mols, atoms, bonds, text = druglike_records(1024, centres=True, gem=True)
        measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text, "device": (up(mols), up(atoms), up(bonds), up(text))},
                "hand-made molecules of drug-like size with candidate centres, every third a gem-dimethyl carbon")
    if hasattr(eng.lib, "mnx_smiles_pack_canonical"):
        lines.append("(s) mnx_smiles_pack_canonical on the two molecules that rank longest, one molecule (one workgroup) per call: device ms "
                     "between two events around the four launches   median [min .. max]")
        for name, rec in longest_ranking_records():
            ms = []
            for i in range(repeats + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                rec["device"] = eng._packed_tables(rec)[0]
                torch.cuda.synchronize()
                a.record()
                recs, order, data, rank, sym_class = eng.smiles_pack(rec, cap=2048, canonical=True)
                b.record()
                torch.cuda.synchronize()
                assert len(data) >= 999 and sorted(rank.tolist()) == list(range(999))
                if i:
                    ms.append(a.elapsed_time(b))
            lines.append(f"  {name:30s} {fmt(ms)} ms (with the copies of Engine.smiles_pack)   -> {len(data)} bytes, "
                         f"{len(set(sym_class.tolist()))} symmetry class")
    m.engine.close()


def dense_of_records(eng, tok, mols, atoms, bonds, text):
    """The dense arrays that mnx_graph_pack turns into these records: ids [n, T] (every atom's symbol, character by character, then
    its two coordinate bins; '<eos>'), lengths, the atom scan over them, and the bond classes as a [n, kmax, kmax] matrix."""
    dev = torch.device("cuda", eng.device)
    n, kmax, rows = len(mols), eng.max_atoms, []
    edges = np.zeros((n, kmax, kmax), np.uint8)
    for b, m in enumerate(mols):
        ids = []
        for a in atoms[m["atom0"]:m["atom0"] + m["n_atoms"]]:
            sym = text[m["text0"] + a["sym0"]:m["text0"] + a["sym0"] + a["sym_len"]].decode()
            ids += [tok.stoi[c] for c in sym] + [tok.offset + int(a["x_bin"]), tok.offset + tok.maxx + int(a["y_bin"])]
        rows.append(ids + [2])
        for x in bonds[m["bond0"]:m["bond0"] + m["n_bonds"]]:
            edges[b, x["i"], x["j"]], edges[b, x["j"], x["i"]] = x["type"], x["rev"]
    T = max(len(r) for r in rows) + 1
    assert T <= 512
    tokens = torch.tensor([r + [0] * (T - len(r)) for r in rows], dtype=torch.int32, device=dev)
    lengths = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    atom_idx, n_atoms = eng.atom_scan(tokens, lengths)
    return {"tokens": tokens, "lengths": lengths, "atom_idx": atom_idx, "n_atoms": n_atoms, "edges": torch.from_numpy(edges).to(dev)}


def part_x(repeats, lines):
    """Abbreviation expansion on the device: one mnx_expand_pack call (three launches) between two events, alternating with one
    mnx_graph_pack call that writes the same molecules from the dense arrays, with mnx_expand_pack followed by
    mnx_smiles_pack_canonical (marks 0), and with the canonical writer on the unexpanded tables. Every output buffer has the
    exact size; the tables stay on the device."""
    import ctypes as C
    from molnextr_amd import engine as E
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    m = molnextr("synthetic", dev, max_batch=32, image_format="gray8", packed_results=True)
    eng = m.engine
    tok = m.tokenizer["chartok_coords"]
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def measure(dense, what):
        rec = eng.graph_pack(dense, keep_device=True)
        ex = eng.expand_pack(rec, keep_device=True)
        n, T, kmax = dense["tokens"].shape[0], dense["tokens"].shape[1], dense["atom_idx"].shape[1]
        sizes = {"in": (len(rec["atoms"]), len(rec["bonds"]), len(rec["text"])), "out": (len(ex["atoms"]), len(ex["bonds"]), len(ex["text"]))}
        cn = {k: eng.smiles_pack(r, canonical=True) for k, r in (("in", rec), ("out", ex))}
        mols_d, totals_d = buf(n * 40), torch.empty(4, dtype=torch.int32, device=dev)
        tab = {k: (buf(v[0] * 24), buf(v[1] * 16), buf(v[2])) for k, v in sizes.items()}
        origin_d = torch.empty(max(sizes["out"][0], 1), dtype=torch.int16, device=dev)
        recs_d = buf(n * 16)
        words = [torch.empty(max(sizes["out"][0], 1), dtype=torch.int16, device=dev) for _ in range(3)]
        out_d = {k: buf(len(v[2])) for k, v in cn.items()}

        def graph_pack():
            a, b, t = tab["in"]
            return eng.lib.mnx_graph_pack(eng.h, ptr(dense["tokens"]), ptr(dense["lengths"]), n, T, ptr(dense["atom_idx"]),
                                          ptr(dense["n_atoms"]), ptr(dense["edges"]), kmax, None, None, None, ptr(mols_d), ptr(a),
                                          sizes["in"][0], ptr(b), sizes["in"][1], ptr(t), sizes["in"][2], ptr(totals_d), stream())

        def expand():
            i, (a, b, t) = rec["device"], tab["out"]
            return eng.lib.mnx_expand_pack(eng.h, ptr(i[0]), n, ptr(i[1]), sizes["in"][0], ptr(i[2]), sizes["in"][1], ptr(i[3]),
                                           sizes["in"][2], ptr(mols_d), ptr(a), sizes["out"][0], ptr(b), sizes["out"][1], ptr(t),
                                           sizes["out"][2], ptr(origin_d), ptr(totals_d), stream())

        def canonical(which, tables):
            return eng.lib.mnx_smiles_pack_canonical(eng.h, ptr(tables[0]), n, ptr(tables[1]), sizes[which][0], ptr(tables[2]),
                                                     sizes[which][1], ptr(tables[3]), sizes[which][2], ptr(recs_d), ptr(words[0]),
                                                     ptr(words[1]), ptr(words[2]), ptr(out_d[which]), len(cn[which][2]), ptr(totals_d),
                                                     0, stream())

        calls = {"mnx_graph_pack": graph_pack, "mnx_expand_pack": expand,
                 "canonical, unexpanded": lambda: canonical("in", rec["device"]),
                 "expand + canonical": lambda: expand() or canonical("out", (mols_d,) + tab["out"])}
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and not int(totals_d[-1] if k == "mnx_graph_pack" or k == "mnx_expand_pack" else totals_d[1]), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        assert tab["out"][0][:sizes["out"][0] * 24].cpu().numpy().tobytes() == ex["atoms"].tobytes()
        assert out_d["out"][:len(cn["out"][2])].cpu().numpy().tobytes() == cn["out"][2]
        flags = ex["mols"]["flags"]
        lines.append(f"(x) one call over {n} {what}: {sizes['in'][0]} atoms, {sizes['in'][1]} bonds -> {sizes['out'][0]} atoms, "
                     f"{sizes['out'][1]} bonds; expanded {int((flags & E.MOL_EXPANDED != 0).sum())} molecules, a label left in "
                     f"{int((flags & E.MOL_LABEL_LEFT != 0).sum())}, refused {int((flags & E.MOL_EXPAND_REFUSED != 0).sum())}")
        lines.append("  device us between two events around the launches, the four alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:24s} {fmt(us[k])} us")
        lines.append(f"  expand / graph_pack, median {statistics.median(us['mnx_expand_pack']) / statistics.median(us['mnx_graph_pack']):.2f}; "
                     f"(expand + canonical) / canonical, median "
                     f"{statistics.median(us['expand + canonical']) / statistics.median(us['canonical, unexpanded']):.2f}; canonical strings "
                     f"with a '*': {sum(b'*' in cn['in'][2][a:a + l] for a, l in zip(cn['in'][0]['text0'].tolist(), cn['in'][0]['len'].tolist()))}"
                     f" -> {sum(b'*' in cn['out'][2][a:a + l] for a, l in zip(cn['out'][0]['text0'].tolist(), cn['out'][0]['len'].tolist()))}")
        return rec

    pages = [W.synthetic_page(i % 15) for i in range(1024)]
    measure(eng.predict(m._transform(pages), ref_batch=32), "images of the synthetic checkpoint (near-complete graphs)")
    for labels, what in ((False, "hand-made molecules of drug-like size (no label: the pass copies)"),
                         (True, "hand-made molecules of drug-like size with a label at every ninth atom")):
        mols, atoms, bonds, text = druglike_records(1024, labels=labels)
        rec = measure(dense_of_records(eng, tok, mols, atoms, bonds, text), what)
        for key, want in (("mols", mols), ("atoms", atoms), ("bonds", bonds)):      # mnx_graph_pack wrote these very molecules
            for name in want.dtype.names:
                if name != "index":          # the decoder position of the atom, which hand-made records do not have
                    assert np.array_equal(rec[key][name], want[name]), (key, name)
        assert rec["text"] == text
    m.engine.close()


def part_n(repeats, lines):
    """Normalisation on the device: one mnx_normalize_pack call (three launches) between two events, alternating with one
    mnx_expand_pack call on the same input tables (the same shape of pass: count, scan, fill, one workgroup per molecule), with
    the canonical writer on the input and with normalize followed by the canonical writer, and with one mnx_kekulize_pack call
    (the same shape of pass again) at the default step limit and at a limit of one step, where every search ends at its second
    pairing: what the two differ by is the serial search lane. Every output buffer has the exact size; the tables stay on the
    device."""
    import ctypes as C
    from molnextr_amd import engine as E
    from molnextr_amd.model import molnextr
    dev = torch.device("cuda", 0)
    m = molnextr("synthetic", dev, max_batch=32, image_format="gray8", packed_results=True)
    eng = m.engine
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def measure(rec, what):
        tables, args = eng._packed_tables(rec)
        n = len(rec["mols"])
        ex, nz, kk = eng.expand_pack(rec), eng.normalize_pack(rec, keep_device=True), eng.kekulize_pack(rec)
        cn = {"in": eng.smiles_pack(rec, canonical=True), "out": eng.smiles_pack(nz, canonical=True)}
        sizes = {k: (len(r["atoms"]), len(r["bonds"]), len(r["text"])) for k, r in (("in", rec), ("x", ex), ("n", nz), ("k", kk))}
        mols_d, totals_d, totals_w = buf(n * 40), torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        tab = {k: (buf(sizes[k][0] * 24), buf(sizes[k][1] * 16), buf(sizes[k][2])) for k in ("x", "n", "k")}
        kek_notes_d = buf(sizes["k"][0])
        origin_d = torch.empty(max(sizes["x"][0], 1), dtype=torch.int16, device=dev)
        notes_d = buf(sizes["n"][0])
        recs_d = buf(n * 16)
        words = [torch.empty(max(sizes["n"][0], 1), dtype=torch.int16, device=dev) for _ in range(3)]
        out_d = buf(max(len(cn["in"][2]), len(cn["out"][2])))

        def table_pass(fn, k, extra):
            a, b, t = tab[k]
            return fn(eng.h, *args, ptr(mols_d), ptr(a), sizes[k][0], ptr(b), sizes[k][1], ptr(t), sizes[k][2], ptr(extra), ptr(totals_d), stream())

        def canonical(head, which):
            return eng.lib.mnx_smiles_pack_canonical(eng.h, *head, ptr(recs_d), ptr(words[0]), ptr(words[1]), ptr(words[2]), ptr(out_d),
                                                     len(cn[which][2]), ptr(totals_w), 0, stream())

        normal_head = [ptr(mols_d), n, ptr(tab["n"][0]), sizes["n"][0], ptr(tab["n"][1]), sizes["n"][1], ptr(tab["n"][2]), sizes["n"][2]]
        normalize = lambda: table_pass(eng.lib.mnx_normalize_pack, "n", notes_d)      # noqa: E731

        def kekulize(max_steps):
            a, b, t = tab["k"]
            return eng.lib.mnx_kekulize_pack(eng.h, *args, ptr(mols_d), ptr(a), sizes["k"][0], ptr(b), sizes["k"][1], ptr(t), sizes["k"][2],
                                             ptr(kek_notes_d), ptr(totals_d), max_steps, stream())

        calls = {"mnx_expand_pack": lambda: table_pass(eng.lib.mnx_expand_pack, "x", origin_d), "mnx_normalize_pack": normalize,
                 "canonical, as it came": lambda: canonical(args, "in"),
                 "normalize + canonical": lambda: normalize() or canonical(normal_head, "out"),
                 "mnx_kekulize_pack, 1 step": lambda: kekulize(1), "mnx_kekulize_pack": lambda: kekulize(0)}
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and not int(totals_d[3]) and not int(totals_w[1]), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        assert tab["n"][2][:sizes["n"][2]].cpu().numpy().tobytes() == nz["text"] and notes_d[:sizes["n"][0]].cpu().numpy().tobytes() == nz["atom_notes"].tobytes()
        assert out_d[:len(cn["out"][2])].cpu().numpy().tobytes() == cn["out"][2]
        assert tab["k"][2][:sizes["k"][2]].cpu().numpy().tobytes() == kk["text"] and kek_notes_d[:sizes["k"][0]].cpu().numpy().tobytes() == kk["atom_notes"].tobytes()
        flags, notes = nz["mols"]["flags"], nz["atom_notes"]
        lines.append(f"(n) one call over {n} {what}: {sizes['in'][0]} atoms, {sizes['in'][1]} bonds, {sizes['in'][2]} -> {sizes['n'][2]} bytes of "
                     f"text; aromatized {int((flags & E.MOL_AROMATIZED != 0).sum())} molecules ({int((notes & E.NOTE_AROMATIZED != 0).sum())} atoms), "
                     f"brackets removed in {int((flags & E.MOL_UNBRACKETED != 0).sum())}, refused {int((flags & E.MOL_NORMALIZE_REFUSED != 0).sum())}; "
                     f"the canonical writer refuses {int((cn['in'][0]['flags'] & E.SMILES_REFUSED != 0).sum())}")
        lines.append(f"    kekulized {int((kk['mols']['flags'] & E.MOL_KEKULIZED != 0).sum())} molecules ({int((kk['atom_notes'] & E.NOTE_KEKULIZED != 0).sum())} atoms), "
                     f"left aromatic in {int((kk['mols']['flags'] & E.MOL_KEKULE_LEFT != 0).sum())}, refused {int((kk['mols']['flags'] & E.MOL_KEKULIZE_REFUSED != 0).sum())}")
        lines.append("  device us between two events around the launches, the six alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:24s} {fmt(us[k])} us")
        lines.append(f"  normalize / expand, median {statistics.median(us['mnx_normalize_pack']) / statistics.median(us['mnx_expand_pack']):.2f}; "
                     f"(normalize + canonical) / canonical, median "
                     f"{statistics.median(us['normalize + canonical']) / statistics.median(us['canonical, as it came']):.2f}")
        ratios = sorted(k / z for k, z in zip(us["mnx_kekulize_pack"], us["mnx_normalize_pack"]))
        search = 1.0 - statistics.median(us["mnx_kekulize_pack, 1 step"]) / statistics.median(us["mnx_kekulize_pack"])
        lines.append(f"  kekulize / normalize, run by run: median {statistics.median(ratios):.2f} [{ratios[0]:.2f} .. {ratios[-1]:.2f}]; "
                     f"the search beyond its first step: {100.0 * search:.0f} % of the call")

    pages = [W.synthetic_page(i % 15) for i in range(1024)]
    measure(eng.graph_pack(eng.predict(m._transform(pages), ref_batch=32)), "images of the synthetic checkpoint (near-complete graphs)")
    for kekule, what in ((False, "hand-made molecules of drug-like size, rings aromatic already (the pass copies them)"),
                         (True, "hand-made molecules of drug-like size, rings in Kekule form")):
        mols, atoms, bonds, text = druglike_records(1024, kekule=kekule)
        measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}, what)
    m.engine.close()


# a label of druglike_records stands inside the chain, so each formula is spelled for two bonds; none is a table name
FORMULAS = (b"[CHOCH3]", b"[CHPh]", b"[CHC(CH3)3]", b"[CHCOOC2H5]", b"[NCH3]", b"[CHNHCOOC(CH3)3]")


def part_f(repeats, lines):
    """Condensed formulas on the device: one mnx_formula_pack call (three launches) between two events, alternating with one
    mnx_expand_pack call on the same input tables, at the default step limit and at a limit of one step. Every output buffer has
    the exact size; the tables stay on the device."""
    import ctypes as C
    from molnextr_amd import engine as E
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def measure(rec, what):
        tables, args = eng._packed_tables(rec)
        n = len(rec["mols"])
        out = {"x": eng.expand_pack(rec), "f": eng.formula_pack(rec), "f1": eng.formula_pack(rec, max_steps=1)}
        sizes = {k: (len(r["atoms"]), len(r["bonds"]), len(r["text"])) for k, r in out.items()}
        mols_d, totals_d = buf(n * 40), torch.zeros(4, dtype=torch.int32, device=dev)
        tab = {k: (buf(v[0] * 24), buf(v[1] * 16), buf(v[2])) for k, v in sizes.items()}
        origin_d = torch.empty(max(max(v[0] for v in sizes.values()), 1), dtype=torch.int16, device=dev)

        def table_pass(fn, k, *tail):
            a, b, t = tab[k]
            return fn(eng.h, *args, ptr(mols_d), ptr(a), sizes[k][0], ptr(b), sizes[k][1], ptr(t), sizes[k][2], ptr(origin_d), ptr(totals_d),
                      *tail, stream())

        calls = {"mnx_expand_pack": lambda: table_pass(eng.lib.mnx_expand_pack, "x"),
                 "mnx_formula_pack, 1 step": lambda: table_pass(eng.lib.mnx_formula_pack, "f1", 1),
                 "mnx_formula_pack": lambda: table_pass(eng.lib.mnx_formula_pack, "f", 0)}
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and not int(totals_d[3]), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        assert tab["f"][0][:sizes["f"][0] * 24].cpu().numpy().tobytes() == out["f"]["atoms"].tobytes()
        assert tab["f"][2][:sizes["f"][2]].cpu().numpy().tobytes() == out["f"]["text"]
        flags = out["f"]["mols"]["flags"]
        lines.append(f"(f) one call over {n} {what}: {len(rec['atoms'])} atoms, {len(rec['bonds'])} bonds -> {sizes['f'][0]} atoms, "
                     f"{sizes['f'][1]} bonds; a formula replaced in {int((flags & E.MOL_FORMULA_EXPANDED != 0).sum())} molecules, left in "
                     f"{int((flags & E.MOL_FORMULA_LEFT != 0).sum())}, step limit in {int((flags & E.MOL_FORMULA_LIMIT != 0).sum())}, refused "
                     f"{int((flags & E.MOL_FORMULA_REFUSED != 0).sum())}; mnx_expand_pack on the same tables -> {sizes['x'][0]} atoms")
        lines.append("  device us between two events around the launches, the three alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:24s} {fmt(us[k])} us")
        search = 1.0 - statistics.median(us["mnx_formula_pack, 1 step"]) / statistics.median(us["mnx_formula_pack"])
        lines.append(f"  formula / expand, median {statistics.median(us['mnx_formula_pack']) / statistics.median(us['mnx_expand_pack']):.2f}; "
                     f"the searches beyond their first step: {100.0 * search:.0f} % of the call")

    for labels, what in ((False, "hand-made molecules of drug-like size (no label: both passes copy)"),
                         (True, "hand-made molecules of drug-like size with a table label at every ninth atom (the formula pass copies)"),
                         (FORMULAS, "hand-made molecules of drug-like size with a condensed formula at every ninth atom (expand copies)")):
        mols, atoms, bonds, text = druglike_records(1024, labels=labels)
        measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}, what)
    eng.close()


def part_k(repeats, lines):
    """The main molecule on the device: one mnx_main_pack call (three launches) between two events, alternating with one
    mnx_expand_pack call on the same input tables. Every output buffer has the exact size; the tables stay on the device."""
    import ctypes as C
    from molnextr_amd import engine as E
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def measure(rec, what):
        tables, args = eng._packed_tables(rec)
        n = len(rec["mols"])
        out = {"x": eng.expand_pack(rec), "k": eng.main_pack(rec)}
        sizes = {k: (len(r["atoms"]), len(r["bonds"]), len(r["text"])) for k, r in out.items()}
        mols_d, totals_d = buf(n * 40), torch.zeros(4, dtype=torch.int32, device=dev)
        tab = {k: (buf(v[0] * 24), buf(v[1] * 16), buf(v[2])) for k, v in sizes.items()}
        origin_d = torch.empty(max(max(v[0] for v in sizes.values()), 1), dtype=torch.int16, device=dev)

        def table_pass(fn, k):
            a, b, t = tab[k]
            return fn(eng.h, *args, ptr(mols_d), ptr(a), sizes[k][0], ptr(b), sizes[k][1], ptr(t), sizes[k][2], ptr(origin_d), ptr(totals_d),
                      stream())

        calls = {"mnx_expand_pack": lambda: table_pass(eng.lib.mnx_expand_pack, "x"),
                 "mnx_main_pack": lambda: table_pass(eng.lib.mnx_main_pack, "k")}
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and not int(totals_d[3]), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        assert tab["k"][0][:sizes["k"][0] * 24].cpu().numpy().tobytes() == out["k"]["atoms"].tobytes()
        assert tab["k"][1][:sizes["k"][1] * 16].cpu().numpy().tobytes() == out["k"]["bonds"].tobytes()
        flags = out["k"]["mols"]["flags"]
        lines.append(f"(k) one call over {n} {what}: {len(rec['atoms'])} atoms, {len(rec['bonds'])} bonds -> {sizes['k'][0]} atoms, "
                     f"{sizes['k'][1]} bonds; atoms dropped in {int((flags & E.MOL_MAIN_KEPT != 0).sum())} molecules, a tie in "
                     f"{int((flags & E.MOL_MAIN_TIE != 0).sum())}, refused {int((flags & E.MOL_MAIN_REFUSED != 0).sum())}")
        lines.append("  device us between two events around the launches, the two alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:24s} {fmt(us[k])} us")
        lines.append(f"  main / expand, median {statistics.median(us['mnx_main_pack']) / statistics.median(us['mnx_expand_pack']):.2f}")

    def thinned(mols, atoms, bonds, text, every=5):
        """the same tables without every fifth bond record of a molecule: most molecules fall into several components"""
        mols, keep = mols.copy(), np.ones(len(bonds), bool)
        for m in mols:
            keep[int(m["bond0"]) + every - 1:int(m["bond0"]) + int(m["n_bonds"]):every] = False
        at = np.concatenate([[0], np.cumsum(keep)])
        first, last = mols["bond0"].astype(np.int64), mols["bond0"].astype(np.int64) + mols["n_bonds"]
        mols["bond0"], mols["n_bonds"] = at[first], at[last] - at[first]
        return mols, atoms, bonds[keep], text

    for labels, thin, what in ((False, False, "hand-made molecules of drug-like size (one component: the pass copies)"),
                               (True, False, "hand-made molecules of drug-like size with a table label at every ninth atom"),
                               (False, True, "hand-made molecules of drug-like size without every fifth bond record")):
        mols, atoms, bonds, text = druglike_records(1024, labels=labels)
        if thin:
            mols, atoms, bonds, text = thinned(mols, atoms, bonds, text)
        measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}, what)
    eng.close()


def part_p(repeats, lines):
    """Path fingerprints on the device: one mnx_fingerprint_pack call between two events, alternating with one
    mnx_smiles_pack_canonical call on the same input tables, and one mnx_tanimoto call over the rows it wrote."""
    import ctypes as C
    from molnextr_amd import engine as E
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def measure(rec, what):
        tables, args = eng._packed_tables(rec)
        n, na = len(rec["mols"]), len(rec["atoms"])
        want, written = eng.fingerprint_pack(rec), eng.smiles_pack(rec, canonical=True)
        fp_d, bits_d = buf(n * 16), torch.empty((n, E.FP_WORDS), dtype=torch.int32, device=dev)
        recs_d, out_d, totals_w = buf(n * 16), buf(len(written[2])), torch.zeros(2, dtype=torch.int32, device=dev)
        words = [torch.empty(max(na, 1), dtype=torch.int16, device=dev) for _ in range(3)]
        both_d, either_d = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        sim_d = torch.empty(n, dtype=torch.float64, device=dev)
        turned_d = torch.roll(torch.from_numpy(want["bits"].view(np.int32)).to(dev), 1, 0).contiguous()

        def fingerprint(max_bonds):
            return eng.lib.mnx_fingerprint_pack(eng.h, *args, ptr(fp_d), ptr(bits_d), max_bonds, 0, stream())

        calls = {"mnx_smiles_pack_canonical": lambda: eng.lib.mnx_smiles_pack_canonical(
                     eng.h, *args, ptr(recs_d), ptr(words[0]), ptr(words[1]), ptr(words[2]), ptr(out_d), len(written[2]), ptr(totals_w), 0, stream()),
                 "mnx_fingerprint_pack, 2 bonds": lambda: fingerprint(2), "mnx_fingerprint_pack": lambda: fingerprint(0),
                 "mnx_tanimoto": lambda: eng.lib.mnx_tanimoto(eng.h, ptr(bits_d), ptr(turned_d), n, ptr(both_d), ptr(either_d), ptr(sim_d), stream())}
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0, k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        assert bits_d.cpu().numpy().view(np.uint32).tobytes() == want["bits"].tobytes() and not int(totals_w[1])
        fp = want["fp"]
        lines.append(f"(p) one call over {n} {what}: {na} atoms, {len(rec['bonds'])} bonds; bits set per molecule median "
                     f"{int(np.median(fp['n_bits']))} [{int(fp['n_bits'].min())} .. {int(fp['n_bits'].max())}], most paths from one directed "
                     f"bond {int(fp['max_paths'].max())}, limited {int((fp['flags'] & E.FP_LIMIT != 0).sum())}, refused "
                     f"{int((fp['flags'] & E.FP_REFUSED != 0).sum())}; mean similarity to the neighbouring row {float(sim_d.mean()):.3f}")
        lines.append("  device us between two events around the launches, the four alternating   median [min .. max]")
        for k in us:
            lines.append(f"  {k:30s} {fmt(us[k])} us")
        lines.append(f"  fingerprint / canonical writer, median {statistics.median(us['mnx_fingerprint_pack']) / statistics.median(us['mnx_smiles_pack_canonical']):.2f}")

    for labels, what in ((False, "hand-made molecules of drug-like size"),
                         (True, "hand-made molecules of drug-like size with a table label at every ninth atom")):
        mols, atoms, bonds, text = druglike_records(1024, labels=labels)
        measure({"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}, what)
    eng.close()


def part_r(repeats, lines):
    """SMILES read on the device: one mnx_smiles_read call (three launches) over the strings of 1024 hand-made molecules of
    drug-like size between two events, alternating with the one mnx_smiles_pack call that writes those strings from the packed
    tables; then the worst strings the reader admits, each alone in a call (one workgroup), against a call on "C"."""
    import ctypes as C
    from molnextr_amd import engine as E
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def timed(calls, check):
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and check(k), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        return us

    def reader(strings):
        """(the call on exact-size buffers, its totals tensor, the result of Engine.smiles_read)"""
        got = eng.smiles_read(strings)
        arena = b"".join(strings)
        offsets = np.zeros(len(strings) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(x) for x in strings])
        d_bytes = torch.frombuffer(bytearray(arena), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int32)).to(dev)
        n, (na, nb, nt) = len(strings), (int(v) for v in got["totals"][:3])
        keep = (d_bytes, d_off, buf(n * 40), buf(n * 16), buf(na * 24), buf(nb * 16), buf(nt), torch.empty(4, dtype=torch.int32, device=dev))

        def call():
            return eng.lib.mnx_smiles_read(eng.h, ptr(keep[0]), len(arena), ptr(keep[1]), n, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), na,
                                           ptr(keep[5]), nb, ptr(keep[6]), nt, ptr(keep[7]), stream())
        return call, keep, got

    mols, atoms, bonds, text = druglike_records(1024)
    rec = {"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}
    tables, args = eng._packed_tables(rec)
    recs, order, data = eng.smiles_pack(rec)
    strings = [data[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in recs]
    recs_d, order_d, out_d = buf(len(mols) * 16), torch.empty(len(atoms), dtype=torch.int16, device=dev), buf(len(data))
    totals_w = torch.empty(2, dtype=torch.int32, device=dev)
    read, keep, got = reader(strings)
    assert not got["read"]["flags"].any() and got["mols"]["n_atoms"].tolist() == mols["n_atoms"].tolist()
    us = timed({"mnx_smiles_pack": lambda: eng.lib.mnx_smiles_pack(eng.h, *args, ptr(recs_d), ptr(order_d), ptr(out_d), len(data), ptr(totals_w), stream()),
                "mnx_smiles_read": read}, lambda k: not int(totals_w[1] if k == "mnx_smiles_pack" else keep[7][3]))
    assert out_d.cpu().numpy().tobytes() == data and keep[6].cpu().numpy().tobytes() == got["text"]
    lines.append(f"(r) one call over {len(mols)} hand-made molecules of drug-like size: {len(atoms)} atoms, {len(bonds)} bonds, {len(data)} "
                 f"bytes of SMILES (mnx_smiles_pack writes them, mnx_smiles_read reads those very strings back)")
    lines.append("  device us between two events around the launches, the two alternating   median [min .. max]")
    for k in us:
        lines.append(f"  {k:18s} {fmt(us[k])} us")
    lines.append(f"  read / write, median {statistics.median(us['mnx_smiles_read']) / statistics.median(us['mnx_smiles_pack']):.2f}")
    worst = {"one atom: C": b"C",
             "4096 bytes of chain, 586 atoms": b"[13CH2]" * 585 + b"C",
             "4096 bytes of nesting, 682 deep": b"[CH](" * 682 + b"[CH]" + b")" * 682,
             "99 ring numbers open at one atom, 677 bytes": b"C" + b"".join(b"%d" % r for r in range(1, 10)) + b"".join(b"%%%02d" % r for r in range(10, 100)) + b"N" + b"".join(b"C%%%02d" % r for r in range(1, 100)),
             "999 atoms in one ring, 999 bonds": b"C1" + b"C" * 997 + b"C1"}
    calls, keeps = {}, {}
    for k, s in worst.items():
        calls[k], keeps[k], got = reader([s])
        assert not int(got["read"]["flags"][0]) & E.READ_REFUSED, (k, got["read"])
        lines.append(f"  {k}: {len(s)} bytes -> {int(got['mols']['n_atoms'][0])} atoms, {int(got['mols']['n_bonds'][0])} bonds, {int(got['read']['n_rings'][0])} ring bonds")
    us = timed(calls, lambda k: not int(keeps[k][7][3]))
    lines.append("  one string per call (one workgroup of 256 in count and in fill, three launches)   median [min .. max]")
    base = statistics.median(us["one atom: C"])
    for k in us:
        lines.append(f"  {k:46s} {fmt(us[k])} us   {statistics.median(us[k]) - base:+.1f} us against one atom")
    eng.close()


def part_v(repeats, lines):
    """Molfile read on the device: one mnx_molfile_read call (three launches) over the V2000 molfiles of 1024 hand-made molecules
    of drug-like size between two events, alternating with the one mnx_molfile_pack call that writes those files and with
    mnx_smiles_read on the SMILES of the same molecules; then the worst files the reader admits, each alone in a call."""
    import ctypes as C
    from molnextr_amd import engine as E
    dev = torch.device("cuda", 0)
    ck = W.synthetic_checkpoint(0)
    eng = Engine(ck["encoder"], ck["decoder"], device=0, max_batch=2)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    buf = lambda k: torch.empty(max(int(k), 1), dtype=torch.uint8, device=dev)      # noqa: E731

    def timed(calls, check):
        us = {k: [] for k in calls}
        for i in range(repeats + 3):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                rc = call()
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and check(k), k
                if i >= 3:
                    us[k].append(a.elapsed_time(b) * 1000.0)
        return us

    def reader(texts, molfiles):
        """(the call on exact-size buffers, its buffers, the result of Engine.molfile_read or Engine.smiles_read)"""
        got = eng.molfile_read(texts) if molfiles else eng.smiles_read(texts)
        arena = b"".join(texts)
        offsets = np.zeros(len(texts) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(x) for x in texts])
        d_bytes = torch.frombuffer(bytearray(arena), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(offsets.view(np.int32)).to(dev)
        n, (na, nb, nt) = len(texts), (int(v) for v in got["totals"][:3])
        keep = (d_bytes, d_off, buf(n * 40), buf(n * 16), buf(na * 24), buf(nb * 16), buf(nt), torch.empty(4, dtype=torch.int32, device=dev))
        tail = (ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), na, ptr(keep[5]), nb, ptr(keep[6]), nt, ptr(keep[7]))

        def call():
            if molfiles:
                return eng.lib.mnx_molfile_read(eng.h, ptr(keep[0]), len(arena), ptr(keep[1]), n, None, 0, *tail, stream())
            return eng.lib.mnx_smiles_read(eng.h, ptr(keep[0]), len(arena), ptr(keep[1]), n, *tail, stream())
        return call, keep, got

    mols, atoms, bonds, text = druglike_records(1024)
    rec = {"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}
    tables, args = eng._packed_tables(rec)
    files, data = eng.molfile_pack(rec)
    texts = [data[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in files]
    srecs, _, sdata = eng.smiles_pack(rec)
    strings = [sdata[int(r["text0"]):int(r["text0"]) + int(r["len"])] for r in srecs]
    files_d, out_d, totals_w = buf(len(mols) * 16), buf(len(data)), torch.empty(2, dtype=torch.int32, device=dev)
    read, keep, got = reader(texts, True)
    sread, skeep, sgot = reader(strings, False)
    assert not (got["read"]["flags"] & E.MOLREAD_REFUSED).any() and got["mols"]["n_atoms"].tolist() == mols["n_atoms"].tolist()
    assert got["mols"]["n_bonds"].tolist() == mols["n_bonds"].tolist() and got["atoms"]["x_bin"].tolist() == atoms["x_bin"].tolist()
    us = timed({"mnx_molfile_pack": lambda: eng.lib.mnx_molfile_pack(eng.h, *args, None, ptr(files_d), ptr(out_d), len(data), ptr(totals_w), stream()),
                "mnx_molfile_read": read, "mnx_smiles_read": sread},
               lambda k: not int(totals_w[1] if k == "mnx_molfile_pack" else (keep if k == "mnx_molfile_read" else skeep)[7][3]))
    assert out_d.cpu().numpy().tobytes() == data and keep[6].cpu().numpy().tobytes() == got["text"]
    lines.append(f"(v) one call over {len(mols)} hand-made molecules of drug-like size: {len(atoms)} atoms, {len(bonds)} bonds, {len(data)} bytes "
                 f"of molfiles (mnx_molfile_pack writes them, mnx_molfile_read reads those very files back), {len(sdata)} bytes of SMILES")
    lines.append("  device us between two events around the launches, the three alternating   median [min .. max]")
    for k in us:
        lines.append(f"  {k:18s} {fmt(us[k])} us")
    lines.append(f"  read / write, median {statistics.median(us['mnx_molfile_read']) / statistics.median(us['mnx_molfile_pack']):.2f}; "
                 f"molfile read / SMILES read, median {statistics.median(us['mnx_molfile_read']) / statistics.median(us['mnx_smiles_read']):.2f}")
    atom = b"    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0"
    head = lambda na, nb: b"\n\n\n%3d%3d  0  0  0  0  0  0  0  0999 V2000\n" % (na, nb)      # noqa: E731
    ring = b"".join(b"%3d%3d  1  0\n" % (k + 1, (k + 1) % 999 + 1) for k in range(999))
    small = head(1, 0) + atom + b"\nM  END\n"
    full = head(999, 999) + (atom + b"\n") * 999 + ring + b"".join(b"A  %3d\nlabel%d\n" % (k + 1, k) for k in range(999)) + b"M  END\n"
    many = head(1, 0) + atom + b"\n" + b"G\n" * (8192 - 6) + b"M  END\n"
    worst = {"one atom": small,
             "999 atoms, 999 bonds, 999 aliases": full,
             "8192 lines": many,
             "262144 bytes, the molecule behind a first line of 100 KB": b"x" * 100000 + full + b"y" * (262144 - 100000 - len(full))}
    assert all(len(s) <= 262144 for s in worst.values()) and len(worst["262144 bytes, the molecule behind a first line of 100 KB"]) == 262144
    calls, keeps = {}, {}
    for k, s in worst.items():
        calls[k], keeps[k], got = reader([s], True)
        assert not int(got["read"]["flags"][0]) & E.MOLREAD_REFUSED, (k, got["read"])
        lines.append(f"  {k}: {len(s)} bytes, {s.count(10)} lines -> {int(got['mols']['n_atoms'][0])} atoms, {int(got['mols']['n_bonds'][0])} bonds, "
                     f"{int(got['mols']['smiles_len'][0])} bytes of symbols")
    us = timed(calls, lambda k: not int(keeps[k][7][3]))
    lines.append("  one file per call (one workgroup of 256 in count and in fill, three launches)   median [min .. max]")
    base = statistics.median(us["one atom"])
    for k in us:
        lines.append(f"  {k:58s} {fmt(us[k])} us   {statistics.median(us[k]) - base:+.1f} us against one atom")
    eng.close()


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
    ap.add_argument("--pack-out", default=None, help="write the dense-against-packed table of part b to this file")
    ap.add_argument("--molfile-out", default=None, help="write the table of part m to this file")
    ap.add_argument("--smiles-out", default=None, help="write the table of part s to this file")
    ap.add_argument("--expand-out", default=None, help="write the table of part x to this file")
    ap.add_argument("--read-out", default=None, help="write the table of part r to this file")
    ap.add_argument("--molread-out", default=None, help="write the table of part v to this file")
    ap.add_argument("--normalize-out", default=None, help="write the table of part n to this file")
    ap.add_argument("--formula-out", default=None, help="write the table of part f to this file")
    ap.add_argument("--main-out", default=None, help="write the table of part k to this file")
    ap.add_argument("--fingerprint-out", default=None, help="write the table of part p to this file")
    ap.add_argument("--pack-only", type=int, default=0, help="run this many mnx_graph_pack calls over 1024 images and exit")
    args = ap.parse_args()
    parts = args.part.split(",")
    if args.pack_only:
        pack_only(args.pack_only)
        return
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
        first = len(lines)
        part_b_packed(args.facade_pages, args.repeats, lines)
        if args.pack_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.pack_out)), exist_ok=True)
            with open(args.pack_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "m" in parts:
        first = len(lines)
        part_m(args.facade_pages, args.repeats, lines)
        if args.molfile_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.molfile_out)), exist_ok=True)
            with open(args.molfile_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "s" in parts:
        first = len(lines)
        part_s(args.repeats, lines)
        if args.smiles_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.smiles_out)), exist_ok=True)
            with open(args.smiles_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "x" in parts:
        first = len(lines)
        part_x(args.repeats, lines)
        if args.expand_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.expand_out)), exist_ok=True)
            with open(args.expand_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "r" in parts:
        first = len(lines)
        part_r(args.repeats, lines)
        if args.read_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.read_out)), exist_ok=True)
            with open(args.read_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "v" in parts:
        first = len(lines)
        part_v(args.repeats, lines)
        if args.molread_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.molread_out)), exist_ok=True)
            with open(args.molread_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "n" in parts:
        first = len(lines)
        part_n(args.repeats, lines)
        if args.normalize_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.normalize_out)), exist_ok=True)
            with open(args.normalize_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "f" in parts:
        first = len(lines)
        part_f(args.repeats, lines)
        if args.formula_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.formula_out)), exist_ok=True)
            with open(args.formula_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "k" in parts:
        first = len(lines)
        part_k(args.repeats, lines)
        if args.main_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.main_out)), exist_ok=True)
            with open(args.main_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    if "p" in parts:
        first = len(lines)
        part_p(args.repeats, lines)
        if args.fingerprint_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.fingerprint_out)), exist_ok=True)
            with open(args.fingerprint_out, "w") as f:
                f.write("\n".join([lines[0]] + lines[first:]) + "\n")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
