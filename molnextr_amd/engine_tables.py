"""The packed-table layer of `class Engine` (engine.py), the Python side of csrc/engine_tables.hip: graph_pack, the two writers,
the five passes from tables to tables, the fingerprint, tanimoto, the nearest-row search, the substructure search and the two
readers. A new pass adds
its method here (one line over _tables_pass), its prototype and flags to abi.py and its row to chain.PASSES."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .abi import (ATOM_DTYPE, BOND_DTYPE, FP_DTYPE, FP_WORDS, MATCH_DTYPE, MATCH_MAX_QUERY, MOL_DTYPE, MOLFILE_DTYPE, MOLREAD_DTYPE,
                  NEAREST_MAX_K, NEAREST_MAX_QUERIES, NEAREST_MAX_ROWS, NEAREST_SKIP_SELF, READ_DTYPE, SMILES_DTYPE, SMILES_MARK_DOUBLE_BOND, SMILES_MARK_TETRAHEDRAL, MnxError, _ptr, _stream)


class TableCalls:
    """A base of Engine, no object of its own: a plain class without __init__. Of the engine its methods use self.lib, self.h,
    self.device and self._check, and nothing else; the class attributes they read (PACK_GUESS, MOLFILE_GUESS, SMILES_GUESS and
    the GROWS / SELECTS / RESPELLS rows) are defined here."""

    # modest first capacities of graph_pack per image (a drug-like molecule has 20-40 heavy atoms, about as many bonds and a
    # SMILES of well under 200 bytes); `totals` sizes the one repeat when a job needs more
    PACK_GUESS = (48, 56, 192)

    def graph_pack(self, out: dict, caps=None, keep_device: bool = False) -> dict:
        """predict's result dict (device tensors) -> the molecules as numpy structured arrays (mnx_graph_pack): {'mols'
        [n] MOL_DTYPE, 'atoms' ATOM_DTYPE, 'bonds' BOND_DTYPE, 'text' bytes, 'totals' uint32 [4]}. With 'atom_scores',
        'edge_scores' and 'overall_score' in `out` the records carry the confidences, otherwise zeros. One D2H copy per table
        (plus the 16 bytes of totals); starts from PACK_GUESS per image (or caps = (atom_cap, bond_cap, text_cap)) and
        repeats at most once with the sizes `totals` reports. keep_device: also 'device' = the four tables as the uint8 device
        tensors they were written to, for molfile_pack and smiles_pack."""
        tokens, lengths = out["tokens"], out["lengths"]
        n, T = tokens.shape
        kmax = out["atom_idx"].shape[1]
        dev = tokens.device
        scored = out.get("edge_scores") is not None
        sc = [out["atom_scores"], out["edge_scores"], out["overall_score"]] if scored else [None, None, None]
        head = [_ptr(tokens), _ptr(lengths), n, T, _ptr(out["atom_idx"]), _ptr(out["n_atoms"]), _ptr(out["edges"]), kmax,
                _ptr(sc[0]), _ptr(sc[1]), _ptr(sc[2])]
        return self._sized_tables("mnx_graph_pack", n, caps if caps is not None else tuple(n * g for g in self.PACK_GUESS),
                                  lambda mols, arenas, totals: self.lib.mnx_graph_pack(self.h, *head, mols, *arenas, totals, _stream()),
                                  dev, keep_device)

    def _sized_tables(self, fn: str, n: int, caps, call, dev, keep_device: bool, side=None) -> dict:
        """One table writer over n molecules at capacities caps = (atom_cap, bond_cap, text_cap) and at most once more with
        the sizes `totals` reports: {'mols' [n] MOL_DTYPE, 'atoms' ATOM_DTYPE, 'bonds' BOND_DTYPE, 'text' bytes, 'totals'
        uint32 [4]}, keep_device: plus 'device' = the four tables as the uint8 device tensors they were written to.
        call(mols, arenas, totals) makes the library call lib.<fn> for one set of arenas and returns its code: mols and
        totals are pointers, arenas = [atoms, atom_cap, bonds, bond_cap, text, text_cap] as the three writers take them. side: the
        torch dtype of an output per atom (expand_pack's `origin`, the `atom_notes`), allocated at every attempt's atom capacity:
        call takes its pointer as a fourth argument, and 'side' is the last attempt's, one element per atom, on the device."""
        mols = torch.empty(n * MOL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        caps = tuple(int(c) for c in caps)
        for attempt in range(2):
            atoms = torch.empty(max(caps[0], 1) * ATOM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            bonds = torch.empty(max(caps[1], 1) * BOND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            text = torch.empty(max(caps[2], 1), dtype=torch.uint8, device=dev)
            arenas = [_ptr(atoms), caps[0], _ptr(bonds), caps[1], _ptr(text), caps[2]]
            per_atom = [] if side is None else [torch.empty(max(caps[0], 1), dtype=side, device=dev)]
            self._check(call(_ptr(mols), arenas, _ptr(totals), *map(_ptr, per_atom)), fn)
            tot = totals.cpu().numpy().view(np.uint32)
            if not tot[3]:
                break
            if attempt:
                raise MnxError(f"{fn}: capacities {caps} too small after sizing them from totals {tot.tolist()}")
            caps = (int(tot[0]), int(tot[1]), int(tot[2]))
        na, nb, nt = int(tot[0]), int(tot[1]), int(tot[2])
        rec = {"mols": mols.cpu().numpy().view(MOL_DTYPE),
               "atoms": atoms[:na * ATOM_DTYPE.itemsize].cpu().numpy().view(ATOM_DTYPE),
               "bonds": bonds[:nb * BOND_DTYPE.itemsize].cpu().numpy().view(BOND_DTYPE),
               "text": text[:nt].cpu().numpy().tobytes(), "totals": tot.copy()}
        if keep_device:
            rec["device"] = (mols, atoms, bonds, text)
        if per_atom:
            rec["side"] = per_atom[0][:na]
        return rec

    def _packed_tables(self, rec: dict):
        """graph_pack's records -> (the four tables as device tensors: those graph_pack(keep_device=True) left, or an upload;
        the leading arguments mols, n, atoms, na, bonds, nb, text, nt of a writer, None for an empty table)"""
        dev = torch.device("cuda", self.device)

        def up(a):
            raw = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
            return torch.frombuffer(bytearray(raw) or bytearray(8), dtype=torch.uint8).to(dev)

        tables = rec.get("device") or tuple(up(rec[k]) for k in ("mols", "atoms", "bonds", "text"))
        args = [_ptr(tables[0]), len(rec["mols"])]
        for t, k in zip(tables[1:], (len(rec["atoms"]), len(rec["bonds"]), len(rec["text"]))):
            args += [_ptr(t) if k else None, k]
        return tables, args

    def _sized_text(self, fn: str, head, cap: int, tail=()) -> bytes:
        """One text writer, lib.<fn>(h, *head, out, out_cap, totals, *tail, stream), at capacity `cap` and at most once more with
        the size `totals` reports: the bytes it wrote."""
        dev = torch.device("cuda", self.device)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        for attempt in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            self._check(getattr(self.lib, fn)(self.h, *head, _ptr(out), cap, _ptr(totals), *tail, _stream()), fn)
            tot = totals.cpu().numpy().view(np.uint32)
            if not tot[1]:
                break
            if attempt:
                raise MnxError(f"{fn}: capacity {cap} too small after sizing it from totals {tot.tolist()}")
            cap = int(tot[0])
        return out[:int(tot[0])].cpu().numpy().tobytes()

    def _byte_arena(self, items, who: str, noun: str, refusal: Optional[str] = None):
        """A reader's items (str or bytes) behind one another: (the arena's bytes, the arena on the device, the uint32 offsets
        [n + 1] on the device, n). An arena of no bytes goes up as eight: a tensor needs an address. refusal: a ValueError text of
        the caller's own, raised where it always stood — behind the refusal of an empty list, in front of the count of the bytes."""
        dev = torch.device("cuda", self.device)
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in items]
        n = len(raw)
        if n < 1:
            raise ValueError(f"{who} needs at least one {noun}")
        if refusal:
            raise ValueError(refusal)
        lens = np.fromiter((len(x) for x in raw), dtype=np.int64, count=n)
        if int(lens.sum()) > 0xFFFFFFFF:
            raise ValueError(f"{who}: more than 2^32 - 1 bytes in one call")
        offsets = np.zeros(n + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum(lens)
        arena = b"".join(raw)
        d_bytes = torch.frombuffer(bytearray(arena) or bytearray(8), dtype=torch.uint8).to(dev)
        return arena, d_bytes, torch.from_numpy(offsets.view(np.int32)).to(dev), n

    def _scale_tensor(self, scale, n: int):
        """molfile_pack's and molfile_read's scale, int [n, 2] = (Sx, Sy) per molecule, as an int32 device tensor; None stays None"""
        if scale is None:
            return None
        return torch.as_tensor(np.ascontiguousarray(scale, dtype=np.int32).reshape(n, 2)).to(torch.device("cuda", self.device))

    MOLFILE_GUESS = 4096     # first capacity of molfile_pack per molecule (30 atoms and 30 bonds take about 2.6 KB)

    def molfile_pack(self, rec: dict, scale=None, cap: Optional[int] = None):
        """graph_pack's records -> (files [n] MOLFILE_DTYPE, bytes): the V2000 molfile of molecule b is
        bytes[files[b]['text0'] : +files[b]['len']] (mnx_molfile_pack; len 0 and a flag for a molecule that gets none).
        scale: int [n, 2] = (Sx, Sy) per molecule in units of 1e-4, None = 100000 each (include/molnextr_hip.h). The records
        go back to the device as they are (or stay there: graph_pack(keep_device=True)); starts from MOLFILE_GUESS bytes per
        molecule (or cap) and repeats at most once with the size `totals` reports."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        sc = self._scale_tensor(scale, n)
        files = torch.empty(n * MOLFILE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        data = self._sized_text("mnx_molfile_pack", args + [_ptr(sc), _ptr(files)], int(cap) if cap is not None else n * self.MOLFILE_GUESS)
        return files.cpu().numpy().view(MOLFILE_DTYPE), data

    SMILES_GUESS = 256        # first capacity of smiles_pack per molecule (a drug-like SMILES is well under 200 bytes)

    def smiles_pack(self, rec: dict, cap: Optional[int] = None, stereo: bool = False, double_bonds: bool = False,
                    canonical: bool = False, symmetry: bool = False):
        """graph_pack's records -> (recs [n] SMILES_DTYPE, order uint16 [atoms], bytes): the graph SMILES of molecule b is
        bytes[recs[b]['text0'] : +recs[b]['len']] (mnx_smiles_pack: valid, not canonical, no stereo, pseudo-atoms as '*'; len 0
        and a flag of SMILES_REFUSED for a molecule that gets none), order[atom0 + k] the position of its atom k in that
        string (SMILES_NO_POSITION without one). The records go back to the device as they are (or stay there:
        graph_pack(keep_device=True)); starts from SMILES_GUESS bytes per molecule (or cap) and repeats at most once with the
        size `totals` reports. stereo: mnx_smiles_pack_stereo — the same string with '@' / '@@' at the marked carbons that a
        wedge begins at (the rule: include/molnextr_hip.h), flags with SMILES_STEREO / SMILES_STEREO_UNRESOLVED. double_bonds:
        mnx_smiles_pack_marks — '/' and '\\' at the double bonds off every cycle that the coordinate bins resolve (the rule: the
        same header), with or without stereo's marks; flags with SMILES_EZ / SMILES_EZ_UNRESOLVED / SMILES_EZ_IMPLIED. Without
        it the calls are the ones made before it existed. canonical: mnx_smiles_pack_canonical — the same writer on canonical
        atom ranks, with the marks that stereo and double_bonds select; returns (recs, order, bytes, rank uint16 [atoms],
        sym_class uint16 [atoms]): the bytes do not depend on the numbering of a drawing's atoms (flags with SMILES_CANON_TIE /
        SMILES_CANON_TIE_INDEX; SMILES_NO_POSITION in rank and sym_class where the molecule was not read). This project's own
        ranking, NOT RDKit's canonical SMILES; the known limit stands in the header. symmetry (canonical only, else ValueError):
        mnx_smiles_pack_symmetric — a candidate centre or double bond with two substituents of one symmetry class, both on bonds
        off every cycle, writes no mark (flags with SMILES_SYM_DROPPED; off for a molecule with a pseudo-atom: expand first);
        returns a sixth value, atom_marks uint8 [atoms]: the ATOM_* bits per atom, ATOM_MARKS_NONE where `order` holds
        SMILES_NO_POSITION. The ranks ignore stereo and a pair on ring bonds is never dropped: the limits stand in the header."""
        if symmetry and not canonical:
            raise ValueError("smiles_pack: symmetry=True needs canonical=True")
        dev = torch.device("cuda", self.device)
        n, na = len(rec["mols"]), len(rec["atoms"])
        tables, args = self._packed_tables(rec)
        recs = torch.empty(n * SMILES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        order = torch.full((max(na, 1),), -1, dtype=torch.int16, device=dev)     # every entry SMILES_NO_POSITION
        marks = (SMILES_MARK_TETRAHEDRAL if stereo else 0) | (SMILES_MARK_DOUBLE_BOND if double_bonds else 0)
        per_atom = [order]                                                       # what the entry point writes per atom, in its order
        if canonical:
            fn, tail = ("mnx_smiles_pack_symmetric" if symmetry else "mnx_smiles_pack_canonical"), (marks,)
            per_atom += [torch.full_like(order, -1), torch.full_like(order, -1)]             # rank, sym_class
            if symmetry:
                per_atom.append(torch.zeros(max(na, 1), dtype=torch.uint8, device=dev))      # atom_marks
        elif double_bonds:
            fn, tail = "mnx_smiles_pack_marks", (marks,)
        else:
            fn, tail = ("mnx_smiles_pack_stereo" if stereo else "mnx_smiles_pack"), ()
        data = self._sized_text(fn, args + [_ptr(recs)] + [_ptr(t) for t in per_atom], int(cap) if cap is not None else n * self.SMILES_GUESS, tail)
        host = [t[:na].cpu().numpy().view(np.uint16) if t.dtype == torch.int16 else t[:na].cpu().numpy() for t in per_atom]
        return (recs.cpu().numpy().view(SMILES_DTYPE), host[0], data, *host[1:])

    # margin, side, key of _tables_pass for the three frames of a pass: one that grows a molecule (room for a label of about ten
    # atoms), one that selects atoms (nothing grows), one that respells them (a new symbol is rarely longer than the old one)
    GROWS, SELECTS, RESPELLS = ((12, 12, 16), torch.int16, "origin"), ((0, 0, 0), torch.int16, "origin"), ((0, 0, 2), torch.uint8, "atom_notes")

    def _tables_pass(self, fn: str, rec: dict, caps, keep_device: bool, margin, side, key: str, tail=()) -> dict:
        """The five passes from tables to tables: lib.<fn>(h, tables, mols_out, arenas, per_atom, totals, *tail, stream) from the
        input's sizes plus margin = (atoms, bonds, text bytes) per molecule, or caps. side, key: the per-atom output's torch dtype
        and its key in the result — int16 -> 'origin' as uint16 [atoms], uint8 -> 'atom_notes'."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        if caps is None:
            caps = tuple(len(rec[k]) + m * n for k, m in zip(("atoms", "bonds", "text"), margin))
        out = self._sized_tables(fn, n, caps,
                                 lambda mols, arenas, totals, per_atom: getattr(self.lib, fn)(self.h, *args, mols, *arenas, per_atom, totals, *tail, _stream()),
                                 dev, keep_device, side=side)
        per_atom = out.pop("side").cpu().numpy()
        out[key] = per_atom.view(np.uint16) if side == torch.int16 else per_atom
        return out

    def expand_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records -> the same molecules with every abbreviation label that has a fragment replaced by the
        fragment's atoms and bonds (mnx_expand_pack; the rule: include/molnextr_hip.h): a dict with graph_pack's keys — 'mols',
        'atoms', 'bonds', 'text', 'totals' — plus 'origin' uint16 [atoms], the input index of the atom every output atom came
        from. molfile_pack and smiles_pack take it as it is. 'text' is the atoms' symbols behind one another, no token SMILES;
        the atoms of a fragment share the label's coordinates; mols['flags'] carries MOL_EXPANDED / MOL_LABEL_LEFT /
        MOL_EXPAND_REFUSED. Starts from the input's sizes plus a margin (or caps = (atom_cap, bond_cap, text_cap)) and repeats
        at most once with the sizes `totals` reports. keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_expand_pack", rec, caps, keep_device, *self.GROWS)

    def formula_pack(self, rec: dict, caps=None, keep_device: bool = False, max_steps: int = 0) -> dict:
        """graph_pack's records (or smiles_read's) -> the same molecules with every condensed-formula label ('CH2CH3', 'N(CH3)2',
        'COOCH3', 'CH2Ph': a symbol without a parse that is in neither name table, 2 to 20 bytes) that the valence search finds a
        structure for replaced by its atoms and bonds (mnx_formula_pack; the rule: include/molnextr_hip.h — this library's own
        repair of the reference's search, no toolkit has parsed the result). A group token inside a label ('Ph' in 'CH2Ph') is
        written as '[Ph]': run expand_pack behind this call. A dict with expand_pack's keys — 'mols', 'atoms', 'bonds', 'text',
        'totals', 'origin' —; mols['flags'] carries MOL_FORMULA_EXPANDED / MOL_FORMULA_LEFT / MOL_FORMULA_LIMIT /
        MOL_FORMULA_REFUSED. max_steps: the placements one label's search may try (0: FORMULA_DEFAULT_STEPS). Sizes itself as
        expand_pack does; keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_formula_pack", rec, caps, keep_device, *self.GROWS, (int(max_steps),))

    def main_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> of every molecule the connected component with the most
        atoms, among equals the one with the lowest atom, every other atom and its bonds dropped (mnx_main_pack; the rule: the
        reference's _keep_main_molecule, include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds',
        'text', 'totals' — plus 'origin' uint16 [atoms], the input index of every kept atom. 'text' is the kept atoms' symbols
        behind one another, as expand_pack's; mols['flags'] carries MOL_MAIN_KEPT / MOL_MAIN_TIE / MOL_MAIN_REFUSED. Run it
        behind expand_pack, so that a label counts with the atoms it stands for, and in front of kekulize_pack. Sized from the
        input — nothing grows — or caps = (atom_cap, bond_cap, text_cap), then once more with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_main_pack", rec, caps, keep_device, *self.SELECTS)

    def normalize_pack(self, rec: dict, caps=None, keep_device: bool = False) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> the same molecules with one normal spelling per atom
        (mnx_normalize_pack; the rule: include/molnextr_hip.h — this library's own, NOT a toolkit's aromaticity model): rings of 5
        and 6 atoms that the rule finds aromatic get lower-case atoms and class-4 bonds, a bracket atom that says no more than a
        reader infers loses its brackets, everything else is respelled as the writers spell it. A dict with graph_pack's keys —
        'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'atom_notes' uint8 [atoms]: NOTE_H_MASK the atom's H count,
        NOTE_AROMATIZED / NOTE_UNBRACKETED / NOTE_COPIED. Atom and bond counts and order are the input's; mols['flags'] carries
        MOL_AROMATIZED / MOL_UNBRACKETED / MOL_NORMALIZE_REFUSED. Starts from the input's sizes (a new symbol is rarely longer
        than the old one; or caps = (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_normalize_pack", rec, caps, keep_device, *self.RESPELLS)

    def kekulize_pack(self, rec: dict, caps=None, keep_device: bool = False, max_steps: int = 0) -> dict:
        """graph_pack's records (or expand_pack's, or smiles_read's) -> the same molecules with every aromatic system that has a
        Kekule structure written as one (mnx_kekulize_pack; the rule: include/molnextr_hip.h): lower-case atoms on type-4 bonds
        become upper-case atoms on double and single bonds, H counts kept; a system without a matching, a blocked one and one
        whose search passes max_steps pairings (0: KEKULE_DEFAULT_STEPS) stay as they came. A Kekule structure is a perfect
        matching; the choice among several is this library's own search order, NOT RDKit's Kekulize. A dict with graph_pack's
        keys — 'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'atom_notes' uint8 [atoms]: NOTE_H_MASK the H count of an
        aromatic atom, NOTE_KEKULIZED / NOTE_KEKULE_LEFT (with NOTE_KEKULE_LIMIT) / NOTE_COPIED. Atom and bond counts and order
        are the input's; mols['flags'] carries MOL_KEKULIZED / MOL_KEKULE_LEFT / MOL_KEKULIZE_REFUSED. Run it behind expand_pack
        and in front of normalize_pack. Sizes itself as normalize_pack does; keep_device: also 'device', as graph_pack."""
        return self._tables_pass("mnx_kekulize_pack", rec, caps, keep_device, *self.RESPELLS, (int(max_steps),))

    def fingerprint_pack(self, rec: dict, max_bonds: int = 0, max_steps: int = 0, keep_device: bool = False) -> dict:
        """graph_pack's records (or any pass's, or smiles_read's) -> {'fp' [n] FP_DTYPE, 'bits' uint32 [n, FP_WORDS]}: of every
        molecule the 2048 bits of its paths of up to max_bonds bonds (mnx_fingerprint_pack; the rule: include/molnextr_hip.h —
        this library's own, after the idea of Daylight's and RDKit's path fingerprints, NOT RDKit's bits). max_bonds 1 .. 7 (0:
        FP_MAX_BONDS); max_steps: the paths one directed bond may begin (0: FP_DEFAULT_STEPS; FP_MAX_STEPS at the most), beyond
        which the molecule gets FP_LIMIT. A molecule with a bit of FP_REFUSED or FP_LIMIT has every word 0; fp['n_bits'] counts
        the bits, fp['max_paths'] is the largest number of paths from one directed bond. Run it behind kekulize_pack and
        normalize_pack, so that an aromatic and a Kekule spelling give the same bits. One launch, nothing to size. keep_device:
        'bits' stays a device tensor (int32 [n, FP_WORDS], the same words), for tanimoto."""
        dev = torch.device("cuda", self.device)
        n = len(rec["mols"])
        tables, args = self._packed_tables(rec)
        recs = torch.empty(n * FP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        bits = torch.empty((n, FP_WORDS), dtype=torch.int32, device=dev)
        self._check(self.lib.mnx_fingerprint_pack(self.h, *args, _ptr(recs), _ptr(bits), int(max_bonds), int(max_steps), _stream()),
                    "mnx_fingerprint_pack")
        return {"fp": recs.cpu().numpy().view(FP_DTYPE), "bits": bits if keep_device else bits.cpu().numpy().view(np.uint32)}

    def tanimoto(self, a, b) -> dict:
        """Two tables of fingerprints [n, FP_WORDS] (fingerprint_pack's 'bits': numpy uint32 or the device tensors), row i of a
        against row i of b -> {'both' uint32 [n], 'either' uint32 [n], 'similarity' float64 [n]}: the bits both rows hold, the
        bits either holds, and their quotient — 0.0 where neither holds a bit: an empty side is a mismatch (mnx_tanimoto)."""
        dev = torch.device("cuda", self.device)
        a, b = self._fp_rows(a, "tanimoto"), self._fp_rows(b, "tanimoto")
        if a.shape != b.shape:
            raise ValueError(f"tanimoto compares row with row: {tuple(a.shape)} against {tuple(b.shape)}")
        n = a.shape[0]
        both, either = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        similarity = torch.empty(n, dtype=torch.float64, device=dev)
        self._check(self.lib.mnx_tanimoto(self.h, _ptr(a), _ptr(b), n, _ptr(both), _ptr(either), _ptr(similarity), _stream()), "mnx_tanimoto")
        return {"both": both.cpu().numpy().view(np.uint32), "either": either.cpu().numpy().view(np.uint32),
                "similarity": similarity.cpu().numpy()}

    def _fp_rows(self, x, who: str) -> torch.Tensor:
        """rows of fingerprints, numpy uint32 or a device int32 tensor [n, FP_WORDS], as a contiguous tensor on the engine's device"""
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.array(x, dtype=np.uint32).view(np.int32))          # a copy: the caller's rows may be read-only
        x = x.to(torch.device("cuda", self.device)).contiguous()
        if x.dim() != 2 or x.shape[1] != FP_WORDS or x.dtype != torch.int32:
            raise ValueError(f"{who} needs [n, {FP_WORDS}] words of 32 bits, not {tuple(x.shape)} {x.dtype}")
        return x

    def tanimoto_search(self, queries, library, k: int = 1, min_similarity: float = 0.0, skip_self: bool = False,
                        keep_device: bool = False) -> dict:
        """Two tables of fingerprints (fingerprint_pack's 'bits': numpy uint32 or device int32 tensors [n, FP_WORDS]) -> for every
        row of `queries` its k nearest rows of `library` by Tanimoto similarity (mnx_tanimoto_search; the rule and the order:
        include/molnextr_hip.h): {'count' uint32 [nq], 'index', 'both', 'either' uint32 [nq, k], 'similarity' float64 [nq, k]}.
        Row q holds count[q] hits — the first k by similarity, among equals the lower index, of those the ones at or above
        min_similarity —, and NEAREST_NONE, 0, 0 and 0.0 behind them. 1 <= k <= NEAREST_MAX_K; the library has at most
        NEAREST_MAX_ROWS rows. skip_self: library row q is no candidate for query q (a set searched in itself). More than
        NEAREST_MAX_QUERIES queries run in chunks of that many; with skip_self that is refused, because a chunk's rows are not
        the library's rows of the same number. This library's own fingerprint, NOT RDKit's. keep_device: the five stay device
        tensors (int32 for the words)."""
        dev = torch.device("cuda", self.device)
        q, lib = self._fp_rows(queries, "tanimoto_search"), self._fp_rows(library, "tanimoto_search")
        nq, nl, k = q.shape[0], lib.shape[0], int(k)
        if nq < 1 or not 1 <= nl <= NEAREST_MAX_ROWS or not 1 <= k <= NEAREST_MAX_K:
            raise ValueError(f"tanimoto_search needs a query, 1 .. {NEAREST_MAX_ROWS} library rows and 1 <= k <= {NEAREST_MAX_K}: "
                             f"{nq} queries, {nl} rows, k = {k}")
        if skip_self and nq > NEAREST_MAX_QUERIES:
            raise ValueError(f"tanimoto_search: skip_self takes at most {NEAREST_MAX_QUERIES} queries (one call): a chunk of {nq} "
                             "queries would skip the wrong rows")
        count = torch.empty(nq, dtype=torch.int32, device=dev)
        index, both, either = (torch.empty((nq, k), dtype=torch.int32, device=dev) for _ in range(3))
        similarity = torch.empty((nq, k), dtype=torch.float64, device=dev)
        step = min(nq, NEAREST_MAX_QUERIES)
        work_bytes = int(self.lib.mnx_tanimoto_search_work_bytes(step, nl, k))
        work = torch.empty(work_bytes // 8, dtype=torch.int64, device=dev)
        for at in range(0, nq, step):
            rows = slice(at, min(at + step, nq))
            self._check(self.lib.mnx_tanimoto_search(self.h, _ptr(q[rows]), rows.stop - at, _ptr(lib), nl, k, float(min_similarity),
                                                     NEAREST_SKIP_SELF if skip_self else 0, _ptr(count[rows]), _ptr(index[rows]),
                                                     _ptr(both[rows]), _ptr(either[rows]), _ptr(similarity[rows]), _ptr(work), work_bytes,
                                                     _stream()), "mnx_tanimoto_search")
        out = {"count": count, "index": index, "both": both, "either": either, "similarity": similarity}
        if keep_device:
            return out
        return {key: t.cpu().numpy() if key == "similarity" else t.cpu().numpy().view(np.uint32) for key, t in out.items()}

    def substructure_match(self, query_rec: dict, target_rec: dict, pairs=None, max_matches: int = 1, max_steps: int = 0,
                           keep_device: bool = False) -> dict:
        """Two sets of records (graph_pack's, any pass's, a reader's; host arrays or keep_device=True outputs, and they may be the
        same dict) -> {'match' [n_pairs] MATCH_DTYPE, 'map' uint16 [n_pairs, MATCH_MAX_QUERY]}: per pair (query index, target
        index) whether the query molecule embeds in the target molecule (mnx_substructure_match; the rule: include/molnextr_hip.h
        — this library's own, NOT RDKit's HasSubstructMatch and not SMARTS). pairs: int [n_pairs, 2]; None pairs one query with
        every target, or item with item where the counts are equal. match['n_matches'] counts the embeddings up to max_matches
        (0: 1), match['steps'] is the longest search of one root, map[p][a] the target atom under query atom a in the first
        embedding (MATCH_NO_ATOM beyond the query or without a match). max_steps: the candidates one root's search may examine
        (0: MATCH_DEFAULT_STEPS; MATCH_MAX_STEPS at the most), beyond which the pair gets MATCH_LIMIT unless max_matches
        embeddings were found. A pair with a bit of MATCH_REFUSED was not searched. Run both sides through kekulize_pack and
        normalize_pack first, so that an aromatic query finds a Kekule drawing. One launch, nothing to size. keep_device: 'map'
        stays a device tensor (int16 [n_pairs, MATCH_MAX_QUERY], the same words)."""
        dev = torch.device("cuda", self.device)
        nq, nt = len(query_rec["mols"]), len(target_rec["mols"])
        if pairs is None:
            if nq != 1 and nq != nt:
                raise ValueError(f"substructure_match pairs one query with every target or item with item: {nq} queries against {nt} targets")
            pairs = np.stack([np.zeros(nt, np.int64) if nq == 1 else np.arange(nt), np.arange(nt)], axis=1)
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        if len(pairs) and (pairs.min() < 0 or pairs.max() > 0xFFFFFFFF):
            raise ValueError("substructure_match: a pair index outside 0 .. 2^32 - 1")
        n = len(pairs)
        q_tables, q_args = self._packed_tables(query_rec)
        t_tables, t_args = self._packed_tables(target_rec)
        d_pairs = torch.from_numpy(pairs.astype(np.uint32).view(np.int32)).to(dev)
        recs = torch.empty(n * MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        maps = torch.empty((n, MATCH_MAX_QUERY), dtype=torch.int16, device=dev)
        self._check(self.lib.mnx_substructure_match(self.h, *q_args, *t_args, _ptr(d_pairs), n, _ptr(recs), _ptr(maps), int(max_matches),
                                                    int(max_steps), _stream()), "mnx_substructure_match")
        return {"match": recs.cpu().numpy().view(MATCH_DTYPE), "map": maps if keep_device else maps.cpu().numpy().view(np.uint16)}

    def smiles_read(self, strings, caps=None, keep_device: bool = False) -> dict:
        """SMILES strings (str or bytes) -> the molecules as packed tables, read on the device (mnx_smiles_read; the rule:
        include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds', 'text', 'totals' — plus 'read' [n]
        READ_DTYPE (flags READ_*, err_pos, n_rings). molfile_pack, smiles_pack(... canonical=True) and expand_pack take it as it
        is. A refused string (READ_REFUSED) is the empty molecule. Starts from PACK_GUESS atoms and bonds per string, one per byte
        at the most (or caps = (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports.
        keep_device: also 'device', as graph_pack."""
        dev = torch.device("cuda", self.device)
        arena, d_bytes, d_off, n = self._byte_arena(strings, "smiles_read", "string")
        recs = torch.empty(n * READ_DTYPE.itemsize, dtype=torch.uint8, device=dev)      # per string: one for both attempts
        if caps is None:        # an atom takes a byte at least, a string has about as many bonds as atoms, and its text is itself
            caps = (min(len(arena), n * self.PACK_GUESS[0]), min(len(arena), n * self.PACK_GUESS[1]), len(arena))
        out = self._sized_tables("mnx_smiles_read", n, caps,
                                 lambda mols, arenas, totals: self.lib.mnx_smiles_read(
                                     self.h, _ptr(d_bytes), len(arena), _ptr(d_off), n, mols, _ptr(recs), *arenas, totals, _stream()),
                                 dev, keep_device)
        out["read"] = recs.cpu().numpy().view(READ_DTYPE)
        return out

    def molfile_read(self, files, scale=None, fit: bool = False, caps=None, keep_device: bool = False) -> dict:
        """V2000 molfiles (bytes or str, one molecule each; model.split_sdf cuts an SDF) -> the molecules as packed tables with
        their coordinate bins and wedge classes, read on the device (mnx_molfile_read; the rule — this library's own, NOT a
        toolkit's valence model: include/molnextr_hip.h): a dict with graph_pack's keys — 'mols', 'atoms', 'bonds', 'text',
        'totals' — plus 'read' [n] MOLREAD_DTYPE (flags MOLREAD_*, err_line, n_marked). Every pass and writer takes it as it is;
        smiles_pack(stereo=True, double_bonds=True) finds the marks a SMILES cannot bring. A refused file (MOLREAD_REFUSED) is the
        empty molecule. scale: int [n, 2] = (Sx, Sy) per file in units of 1e-4, None = 100000 each — molfile_pack's argument, and
        with the scale a file was written at the bins come back exactly; fit=True (no scale then): one uniform scale per file that
        fits its atoms into the bins, for files drawn elsewhere. Starts from one atom and one bond per 48 bytes (or caps =
        (atom_cap, bond_cap, text_cap)) and repeats at most once with the sizes `totals` reports. keep_device: also 'device', as
        graph_pack."""
        dev = torch.device("cuda", self.device)
        arena, d_bytes, d_off, n = self._byte_arena(files, "molfile_read", "file",
                                                    "molfile_read: fit=True takes no scale" if fit and scale is not None else None)
        sc = self._scale_tensor(scale, n)
        recs = torch.empty(n * MOLREAD_DTYPE.itemsize, dtype=torch.uint8, device=dev)   # per file: one for both attempts
        if caps is None:        # an atom line has 31 bytes at least, a bond line 12 in the writer's files; a symbol is short
            caps = (len(arena) // 48 + n, len(arena) // 48 + n, len(arena) // 16 + n)
        out = self._sized_tables("mnx_molfile_read", n, caps,
                                 lambda mols, arenas, totals: self.lib.mnx_molfile_read(
                                     self.h, _ptr(d_bytes), len(arena), _ptr(d_off), n, _ptr(sc), int(bool(fit)), mols, _ptr(recs), *arenas,
                                     totals, _stream()),
                                 dev, keep_device)
        out["read"] = recs.cpu().numpy().view(MOLREAD_DTYPE)
        return out
