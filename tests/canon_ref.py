"""The oracle of mnx_smiles_pack_canonical (include/molnextr_hip.h), sharing no code with the kernel:

* the RANKS — ranks(): the rule of the header in plain Python. A key is a Python tuple (the atom's written bytes and its bond
  count; then the old rank and the sorted list of (neighbour's rank, bond class) pairs), a rank is the position of the key
  in the sorted list of all keys, a tie goes to the smallest (x_bin, y_bin, atom index);
* the STRING — smiles(): the molecule renumbered by its ranks (stereo_ref.renumber) and written by the existing oracle of
  mnx_smiles_pack_marks (ez_ref.smiles, which is smiles_ref.smiles for marks == 0), each pinned by its own tests;
* pack() as the other reference modules have it, and redraw(): the same molecule on new coordinates."""
from collections import Counter

import numpy as np

import ez_ref as E
import molfile_ref as M
import smiles_ref as S
import stereo_ref as T
from molnextr_amd.engine import SMILES_DTYPE

FLAG_TIE, FLAG_TIE_INDEX = 8192, 16384
NO_RANK = 0xFFFF
BOND_CLASS = {1: 0, 5: 0, 6: 0, 2: 1, 3: 2, 4: 3}         # every other `type` is class 4


def rank_of(keys):
    """r(a) = the number of keys strictly smaller than key a"""
    first = {}
    for at, k in enumerate(sorted(keys)):
        first.setdefault(k, at)
    return [first[k] for k in keys]


def refine(rank, around):
    """refinement rounds while a round raises the number of distinct ranks"""
    while True:
        new = rank_of([(rank[a], tuple(sorted((rank[n], c) for n, c in around[a]))) for a in range(len(rank))])
        if len(set(new)) <= len(set(rank)):
            assert new == rank, "a round that splits no class changes no rank"
            return rank
        rank = new


def ranks(symbols, xy, bonds, tables=None):
    """One molecule with valid bonds, no pair twice -> (rank of every atom: a permutation, its symmetry class, FLAG_TIE* bits)"""
    tables = M.name_tables() if tables is None else tables
    n = len(symbols)
    around = [[] for _ in range(n)]
    for i, j, ty, _ in bonds:
        around[i].append((j, BOND_CLASS.get(ty, 4)))
        around[j].append((i, BOND_CLASS.get(ty, 4)))
    rank = refine(rank_of([(S.atom_text(s, tables)[0].encode("ascii"), len(around[a])) for a, s in enumerate(symbols)]), around)
    sym_class, flags = list(rank), 0
    while len(set(rank)) < n:
        v = min(r for r, k in Counter(rank).items() if k > 1)
        tied = [a for a in range(n) if rank[a] == v]
        keep = min(tied, key=lambda a: (xy[a][0], xy[a][1], a))
        flags |= FLAG_TIE
        if sum(tuple(xy[a]) == tuple(xy[keep]) for a in tied) > 1:
            flags |= FLAG_TIE_INDEX
        rank = refine([r + 1 if r == v and a != keep else r for a, r in enumerate(rank)], around)
    assert sorted(rank) == list(range(n))
    return rank, sym_class, flags


def smiles(symbols, xy, bonds, marks=0, tables=None):
    """One molecule: (text or None, written position of every atom or None, flags, n_rings, rank, sym_class); rank and sym_class
    are None for a molecule with the same atom pair in two bond records"""
    tables = M.name_tables() if tables is None else tables
    if len({frozenset(b[:2]) for b in bonds}) != len(bonds):
        text, pos, flags, n_rings = E.smiles(symbols, xy, bonds, marks, tables)[:4]
        assert text is None and flags & S.FLAG_DUPLICATE
        return None, None, flags, n_rings, None, None
    rank, sym_class, tie = ranks(symbols, xy, bonds, tables)
    moved = T.renumber((symbols, xy, bonds), rank, np.random.default_rng(0))
    text, pos, flags, n_rings = E.smiles(*moved, marks, tables)[:4]
    return text, (None if pos is None else [pos[rank[a]] for a in range(len(symbols))]), flags | tie, n_rings, rank, sym_class


def pack(mols, atoms, bonds, text, marks=0, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None,
         order_fill=S.NO_POSITION):
    """mnx_smiles_pack_canonical on host arrays, as ez_ref.pack: {'recs', 'order', 'rank', 'sym_class', 'out', 'total'}"""
    tables = M.name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    recs = np.zeros(len(mols), SMILES_DTYPE)
    order, rank, sym_class = (np.full(n_a, order_fill, np.uint16) for _ in range(3))
    chunks, at = [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        flags = S.FLAG_TRUNCATED if int(m["flags"]) & 1 else 0
        if na > 999 or nb > 999:
            flags |= S.FLAG_TOO_LARGE
        if a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t:
            flags |= S.FLAG_BEYOND
        data, where, n_rings, r, c = None, None, 0, None, None
        if not flags & 3:
            A, B = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            if any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in A) or \
                    any(int(x["i"]) >= na or int(x["j"]) >= na or int(x["i"]) == int(x["j"]) for x in B):
                flags |= S.FLAG_BEYOND
            else:
                syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in A]
                data, where, f, n_rings, r, c = smiles(syms, [(int(a["x_bin"]), int(a["y_bin"])) for a in A],
                                                       [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in B], marks, tables)
                flags |= f
        end = min(a0 + na, n_a)
        order[a0:end] = S.NO_POSITION if data is None else where
        rank[a0:end] = NO_RANK if r is None else r
        sym_class[a0:end] = NO_RANK if c is None else c
        data = data or ""
        recs[b] = (min(at, 0xFFFFFFFF), len(data), flags, n_rings)
        chunks.append(data.encode("ascii"))
        at += len(data)
    return {"recs": recs, "order": order, "rank": rank, "sym_class": sym_class, "out": b"".join(chunks), "total": at}


def redraw(mol, rng, bins=2048):
    """the same atoms and bonds drawn anew: every atom on a random bin"""
    symbols, xy, bonds = mol
    return symbols, [(int(x), int(y)) for x, y in rng.integers(0, bins, (len(symbols), 2))], bonds
