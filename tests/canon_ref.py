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

FLAG_TIE, FLAG_TIE_INDEX = 8192, 16384
NO_RANK = S.NO_POSITION          # 0xFFFF: what pack() leaves where a molecule got no ranks
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
    return S.pack_with(lambda syms, xy, B, tb: smiles(syms, xy, B, marks, tb), mols, atoms, bonds, text, tables, n_atom_records,
                       n_bond_records, n_text_bytes, order_fill, extra=("rank", "sym_class"))


def redraw(mol, rng, bins=2048):
    """the same atoms and bonds drawn anew: every atom on a random bin"""
    symbols, xy, bonds = mol
    return symbols, [(int(x), int(y)) for x, y in rng.integers(0, bins, (len(symbols), 2))], bonds
