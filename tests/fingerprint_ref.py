"""The oracle of mnx_fingerprint_pack and mnx_tanimoto (include/molnextr_hip.h, "Path fingerprints") in plain Python, written from
the rule: a recursive walk over adjacency lists and a set of bit numbers where the kernel walks on a stack in on-chip memory and
ORs into words; the forward and the backward hash are both taken from the whole path, nothing is incremental. The atom text is
smiles_ref.atom_text (pinned by the writers' tests), the admission smiles_ref.pack_with's. It shares no code with the kernel."""
import numpy as np

import molfile_ref as M
import smiles_ref as S
from molnextr_amd.engine import FP_DTYPE

TOO_LARGE, BEYOND, PSEUDO, TRUNCATED, BAD_BOND, LIMIT = 1, 2, 4, 8, 16, 1 << 16
WORDS, BITS, MAX_BONDS, DEFAULT_STEPS, MAX_STEPS = 64, 2048, 7, 4096, 1 << 20
LIMITED_PATHS = 0xFFFFFFFF
MASK = 0xFFFFFFFF


def fnv1a(words):
    """FNV-1a over a sequence of numbers below 2^32 (or of bytes)"""
    h = 2166136261
    for w in words:
        h = ((h ^ w) * 16777619) & MASK
    return h


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK
    return h ^ h >> 16


def atom_key(sym: bytes, tables):
    return fmix32(fnv1a(S.atom_text(sym, tables)[0].encode("ascii")))


def bond_word(ty: int) -> int:
    return {1: 1, 5: 1, 6: 1, 2: 2, 3: 3, 4: 4}.get(ty, 5)


def path_bits(seq):
    """the two bit numbers of a path from its word sequence k(a0), c1, k(a1), .., cL, k(aL)"""
    p = fmix32(min(fnv1a(seq), fnv1a(seq[::-1])))
    return p & 2047, p >> 11 & 2047


class Limited(Exception):
    pass


def fingerprint(symbols, bonds, max_bonds=0, max_steps=0, tables=None):
    """One molecule with valid bonds, no pair twice: (the set of its bit numbers or None when limited, the largest P(s))"""
    tables = M.name_tables() if tables is None else tables
    max_bonds, max_steps = max_bonds or MAX_BONDS, max_steps or DEFAULT_STEPS
    keys = [atom_key(s, tables) for s in symbols]
    around = [[] for _ in symbols]
    for i, j, ty, _ in bonds:
        around[i].append((j, bond_word(ty)))
        around[j].append((i, bond_word(ty)))
    bits = set()
    for k in keys:
        bits.update(path_bits([k]))
    count = [0]

    def extend(atoms, seq):
        """every path that continues the one held"""
        if len(atoms) - 1 == max_bonds:
            return
        for n, c in around[atoms[-1]]:
            if n in atoms:
                continue
            count[0] += 1
            if count[0] > max_steps:
                raise Limited
            longer = seq + [c, keys[n]]
            bits.update(path_bits(longer))
            extend(atoms + [n], longer)

    most = 0
    try:
        for a in range(len(symbols)):
            for n, c in around[a]:                    # the directed bond a -> n and the paths that begin with it
                count[0] = 1
                first = [keys[a], c, keys[n]]
                bits.update(path_bits(first))
                extend([a, n], first)
                most = max(most, count[0])
    except Limited:
        return None, LIMITED_PATHS
    return bits, most


def words_of(bits):
    w = np.zeros(WORDS, np.uint32)
    for t in bits:
        w[t >> 5] |= np.uint32(1 << (t & 31))
    return w


def pack(mols, atoms, bonds, text, max_bonds=0, max_steps=0, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_fingerprint_pack on host arrays: {'fp' FP_DTYPE [n], 'bits' uint32 [n, 64]}. The n_* default to the sizes of the arrays;
    smaller ones make the molecules whose records reach beyond them refused (bit 1)."""
    tables = M.name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    fp, words = np.zeros(len(mols), FP_DTYPE), np.zeros((len(mols), WORDS), np.uint32)
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        flags = TRUNCATED if int(m["flags"]) & 1 else 0
        if na > 999 or nb > 999:
            flags |= TOO_LARGE
        if a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t:
            flags |= BEYOND
        if flags & (TOO_LARGE | BEYOND):
            fp[b] = (flags, 0, 0, 0)
            continue
        A, B = atoms[a0:a0 + na], bonds[b0:b0 + nb]
        if any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in A):
            fp[b] = (flags | BEYOND, 0, 0, 0)
            continue
        syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in A]
        if any(S.atom_text(s, tables)[2] for s in syms):
            flags |= PSEUDO
        pairs = [(int(x["i"]), int(x["j"])) for x in B]
        if any(i >= na or j >= na or i == j for i, j in pairs) or len({frozenset(p) for p in pairs}) != len(pairs):
            fp[b] = (flags | BAD_BOND, 0, 0, 0)
            continue
        bits, most = fingerprint(syms, [(i, j, int(x["type"]), int(x["rev"])) for (i, j), x in zip(pairs, B)], max_bonds, max_steps, tables)
        if bits is None:
            fp[b] = (flags | LIMIT, 0, LIMITED_PATHS, 0)
            continue
        words[b] = words_of(bits)
        fp[b] = (flags, len(bits), most, 0)
    return {"fp": fp, "bits": words}


def tanimoto(a, b):
    """mnx_tanimoto on host arrays [n, 64]: {'both', 'either' uint32 [n], 'similarity' float64 [n]}"""
    a, b = np.asarray(a, np.uint32).reshape(-1, WORDS), np.asarray(b, np.uint32).reshape(-1, WORDS)
    count = lambda x: np.array([sum(bin(int(w)).count("1") for w in row) for row in x], np.uint32)      # noqa: E731
    both, either = count(a & b), count(a | b)
    return {"both": both, "either": either,
            "similarity": np.array([int(x) / int(y) if y else 0.0 for x, y in zip(both, either)], np.float64)}
