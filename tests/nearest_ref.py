"""The oracle of mnx_tanimoto_search (include/molnextr_hip.h, "Nearest rows") in plain Python and numpy, written from the rule and
sharing no code with csrc/nearest_select.h: per query the bit counts of Q & R and Q | R over ALL library rows from a byte table
(each on its own — not bits(Q) + bits(R) - both, the identity the kernel uses), a full sort by the key (the fraction as a
fractions.Fraction, largest first, then the index), the cut at k and, on int / int, at min_similarity."""
import fractions
import functools

import numpy as np

NONE = 0xFFFFFFFF
WORDS = 64
BYTE_BITS = np.array([bin(v).count("1") for v in range(256)], np.uint32)


def bit_counts(rows):
    """the bits set in every row of a uint32 array [n, 64]"""
    return BYTE_BITS[np.ascontiguousarray(rows, np.uint32).view(np.uint8)].sum(axis=1, dtype=np.uint32)


def words_of(bits):
    """a row with exactly the bits of `bits` (numbers 0 .. 2047) set"""
    row = np.zeros(WORDS, np.uint32)
    for t in bits:
        row[t >> 5] |= np.uint32(1 << (t & 31))
    return row


@functools.lru_cache(maxsize=None)
def fraction(both, either):
    """both / either exactly, 0 / 0 as 0 / 1"""
    return fractions.Fraction(both, either or 1)


def full_order(both, either):
    """the indices of all rows in the order of the rule: Fraction(both, either) falling (0 / 0 as 0 / 1), then the index rising. The
    fractions are ranked exactly — every distinct pair once —, the rows then sorted by (rank, index)."""
    both, either = np.asarray(both, np.int64), np.asarray(either, np.int64)
    rows = list(zip(both.tolist(), either.tolist()))
    pairs = sorted(set(rows), key=lambda p: fraction(*p), reverse=True)
    rank, at = {}, -1
    for n, p in enumerate(pairs):
        if n == 0 or fraction(*p) != fraction(*pairs[n - 1]):
            at += 1
        rank[p] = at
    ranks = np.array([rank[p] for p in rows], np.int64)
    return np.lexsort((np.arange(len(both)), ranks))


def first_k(candidates, k):
    """(both, either, index) triples, in any order -> the first k of them in the order of the rule (fewer when there are fewer)"""
    ordered = sorted(candidates, key=lambda c: (-fraction(c[0], c[1]), c[2]))
    return ordered[:k]


def search(queries, library, k=1, min_similarity=0.0, skip_self=False):
    """mnx_tanimoto_search on host arrays [nq, 64] and [nl, 64]: {'count' uint32 [nq], 'index', 'both', 'either' uint32 [nq, k],
    'similarity' float64 [nq, k]}"""
    queries, library = (np.ascontiguousarray(x, np.uint32).reshape(-1, WORDS) for x in (queries, library))
    nq = len(queries)
    out = {"count": np.zeros(nq, np.uint32), "index": np.full((nq, k), NONE, np.uint32), "both": np.zeros((nq, k), np.uint32),
           "either": np.zeros((nq, k), np.uint32), "similarity": np.zeros((nq, k), np.float64)}
    for q, row in enumerate(queries):
        both, either = bit_counts(library & row), bit_counts(library | row)
        order = [int(i) for i in full_order(both, either) if not (skip_self and int(i) == q)][:k]
        kept = [i for i in order if (int(both[i]) / int(either[i]) if either[i] else 0.0) >= min_similarity]
        out["count"][q] = len(kept)
        for j, i in enumerate(kept):
            out["index"][q, j], out["both"][q, j], out["either"][q, j] = i, both[i], either[i]
            out["similarity"][q, j] = int(both[i]) / int(either[i]) if either[i] else 0.0
    return out
