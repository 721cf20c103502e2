"""CPU: the rule of mnx_tanimoto_search (include/molnextr_hip.h, "Nearest rows") as the oracle of tests/nearest_ref.py states it, on
rows made by hand; csrc/nearest_select.h — the comparator, the insertion and the merge the kernels run — as a program of its own
under the host compiler's sanitizers against the oracle's full sort; the header's declarations and geometry; and the sizing
function, which needs no device."""
import os
import random
import re
import shutil
import subprocess

import numpy as np

import nearest_ref as N
from molnextr_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molnextr_hip.h")


# ------------------------------------------------------------------------------------ the oracle on hand-made rows
def test_oracle_identities():
    a, b, empty = N.words_of({1, 40, 2047}), N.words_of({2, 41}), N.words_of(())
    lib = np.stack([b, a, empty])
    hit = N.search([a], lib, k=3)
    assert hit["count"].tolist() == [3] and hit["index"].tolist() == [[1, 0, 2]]                  # itself, then the lower index of two zeros
    assert hit["similarity"].tolist() == [[1.0, 0.0, 0.0]] and hit["both"].tolist() == [[3, 0, 0]] and hit["either"].tolist() == [[3, 5, 3]]
    # both rows empty: 0.0, kept at min_similarity 0 only
    assert N.search([empty], [empty], k=1)["count"].tolist() == [1] and N.search([empty], [empty], k=1)["similarity"].tolist() == [[0.0]]
    nothing = N.search([empty], [empty], k=2, min_similarity=np.nextafter(0.0, 1.0))
    assert nothing["count"].tolist() == [0] and nothing["index"].tolist() == [[N.NONE, N.NONE]] and nothing["either"].tolist() == [[0, 0]]
    # 1/2 and 2/4 tie, the lower index wins, whichever of the two it is
    q = N.words_of({0, 1})
    half, two_of_four = N.words_of({0}), N.words_of({0, 1, 2, 3})
    for lib, want in (([two_of_four, half], [[2, 4], [1, 2]]), ([half, two_of_four], [[1, 2], [2, 4]])):
        tie = N.search([q], lib, k=2)
        assert tie["index"].tolist() == [[0, 1]] and tie["similarity"].tolist() == [[0.5, 0.5]]
        assert [[int(x), int(y)] for x, y in zip(tie["both"][0], tie["either"][0])] == want
    # the threshold is the exact double; a row beyond k is not reported
    third = N.search([N.words_of({1})], [N.words_of({1, 2, 3}), N.words_of({1})], k=2, min_similarity=1 / 3)
    assert third["count"].tolist() == [2] and third["index"].tolist() == [[1, 0]]
    assert N.search([N.words_of({1})], [N.words_of({1, 2, 3})], k=1, min_similarity=np.nextafter(1 / 3, 1.0))["count"].tolist() == [0]
    # skip_self removes the self row and nothing else
    rows = np.stack([a, b, a])
    assert N.search(rows, rows, k=2)["index"].tolist() == [[0, 2], [1, 0], [0, 2]]
    other = N.search(rows, rows, k=2, skip_self=True)
    assert other["index"].tolist() == [[2, 1], [0, 2], [0, 1]] and other["similarity"][:, 0].tolist() == [1.0, 0.0, 1.0]
    # k beyond the library: what there is
    assert N.search([a], [b], k=3)["count"].tolist() == [1] and N.search([a], [b], k=3, skip_self=True)["count"].tolist() == [0]


def test_the_byte_table_counts_bits():
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 1 << 32, (7, 64), dtype=np.uint64).astype(np.uint32)
    assert N.bit_counts(rows).tolist() == [sum(bin(int(w)).count("1") for w in r) for r in rows]
    assert N.bit_counts(np.full((1, 64), 0xFFFFFFFF, np.uint32)).tolist() == [2048]


# ------------------------------------------------------------------------------------ the selection under the sanitizers
def candidate_sets(rng):
    """sets of (both, either, index) with many equal fractions, indices up to 2^32 - 2, an either of 0, and sizes below and above k"""
    sets = []
    for size, top in ((0, 8), (1, 8), (2, 4), (5, 3), (63, 6), (64, 2048), (65, 12), (200, 5), (700, 2048)):
        index = rng.sample(range(0xFFFFFFFF), size) if size < 100 else rng.sample(range(size * 3), size)
        cands = []
        for i in index:
            either = rng.randint(0, top)
            cands.append((rng.randint(0, either), either, i))
        sets.append(cands)
    sets.append([(1, 2, 9), (2, 4, 3), (3, 6, 7), (1, 3, 0), (0, 0, 1), (0, 5, 2), (2048, 2048, 4), (2047, 2048, 5), (1023, 1024, 6)])
    return sets


def test_the_selection_header_under_the_sanitizers(tmp_path):
    """tools/nearest_host.cpp — a main() around csrc/nearest_select.h, every list exactly k entries on the heap — built with
    -fsanitize=address,undefined and run once, as a plain executable: the same candidates in five shuffled orders, dealt to 1, 2, 7
    and NEAREST_MAX_LISTS lists, at k of 1, 3 and 64, give the first k of the oracle's full sort every time, and the sanitizers
    report nothing (a report ends the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "nearest_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "nearest_host.cpp"), "-o", exe], check=True)
    rng = random.Random(11)
    lines, want = [], []
    for cands in candidate_sets(rng):
        for k in (1, 3, 64):
            first = N.first_k(cands, k)
            expect = " ".join("%d %d %d" % c for c in first + [(0, 0, N.NONE)] * (k - len(first)))
            for shuffle in range(5):
                order = cands[:]
                rng.shuffle(order)
                for n_lists in (1, 2, 7, abi.NEAREST_MAX_LISTS):
                    dealt = [order[w::n_lists] for w in range(n_lists)] if shuffle % 2 else \
                        [order[len(order) * w // n_lists:len(order) * (w + 1) // n_lists] for w in range(n_lists)]
                    lines.append("%d %d" % (k, n_lists))
                    lines += [" ".join([str(len(part))] + ["%d %d %d" % c for c in part]) for part in dealt]
                    want.append(expect)
    run = subprocess.run([exe], input="%d\n%s\n" % (len(want), "\n".join(lines)), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    assert len(want) == 10 * 3 * 5 * 4
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {n}"
    for text in ("1\n0 1\n0\n", "1\n65 1\n0\n", "1\n1 1\n1 3 2 0\n", "1\n1 1\n1 0 2049 0\n", "1\n1 1\n1 0 0 4294967295\n"):
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2


# ------------------------------------------------------------------------------------ the header and the binding
def test_header_declares_the_search():
    hdr = open(HEADER).read()
    for name in ("mnx_tanimoto_search", "mnx_tanimoto_search_work_bytes"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in abi.PROTOTYPES and hasattr(abi.load_library(), name)
    for name, value in (("MNX_NEAREST_MAX_K", "64u"), ("MNX_NEAREST_MAX_QUERIES", "4096u"), ("MNX_NEAREST_MAX_ROWS", "(1u << 24)"),
                        ("MNX_NEAREST_NONE", "0xFFFFFFFFu"), ("MNX_NEAREST_SKIP_SELF", "1u")):
        assert "#define %s %s\n" % (name, value) in hdr, name
    for name in ("QUERY_TILE", "SLAB_ROWS", "MAX_LISTS"):
        assert "#define MNX_NEAREST_%s %du\n" % (name, getattr(abi, "NEAREST_" + name)) in hdr, name
    assert abi.NEAREST_MAX_LISTS * abi.NEAREST_SLAB_ROWS <= 131072
    assert abi.NEAREST_QUERY_TILE >= 1 and abi.NEAREST_MAX_LISTS >= 2
    assert (abi.NEAREST_MAX_K, abi.NEAREST_MAX_QUERIES, abi.NEAREST_MAX_ROWS, abi.NEAREST_NONE, abi.NEAREST_SKIP_SELF) == (64, 4096, 1 << 24, N.NONE, 1)
    assert "MNX_ABI_VERSION 7" in hdr and abi.ABI_VERSION == 7
    assert "THE FINGERPRINT IS THIS LIBRARY'S OWN" in hdr


def test_work_bytes_is_bounded_monotone_and_zero_when_refused():
    size = abi.load_library().mnx_tanimoto_search_work_bytes
    T, S, L = abi.NEAREST_QUERY_TILE, abi.NEAREST_SLAB_ROWS, abi.NEAREST_MAX_LISTS
    nqs = sorted({1, 2, T - 1, T, T + 1, 2 * T, 3 * T, 3 * T + 1, 4 * T, 1000, 1024, 4095, 4096})
    nls = sorted({1, 2, S - 1, S, S + 1, 2 * S + 3, 65536, L * S - 1, L * S, L * S + 1, L * S + S + 1, 1 << 20, (1 << 24) - 1, 1 << 24})
    ks = (1, 2, 3, 8, 63, 64)
    table = {(nq, nl, k): size(nq, nl, k) for nq in nqs for nl in nls for k in ks}
    for (nq, nl, k), b in table.items():
        assert 0 < b <= nq * k * 8 * L and b % 8 == 0, (nq, nl, k, b)
        assert b >= k * 8 * nq                                                                      # a list per query at least
    for axis, values in enumerate((nqs, nls, ks)):
        for key, b in table.items():
            at = values.index(key[axis])
            if at + 1 < len(values):
                nxt = list(key)
                nxt[axis] = values[at + 1]
                assert table[tuple(nxt)] >= b, (key, tuple(nxt))
    assert size(1, 1, 1) == 8 and size(T, S, 64) == T * 64 * 8
    for refused in ((0, 1, 1), (-1, 1, 1), (4097, 1, 1), (1, 0, 1), (1, (1 << 24) + 1, 1), (1, 1, 0), (1, 1, 65)):
        assert size(*refused) == 0, refused
