"""CPU: the rule of mnx_fingerprint_pack and mnx_tanimoto (include/molnextr_hip.h, "Path fingerprints") as the oracle of
tests/fingerprint_ref.py states it — hand-made molecules with their bits written out, the properties that need no oracle
(numbering, drawing, substructure, the longest path, wedges), the step limit on complete graphs, the admission, the identities of
the similarity, the names the engine loads against the header, and the walk of the kernel itself (csrc/path_search.h) under the
host compiler's sanitizers, as a program of its own."""
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np

import canon_ref as K
import fingerprint_ref as F
import molfile_ref as M
import stereo_ref as T
from molnextr_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = M.name_tables()
ATOMS = [b"C", b"N", b"O", b"c", b"n", b"Cl", b"[NH3+]", b"[O-]", b"[13CH3]", b"S", b"[R1]", b"R", b"[999Og]"]


def bits_of(mol, **kw):
    """the set of bit numbers of one molecule (symbols, xy, bonds), None when limited"""
    return F.fingerprint(mol[0], mol[2], tables=TABLES, **kw)[0]


def chain(symbols, ty=1):
    return list(symbols), [(0, 0)] * len(symbols), [(k, k + 1, ty, ty) for k in range(len(symbols) - 1)]


def complete(n):
    return [b"C"] * n, [(0, 0)] * n, [(i, j, 1, 1) for i, j in itertools.combinations(range(n), 2)]


def random_graph(rng, n_atoms, extra):
    """a tree over n_atoms atoms of ATOMS with up to `extra` more bonds, no pair twice, every bond type 0 .. 7"""
    bonds = {(int(rng.integers(0, k)), k) for k in range(1, n_atoms)}
    for _ in range(extra if n_atoms >= 3 else 0):
        i, j = sorted(int(v) for v in rng.choice(n_atoms, 2, replace=False))
        bonds.add((i, j))
    return ([ATOMS[k] for k in rng.integers(0, len(ATOMS), n_atoms)], [(int(x), int(y)) for x, y in rng.integers(0, 64, (n_atoms, 2))],
            [(i, j, int(rng.integers(0, 8)), int(rng.integers(0, 8))) for i, j in sorted(bonds)])


@functools.lru_cache(maxsize=None)
def molecules():
    rng = np.random.default_rng(2048)
    return [random_graph(rng, int(rng.integers(1, 25)), int(rng.integers(0, 4))) for _ in range(40)]


# ---------------------------------------------------------------------------------------------------------------- by hand
K_C, K_O = 0xBD642306, 0xC4AE7453          # fmix32(fnv1a(b"C")), fmix32(fnv1a(b"O"))


def test_the_hashes_by_hand():
    """FNV-1a and murmur3's finaliser on values anyone can check: the empty sequence is the offset basis, one zero word multiplies
    it by the prime, fmix32 fixes 0 and sends 1 to the published 0x514E28B7"""
    assert F.fnv1a([]) == 2166136261 and F.fnv1a([0]) == 2166136261 * 16777619 % 2 ** 32 and F.fnv1a(b"a") == 0xE40C292C
    assert F.fmix32(0) == 0 and F.fmix32(1) == 0x514E28B7
    assert F.atom_key(b"C", TABLES) == K_C and F.atom_key(b"O", TABLES) == K_O
    assert [F.bond_word(t) for t in range(9)] == [5, 1, 2, 3, 4, 1, 1, 5, 5]


def test_methane_carbon_monoxide_and_methanol():
    """methane: one path, two bits at the most; CO: the two atoms and one path, whose hash does not depend on the end it is read
    from; C=O differs from CO in the bits of that path alone"""
    assert bits_of(chain([b"C"])) == {1251, 1837}
    assert bits_of(chain([b"C", b"O"])) == {1251, 1837, 1638, 1876, 459, 1826}
    assert bits_of(chain([b"O", b"C"])) == bits_of(chain([b"C", b"O"]))
    assert bits_of(chain([b"C", b"O"], ty=2)) == {1251, 1837, 1638, 1876, 789, 1443}
    assert set(F.path_bits([K_C, 1, K_O])) == {459, 1826} == set(F.path_bits([K_O, 1, K_C])) and set(F.path_bits([K_O])) == {1638, 1876}
    out = F.pack(*M.build_tables([chain([b"C"]), chain([b"C", b"O"]), chain([])]), tables=TABLES)
    assert out["fp"]["n_bits"].tolist() == [2, 6, 0] and out["fp"]["max_paths"].tolist() == [0, 1, 0] and not out["fp"]["flags"].any()
    assert sorted(t for t in range(2048) if out["bits"][0][t >> 5] >> (t & 31) & 1) == [1251, 1837]


# ---------------------------------------------------------------------------------------------------------------- properties
def test_numbering_and_drawing_change_nothing():
    rng = np.random.default_rng(7)
    for mol in molecules():
        want = bits_of(mol)
        assert want is not None
        # a renumbering swaps `type` and `rev` where the ends swap: the rule reads `type` alone, so compare on symmetric records
        sym = (mol[0], mol[1], [(i, j, ty, ty) for i, j, ty, _ in mol[2]])
        moved = T.renumber(sym, [int(p) for p in rng.permutation(len(mol[0]))], rng)
        assert bits_of(moved) == bits_of(sym) == want
        assert bits_of(K.redraw(mol, rng)) == want


def test_a_substructure_sets_a_subset():
    small, large = bits_of(chain([b"C", b"C", b"O"])), bits_of(chain([b"C", b"C", b"O", b"C"]))
    assert small < large


def test_no_path_is_longer_than_max_bonds():
    """9 different atoms in a chain: the one path of 8 bonds sets no bit at max_bonds = 7 (its two bit numbers, 711 and 1912, are
    held by no shorter path of this chain — checked here, so the test cannot pass by a collision), and both at no limit on the
    walk but the oracle's own: extending by hand"""
    symbols = [b"C", b"N", b"O", b"S", b"Cl", b"Br", b"I", b"F", b"P"]
    mol = chain(symbols)
    keys = [F.atom_key(s, TABLES) for s in symbols]
    whole = set(F.path_bits([w for k in keys for w in (k, 1)][:-1]))
    got = bits_of(mol, max_bonds=7)
    assert whole == {711, 1912} and not whole & got
    for k in range(1, 8):
        assert bits_of(mol, max_bonds=k) <= bits_of(mol, max_bonds=k + 1 if k < 7 else 7)
    assert bits_of(mol, max_bonds=0) == got                    # 0 means 7
    seven = set(F.path_bits([w for k in keys[:8] for w in (k, 1)][:-1]))
    assert seven <= got and not seven <= bits_of(mol, max_bonds=6)


def test_a_wedge_is_a_single_bond():
    for ty in (5, 6):
        assert bits_of(chain([b"C", b"N", b"O"], ty=ty)) == bits_of(chain([b"C", b"N", b"O"]))
    assert bits_of(chain([b"C", b"N", b"O"], ty=0)) == bits_of(chain([b"C", b"N", b"O"], ty=7)) != bits_of(chain([b"C", b"N", b"O"]))


def test_a_ring_is_never_closed():
    """benzene: every directed bond begins the 5 paths that go on round the ring, of 1 .. 5 bonds"""
    ring = [b"c"] * 6, [(0, 0)] * 6, [(k, (k + 1) % 6, 4, 4) for k in range(6)]
    assert F.fingerprint(ring[0], ring[2], tables=TABLES)[1] == 5
    assert bits_of(ring) == bits_of(ring, max_bonds=5) != bits_of(ring, max_bonds=4)


# ---------------------------------------------------------------------------------------------------------------- the step limit
@functools.lru_cache(maxsize=None)
def complete_graph(n, max_steps=0):
    syms, _, bonds = complete(n)
    return F.fingerprint(syms, bonds, max_steps=max_steps, tables=TABLES)


def test_the_step_limit_on_complete_graphs():
    """P(s) on the complete graph on n atoms is the number of ways to go on from a bond through distinct atoms, up to 6 more bonds:
    the sum over k of (n - 2)(n - 3) .. (n - 1 - k), 1957 for n = 8 and 8660 for n = 9"""
    count = lambda n: sum(int(np.prod([n - 2 - q for q in range(k)])) for k in range(7))        # noqa: E731
    assert (count(8), count(9)) == (1957, 8660)
    bits, most = complete_graph(8)
    assert most == 1957 and bits
    assert complete_graph(9) == (None, F.LIMITED_PATHS)
    bits, most = complete_graph(9, 8660)
    assert most == 8660 and bits
    assert complete_graph(9, 8659) == (None, F.LIMITED_PATHS)
    out = F.pack(*M.build_tables([complete(9), chain([b"C", b"O"])]), tables=TABLES)
    assert out["fp"]["flags"].tolist() == [F.LIMIT, 0] and out["fp"]["max_paths"].tolist() == [F.LIMITED_PATHS, 1]
    assert not out["bits"][0].any() and out["fp"]["n_bits"].tolist() == [0, 6]
    assert (F.DEFAULT_STEPS, F.MAX_STEPS, F.MAX_BONDS, F.WORDS) == (engine.FP_DEFAULT_STEPS, engine.FP_MAX_STEPS, engine.FP_MAX_BONDS, engine.FP_WORDS)


def test_admission():
    ok = chain([b"C", b"[NH3+]", b"O"])
    mols, atoms, bonds, text = M.build_tables([
        ok, chain([b"C"] * 1000), chain([b"C"] * 999), ([b"C", b"N"], [(0, 0)] * 2, [(0, 2, 1, 1)]), ([b"C", b"N"], [(0, 0)] * 2, [(1, 1, 1, 1)]),
        ([b"C", b"N"], [(0, 0)] * 2, [(0, 1, 1, 1), (1, 0, 2, 2)]), chain([b"C", b"Ph", b"[Xx]"]), ([b"R", b"N"], [(0, 0)] * 2, [(0, 0, 1, 1)]), ok])
    mols["flags"][8] = 1 | 1 << 10                                         # truncated; the bits of the passes are not copied
    out = F.pack(mols, atoms, bonds, text, tables=TABLES)
    assert out["fp"]["flags"].tolist() == [0, F.TOO_LARGE, 0, F.BAD_BOND, F.BAD_BOND, F.BAD_BOND, F.PSEUDO, F.PSEUDO | F.BAD_BOND, F.TRUNCATED]
    assert out["fp"]["max_paths"].tolist() == [2, 0, 7, 0, 0, 0, 2, 0, 2]
    assert [bool(w.any()) for w in out["bits"]] == [True, False, True, False, False, False, True, False, True]
    assert (out["bits"][0] == out["bits"][8]).all()
    cut = F.pack(mols, atoms, bonds, text, tables=TABLES, n_text_bytes=len(text) - 1)
    assert cut["fp"]["flags"].tolist()[-1] == F.TRUNCATED | F.BEYOND and cut["fp"]["flags"].tolist()[:-1] == out["fp"]["flags"].tolist()[:-1]
    assert (engine.FP_TOO_LARGE, engine.FP_BEYOND_TABLES, engine.FP_PSEUDO_ATOM, engine.FP_TRUNCATED, engine.FP_BAD_BOND, engine.FP_LIMIT) == \
        (F.TOO_LARGE, F.BEYOND, F.PSEUDO, F.TRUNCATED, F.BAD_BOND, F.LIMIT) == (1, 2, 4, 8, 16, 65536)
    assert engine.FP_DTYPE.itemsize == 16 and engine.FP_DTYPE.names == ("flags", "n_bits", "max_paths", "reserved")


# ---------------------------------------------------------------------------------------------------------------- similarity
def test_tanimoto_identities():
    rows = np.stack([F.words_of(bits_of(m)) for m in molecules()[:12]] + [np.zeros(F.WORDS, np.uint32)])
    n = len(rows)
    same = F.tanimoto(rows, rows)
    assert same["similarity"].tolist() == [1.0] * (n - 1) + [0.0] and (same["both"] == same["either"]).all() and same["either"][-1] == 0
    a, b = rows[np.arange(n)], rows[(np.arange(n) + 1) % n]
    ab, ba = F.tanimoto(a, b), F.tanimoto(b, a)
    assert ab["similarity"].tolist() == ba["similarity"].tolist() and ((0 <= ab["similarity"]) & (ab["similarity"] <= 1)).all()
    assert (ab["both"] <= ab["either"]).all()
    low, high = np.zeros(F.WORDS, np.uint32), np.zeros(F.WORDS, np.uint32)
    low[:32], high[32:] = 0xFFFFFFFF, 0xFFFFFFFF
    d = F.tanimoto([low, low], [high, low | high])
    assert d["both"].tolist() == [0, 1024] and d["either"].tolist() == [2048, 2048] and d["similarity"].tolist() == [0.0, 0.5]
    third = F.tanimoto([F.words_of({1})], [F.words_of({1, 2, 3})])
    assert third["similarity"].tolist() == [1 / 3]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_names_the_engine_loads_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "molnextr_hip.h")).read()
    for name in ("mnx_fingerprint_pack", "mnx_tanimoto"):
        assert name in engine.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert re.search(r"#define MNX_ABI_VERSION 7\b", hdr) and engine.ABI_VERSION == 7
    for name, value in (("MNX_FP_LIMIT", "65536u"), ("MNX_FP_BAD_BOND", "16u"), ("MNX_FP_DEFAULT_STEPS", "4096u"),
                        ("MNX_FP_MAX_STEPS", "(1u << 20)"), ("MNX_FP_MAX_BONDS", "7u"), ("MNX_FP_WORDS", "64u")):
        assert "#define %s %s\n" % (name, value) in hdr, name
    assert "NOT produce RDKit's bits" in hdr


# ------------------------------------------------------------------------------------ the walk under the sanitizers
def walk_input(cases):
    """what tools/paths_host.cpp reads, from (molecule, max_bonds, max_steps) with both limits resolved"""
    lines = [str(len(cases))]
    for (symbols, _, bonds), max_bonds, max_steps in cases:
        lines.append("%d %d %d %d" % (len(symbols), len(bonds), max_bonds, max_steps))
        lines.append(" ".join(str(F.atom_key(s, TABLES)) for s in symbols))
        lines += ["%d %d %d" % (i, j, F.bond_word(ty)) for i, j, ty, _ in bonds]
    return "\n".join(lines) + "\n"


def test_the_walk_header_under_the_sanitizers(tmp_path):
    """tools/paths_host.cpp — a main() around csrc/path_search.h, its stack exactly the 8 levels a walk may touch — built with
    -fsanitize=address,undefined and run once, as a plain executable, over the molecules of this file at every path length, the
    complete graphs at and beside their limits, a chain of 999 atoms and a star: its words, bit counts and path counts are the
    oracle's, and the sanitizers report nothing (a report ends the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "paths_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "paths_host.cpp"), "-o", exe], check=True)
    star = [b"C"] + [b"N", b"O"] * 10, [(0, 0)] * 21, [(0, k, 1, 1) for k in range(1, 21)]
    cases = [(m, 1 + k % 7, F.DEFAULT_STEPS) for k, m in enumerate(molecules())] + [(m, 7, 3) for m in molecules()[:8]]
    cases += [(complete(8), 7, F.DEFAULT_STEPS), (complete(9), 7, F.DEFAULT_STEPS), (complete(9), 7, 8660), (complete(9), 7, 8659),
              (chain([b"C", b"N", b"O"] * 333), 7, F.DEFAULT_STEPS), (star, 7, F.DEFAULT_STEPS), (chain([]), 7, 1), (chain([b"C"]), 1, 1)]
    run = subprocess.run([exe], input=walk_input(cases), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(cases) + 1 and got[-1] == ""
    limited = 0
    for line, (mol, max_bonds, max_steps) in zip(got, cases):
        bits, most = (complete_graph(9, max_steps if max_steps != F.DEFAULT_STEPS else 0) if len(mol[2]) == 36 else
                      F.fingerprint(mol[0], mol[2], max_bonds, max_steps, TABLES))
        limited += bits is None
        want = [most, len(bits or ())] + F.words_of(bits or ()).tolist()
        assert [int(x) for x in line.split()] == want, (len(mol[0]), max_bonds, max_steps)
    assert limited >= 4
    for text in ("1\n2 1 7 9\n1 2\n0 2 1\n", "1\n2 1 8 9\n1 2\n0 1 1\n", "1\n2 2 7 9\n1 2\n0 1 1\n1 0 1\n"):     # no atom; 8 bonds; a pair twice
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2
