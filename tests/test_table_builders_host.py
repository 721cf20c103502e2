"""CPU: the host work of mnx_set_vocab_text, mnx_set_symbol_tables and mnx_set_fragments — csrc/table_host.h, which validates the
caller's offsets and records and lays out the image the device reads — through tools/tables_host.cpp, built with the host compiler's
sanitizers and run once over every case of this file: the shipped tables are accepted and their images are the ones this file
restates from the comments of csrc/table_types.h; every refusal comes with its exact message; the boundaries of each setter."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from molnextr_amd import fragments as F
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE, symbol_tables, vocab_text
from molnextr_amd.tokenizer import CharTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {}          # name -> (the case's text for tools/tables_host.cpp, the lines it must print)


def items(a):
    """a list as the program reads it: its length, then its items"""
    a = list(a)
    return " ".join(map(str, [len(a)] + a))


def part(b, element):
    """a part of the fragment image: room for at least one element, padded with zeros to a multiple of 8 bytes"""
    n = max(len(b), element)
    return b + bytes(n + -n % 8 - len(b))


# ------------------------------------------------------------------------------------------------------ mnx_set_vocab_text
def vocab_case(name, expect, text, offsets, n=None, sym_offset=None, null=0):
    n = len(offsets) - 1 if n is None else n
    sym_offset = n if sym_offset is None else sym_offset
    line = "V %d %d %d %s %s" % (sym_offset, n, null, items(offsets), items(text))
    if isinstance(expect, str):
        CASES[name] = (line, ["refused mnx_set_vocab_text: " + expect])
        return
    # VocabText: len[256], the bytes of id i's name (0 beyond the ids that were set); name[256][8]
    lens, names = bytearray(256), bytearray(256 * 8)
    for i in range(n):
        own = text[offsets[i]:offsets[i + 1]]
        lens[i] = len(own)
        names[8 * i:8 * i + len(own)] = own
    CASES[name] = (line, ["ok", (bytes(lens) + bytes(names)).hex()])


VT, VO, VN = vocab_text(CharTokenizer(64))
VO = VO.tolist()
vocab_case("vocab: the shipped names", True, VT, VO)
vocab_case("vocab: 256 names of 8 bytes, 0 bytes and 1 byte", True, b"".join(b"%08d" % i for i in range(100)) + b"x" * 56,
           [8 * i for i in range(101)] + [800] * 100 + list(range(801, 857)))
vocab_case("vocab: one name", True, b"C", [0, 1])
for what, kw in {"bytes null": {"null": 1}, "offsets null": {"null": 2}, "n = 0": {"n": 0, "sym_offset": 0}, "n = 257": {"n": 257, "sym_offset": 257}}.items():
    vocab_case("vocab: " + what, "null pointer or n outside 1..256", VT, VO, **kw)
vocab_case("vocab: fewer names than symbol ids", "n = %d names, but the vocabulary has cfg.sym_offset = %d symbol ids" % (VN - 1, VN), VT, VO[:-1],
           sym_offset=VN)
vocab_case("vocab: offsets begin at 1", "offsets[0] must be 0", b"xCN", [1, 2, 3])
vocab_case("vocab: a name of 9 bytes", "name of id 1 is longer than 8 bytes or its offsets decrease", b"C123456789", [0, 1, 10])
vocab_case("vocab: offsets decrease", "name of id 2 is longer than 8 bytes or its offsets decrease", b"CNO", [0, 1, 3, 2])


# ------------------------------------------------------------------------------------------------------ mnx_set_symbol_tables
def symbol_case(name, expect, names, kinds=None, offsets=None, n=None, null=0):
    text = b"".join(names)
    kinds = [2] * len(names) if kinds is None else kinds
    offsets = np.cumsum([0] + [len(b) for b in names]).tolist() if offsets is None else offsets
    n = len(names) if n is None else n
    line = "S %d %d %s %s %s" % (n, null, items(offsets), items(kinds), items(text))
    if isinstance(expect, str):
        CASES[name] = (line, ["refused mnx_set_symbol_tables: " + expect])
        return
    # SymbolTables: int n; len[512], the bytes of name i; kind[512]; name[512][16]
    lens, kind, table = bytearray(512), bytearray(512), bytearray(512 * 16)
    for i, b in enumerate(names):
        lens[i], kind[i] = len(b), kinds[i]
        table[16 * i:16 * i + len(b)] = b
    CASES[name] = (line, ["ok", (struct.pack("<i", n) + bytes(lens) + bytes(kind) + bytes(table)).hex()])


ST, SO, SK, SN = symbol_tables()
SO, SK = SO.tolist(), SK.tolist()
SHIPPED_NAMES = [ST[SO[i]:SO[i + 1]] for i in range(SN)]
symbol_case("symbols: the shipped names", True, SHIPPED_NAMES, SK)
symbol_case("symbols: n = 0", True, [])
symbol_case("symbols: n = 0 and null pointers", True, [], null=7)
symbol_case("symbols: n = 512, 16 bytes each", True, [b"n%015d" % i for i in range(512)], [1 + i % 2 for i in range(512)])
symbol_case("symbols: a prefix in front of the longer name", True, [b"a", b"ab", b"b"])
symbol_case("symbols: n = 513", "n outside 0..512", [b"a"], n=513)
symbol_case("symbols: n = -1", "n outside 0..512", [b"a"], n=-1)
for bit, what in enumerate(("bytes", "offsets", "kinds")):
    symbol_case("symbols: %s null" % what, "null pointer", [b"a", b"b"], null=1 << bit)
symbol_case("symbols: offsets begin at 1", "offsets[0] must be 0", [b"xa", b"b"], offsets=[1, 2, 3])
LONG = "name 1 is empty or longer than 16 bytes, or its offsets decrease"
symbol_case("symbols: an empty name", LONG, [b"a", b"", b"b"])
symbol_case("symbols: a name of 17 bytes", LONG, [b"a", b"b" * 17])
symbol_case("symbols: offsets decrease", LONG, [b"abcde", b"f"], offsets=[0, 5, 3])
symbol_case("symbols: kind 0", "kinds[1] must be 1 (R-group) or 2 (abbreviation)", [b"a", b"b"], [1, 0])
symbol_case("symbols: kind 3", "kinds[0] must be 1 (R-group) or 2 (abbreviation)", [b"a", b"b"], [3, 2])
ORDER = "names must be strictly ascending bytewise; name %d is not behind its predecessor"
symbol_case("symbols: the same name twice", ORDER % 2, [b"a", b"b", b"b"])
symbol_case("symbols: a prefix behind the longer name", ORDER % 1, [b"ab", b"a"])
symbol_case("symbols: descending", ORDER % 1, [b"b", b"a"])
symbol_case("symbols: bytes above 127 sort as unsigned", ORDER % 1, [b"\xc3\xa9", b"z"])


# ------------------------------------------------------------------------------------------------------ mnx_set_fragments
def fragment_image(mols, atoms, bonds, text, frag_of_name):
    """The image of table_types.h (FragRec / FragView), restated: ONE allocation of five parts, each 8-byte aligned and none empty — the
    int32 table of fragment indices parallel to the names; the records {atom0, bond0, text0: where the fragment's atoms / bonds /
    symbol bytes begin in the three arrays; n_atoms, n_bonds, n_bonds0 (its bonds from atom 0), text_len} of 3 x uint32 + 4 x uint16;
    per atom sym0 | sym_len << 16, sym0 counted from the fragment's text0; per bond i | j << 8 | type << 16, a fragment's bonds sorted
    by (i, j); every fragment's symbols behind one another. Returns (the five offsets, the bytes)."""
    recs, fa, fb, ft = b"", [], [], b""
    for m in mols:
        a0, b0, t0 = len(fa), len(fb), len(ft)
        for a in atoms[int(m["atom0"]):int(m["atom0"]) + int(m["n_atoms"])]:
            begin = int(m["text0"]) + int(a["sym0"])
            fa.append(len(ft) - t0 | int(a["sym_len"]) << 16)
            ft += text[begin:begin + int(a["sym_len"])]
        own = sorted((int(b["i"]), int(b["j"]), int(b["type"])) for b in bonds[int(m["bond0"]):int(m["bond0"]) + int(m["n_bonds"])])
        fb += [i | j << 8 | ty << 16 for i, j, ty in own]
        recs += struct.pack("<3I4H", a0, b0, t0, int(m["n_atoms"]), len(own), sum(i == 0 for i, j, ty in own), len(ft) - t0)
    parts = [part(np.asarray(frag_of_name, "<i4").tobytes(), 4), part(recs, 20), part(np.asarray(fa, "<u4").tobytes(), 4),
             part(np.asarray(fb, "<u4").tobytes(), 4), part(ft, 1)]
    return np.cumsum([0] + [len(p) for p in parts[:-1]]).tolist(), b"".join(parts)


def fragment_case(name, expect, tables, kinds, edit=None, **over):
    """one mnx_set_fragments call: `tables` of fragments.fragment_tables() after edit(mols, atoms, bonds, frag_of_name); `over` replaces
    the counts passed beside the arrays (n_frags, na, nb, nt, n_names, st_n) or names the null pointers (null)"""
    mols, atoms, bonds, text, fo = (x.copy() if isinstance(x, np.ndarray) else x for x in tables)
    if edit:
        edit(mols, atoms, bonds, fo)
    a = {"n_frags": len(mols), "na": len(atoms), "nb": len(bonds), "nt": len(text), "n_names": len(fo), "st_n": len(kinds), "null": 0}
    a.update(over)
    line = "F %d %d %d %d %d %d %d\n" % tuple(a.values())
    line += "%d %s\n" % (len(mols), " ".join("%d %d %d %d %d %d" % tuple(int(m[k]) for k in MOL_DTYPE.names[:6]) for m in mols))
    line += "%d %s\n" % (len(atoms), " ".join("%d %d" % (a["sym0"], a["sym_len"]) for a in atoms))
    line += "%d %s\n" % (len(bonds), " ".join("%d %d %d %d" % (b["i"], b["j"], b["type"], b["rev"]) for b in bonds))
    line += "%s %s %s" % (items(text), items(fo.tolist()), items(kinds))
    if isinstance(expect, str):
        CASES[name] = (line, ["refused mnx_set_fragments: " + expect])
        return
    off, image = fragment_image(mols, atoms, bonds, text, fo)
    CASES[name] = (line, ["ok %d %d %d %d %d" % tuple(off), image.hex()])


LIB = F.fragment_tables()
NF = len(LIB[0])
EMPTY = (np.zeros(0, MOL_DTYPE), np.zeros(0, ATOM_DTYPE), np.zeros(0, BOND_DTYPE), b"", np.zeros(0, np.int32))
fragment_case("fragments: the shipped library", True, LIB, SK)


def reversed_bonds(mols, atoms, bonds, fo):
    for m in mols:
        b0, nb = int(m["bond0"]), int(m["n_bonds"])
        bonds[b0:b0 + nb] = bonds[b0:b0 + nb][::-1]


fragment_case("fragments: every fragment's bonds handed over in reverse", True, LIB, SK, reversed_bonds)
OWN = F.fragment_tables({"Fmoc": "C1CCCCC1" + "C" * 24 + "(=O)O", "Ph": "N#C", "OMe": "[Si](C)(C)C.Cl"})
assert OWN[0]["n_atoms"].max() == 32
fragment_case("fragments: 32 atoms", True, OWN, SK)
fragment_case("fragments: n_frags = 0", True, (LIB[0][:0], LIB[1], LIB[2], LIB[3], np.full(SN, -1, np.int32)), SK)
fragment_case("fragments: empty tables and no name", True, EMPTY, [])
fragment_case("fragments: empty tables, no name, null pointers", True, EMPTY, [], null=31)
fragment_case("fragments: n_frags = 513", "n_frags outside 0..512", LIB, SK, n_frags=513)
fragment_case("fragments: n_frags = -1", "n_frags outside 0..512", LIB, SK, n_frags=-1)
fragment_case("fragments: other names", "n_names must be the n of mnx_set_symbol_tables (%d)" % SN, LIB, SK, n_names=SN - 1)
for bit, what in enumerate(("frags", "atoms", "bonds", "text", "frag_of_name")):
    fragment_case("fragments: %s null" % what, "null pointer", LIB, SK, null=1 << bit)


def field(table, name, value, k=0):
    def edit(*tables):
        tables[table][name][k] = value
    return edit


fragment_case("fragments: 0 atoms", "fragment 0 has 0 atoms; 1 to 32 required", LIB, SK, field(0, "n_atoms", 0))
fragment_case("fragments: 33 atoms", "fragment 1 has 33 atoms; 1 to 32 required", LIB, SK, field(0, "n_atoms", 33, 1))
BEHIND = "fragment %d: its records end behind a table"
for key in ("atom0", "bond0", "text0"):
    fragment_case("fragments: %s behind its table" % key, BEHIND % 0, LIB, SK, field(0, key, 1 << 30))
fragment_case("fragments: atom0 + n_atoms wraps 32 bits", BEHIND % 0, LIB, SK, field(0, "atom0", 0xFFFFFFFF))
CUT = int(np.nonzero(LIB[0]["atom0"] + LIB[0]["n_atoms"] > 3)[0][0])
fragment_case("fragments: fewer atom records than the fragments use", BEHIND % CUT, LIB, SK, na=3)
fragment_case("fragments: the last fragment's text is one byte short", BEHIND % (NF - 1), LIB, SK, nt=len(LIB[3]) - 1)
SYMBOL = "fragment 0, atom 0: a symbol has 1 to 8 bytes"
fragment_case("fragments: a symbol of 0 bytes", SYMBOL, LIB, SK, field(1, "sym_len", 0))
fragment_case("fragments: a symbol of 9 bytes", SYMBOL, LIB, SK, field(1, "sym_len", 9))
fragment_case("fragments: a symbol behind the text", "fragment 0, atom 0: its symbol ends behind the text", LIB, SK, field(1, "sym0", 1 << 20))
LAST_ATOM = int(LIB[0]["atom0"][-1] + LIB[0]["n_atoms"][-1] - 1)
fragment_case("fragments: the last symbol ends one byte behind the text",
              "fragment %d, atom %d: its symbol ends behind the text" % (NF - 1, LIB[0]["n_atoms"][-1] - 1), LIB, SK,
              field(1, "sym_len", int(LIB[1]["sym_len"][LAST_ATOM]) + 1, LAST_ATOM))
FB = int(np.nonzero(LIB[0]["n_bonds"] > 1)[0][0])                                   # the first fragment with two bonds ...
KB = int(LIB[0]["bond0"][FB])                                                       # ... and its first bond
PAIR = "fragment %d, bond 0: i < j < n_atoms required" % FB
TYPE = "fragment %d, bond 0: type 1 to 4 and rev == type required" % FB
fragment_case("fragments: i >= j", PAIR, LIB, SK, field(2, "i", 31, KB))
fragment_case("fragments: i == j", PAIR, LIB, SK, field(2, "i", int(LIB[2]["j"][KB]), KB))
fragment_case("fragments: j >= n_atoms", PAIR, LIB, SK, field(2, "j", int(LIB[0]["n_atoms"][FB]), KB))
fragment_case("fragments: j = 32", PAIR, LIB, SK, field(2, "j", 32, KB))
fragment_case("fragments: type 0", TYPE, LIB, SK, field(2, "type", 0, KB))
fragment_case("fragments: type 5", TYPE, LIB, SK, field(2, "type", 5, KB))
fragment_case("fragments: rev != type", TYPE, LIB, SK, field(2, "rev", int(LIB[2]["type"][KB]) % 4 + 1, KB))


def twice(mols, atoms, bonds, fo):
    bonds["i"][KB + 1], bonds["j"][KB + 1] = bonds["i"][KB], bonds["j"][KB]


fragment_case("fragments: a pair of atoms twice", "fragment %d: the same pair of atoms in two bonds" % FB, LIB, SK, twice)
RANGE = "frag_of_name[0] outside -1..%d" % (NF - 1)
fragment_case("fragments: frag_of_name = n_frags", RANGE, LIB, SK, field(3, slice(None), NF))
fragment_case("fragments: frag_of_name = -2", RANGE, LIB, SK, field(3, slice(None), -2))
fragment_case("fragments: frag_of_name with no fragment at all", "frag_of_name[0] outside -1..-1",
              (LIB[0][:0], LIB[1], LIB[2], LIB[3], np.zeros(SN, np.int32)), SK)
RGROUP = SK.index(1)
fragment_case("fragments: a fragment for an R-group", "frag_of_name[%d]: only an abbreviation (kind 2) takes a fragment" % RGROUP, LIB, SK,
              field(3, slice(None), 0, RGROUP))


# ------------------------------------------------------------------------------------------------------ one build, one run
@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """what tools/tables_host.cpp prints for every case: built with -fsanitize=address,undefined -fno-sanitize-recover=all and run
    once, as a plain executable (a report of a sanitizer ends the program with a status other than 0)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("tables_host") / "tables_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "tables_host.cpp"), "-o", exe], check=True)
    text = "%d\n" % len(CASES) + "".join(line + "\n" for line, _ in CASES.values())
    run = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == ""
    out, at = {}, 0
    for name, (_, want) in CASES.items():
        out[name] = got[at:at + len(want)]
        at += len(want)
    assert at == len(got) - 1, (at, len(got))
    return out


def accepted(name):
    return CASES[name][1][0].startswith("ok")


def test_the_shipped_tables_are_accepted_and_their_images_are_the_restated_ones(printed):
    for name in ("vocab: the shipped names", "symbols: the shipped names", "fragments: the shipped library"):
        assert printed[name][0].startswith("ok") and printed[name] == CASES[name][1], name
    off, image = fragment_image(*LIB)
    assert all(o % 8 == 0 for o in off) and len(image) % 8 == 0 and off[1] == (4 * SN + 7) // 8 * 8
    # sorting is part of the image: bonds handed over in reverse give the very bytes of the shipped order
    assert printed["fragments: every fragment's bonds handed over in reverse"] == printed["fragments: the shipped library"]


@pytest.mark.parametrize("name", [k for k in CASES if not accepted(k)])
def test_every_refusal_with_its_message(printed, name):
    assert printed[name] == CASES[name][1]


@pytest.mark.parametrize("name", [k for k in CASES if accepted(k)])
def test_accepted_tables_and_the_boundaries(printed, name):
    got, want = printed[name], CASES[name][1]
    assert got[0] == want[0] and len(got[1]) == len(want[1])
    assert got[1] == want[1], next(i // 2 for i in range(0, len(want[1]), 2) if got[1][i:i + 2] != want[1][i:i + 2])


def test_the_cases_cover_every_message_of_the_header():
    """every string the three builders can refuse with occurs among the expected lines"""
    src = open(os.path.join(ROOT, "molnextr_amd", "csrc", "table_host.h")).read()
    wanted = " ".join(want[0] for _, want in CASES.values())
    for piece in ("null pointer or n outside 1..256", "symbol ids", "offsets[0] must be 0", "is longer than 8 bytes or its offsets decrease",
                  "n outside 0..512", "null pointer", "is empty or longer than 16 bytes, or its offsets decrease",
                  "must be 1 (R-group) or 2 (abbreviation)", "names must be strictly ascending bytewise", "n_frags outside 0..512",
                  "n_names must be the n of mnx_set_symbol_tables", "atoms; 1 to 32 required", ": its records end behind a table",
                  ": a symbol has 1 to 8 bytes", ": its symbol ends behind the text", ": i < j < n_atoms required",
                  ": type 1 to 4 and rev == type required", ": the same pair of atoms in two bonds", "] outside -1..",
                  "]: only an abbreviation (kind 2) takes a fragment"):
        assert piece in src and piece in wanted, piece
    assert src.count("return bad(") + src.count('return "mnx_set_vocab_text') == 22
