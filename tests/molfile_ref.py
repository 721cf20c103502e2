"""The oracle of mnx_molfile_pack (include/molnextr_hip.h): CTfile V2000 molfiles from the packed molecule records
(MOL_DTYPE / ATOM_DTYPE / BOND_DTYPE arrays and the text bytes), in plain Python — the symbol interpretation of the
reference's _convert_graph_to_smiles (chemical.py:886-903) with a regular expression for the SMILES atom, the integer
coordinate rule, the line formats with the % operator. Shares no code with the kernels."""
import re

import numpy as np

from molnextr_amd import chem
from molnextr_amd.engine import MOLFILE_DTYPE

ELEMENTS = ("H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo "
            "Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl "
            "Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
assert len(ELEMENTS) == len(set(ELEMENTS)) == 118
_LONGEST_FIRST = "|".join(sorted(ELEMENTS, key=len, reverse=True)).encode()
BRACKET_ATOM = re.compile(rb"\[(\d+)?(se|as|[bcnops]|\*|" + _LONGEST_FIRST + rb")(@@?)?(H\d?)?(\++|-+|[+-]\d+)?(:\d+)?\]")
PLAIN_ATOMS = {s.encode() for s in "B C N O P S F Cl Br I b c n o p s *".split()}
CHIRAL_CARBONS = (b"[C@]", b"[C@@]", b"[C@H]", b"[C@@H]")
FLAG_TOO_LARGE, FLAG_BEYOND, FLAG_PSEUDO, FLAG_TRUNCATED = 1, 2, 4, 8
DEFAULT_SCALE = 100000
HEADER = "\n  MolNexTR          2D\n\n"


def name_tables():
    """{name bytes: kind} of the reference's tables: 1 R-group (tested first, so it wins a name in both), 2 abbreviation"""
    t = {s.encode("utf-8"): 2 for s in chem.ABBREVIATIONS}
    t.update({s.encode("utf-8"): 1 for s in chem.RGROUP_SYMBOLS})
    return t


def parse_smiles_atom(sym: bytes):
    """(element capitalised, bracket, H count, charge, isotope) of the whole symbol as a SMILES atom, None = no parse"""
    if sym in PLAIN_ATOMS:
        return ("R" if sym == b"*" else sym.decode().capitalize()), False, 0, 0, 0
    m = BRACKET_ATOM.fullmatch(sym)
    if m is None:
        return None
    iso, el, _, h, q, _ = m.groups()
    isotope = int(iso) if iso else 0
    hcount = 0 if not h else int(h[1:]) if len(h) > 1 else 1
    charge = 0
    if q:
        mag = int(q[1:]) if q[1:].isdigit() else len(q)
        charge = mag if q[:1] == b"+" else -mag
    if isotope > 999 or abs(charge) > 15:
        return None
    return ("R" if el == b"*" else el.decode().capitalize()), True, hcount, charge, isotope


def interpret(sym: bytes, tables) -> dict:
    """One atom: {'symbol' (the 3-byte column's text), 'pseudo', 'bracket', 'h', 'charge', 'isotope', 'rgroup' (number or 0),
    'alias' (bytes or None), 'chiral'}"""
    inner = sym[1:-1] if len(sym) >= 2 and sym[:1] == b"[" and sym[-1:] == b"]" else sym
    a = {"pseudo": False, "bracket": False, "h": 0, "charge": 0, "isotope": 0, "rgroup": 0, "alias": None,
         "chiral": sym in CHIRAL_CARBONS}
    kind = tables.get(inner)
    parsed = parse_smiles_atom(sym) if kind is None else None
    if parsed is not None:
        a["symbol"], a["bracket"], a["h"], a["charge"], a["isotope"] = parsed
        return a
    a["pseudo"], a["symbol"] = True, "R"
    if kind == 1 and re.fullmatch(rb"R\d+", inner) and 1 <= int(inner[1:]) <= 999:
        a["symbol"], a["rgroup"] = "R#", int(inner[1:])
    if inner:
        cut = inner[:70]
        while len(inner) > 70 and cut and (inner[len(cut)] & 0xC0) == 0x80:      # not through a UTF-8 character
            cut = cut[:-1]
        a["alias"] = bytes(63 if c < 0x20 or c == 0x7F else c for c in cut) or None
    return a


def coordinate(u: int) -> str:
    return "%5d.%04d" % (u // 10000, u % 10000)


def units(x_bin: int, y_bin: int, sx: int, sy: int, den: int):
    """(ux, uy) in units of 1e-4: round-half-up of bin * S / den in integers, y pointing up"""
    xb, yb = min(int(x_bin), den), min(int(y_bin), den)
    return (2 * xb * sx + den) // (2 * den), (2 * (den - yb) * sy + den) // (2 * den)


def _prop_lines(tag, pairs):
    out = []
    for k in range(0, len(pairs), 8):
        chunk = pairs[k:k + 8]
        out.append("M  %s%3d" % (tag, len(chunk)) + "".join(" %3d %3d" % p for p in chunk))
    return out


ORDER = {1: 1, 2: 2, 3: 3, 5: 1, 6: 1}


def molfile(symbols, xy_bins, bonds, sx=DEFAULT_SCALE, sy=DEFAULT_SCALE, den=63, tables=None):
    """The molfile (bytes) of one molecule: symbols [bytes], xy_bins [(x_bin, y_bin)], bonds [(i, j, type, rev)]"""
    tables = name_tables() if tables is None else tables
    atoms = [interpret(s, tables) for s in symbols]
    lines = ["%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (len(atoms), len(bonds))]
    for k, (a, (xb, yb)) in enumerate(zip(atoms, xy_bins)):
        ux, uy = units(xb, yb, sx, sy, den)
        val = 0
        if not a["pseudo"] and a["bracket"]:
            mine = [b for b in bonds if k in (b[0], b[1])]
            if not any(b[2] == 4 for b in mine):
                total = a["h"] + sum(ORDER.get(b[2], 0) for b in mine)
                val = 15 if total == 0 else 0 if total > 14 else total
        lines.append("%s%s%s %-3s 0  0  0  0  0%3d  0  0  0  0  0  0" % (coordinate(ux), coordinate(uy), coordinate(0), a["symbol"], val))
        assert len(lines[-1]) == 69
    for i, j, ty, rv in bonds:
        swap = atoms[j]["chiral"] and rv in (5, 6)
        cls = rv if swap else ty
        first, second = (j, i) if swap else (i, j)
        bt = cls if 1 <= cls <= 4 else 1 if cls in (5, 6) else 8
        lines.append("%3d%3d%3d%3d" % (first + 1, second + 1, bt, {5: 1, 6: 6}.get(cls, 0)))
        assert len(lines[-1]) == 12
    body = ("\n".join(lines) + "\n").encode("ascii")
    for k, a in enumerate(atoms):
        if a["alias"]:
            body += b"A  %3d\n" % (k + 1) + a["alias"] + b"\n"
    props = _prop_lines("CHG", [(k + 1, a["charge"]) for k, a in enumerate(atoms) if a["charge"]])
    props += _prop_lines("ISO", [(k + 1, a["isotope"]) for k, a in enumerate(atoms) if a["isotope"]])
    props += _prop_lines("RGP", [(k + 1, a["rgroup"]) for k, a in enumerate(atoms) if a["rgroup"]])
    props.append("M  END")
    return HEADER.encode() + body + ("\n".join(props) + "\n").encode("ascii"), any(a["pseudo"] for a in atoms)


def pack(mols, atoms, bonds, text, scale=None, den=63, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_molfile_pack on host arrays: {'files' MOLFILE_DTYPE [n], 'out' bytes, 'total' int}. The n_* default to the sizes of
    the arrays; smaller ones make the molecules whose records reach beyond them refused (flag bit 1)."""
    tables = name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    files = np.zeros(len(mols), MOLFILE_DTYPE)
    chunks, at = [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        flags = FLAG_TRUNCATED if int(m["flags"]) & 1 else 0
        if na > 999 or nb > 999:
            flags |= FLAG_TOO_LARGE
        if a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t:
            flags |= FLAG_BEYOND
        data = b""
        if not flags & 3:
            A, B = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            if any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in A) or any(int(x["i"]) >= na or int(x["j"]) >= na for x in B):
                flags |= FLAG_BEYOND
            else:
                syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in A]
                sx, sy = (DEFAULT_SCALE, DEFAULT_SCALE) if scale is None else (min(max(int(s), 1), 10000000) for s in scale[b])
                data, pseudo = molfile(syms, [(int(a["x_bin"]), int(a["y_bin"])) for a in A],
                                       [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in B], sx, sy, den, tables)
                flags |= FLAG_PSEUDO if pseudo else 0
        files[b] = (min(at, 0xFFFFFFFF), len(data), flags, 0)
        chunks.append(data)
        at += len(data)
    return {"files": files, "out": b"".join(chunks), "total": at}


def build_tables(molecules):
    """Packed records of hand-made molecules [(symbols [bytes], xy_bins, bonds [(i, j, type, rev)])]: (mols, atoms, bonds, text)
    as mnx_graph_pack lays them out — the molecule's text is its symbols behind one another."""
    from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE
    mols = np.zeros(len(molecules), MOL_DTYPE)
    A, B, text = [], [], b""
    for b, (syms, xy, bonds) in enumerate(molecules):
        own = b"".join(syms)
        mols[b] = (len(A), len(syms), len(B), len(bonds), len(text), len(own), 0, 0, 0.0)
        off = 0
        for k, (s, (x, y)) in enumerate(zip(syms, xy)):
            A.append((off, len(s), k, x, y, 0.0))
            off += len(s)
        B += [(i, j, ty, rv, 0.0) for i, j, ty, rv in bonds]
        text += own
    return mols, np.array(A, ATOM_DTYPE).reshape(-1), np.array(B, BOND_DTYPE).reshape(-1), text
