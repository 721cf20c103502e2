"""The oracle of mnx_expand_pack (include/molnextr_hip.h) in plain Python, tables in and tables out: abbreviation labels
replaced by the atoms and bonds of their fragments. It shares no code with the kernel or with molnextr_amd/fragments.py: the
fragment SMILES are read by smiles_ref.read (the reader of what mnx_smiles_pack emits) behind a check of the narrower grammar, the
atom interpretation is molfile_ref's, and the new tables are put together as Python lists and sorted, where the kernel scans."""
import json
import os
import re

import numpy as np

import molfile_ref as M
import smiles_ref as S
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE

EXPANDED, LABEL_LEFT, REFUSED = 2, 4, 8
MAX_FRAGMENT, MAX_ATOMS = 32, 2047
JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "molnextr_amd", "vocab", "fragments.json")
GRAMMAR = re.compile(r"(?:Cl|Br|[BCNOPSFIbcnops]|\[[^\[\]*@:]+\]|[-=#().]|[1-9])+")
SYMBOL_TYPE = {"-": 1, "=": 2, "#": 3}


def _lower(token: str) -> bool:
    return token.strip("[]").lstrip("0123456789")[:1].islower()


def read_fragment(smiles: str, tables=None):
    """(symbols [bytes], bonds [(i, j, type)] sorted, i < j); ValueError outside the grammar of fragments.json"""
    tables = M.name_tables() if tables is None else tables
    if GRAMMAR.fullmatch(smiles) is None:
        raise ValueError(f"{smiles!r} is outside the fragment grammar")
    atoms, joined = S.read(smiles)
    if not 1 <= len(atoms) <= MAX_FRAGMENT:
        raise ValueError(f"{smiles!r}: {len(atoms)} atoms")
    for a in atoms:
        if M.interpret(a.encode(), tables)["pseudo"] or len(a) > 8:
            raise ValueError(f"{smiles!r}: {a!r} is no parsed atom of at most 8 bytes")
    bonds = []
    for (a, b), symbol in joined.items():
        if symbol not in ("", "-", "=", "#"):
            raise ValueError(f"{smiles!r}: bond {symbol!r}")
        bonds.append((a, b, SYMBOL_TYPE[symbol] if symbol else 4 if _lower(atoms[a]) and _lower(atoms[b]) else 1))
    return [a.encode() for a in atoms], sorted(bonds)


def library(path=JSON, tables=None):
    """{name bytes: (symbols, bonds)} of fragments.json"""
    with open(path) as f:
        return {k.encode("utf-8"): read_fragment(v, tables) for k, v in json.load(f)["fragments"].items()}


def fragment_of(sym: bytes, frags, tables):
    """the fragment an atom's symbol expands to, or None: brackets stripped, R-group table first, then the abbreviations"""
    inner = sym[1:-1] if len(sym) >= 2 and sym[:1] == b"[" and sym[-1:] == b"]" else sym
    return frags.get(inner) if tables.get(inner) == 2 else None


def expand_molecule(symbols, atoms, bonds, frags, tables):
    """One admitted molecule: symbols [bytes], atoms [(index, x_bin, y_bin, score)], bonds [(i, j, type, rev, score)] ->
    (symbols, atoms, bonds, origin, flags) of the expanded one"""
    n = len(symbols)
    out_sym, out_atoms, origin = list(symbols), list(atoms), list(range(n))
    keyed = [((b[0], 0, k), b) for k, b in enumerate(bonds)]
    flags = 0
    for at in range(n):
        frag = fragment_of(symbols[at], frags, tables)
        if frag is None:
            if M.interpret(symbols[at], tables)["pseudo"]:
                flags |= LABEL_LEFT
            continue
        flags |= EXPANDED
        fsym, fbonds = frag
        where = [at] + list(range(len(out_sym), len(out_sym) + len(fsym) - 1))
        out_sym[at] = fsym[0]
        out_sym += fsym[1:]
        out_atoms += [atoms[at]] * (len(fsym) - 1)
        origin += [at] * (len(fsym) - 1)
        for i, j, ty in fbonds:
            keyed.append(((where[i], 1, where[j]), (where[i], where[j], ty, ty, atoms[at][3])))
    return out_sym, out_atoms, [b for _, b in sorted(keyed, key=lambda e: e[0])], origin, flags


def pack(mols, atoms, bonds, text, frags=None, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_expand_pack on host arrays: {'mols', 'atoms', 'bonds', 'text', 'origin', 'totals'}"""
    tables = M.name_tables() if tables is None else tables
    frags = library(tables=tables) if frags is None else frags
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    out_mols = np.zeros(len(mols), MOL_DTYPE)
    A, B, origin, chunks, at_text = [], [], [], [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        keep = int(m["flags"]) & 1
        refused = a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t or na > MAX_ATOMS
        if not refused:
            ma, mb = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            rows = [int(x["i"]) for x in mb]
            refused = (any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in ma) or
                       any(int(x["i"]) >= na or int(x["j"]) >= na for x in mb) or rows != sorted(rows))
        if refused:
            out_mols[b] = (len(A), 0, len(B), 0, at_text, 0, keep | REFUSED, 0, float(m["overall_score"]))
            continue
        syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma]
        s2, a2, b2, o2, flags = expand_molecule(
            syms, [(int(a["index"]), int(a["x_bin"]), int(a["y_bin"]), float(a["score"])) for a in ma],
            [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"]), float(x["score"])) for x in mb], frags, tables)
        own = b"".join(s2)
        out_mols[b] = (len(A), len(s2), len(B), len(b2), at_text, len(own), keep | flags, 0, float(m["overall_score"]))
        off = 0
        for s, (index, x, y, score) in zip(s2, a2):
            A.append((off, len(s), index, x, y, score))
            off += len(s)
        B += b2
        origin += o2
        chunks.append(own)
        at_text += len(own)
    return {"mols": out_mols, "atoms": np.array(A, ATOM_DTYPE).reshape(-1), "bonds": np.array(B, BOND_DTYPE).reshape(-1),
            "text": b"".join(chunks), "origin": np.array(origin, np.uint16), "totals": (len(A), len(B), at_text)}


def molecules(rec):
    """(symbols, xy, bonds [(i, j, type, rev)]) of every molecule of packed tables: what the writers' oracles take"""
    out = []
    for m in rec["mols"]:
        a0, na, b0, nb, t0 = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0"))
        ma, mb = rec["atoms"][a0:a0 + na], rec["bonds"][b0:b0 + nb]
        out.append(([rec["text"][t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma],
                    [(int(a["x_bin"]), int(a["y_bin"])) for a in ma],
                    [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in mb]))
    return out
