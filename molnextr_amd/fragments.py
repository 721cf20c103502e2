"""The fragment library of mnx_expand_pack (include/molnextr_hip.h): vocab/fragments.json — abbreviation name -> fragment SMILES,
written for this project from what each abbreviation means chemically — read into packed tables of the record types of
mnx_graph_pack, as mnx_set_fragments takes them. Host side, no toolkit.

The grammar of a fragment SMILES is a subset of what mnx_smiles_pack writes: organic-subset atoms (B C N O P S F Cl Br I,
b c n o p s) and bracket atoms; the bonds - = #, and nothing for a single bond or, between two aromatic atoms, an aromatic bond;
branches in parentheses; ring closure digits 1 to 9; '.' between the parts of an ionic pair. No stereo, no '%nn', no ':' or '~'.
The first atom is the attachment atom: every bond of the label goes to it. Anything else raises ValueError, and so does a
fragment of no atom or of more than MAX_ATOMS, an atom symbol of more than 8 bytes, and an atom symbol that the writers would
not read as an atom of the grammar (chem.classify_symbol: a fragment atom must never itself look like a table name)."""
import json
import os
import re

import numpy as np

from .chem import ABBREVIATIONS, classify_symbol

MAX_ATOMS = 32
MAX_SYMBOL = 8
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vocab", "fragments.json")
_ATOM = re.compile(r"Cl|Br|[BCNOPSFIbcnops]|\[[^\[\]]+\]")
# a bracket atom as the writers read one (include/molnextr_hip.h), without the chirality mark and the atom class
_BRACKET = re.compile(r"\[(\d{1,3})?([A-Z][a-z]?|se|as|[bcnops])(H\d?)?(\++|-+|[+-]\d+)?\]")
_ELEMENTS = frozenset(
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh "
    "Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr "
    "Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og".split())
_BOND = {"-": 1, "=": 2, "#": 3}


def _check_atom(sym: str, where: str):
    if len(sym.encode("utf-8")) > MAX_SYMBOL:
        raise ValueError(f"{where}: atom {sym!r} is longer than {MAX_SYMBOL} bytes")
    if sym[0] == "[":
        m = _BRACKET.fullmatch(sym)
        ok = m is not None and (m.group(2)[0].islower() or m.group(2) in _ELEMENTS)
        if ok and m.group(4):
            q = m.group(4)
            ok = (int(q[1:]) if q[1:].isdigit() else len(q)) <= 15
        if not ok:
            raise ValueError(f"{where}: {sym!r} is no bracket atom of the grammar")
    if classify_symbol(sym) != "atom":
        raise ValueError(f"{where}: atom {sym!r} is a name of the R-group / abbreviation tables")


def parse(smiles: str, where: str = "fragment"):
    """One fragment SMILES -> (symbols [str], bonds [(i, j, type)] with i < j, sorted): type 1 2 3, 4 for an aromatic bond."""
    symbols, bonds, stack, rings = [], {}, [], {}
    prev, pending, k = None, None, 0

    def join(a, b, symbol):
        if symbol is None:
            ty = 4 if _aromatic(symbols[a]) and _aromatic(symbols[b]) else 1
        else:
            ty = _BOND[symbol]
        key = (min(a, b), max(a, b))
        if a == b or key in bonds:
            raise ValueError(f"{where}: a bond twice or from an atom to itself in {smiles!r}")
        bonds[key] = ty

    while k < len(smiles):
        m = _ATOM.match(smiles, k)
        if m:
            _check_atom(m.group(), where)
            symbols.append(m.group())
            me = len(symbols) - 1
            if prev is not None:
                join(prev, me, pending)
            elif pending is not None:
                raise ValueError(f"{where}: a bond symbol in front of an atom without a neighbour in {smiles!r}")
            prev, pending, k = me, None, m.end()
            continue
        c = smiles[k]
        k += 1
        if c in _BOND:
            if prev is None or pending is not None:
                raise ValueError(f"{where}: misplaced {c!r} in {smiles!r}")
            pending = c
        elif c in "123456789":
            if prev is None:
                raise ValueError(f"{where}: a ring digit in front of the first atom in {smiles!r}")
            if c in rings:
                a, symbol = rings.pop(c)
                if pending is not None and symbol is not None and pending != symbol:
                    raise ValueError(f"{where}: two bond symbols at ring closure {c} in {smiles!r}")
                join(a, prev, pending if pending is not None else symbol)
            else:
                rings[c] = (prev, pending)
            pending = None
        elif c == "(":
            if prev is None or pending is not None:
                raise ValueError(f"{where}: misplaced '(' in {smiles!r}")
            stack.append(prev)
        elif c == ")":
            if not stack or pending is not None:
                raise ValueError(f"{where}: misplaced ')' in {smiles!r}")
            prev = stack.pop()
        elif c == ".":
            if prev is None or pending is not None or stack:
                raise ValueError(f"{where}: misplaced '.' in {smiles!r}")
            prev = None
        else:
            raise ValueError(f"{where}: {c!r} is outside the grammar of a fragment in {smiles!r}")
    if rings or stack or pending is not None or (prev is None and symbols):
        raise ValueError(f"{where}: unclosed ring, branch or bond in {smiles!r}")
    if not 1 <= len(symbols) <= MAX_ATOMS:
        raise ValueError(f"{where}: {len(symbols)} atoms in {smiles!r}; 1 to {MAX_ATOMS} are supported")
    return symbols, sorted((i, j, ty) for (i, j), ty in bonds.items())


def _aromatic(sym: str) -> bool:
    return (sym[1:].lstrip("0123456789") if sym[0] == "[" else sym)[0].islower()


def load(path: str = _PATH) -> dict:
    """{name: fragment SMILES} of vocab/fragments.json; every name must be a key of the abbreviation table"""
    with open(path) as f:
        table = json.load(f)["fragments"]
    unknown = sorted(set(table) - ABBREVIATIONS)
    if unknown:
        raise ValueError(f"fragments.json: {unknown} are no abbreviations of vocab/abbreviations.json")
    return table


def pack(table: dict):
    """{name: SMILES} -> (mols MOL_DTYPE [n_frags], atoms ATOM_DTYPE, bonds BOND_DTYPE, text bytes, names [n_frags] of lists):
    one record per DISTINCT fragment SMILES (synonyms share it), in sorted order of the SMILES; names[f] = its names."""
    from .abi import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE
    by_smiles = {}
    for name, smi in table.items():
        by_smiles.setdefault(smi, []).append(name)
    order = sorted(by_smiles)
    mols = np.zeros(len(order), MOL_DTYPE)
    A, B, text = [], [], b""
    for f, smi in enumerate(order):
        symbols, bonds = parse(smi, "fragment of " + "/".join(sorted(by_smiles[smi])))
        own = "".join(symbols).encode("ascii")
        mols[f] = (len(A), len(symbols), len(B), len(bonds), len(text), len(own), 0, 0, 0.0)
        off = 0
        for s in symbols:
            A.append((off, len(s), 0, 0, 0, 0.0))
            off += len(s)
        B += [(i, j, ty, ty, 0.0) for i, j, ty in bonds]
        text += own
    return (mols, np.array(A, ATOM_DTYPE).reshape(-1), np.array(B, BOND_DTYPE).reshape(-1), text,
            [sorted(by_smiles[s]) for s in order])


def fragment_tables(table: dict = None):
    """mnx_set_fragments arguments: (mols, atoms, bonds, text, frag_of_name int32 [n_names]) — frag_of_name is parallel to the
    names of engine.symbol_tables(): the fragment of name k, or -1. A name that the symbol tables list as an R-group (it is in
    both of the reference's tables) takes no fragment."""
    from .engine import symbol_tables
    mols, atoms, bonds, text, names = pack(load() if table is None else table)
    raw, offsets, kinds, n = symbol_tables()
    index = {raw[offsets[k]:offsets[k + 1]]: k for k in range(n)}
    frag_of_name = np.full(n, -1, np.int32)
    for f, group in enumerate(names):
        for name in group:
            k = index.get(name.encode("utf-8"))
            if k is None or kinds[k] != 2:
                raise ValueError(f"fragment name {name!r} is no abbreviation of the symbol tables")
            frag_of_name[k] = f
    return mols, atoms, bonds, text, frag_of_name
