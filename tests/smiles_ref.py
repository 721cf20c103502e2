"""The oracle of mnx_smiles_pack (include/molnextr_hip.h) in two parts that share no code with each other or with the kernel:

* the WRITER — graph SMILES from the packed molecule records in plain Python: a recursive depth-first search over sorted
  neighbour lists, ring numbers from a set of numbers in use, the string put together by recursion. The atom interpretation is
  molfile_ref's (pinned by the molfile tests);
* the READER — read(smiles) for exactly the grammar the writer emits (atoms, bracket atoms, ( ) . - = # : ~, digits and %nn):
  no toolkit is at hand to parse the output, so reading it back is the validity check."""
import re
import sys
from itertools import count

import numpy as np

import molfile_ref as M
from molnextr_amd.engine import SMILES_DTYPE

(FLAG_TOO_LARGE, FLAG_BEYOND, FLAG_PSEUDO, FLAG_TRUNCATED, FLAG_DUPLICATE, FLAG_RINGS, FLAG_WEDGES, FLAG_UNKNOWN) = (
    1, 2, 4, 8, 16, 32, 64, 128)
NO_POSITION = 0xFFFF
CLASS_SYMBOL = {1: "", 5: "", 6: "", 2: "=", 3: "#", 4: ":"}          # the class as read back; '' = a single bond


# ---------------------------------------------------------------------------------------------------------------- writer
def atom_text(sym: bytes, tables):
    """(text, aromatic, pseudo) of one atom"""
    a = M.interpret(sym, tables)
    if a["pseudo"]:
        return ("[%d*]" % a["rgroup"] if a["rgroup"] else "*"), False, True
    if not a["bracket"]:
        return sym.decode("ascii"), sym.islower(), False
    el = M.BRACKET_ATOM.fullmatch(sym).group(2).decode("ascii")          # the element as spelled
    h = "" if a["h"] == 0 else "H" if a["h"] == 1 else "H%d" % a["h"]
    q = a["charge"]
    charge = "" if q == 0 else ("+" if q > 0 else "-") + (str(abs(q)) if abs(q) > 1 else "")
    return "[%s%s%s%s]" % (a["isotope"] or "", el, h, charge), el.islower(), False


def bond_text(cls: int, both_aromatic: bool) -> str:
    if cls in (1, 5, 6):
        return "-" if both_aromatic else ""
    if cls == 4:
        return "" if both_aromatic else ":"
    return {2: "=", 3: "#"}.get(cls, "~")


def ring_digits(r: int) -> str:
    return str(r) if r < 10 else "%%%02d" % r


def smiles(symbols, bonds, tables=None):
    """One molecule: symbols [bytes], bonds [(i, j, type, rev)] with valid i != j -> (text or None, written position of every
    atom or None, flags, n_rings)"""
    tables = M.name_tables() if tables is None else tables
    n = len(symbols)
    atoms = [atom_text(s, tables) for s in symbols]
    flags = FLAG_PSEUDO if any(a[2] for a in atoms) else 0
    nbrs = [[] for _ in range(n)]
    for i, j, ty, _ in bonds:
        nbrs[i].append((j, ty))
        nbrs[j].append((i, ty))
    for a in nbrs:
        a.sort()
    duplicate = len({frozenset(b[:2]) for b in bonds}) != len(bonds)

    order, pos, children, rings, roots = [], {}, [[] for _ in range(n)], [[] for _ in range(n)], []

    def visit(a, parent):
        pos[a] = len(order)
        order.append(a)
        for nb, ty in nbrs[a]:
            if nb == parent:
                continue
            if nb not in pos:
                children[a].append((nb, ty))
                visit(nb, a)
            else:
                rings[a].append((nb, ty))

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 1000))
    try:
        for a in range(n):
            if a not in pos:
                roots.append(a)
                visit(a, None)
        n_rings = len(bonds) - n + len(roots)
        if duplicate:
            return None, None, flags | FLAG_DUPLICATE, n_rings

        in_use, number, items = set(), {}, [""] * n
        for p, a in enumerate(order):
            ends = sorted(rings[a], key=lambda e: pos[e[0]])
            closed = []
            for nb, ty in ends:
                if pos[nb] < p:
                    items[a] += ring_digits(number[nb, a])
                    closed.append(number[nb, a])
            for nb, ty in ends:
                if pos[nb] > p:
                    r = next(k for k in count(1) if k not in in_use)
                    if r > 99:
                        return None, None, flags | FLAG_RINGS, n_rings
                    in_use.add(r)
                    number[a, nb] = r
                    items[a] += bond_text(ty, atoms[a][1] and atoms[nb][1]) + ring_digits(r)
            in_use.difference_update(closed)                   # free from the next atom on

        def write(a):
            s = atoms[a][0] + items[a]
            for k, (c, ty) in enumerate(children[a]):
                t = bond_text(ty, atoms[a][1] and atoms[c][1]) + write(c)
                s += t if k == len(children[a]) - 1 else "(" + t + ")"
            return s

        text = ".".join(write(r) for r in roots)
    finally:
        sys.setrecursionlimit(limit)
    if any(b[2] in (5, 6) for b in bonds):
        flags |= FLAG_WEDGES
    if any(not 1 <= b[2] <= 6 for b in bonds):
        flags |= FLAG_UNKNOWN
    return text, [pos[a] for a in range(n)], flags, n_rings


def pack_with(writer, mols, atoms, bonds, text, tables, n_atom_records, n_bond_records, n_text_bytes, order_fill, extra=()):
    """The loop of every pack() of the SMILES oracles: which molecules are admitted (the flag bits 0, 1 and 3), their symbols,
    bins and bonds to writer(symbols, xy, bonds, tables) -> (text or None, written positions or None, flags, n_rings, then one
    per-atom list or None for every name in `extra`), the records and the bytes behind one another. Returns {'recs', 'order',
    *extra, 'out', 'total'}; a per-atom array holds NO_POSITION where the writer gave None and order_fill where the call
    writes nothing."""
    tables = M.name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    recs = np.zeros(len(mols), SMILES_DTYPE)
    per_atom = {k: np.full(n_a, order_fill, np.uint16) for k in ("order",) + tuple(extra)}
    chunks, at = [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        flags = FLAG_TRUNCATED if int(m["flags"]) & 1 else 0
        if na > 999 or nb > 999:
            flags |= FLAG_TOO_LARGE
        if a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t:
            flags |= FLAG_BEYOND
        written = (None, None, 0, 0) + (None,) * len(extra)
        if not flags & 3:
            A, B = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            if any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in A) or \
                    any(int(x["i"]) >= na or int(x["j"]) >= na or int(x["i"]) == int(x["j"]) for x in B):
                flags |= FLAG_BEYOND
            else:
                syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in A]
                written = writer(syms, [(int(a["x_bin"]), int(a["y_bin"])) for a in A],
                                 [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in B], tables)
                flags |= written[2]
        data = written[0]
        for arr, v in zip(per_atom.values(), (None if data is None else written[1],) + tuple(written[4:])):
            arr[a0:min(a0 + na, n_a)] = NO_POSITION if v is None else v
        data = data or ""
        recs[b] = (min(at, 0xFFFFFFFF), len(data), flags, written[3])
        chunks.append(data.encode("ascii"))
        at += len(data)
    return {"recs": recs, **per_atom, "out": b"".join(chunks), "total": at}


def pack(mols, atoms, bonds, text, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None, order_fill=NO_POSITION):
    """mnx_smiles_pack on host arrays: {'recs' SMILES_DTYPE [n], 'order' uint16 [n_atom_records], 'out' bytes, 'total' int}. The
    n_* default to the sizes of the arrays; smaller ones make the molecules whose records reach beyond them refused (flag bit
    1). order_fill: what the entries of `order` that the call does not write hold."""
    return pack_with(lambda syms, xy, B, tb: smiles(syms, B, tb), mols, atoms, bonds, text, tables, n_atom_records, n_bond_records,
                     n_text_bytes, order_fill)


# ---------------------------------------------------------------------------------------------------------------- reader
ORGANIC = ("Cl", "Br", "B", "C", "N", "O", "P", "S", "F", "I", "b", "c", "n", "o", "p", "s", "*")
# a bracket atom as it is emitted: no leading zero, no chirality mark, no class, 'H' alone for one hydrogen, a bare sign for +-1
EMITTED_ATOM = re.compile(r"\[(?:[1-9]\d{0,2})?([A-Z][a-z]?|se|as|[bcnops]|\*)(?:H[2-9]?)?(?:[+-](?:[2-9]|1[0-5])?)?\]")


def read(smiles: str):
    """(atom texts in written order, {(a, b): symbol} with a < b in written order); symbol '' for a bond written as nothing.
    Raises ValueError on anything outside the grammar mnx_smiles_pack emits, an unclosed ring or branch, a dangling bond."""
    atoms, bonds, open_rings, stack = [], {}, {}, []
    prev, pending, k, dot = None, None, 0, True          # dot: the next atom starts a component

    def join(a, b, symbol):
        key = (min(a, b), max(a, b))
        if a == b or key in bonds:
            raise ValueError(f"bond {key} twice or to itself")
        bonds[key] = symbol

    while k < len(smiles):
        c = smiles[k]
        if c == "[":
            end = smiles.find("]", k)
            if end < 0:
                raise ValueError("unclosed bracket atom")
            token, k = smiles[k:end + 1], end + 1
            m = EMITTED_ATOM.fullmatch(token)
            if m is None or (m.group(1)[:1].isupper() and m.group(1) not in M.ELEMENTS):
                raise ValueError(f"bad bracket atom {token}")
        elif smiles.startswith(ORGANIC, k):
            token = next(t for t in ORGANIC if smiles.startswith(t, k))
            k += len(token)
        else:
            token = None
        if token is not None:
            atoms.append(token)
            me = len(atoms) - 1
            if prev is not None and not dot:
                join(prev, me, pending or "")
            elif pending:
                raise ValueError("a bond symbol in front of the first atom of a component")
            prev, pending, dot = me, None, False
            continue
        k += 1
        if c in "-=#:~":
            if pending is not None or prev is None or dot:
                raise ValueError(f"misplaced bond symbol at {k - 1}")
            pending = c
        elif c.isdigit() or c == "%":
            if c == "%":
                if not (smiles[k:k + 2].isdigit() and len(smiles[k:k + 2]) == 2):
                    raise ValueError("'%' without two digits")
                r, k = int(smiles[k:k + 2]), k + 2
            else:
                r = int(c)
            if prev is None or dot or r == 0:
                raise ValueError(f"misplaced ring number at {k - 1}")
            if r in open_rings:
                if pending is not None:
                    raise ValueError("a bond symbol at a ring closure")
                a, symbol = open_rings.pop(r)
                join(a, prev, symbol)
            else:
                open_rings[r] = (prev, pending or "")
                pending = None
        elif c == "(":
            if prev is None or pending is not None or dot:
                raise ValueError("misplaced '('")
            stack.append(prev)
        elif c == ")":
            if not stack or pending is not None or dot:
                raise ValueError("misplaced ')'")
            prev = stack.pop()
        elif c == ".":
            if prev is None or pending is not None or stack or dot:
                raise ValueError("misplaced '.'")
            dot = True
        else:
            raise ValueError(f"unexpected {c!r} at {k - 1}")
    if open_rings or stack or pending is not None or (dot and atoms):
        raise ValueError("unclosed ring, branch or bond")
    return atoms, bonds
