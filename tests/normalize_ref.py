"""The oracle of mnx_normalize_pack (include/molnextr_hip.h) in plain Python, tables in and tables out, written from the header's
rule: one normal spelling per atom — aromatic rings of 5 and 6 atoms perceived from Kekule drawings, hydrogens counted, brackets
dropped where a reader infers what they say. It shares no code with the kernel: the atom interpretation is molfile_ref's (a regular
expression), the rings are found by a recursive search and kept as sets of bonds, the verdicts are dicts and sets, the symbols are
put together with the % operator. THE RULE IS THE PROJECT'S OWN: no toolkit has checked it."""
import numpy as np

import molfile_ref as M
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE

AROMATIZED, UNBRACKETED, REFUSED = 16, 32, 64
NOTE_AROMATIZED, NOTE_UNBRACKETED, NOTE_COPIED = 16, 32, 64
MAX_RECORDS = 999
ORDER = {1: 1, 5: 1, 6: 1, 2: 2, 3: 3}
VALENCES = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "P": (3, 5), "S": (2, 4, 6), "F": (1,), "Cl": (1,), "Br": (1,), "I": (1,)}


def inferred_h(element: str, bo: int) -> int:
    return next((v - bo for v in VALENCES[element] if v >= bo), 0)


def lower_case(sym: bytes) -> bool:
    body = sym[1:].lstrip(b"0123456789") if sym[:1] == b"[" else sym
    return body[:1].islower()


def spell(isotope, element, aromatic, h, charge, inferred):
    """(bytes, written without brackets)"""
    el = element.lower() if aromatic else element
    if element in VALENCES and not isotope and charge == 0 and h == inferred:
        return el.encode(), True
    hs = "" if h == 0 else "H" if h == 1 else "H%d" % h
    qs = "" if charge == 0 else ("+" if charge > 0 else "-") + ("%d" % abs(charge) if abs(charge) > 1 else "")
    return ("[%s%s%s%s]" % (isotope or "", el, hs, qs)).encode(), False


def normalize_molecule(symbols, bonds, tables):
    """One admitted molecule: symbols [bytes], bonds [(i, j, type, rev, ...)] with valid i, j -> (symbols, [(type, rev)] per bond,
    notes per atom, flags)"""
    n = len(symbols)
    atoms = [M.interpret(s, tables) for s in symbols]
    at = [[] for _ in range(n)]                   # per atom: (neighbour, order, bond number)
    excluded = set()
    for k, bond in enumerate(bonds):
        i, j, ty = bond[:3]
        if ty not in ORDER or i == j:
            excluded.update((i, j))
            continue
        at[i].append((j, ORDER[ty], k))
        at[j].append((i, ORDER[ty], k))
    copied = {a for a in range(n) if atoms[a]["pseudo"] or atoms[a]["symbol"] == "R" or lower_case(symbols[a]) or a in excluded}
    bo = [sum(o for _, o, _ in at[a]) for a in range(n)]
    deg = [len(at[a]) for a in range(n)]
    H = {}
    for a in range(n):
        if a not in copied:
            H[a] = atoms[a]["h"] if atoms[a]["bracket"] else inferred_h(atoms[a]["symbol"], bo[a])

    kind = {}
    for a in H:
        el, q = atoms[a]["symbol"], atoms[a]["charge"]
        orders = [o for _, o, _ in at[a]]
        if el not in ("C", "N", "O", "S") or atoms[a]["chiral"] or deg[a] > 3 or 3 in orders:
            continue
        if len({v for v, _, _ in at[a]}) != deg[a]:
            continue
        doubles = orders.count(2)
        if doubles == 1 and ((el == "C" and q == 0) or (el == "N" and q in (0, 1))):
            kind[a] = "d"
        elif doubles == 0 and ((el == "N" and q == 0 and deg[a] + H[a] == 3) or (el in "OS" and q == 0 and deg[a] == 2 and H[a] == 0) or
                               (el == "C" and q == -1 and deg[a] + H[a] == 3)):
            kind[a] = "p"
        elif doubles == 0 and el == "C" and q == 1:
            kind[a] = "e"

    # the enumerated rings: every simple cycle of 5 or 6 candidates, once, as (its atoms in order, the set of its bond numbers)
    rings = {}

    def extend(walk, used):
        for v, _, k in at[walk[-1]]:
            if v == walk[0] and len(walk) in (5, 6) and k not in used:
                rings.setdefault(frozenset(used | {k}), list(walk))
            elif v in kind and v not in walk and len(walk) < 6:
                extend(walk + [v], used | {k})

    for a in sorted(kind):
        extend([a], frozenset())
    ring_bonds = set().union(*rings) if rings else set()
    on_ring = {a for walk in rings.values() for a in walk}

    aromatic_atoms, aromatic_bonds = set(), set()
    for ks, walk in rings.items():
        electrons = 0
        for a in walk:
            if kind[a] == "p":
                electrons += 2
            elif kind[a] == "d":
                x, _, k = next(e for e in at[a] if e[1] == 2)
                if k in ring_bonds:
                    electrons += 1
                elif not (atoms[a]["symbol"] == "C" and not atoms[x]["pseudo"] and atoms[x]["symbol"] in ("O", "N", "S") and x not in on_ring):
                    electrons = None
                    break
        if electrons == 6:
            aromatic_atoms.update(walk)
            aromatic_bonds.update(ks)

    out, notes, flags = [], [], 0
    for a in range(n):
        if a in copied:
            out.append(symbols[a])
            notes.append(NOTE_COPIED | (atoms[a]["h"] if not atoms[a]["pseudo"] else 0))
            continue
        if atoms[a]["chiral"]:
            out.append(symbols[a])
            notes.append(H[a])
            continue
        el, arom = atoms[a]["symbol"], a in aromatic_atoms
        if not arom:
            reader = inferred_h(el, bo[a]) if el in VALENCES else None
        else:
            reader = 3 - deg[a] if el == "C" else 0
        text, plain = spell(atoms[a]["isotope"], el, arom, H[a], atoms[a]["charge"], reader)
        note = H[a] | (NOTE_AROMATIZED if arom else 0) | (NOTE_UNBRACKETED if plain and atoms[a]["bracket"] else 0)
        flags |= (AROMATIZED if arom else 0) | (UNBRACKETED if plain and atoms[a]["bracket"] else 0)
        out.append(text)
        notes.append(note)
    return out, [(4, 4) if k in aromatic_bonds else (b[2], b[3]) for k, b in enumerate(bonds)], notes, flags


def pack(mols, atoms, bonds, text, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_normalize_pack on host arrays: {'mols', 'atoms', 'bonds', 'text', 'atom_notes', 'totals'}"""
    tables = M.name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    out_mols = np.zeros(len(mols), MOL_DTYPE)
    A, B, notes, chunks, at_text = [], [], [], [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        keep = int(m["flags"]) & 1
        refused = a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t or na > MAX_RECORDS or nb > MAX_RECORDS
        if not refused:
            ma, mb = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            refused = (any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in ma) or
                       any(int(x["i"]) >= na or int(x["j"]) >= na for x in mb))
        if refused:
            out_mols[b] = (len(A), 0, len(B), 0, at_text, 0, keep | REFUSED, 0, float(m["overall_score"]))
            continue
        syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma]
        s2, types, n2, flags = normalize_molecule(syms, [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in mb], tables)
        own = b"".join(s2)
        out_mols[b] = (len(A), na, len(B), nb, at_text, len(own), keep | flags, 0, float(m["overall_score"]))
        off = 0
        for s, a in zip(s2, ma):
            A.append((off, len(s), int(a["index"]), int(a["x_bin"]), int(a["y_bin"]), float(a["score"])))
            off += len(s)
        B += [(int(x["i"]), int(x["j"]), ty, rv, float(x["score"])) for x, (ty, rv) in zip(mb, types)]
        notes += n2
        chunks.append(own)
        at_text += len(own)
    return {"mols": out_mols, "atoms": np.array(A, ATOM_DTYPE).reshape(-1), "bonds": np.array(B, BOND_DTYPE).reshape(-1),
            "text": b"".join(chunks), "atom_notes": np.array(notes, np.uint8), "totals": (len(A), len(B), at_text)}
