"""The oracle of mnx_kekulize_pack (include/molnextr_hip.h) in plain Python, tables in and tables out, written from the header's
rule: every system of lower-case atoms on type-4 bonds gets the first perfect matching of its needy atoms in the header's order and
is written in upper case with double and single bonds, or stays exactly as it came. It shares no code with the kernel: the atom
interpretation is molfile_ref's (a regular expression), systems are sets, the search is recursive over a dict of partners, the
symbols are normalize_ref's spelling. check_kekule() at the end judges an output without knowing anything of the search. THE CHOICE
AMONG SEVERAL VALID MATCHINGS IS THE PROJECT'S OWN ORDER: it is not RDKit's Kekulize, and no toolkit has checked it."""
import sys

import numpy as np

import molfile_ref as M
import normalize_ref as N
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE

KEKULIZED, KEKULE_LEFT, REFUSED = 128, 256, 512
NOTE_KEKULIZED, NOTE_LEFT, NOTE_COPIED, NOTE_LIMIT = 16, 32, 64, 128
DEFAULT_STEPS = 16384
MAX_RECORDS = 999
ORDER = {1: 1, 5: 1, 6: 1, 4: 1, 2: 2, 3: 3}
OK, NO_MATCHING, LIMIT, BLOCKED = "ok", "no matching", "limit", "blocked"


def valence(element: str, charge: int):
    """v of the header's needy rule, None for a pair it does not list"""
    if element == "C":
        return {0: 4, 1: 3, -1: 3}.get(charge)
    if element in ("N", "P"):
        return {0: 3, 1: 4}.get(charge)
    if element == "B":
        return {0: 3, -1: 4}.get(charge)
    if element == "As":
        return {0: 3}.get(charge)
    if element in ("O", "S", "Se"):
        return {0: 2, 1: 3}.get(charge)
    return None


class _Limit(Exception):
    pass


def first_matching(needy, adj, max_steps, prune=True):
    """needy: the system's needy atoms ascending; adj[a]: a's needy neighbours ascending -> (result, {atom: partner}, steps,
    pruned pairings). Depth first in the header's order; prune=False searches without undoing stranding pairings at once."""
    if len(needy) % 2 or any(not adj[a] for a in needy):
        return NO_MATCHING, {}, 0, 0
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))
    matched, count = {}, {"steps": 0, "pruned": 0}

    def extend():
        a = next((x for x in needy if x not in matched), None)
        if a is None:
            return True
        for v in adj[a]:
            if v in matched:
                continue
            count["steps"] += 1
            if count["steps"] > max_steps:
                raise _Limit
            matched[a], matched[v] = v, a
            stranded = any(w not in matched and all(x in matched for x in adj[w]) for u in (a, v) for w in adj[u])
            if prune and stranded:
                count["pruned"] += 1
            elif extend():
                return True
            del matched[a], matched[v]
        return False

    try:
        found = extend()
    except _Limit:
        return LIMIT, {}, count["steps"], count["pruned"]
    return (OK, dict(matched), count["steps"], count["pruned"]) if found else (NO_MATCHING, {}, count["steps"], count["pruned"])


def aromatic_atoms(symbols, tables):
    atoms = [M.interpret(s, tables) for s in symbols]
    return atoms, {a for a, s in enumerate(symbols) if not atoms[a]["pseudo"] and N.lower_case(s)}


def hydrogens_and_needy(atoms, aromatic, bonds):
    """bo per atom, and for the aromatic atoms H and whether the atom is needy"""
    bo = [0] * len(atoms)
    for i, j, ty in (b[:3] for b in bonds):
        bo[i] += ORDER.get(ty, 0)
        bo[j] += ORDER.get(ty, 0)
    H, needy = {}, set()
    for a in aromatic:
        H[a] = atoms[a]["h"] if atoms[a]["bracket"] else max(0, 3 - bo[a]) if atoms[a]["symbol"] == "C" else 0
        v = valence(atoms[a]["symbol"], atoms[a]["charge"])
        if v is not None and v - bo[a] - H[a] == 1:
            needy.add(a)
    return bo, H, needy


def kekulize_molecule(symbols, bonds, tables, max_steps=0, prune=True):
    """One admitted molecule: symbols [bytes], bonds [(i, j, type, rev)] with valid i, j -> (symbols, [(type, rev)] per bond, notes
    per atom, flags, systems [{'root', 'atoms', 'needy', 'result', 'steps', 'pruned', 'adj'}])"""
    max_steps = max_steps or DEFAULT_STEPS
    n = len(symbols)
    atoms, aromatic = aromatic_atoms(symbols, tables)
    bo, H, needy = hydrogens_and_needy(atoms, aromatic, bonds)

    # systems: the connected components of the aromatic atoms under the type-4 records between two of them
    system_of = {a: {a} for a in aromatic}
    for i, j, ty in (b[:3] for b in bonds):
        if ty == 4 and i in aromatic and j in aromatic and system_of[i] is not system_of[j]:
            merged = system_of[i] | system_of[j]
            for a in merged:
                system_of[a] = merged
    blocked = set()
    for a in aromatic:
        mine = [b for b in bonds if a in b[:2]]
        others = [b[1] if b[0] == a else b[0] for b in mine]
        if (any(b[2] == 4 and o not in aromatic for b, o in zip(mine, others)) or sum(b[2] == 4 for b in mine) > 3 or
                len(set(others)) != len(others) or a in others or any(not 1 <= b[2] <= 6 for b in mine)):
            blocked.add(a)

    partner, systems, left, limit = {}, [], set(), set()
    for atoms_of in sorted({frozenset(s) for s in system_of.values()}, key=min):
        info = {"root": min(atoms_of), "atoms": sorted(atoms_of), "needy": sorted(atoms_of & needy), "steps": 0, "pruned": 0, "adj": {}}
        if atoms_of & blocked:
            info["result"] = BLOCKED
        else:
            adj = {a: [] for a in info["needy"]}
            for i, j, ty in (b[:3] for b in bonds):
                if ty == 4 and i in adj and j in adj:
                    adj[i].append(j)
                    adj[j].append(i)
            info["adj"] = adj = {a: sorted(v) for a, v in adj.items()}
            info["result"], pairs, info["steps"], info["pruned"] = first_matching(info["needy"], adj, max_steps, prune)
            partner.update(pairs)
        if info["result"] != OK:
            left |= atoms_of
            if info["result"] == LIMIT:
                limit |= atoms_of
        systems.append(info)

    out, notes, flags = [], [], 0
    for a in range(n):
        if a not in aromatic:
            out.append(symbols[a])
            notes.append(NOTE_COPIED)
        elif a in left:
            out.append(symbols[a])
            notes.append(H[a] | NOTE_LEFT | (NOTE_LIMIT if a in limit else 0))
            flags |= KEKULE_LEFT
        else:
            el, new_bo = atoms[a]["symbol"], bo[a] + (1 if a in partner else 0)
            reader = N.inferred_h(el, new_bo) if el in N.VALENCES else None
            out.append(N.spell(atoms[a]["isotope"], el, False, H[a], atoms[a]["charge"], reader)[0])
            notes.append(H[a] | NOTE_KEKULIZED)
            flags |= KEKULIZED
    types = []
    for i, j, ty, rev in (b[:4] for b in bonds):
        rewritten = ty == 4 and i in aromatic and j in aromatic and i not in left and j not in left
        types.append(((2, 2) if partner.get(i) == j else (1, 1)) if rewritten else (ty, rev))
    return out, types, notes, flags, systems


def pack(mols, atoms, bonds, text, tables=None, max_steps=0, n_atom_records=None, n_bond_records=None, n_text_bytes=None, prune=True):
    """mnx_kekulize_pack on host arrays: {'mols', 'atoms', 'bonds', 'text', 'atom_notes', 'totals', 'systems' (per molecule, [] for
    a refused one)}"""
    tables = M.name_tables() if tables is None else tables
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    out_mols = np.zeros(len(mols), MOL_DTYPE)
    A, B, notes, chunks, at_text, systems = [], [], [], [], 0, []
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
            systems.append([])
            continue
        syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma]
        s2, types, n2, flags, info = kekulize_molecule(
            syms, [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"])) for x in mb], tables, max_steps, prune)
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
        systems.append(info)
    return {"mols": out_mols, "atoms": np.array(A, ATOM_DTYPE).reshape(-1), "bonds": np.array(B, BOND_DTYPE).reshape(-1),
            "text": b"".join(chunks), "atom_notes": np.array(notes, np.uint8), "totals": (len(A), len(B), at_text), "systems": systems}


# ---------------------------------------------------------------------------------------------------------- the validity check
def _molecules(rec):
    """per molecule (symbols, atom records without sym0, bond records as tuples), None for one of no size that is flagged REFUSED"""
    text = bytes(rec["text"])
    for m in rec["mols"]:
        a0, na, b0, nb, t0 = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0"))
        ma, mb = rec["atoms"][a0:a0 + na], rec["bonds"][b0:b0 + nb]
        yield ([text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma],
               [(int(a["index"]), int(a["x_bin"]), int(a["y_bin"]), float(a["score"])) for a in ma],
               [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"]), float(x["score"])) for x in mb], a0, int(m["flags"]))


def check_kekule(inp, out, tables=None):
    """Whether `out` (tables and atom_notes) is a valid kekulisation of `inp`, judged without the search: a list of violations, empty
    when there is none. In a system noted KEKULIZED there is no lower-case atom and no type-4 record; every formerly needy atom has
    exactly one type-2 record among its former type-4 records and every other atom of the system none; H and charge (and isotope
    and element) are equal per atom; everything outside such systems is byte-equal."""
    tables = M.name_tables() if tables is None else tables
    bad = []
    if len(inp["mols"]) != len(out["mols"]):
        return ["%d molecules, not %d" % (len(out["mols"]), len(inp["mols"]))]
    for b, (p, q) in enumerate(zip(_molecules(inp), _molecules(out))):
        who = "molecule %d: " % b
        if q[4] & REFUSED:
            if q[0] or q[2]:
                bad.append(who + "refused with records")
            continue
        if len(p[0]) != len(q[0]) or len(p[2]) != len(q[2]):
            bad.append(who + "atom or bond count changed")
            continue
        if p[1] != q[1]:
            bad.append(who + "index, bins or score of an atom changed")
        notes = [int(x) for x in out["atom_notes"][q[3]:q[3] + len(q[0])]]
        done = {a for a, x in enumerate(notes) if x & NOTE_KEKULIZED}
        if bool(done) != bool(q[4] & KEKULIZED):
            bad.append(who + "MNX_MOL_KEKULIZED disagrees with the notes")
        atoms_in, aromatic = aromatic_atoms(p[0], tables)
        bo_in, H, needy = hydrogens_and_needy(atoms_in, aromatic, p[2])
        if not done <= aromatic:
            bad.append(who + "an atom noted KEKULIZED was no aromatic atom")
            continue
        atoms_out = [M.interpret(s, tables) for s in q[0]]
        bo_out = hydrogens_and_needy(atoms_out, set(), q[2])[0]
        doubles = {a: 0 for a in done}
        for k, (x, y) in enumerate(zip(p[2], q[2])):
            former = x[2] == 4 and x[0] in done and x[1] in done
            if x[2] == 4 and (x[0] in done) != (x[1] in done):
                bad.append(who + "bond %d: a type-4 record leaves a system noted KEKULIZED" % k)
            if not former:
                if x != y:
                    bad.append(who + "bond %d outside the kekulised systems changed: %r -> %r" % (k, x, y))
                continue
            if (x[0], x[1], x[4]) != (y[0], y[1], y[4]) or (y[2], y[3]) not in ((1, 1), (2, 2)):
                bad.append(who + "bond %d: %r -> %r" % (k, x, y))
            if y[2] == 2:
                doubles[x[0]] += 1
                doubles[x[1]] += 1
        for a in range(len(p[0])):
            if a not in done:
                if p[0][a] != q[0][a]:
                    bad.append(who + "atom %d outside the kekulised systems changed: %r -> %r" % (a, p[0][a], q[0][a]))
                continue
            if N.lower_case(q[0][a]) or atoms_out[a]["pseudo"]:
                bad.append(who + "atom %d is still lower case or no atom: %r" % (a, q[0][a]))
                continue
            if doubles[a] != (1 if a in needy else 0):
                bad.append(who + "atom %d (%s) has %d double bonds in its system" % (a, "needy" if a in needy else "not needy", doubles[a]))
            el = atoms_out[a]["symbol"]
            h_out = atoms_out[a]["h"] if atoms_out[a]["bracket"] else N.inferred_h(el, bo_out[a]) if el in N.VALENCES else 0
            same = all(atoms_in[a][k] == atoms_out[a][k] for k in ("symbol", "charge", "isotope"))
            if not same or h_out != H[a] or (notes[a] & 15) != H[a]:
                bad.append(who + "atom %d: %r (H %d) -> %r (H %d, noted %d)" % (a, p[0][a], H[a], q[0][a], h_out, notes[a] & 15))
    return bad
