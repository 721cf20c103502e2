"""The oracle of mnx_formula_pack (include/molnextr_hip.h) in plain Python, tables in and tables out, written from the header's
rule: condensed-formula labels replaced by the atoms and bonds they spell. It shares no code with the kernel or with
formula_search.h: the tokens come from a regular expression and a dict, the units are a nested list that is written out by a
recursive function, the search is a recursion over immutable states (where the kernel steps back in two arrays), and the new
tables are put together as Python lists and sorted, where the kernel scans. THE RULE IS THE PROJECT'S OWN: no toolkit has
checked it."""
import re

import numpy as np

import expand_ref as X
import molfile_ref as M
import normalize_ref as N
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE

FORMULA_EXPANDED, FORMULA_LEFT, FORMULA_LIMIT, FORMULA_REFUSED = 1 << 10, 1 << 11, 1 << 16, 1 << 17
OK, NO_STRUCTURE, LIMIT = 0, 1, 2
DEFAULT_STEPS, MAX_UNITS, MAX_HEAVY, MAX_DEPTH, MAX_ATOMS = 4096, 96, 32, 3, 2047
VALENCES = {"H": (1,), "B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "F": (1,), "Cl": (1,), "Br": (1,), "I": (1,), "Si": (4,),
            "P": (5, 3), "S": (6, 4, 2)}
ORDER = {1: 1, 5: 1, 6: 1, 2: 2, 3: 3}
RUN = re.compile(rb"[A-Z][a-z]*")


class Stays(Exception):
    """the label has no tokenisation or is too large"""


def group_names(frags=None):
    """the names a group token may be: the abbreviations that have a fragment"""
    return set(X.library() if frags is None else frags)


def tokens_of(label: bytes, groups):
    """[('(',) | (')',) | ('n', count) | ('el', symbol) | ('grp', name bytes)]"""
    out, p = [], 0
    while p < len(label):
        c = label[p:p + 1]
        if c in (b"(", b")"):
            out.append((c.decode(),))
            p += 1
            continue
        if c.isdigit():
            q = p
            while q < len(label) and label[q:q + 1].isdigit():
                q += 1
            if not 1 <= int(label[p:q]) <= 99:
                raise Stays("count")
            out.append(("n", int(label[p:q])))
            p = q
            continue
        run = RUN.match(label, p)
        if run is not None and run.group().decode() in VALENCES:
            out.append(("el", run.group().decode()))
            p = run.end()
            continue
        if not c.isalpha() or not c.isascii():
            raise Stays("byte")
        hit = next((label[p:p + n] for n in range(min(16, len(label) - p), 0, -1) if label[p:p + n] in groups), None)
        if hit is None:
            raise Stays("name")
        out.append(("grp", hit))
        p += len(hit)
    return out


def units_of(tokens):
    """the nested list of (unit, count): unit an ('el', s), a ('grp', name) or a list of such pairs"""
    stack = [[]]
    k = 0
    while k < len(tokens):
        t = tokens[k]
        k += 1
        if t[0] == "(":
            if len(stack) > MAX_DEPTH:
                raise Stays("depth")
            stack.append([])
            continue
        if t[0] == "n":
            raise Stays("a count in no unit's place")
        if t[0] == ")":
            if len(stack) == 1 or not stack[-1]:
                raise Stays("parenthesis")
            unit = stack.pop()
        else:
            unit = t
        count = 1
        if k < len(tokens) and tokens[k][0] == "n":
            count = tokens[k][1]
            k += 1
        stack[-1].append((unit, count))
    if len(stack) != 1:
        raise Stays("parenthesis")
    return stack[0]


def written_out(units):
    """the flat items of the units: ('el', s) | ('grp', name) | ('H', k) | '(' | ')'"""
    out, k = [], 0

    def some(unit, count):
        if unit == ("el", "H"):
            out.append(("H", count))
        else:
            out.extend([unit] * count)

    while k < len(units):
        unit, count = units[k]
        k += 1
        if isinstance(unit, list):
            inner = written_out(unit)
            for _ in range(count):
                out += ["("] + inner + [")"]
        elif unit == ("el", "C") and count > 1 and k < len(units) and not isinstance(units[k][0], list) and units[k][0][0] == "el":
            x, m = units[k]
            k += 1
            for _ in range(count):
                some(unit, 1)
                if m // count:
                    some(x, m // count)
            if m % count:
                some(x, m % count)
        else:
            some(unit, count)
        if len(out) > MAX_UNITS:
            raise Stays("units")
    return out


def turned_round(items):
    return [{"(": ")", ")": "("}.get(x, x) for x in reversed(items)]


def one_direction(items, start, budget):
    """atoms [[what, parent, order, h]] or None; budget [steps, limit]: LimitReached beyond it"""
    partner, opened = {}, []
    for p, x in enumerate(items):
        if x == "(":
            opened.append(p)
        elif x == ")":
            partner[p] = opened.pop()

    def step():
        budget[0] += 1
        if budget[0] > budget[1]:
            raise LimitReached

    # state: cur (None: none yet, the next atom hangs on `hang`), free, atoms (tuple of tuples), branches {index of '(': (cur, free, first)}
    def go(p, cur, hang, free, atoms, branches):
        if p == len(items):
            return atoms if cur is not None and free == 0 else None
        x = items[p]
        if x == "(":
            if cur is None:
                return go(p + 1, cur, hang, free, atoms, branches)
            if free < 1:
                return None
            if free > 1:
                return go(p + 1, None, cur, 0, atoms, {**branches, p: (cur, free, len(atoms))})
            return go(p + 1, cur, hang, free, atoms, branches)
        if x == ")":
            if partner[p] not in branches:
                return go(p + 1, cur, hang, free, atoms, branches)
            back, had, first = branches[partner[p]]
            order = 1 + free
            if cur is None or order > 3 or order > had:
                return None
            raised = atoms[:first] + ((atoms[first][0], atoms[first][1], order, atoms[first][3]),) + atoms[first + 1:]
            return go(p + 1, back, None, had - order, raised, branches)
        if x[0] == "H":
            step()
            if cur is None or free < x[1]:
                return None
            a = atoms[cur]
            return go(p + 1, cur, hang, free - x[1], atoms[:cur] + ((a[0], a[1], a[2], a[3] + x[1]),) + atoms[cur + 1:], branches)
        for v in (VALENCES[x[1]] if x[0] == "el" else (1,)):
            step()
            k = len(atoms)
            if cur is None:
                begin = start if k == 0 else 1
                found = go(p + 1, k, None, v - begin, atoms + ((x, hang, begin if k else 0, 0),), branches) if v >= begin else None
            elif free == 0:
                found = None
            elif free > v:
                found = go(p + 1, cur, None, free - v, atoms + ((x, cur, v, 0),), branches) if v <= 3 else None
            else:
                found = go(p + 1, k, None, v - free, atoms + ((x, cur, free, 0),), branches) if free <= 3 else None
            if found is not None:
                return found
        return None

    return go(0, None, None, 0, (), {})


class LimitReached(Exception):
    pass


def search(label: bytes, start: int, groups, max_steps=0):
    """(status, atoms [(what, parent, order, h)], steps): what ('el', symbol) or ('grp', name); parent None for atom 0"""
    if not 2 <= len(label) <= 20 or start > 6:
        return NO_STRUCTURE, None, 0
    try:
        items = written_out(units_of(tokens_of(label, groups)))
    except Stays:
        return NO_STRUCTURE, None, 0
    heavy = sum(1 for x in items if x not in ("(", ")") and x[0] != "H")
    if heavy == 0 or heavy > MAX_HEAVY or len(items) > MAX_UNITS:
        return NO_STRUCTURE, None, 0
    budget = [0, max_steps or DEFAULT_STEPS]
    try:
        for direction in (items, turned_round(items)):
            atoms = one_direction(direction, start, budget)
            if atoms is not None:
                return OK, [tuple(a) for a in atoms], budget[0]
    except LimitReached:
        return LIMIT, None, budget[0]
    return NO_STRUCTURE, None, budget[0]


def spelled(atoms, start):
    """the symbols of a structure's atoms"""
    out = []
    for k, (what, _, order, h) in enumerate(atoms):
        if what[0] == "grp":
            out.append(b"[" + what[1] + b"]")
            continue
        bo = (start if k == 0 else order) + sum(a[2] for a in atoms[k + 1:] if a[1] == k)
        inferred = N.inferred_h(what[1], bo) if what[1] in N.VALENCES else 0
        out.append(N.spell(0, what[1], False, h, 0, inferred)[0])
    return out


def candidate(sym: bytes, tables):
    """the label an atom's symbol is a candidate with (brackets stripped), or None"""
    inner = sym[1:-1] if len(sym) >= 2 and sym[:1] == b"[" and sym[-1:] == b"]" else sym
    if inner in tables or not M.interpret(sym, tables)["pseudo"] or not 2 <= len(inner) <= 20:
        return None
    return inner


def formula_molecule(symbols, atoms, bonds, groups, tables, max_steps=0):
    """One admitted molecule: symbols [bytes], atoms [(index, x_bin, y_bin, score)], bonds [(i, j, type, rev, score)] ->
    (symbols, atoms, bonds, origin, flags, found {atom: structure}, left [atoms])"""
    n = len(symbols)
    out_sym, out_atoms, origin = list(symbols), list(atoms), list(range(n))
    keyed = [((b[0], 0, k), b) for k, b in enumerate(bonds)]
    flags, found, left = 0, {}, []
    for at in range(n):
        label = candidate(symbols[at], tables)
        if label is None:
            continue
        mine = [b[2] for b in bonds if b[0] == at or b[1] == at]
        status, structure = NO_STRUCTURE, None
        if all(ty in ORDER for ty in mine):
            start = sum(ORDER[ty] for ty in mine)
            status, structure, _ = search(label, start, groups, max_steps)
        if status != OK:
            flags |= FORMULA_LEFT | (FORMULA_LIMIT if status == LIMIT else 0)
            left.append(at)
            continue
        flags |= FORMULA_EXPANDED
        found[at] = structure
        fsym = spelled(structure, start)
        where = [at] + list(range(len(out_sym), len(out_sym) + len(fsym) - 1))
        out_sym[at] = fsym[0]
        out_sym += fsym[1:]
        out_atoms += [atoms[at]] * (len(fsym) - 1)
        origin += [at] * (len(fsym) - 1)
        for k, (_, parent, order, _) in enumerate(structure):
            if k:
                keyed.append(((where[parent], 1, where[k]), (where[parent], where[k], order, order, atoms[at][3])))
    return out_sym, out_atoms, [b for _, b in sorted(keyed, key=lambda e: e[0])], origin, flags, found, left


def pack(mols, atoms, bonds, text, frags=None, tables=None, max_steps=0, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_formula_pack on host arrays: {'mols', 'atoms', 'bonds', 'text', 'origin', 'totals', 'found', 'left' (per molecule)}"""
    tables = M.name_tables() if tables is None else tables
    groups = group_names(frags)
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    out_mols = np.zeros(len(mols), MOL_DTYPE)
    A, B, origin, chunks, at_text, all_found, all_left = [], [], [], [], 0, [], []
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
            out_mols[b] = (len(A), 0, len(B), 0, at_text, 0, keep | FORMULA_REFUSED, 0, float(m["overall_score"]))
            all_found.append({})
            all_left.append([])
            continue
        syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in ma]
        s2, a2, b2, o2, flags, found, left = formula_molecule(
            syms, [(int(a["index"]), int(a["x_bin"]), int(a["y_bin"]), float(a["score"])) for a in ma],
            [(int(x["i"]), int(x["j"]), int(x["type"]), int(x["rev"]), float(x["score"])) for x in mb], groups, tables, max_steps)
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
        all_found.append(found)
        all_left.append(left)
    return {"mols": out_mols, "atoms": np.array(A, ATOM_DTYPE).reshape(-1), "bonds": np.array(B, BOND_DTYPE).reshape(-1),
            "text": b"".join(chunks), "origin": np.array(origin, np.uint16), "totals": (len(A), len(B), at_text),
            "found": all_found, "left": all_left}
