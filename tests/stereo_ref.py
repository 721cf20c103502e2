"""The oracle of mnx_smiles_pack_stereo (include/molnextr_hip.h) in three parts that share no code with the kernel:

* the WRITER — smiles() / pack(): the graph SMILES with '@' / '@@' in plain Python. Its own walk (an explicit stack over sorted
  neighbour lists), its own neighbour order of the string at every centre, its own determinant (the sum over the six
  permutations). The atoms' texts and the bond symbols are smiles_ref's (pinned by the tests of the plain writer);
* the READER — centres(text): for every atom of a written string its neighbours AS THE STRING ORDERS THEM (the preceding atom,
  the H of the bracket, the ring digits, the branches), and handedness(): '@' or '@@' of four points in floating point by the
  OpenSMILES wording — seen from the first, do the other three run anticlockwise? — through angles, not a determinant. A
  missing H stands opposite to the sum of the three vectors;
* the generated molecules that the CPU and the GPU tests share, and what they cover (coverage())."""
import math
import re
from itertools import permutations

import numpy as np

import molfile_ref as M
import smiles_ref as S

FLAG_STEREO, FLAG_UNRESOLVED = 256, 512
WITH_H = (b"[C@H]", b"[C@@H]")
MARKS = {-1: "@", 1: "@@", 0: ""}


# ---------------------------------------------------------------------------------------------------------------- writer
def det(r):
    """3x3 determinant of integer rows, by the permutation sum"""
    total = 0
    for p in permutations(range(3)):
        inversions = sum(p[a] > p[b] for a in range(3) for b in range(a + 1, 3))
        total += (-1) ** inversions * r[0][p[0]] * r[1][p[1]] * r[2][p[2]]
    return total


def seen_class(bond, c):
    """edges[c][n]: the class of the bond record (i, j, type, rev) as atom c sees it"""
    return bond[2] if c == bond[0] else bond[3]


def vector(xy, c, n, cls):
    return (xy[n][0] - xy[c][0], xy[c][1] - xy[n][1], {5: 1, 6: -1}.get(cls, 0))


def smiles(symbols, xy, bonds, tables=None):
    """One molecule: symbols [bytes], xy [(x_bin, y_bin)], bonds [(i, j, type, rev)] with valid i != j -> (text or None, written
    position of every atom or None, flags, n_rings, {centre: its record}); a centre's record = {'mark' '@' / '@@' / '', 'order'
    the neighbours as the string orders them ('H' for the implicit hydrogen), 'd', 'candidate', 'seen' {neighbour: class}, 'wedge'
    one of them is 5 or 6, 'parent' it has one, 'rings' how many ring items}"""
    tables = M.name_tables() if tables is None else tables
    n = len(symbols)
    atoms = [S.atom_text(s, tables) for s in symbols]
    flags = S.FLAG_PSEUDO if any(a[2] for a in atoms) else 0
    around = [[] for _ in range(n)]
    for b in bonds:
        around[b[0]].append((b[1], b))
        around[b[1]].append((b[0], b))
    for a in around:
        a.sort(key=lambda e: e[0])
    duplicate = len({frozenset(b[:2]) for b in bonds}) != len(bonds)

    # the walk: an explicit stack of (atom, index of its next neighbour)
    written, pos, parent, children, rings, roots = [], {}, {}, [[] for _ in range(n)], [[] for _ in range(n)], []
    for root in range(n):
        if root in pos:
            continue
        roots.append(root)
        pos[root], parent[root] = len(written), None
        written.append(root)
        stack = [[root, 0]]
        while stack:
            a, k = stack[-1]
            if k == len(around[a]):
                stack.pop()
                continue
            stack[-1][1] += 1
            nb, bond = around[a][k]
            if nb == parent[a]:
                continue
            if nb in pos:
                rings[a].append((nb, bond))
                continue
            pos[nb], parent[nb] = len(written), a
            written.append(nb)
            children[a].append((nb, bond))
            stack.append([nb, 0])
    n_rings = len(bonds) - n + len(roots)
    if duplicate:
        return None, None, flags | S.FLAG_DUPLICATE, n_rings, {}

    # ring numbers: closures first, then openings, each in ascending written position of the other end
    free_from_next, in_use, number, items, ring_order = [], set(), {}, [""] * n, [[] for _ in range(n)]
    for p, a in enumerate(written):
        in_use -= set(free_from_next)
        free_from_next = []
        for nb, bond in sorted((r for r in rings[a] if pos[r[0]] < p), key=lambda r: pos[r[0]]):
            items[a] += S.ring_digits(number[nb, a])
            free_from_next.append(number[nb, a])
            ring_order[a].append(nb)
        for nb, bond in sorted((r for r in rings[a] if pos[r[0]] > p), key=lambda r: pos[r[0]]):
            r = min(set(range(1, len(in_use) + 2)) - in_use)
            if r > 99:
                return None, None, flags | S.FLAG_RINGS, n_rings, {}
            in_use.add(r)
            number[a, nb] = r
            items[a] += S.bond_text(bond[2], atoms[a][1] and atoms[nb][1]) + S.ring_digits(r)
            ring_order[a].append(nb)

    # the marks
    centre, mark = {}, [""] * n
    for c in range(n):
        if symbols[c] not in M.CHIRAL_CARBONS:
            continue
        h = 1 if symbols[c] in WITH_H else 0
        seen = {nb: seen_class(bond, c) for nb, bond in around[c]}
        wedge = any(v in (5, 6) for v in seen.values())
        single = all(bond[2] in (1, 5, 6) for _, bond in around[c])
        order = ([parent[c]] if parent[c] is not None else []) + (["H"] if h else []) + ring_order[c] + [k for k, _ in children[c]]
        rec = {"mark": "", "order": order, "d": None, "seen": seen, "wedge": wedge, "parent": parent[c] is not None,
               "rings": len(ring_order[c]),
               "candidate": wedge and single and not atoms[c][2] and len(around[c]) + h == 4}
        if rec["candidate"]:
            v = [vector(xy, c, k, seen[k]) for k in order if k != "H"]
            if h:
                d = det(v)
                if order.index("H") % 2:
                    d = -d
            else:
                d = det([[v[k][q] - v[0][q] for q in range(3)] for k in (1, 2, 3)])
            rec["d"] = d
            rec["mark"] = mark[c] = MARKS[(d > 0) - (d < 0)]
        centre[c] = rec

    def text_of(a):
        t = atoms[a][0]
        return t[:2] + mark[a] + t[2:] if mark[a] else t

    # the string, children before their parent: a long path needs no deep recursion
    sub = [None] * n
    for a in reversed(written):
        s = text_of(a) + items[a]
        for k, (c, bond) in enumerate(children[a]):
            t = S.bond_text(bond[2], atoms[a][1] and atoms[c][1]) + sub[c]
            s += t if k == len(children[a]) - 1 else "(" + t + ")"
            sub[c] = None
        sub[a] = s
    text = ".".join(sub[r] for r in roots)

    if any(mark):
        flags |= FLAG_STEREO
    if any(r["wedge"] and not r["mark"] for r in centre.values()):
        flags |= FLAG_UNRESOLVED
    if any(b[2] in (5, 6) and not mark[b[0]] and not mark[b[1]] for b in bonds):
        flags |= S.FLAG_WEDGES
    if any(not 1 <= b[2] <= 6 for b in bonds):
        flags |= S.FLAG_UNKNOWN
    return text, [pos[a] for a in range(n)], flags, n_rings, centre


def pack(mols, atoms, bonds, text, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None, order_fill=S.NO_POSITION):
    """mnx_smiles_pack_stereo on host arrays, as smiles_ref.pack: {'recs', 'order', 'out', 'total'}"""
    return S.pack_with(lambda syms, xy, B, tb: smiles(syms, xy, B, tb)[:4], mols, atoms, bonds, text, tables, n_atom_records,
                       n_bond_records, n_text_bytes, order_fill)


# ---------------------------------------------------------------------------------------------------------------- reader
ATOM = re.compile(r"\[[^\]]*\]|Cl|Br|[BCNOPSFIbcnops*]")
MARKED = re.compile(r"\[C(@@?)(H?)\]")


def centres(text: str):
    """[(token, neighbours)] for the atoms of a written string in written order; neighbours = written indices, and 'H', in the
    order in which the string names them at that atom"""
    atoms, open_rings, stack = [], {}, []
    prev, k, dot = None, 0, True
    while k < len(text):
        m = ATOM.match(text, k)
        if m:
            token, k = m.group(), m.end()
            me = len(atoms)
            atoms.append((token, []))
            if prev is not None and not dot:
                atoms[me][1].append(prev)
                atoms[prev][1].append(me)
            stereo = MARKED.fullmatch(token)
            if stereo and stereo.group(2):
                atoms[me][1].append("H")
            prev, dot = me, False
            continue
        c = text[k]
        k += 1
        if c.isdigit() or c == "%":
            r = int(c) if c != "%" else int(text[k:k + 2])
            k += 0 if c != "%" else 2
            if r in open_rings:
                other, slot = open_rings.pop(r)
                atoms[other][1][slot] = prev
                atoms[prev][1].append(other)
            else:
                open_rings[r] = (prev, len(atoms[prev][1]))
                atoms[prev][1].append(None)
        elif c == "(":
            stack.append(prev)
        elif c == ")":
            prev = stack.pop()
        elif c == ".":
            dot = True
        elif c not in "-=#:~":
            raise ValueError(f"unexpected {c!r} in {text!r}")
    assert not open_rings and not stack
    return atoms


def handedness(points):
    """'@' when, seen from points[0], points[1] -> [2] -> [3] run anticlockwise, '@@' when clockwise; floating point, by angles
    around the centre of the three in the plane across the line of sight"""
    p = [np.asarray(q, float) for q in points]
    g = (p[1] + p[2] + p[3]) / 3.0
    w = p[0] - g
    w /= np.linalg.norm(w)
    axis = np.zeros(3)
    axis[int(np.argmin(np.abs(w)))] = 1.0
    e1 = np.cross(w, axis)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(w, e1)                 # e1, e2, w right-handed: from w's side e1 -> e2 turns anticlockwise
    angle = [math.atan2(float(np.dot(q - g, e2)), float(np.dot(q - g, e1))) for q in p[1:]]
    first, second = (angle[1] - angle[0]) % (2 * math.pi), (angle[2] - angle[0]) % (2 * math.pi)
    return "@" if first < second else "@@"


def read_back(text, pos, xy, bonds):
    """every MARKED atom of a written string, from the string and the drawing alone: {atom: (the mark written, the handedness
    of the drawing in the string's neighbour order, that order in atom indices)}"""
    atom_at = {p: a for a, p in enumerate(pos)}
    seen = {}
    for b in bonds:
        seen[b[0], b[1]], seen[b[1], b[0]] = b[2], b[3]
    out = {}
    for p, (token, nbrs) in enumerate(centres(text)):
        m = MARKED.fullmatch(token)
        if not m:
            continue
        c = atom_at[p]
        order = [k if k == "H" else atom_at[k] for k in nbrs]
        vec = {k: np.array(vector(xy, c, k, seen[c, k]), float) for k in order if k != "H"}
        if "H" in order:
            vec["H"] = -sum(vec.values())
        out[c] = (m.group(1), handedness([vec[k] for k in order]), order)
    return out


def parity(a, b):
    """0 when the order b is an even permutation of the order a, 1 when odd"""
    where = [a.index(k) for k in b]
    return sum(where[x] > where[y] for x in range(len(where)) for y in range(x + 1, len(where))) % 2


# ---------------------------------------------------------------------------------------------------------------- molecules
MIRROR = {5: 6, 6: 5}
PLAIN = (b"C", b"C", b"C", b"N", b"O")


def generate(rng, n_atoms, ring_bonds, components=1):
    """A forest of `components` trees over n_atoms atoms plus up to ring_bonds further bonds, degree at most 4, bins 0..63; an
    atom of degree 4 (3) may become [C@] / [C@@] ([C@H] / [C@@H]) with one or two of its bonds wedged or dashed as IT sees them.
    Returns (symbols, xy, bonds) with i < j and the records in random order."""
    deg, pairs = [0] * n_atoms, {}
    starts = set(rng.choice(np.arange(1, n_atoms), components - 1, replace=False).tolist()) if components > 1 else set()
    for a in range(1, n_atoms):
        if a in starts:
            continue
        free = [k for k in range(a) if deg[k] < 4]
        k = free[int(rng.integers(len(free)))] if rng.random() < 0.5 else free[-1]       # bushy or chain-like
        pairs[k, a] = [1, 1]
        deg[k] += 1
        deg[a] += 1
    for _ in range(ring_bonds):
        i, j = sorted(int(v) for v in rng.choice(n_atoms, 2, replace=False))
        if (i, j) not in pairs and deg[i] < 4 and deg[j] < 4:
            pairs[i, j] = [1, 1]
            deg[i] += 1
            deg[j] += 1
    symbols = [PLAIN[int(rng.integers(len(PLAIN)))] for _ in range(n_atoms)]
    chosen = [a for a in range(n_atoms) if deg[a] in (3, 4) and rng.random() < 0.6]
    for c in chosen:
        mine = [p for p in pairs if c in p and pairs[p] == [1, 1]]
        if not mine:
            continue
        at = rng.random() < 0.5
        symbols[c] = ((b"[C@]", b"[C@@]") if deg[c] == 4 else (b"[C@H]", b"[C@@H]"))[int(at)]
        for k in rng.choice(len(mine), min(len(mine), 1 + int(rng.random() < 0.3)), replace=False):
            cls = 5 if rng.random() < 0.6 else 6
            pairs[mine[k]] = [cls, MIRROR[cls]] if c == mine[k][0] else [MIRROR[cls], cls]
    for (i, j), v in pairs.items():                       # a few double bonds away from every marked carbon
        if v == [1, 1] and symbols[i] in PLAIN and symbols[j] in PLAIN and rng.random() < 0.1:
            pairs[i, j] = [2, 2]
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (n_atoms, 2))]
    keys = list(pairs)
    return symbols, xy, [(i, j, *pairs[i, j]) for i, j in (keys[k] for k in rng.permutation(len(keys)))]


def generated_set(count=300, seed=20):
    """trees and ring systems of 10-60 atoms, every fourth of two or three components"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(10, 61))
        out.append(generate(rng, n, int(rng.integers(0, n // 3 + 1)) if k % 2 else 0, components=1 + (k % 4 == 3) * int(rng.integers(1, 3))))
    return out


def renumber(mol, perm, rng):
    """the same drawing with atom a numbered perm[a]; bond records with i < j, in random order"""
    symbols, xy, bonds = mol
    n = len(symbols)
    inverse = [0] * n
    for a, p in enumerate(perm):
        inverse[p] = a
    moved = [(perm[i], perm[j], ty, rv) if perm[i] < perm[j] else (perm[j], perm[i], rv, ty) for i, j, ty, rv in bonds]
    return [symbols[inverse[p]] for p in range(n)], [xy[inverse[p]] for p in range(n)], [moved[k] for k in rng.permutation(len(moved))]


def coverage(mols):
    """what the oracle's output over `mols` covers: counts of marks and of the situations of the marked centres"""
    c = dict.fromkeys(("@", "@@", "root", "H0", "H1", "four", "ring1", "ring2", "dash", "two wedges", "candidates", "unresolved"), 0)
    for symbols, xy, bonds in mols:
        text, pos, flags, n_rings, centre = smiles(symbols, xy, bonds)
        for a, r in centre.items():
            c["candidates"] += r["candidate"]
            c["unresolved"] += r["candidate"] and not r["mark"]
            if not r["mark"]:
                continue
            c[r["mark"]] += 1
            c["root"] += not r["parent"]
            c["H0"] += r["order"][0] == "H"
            c["H1"] += r["order"][1] == "H"
            c["four"] += "H" not in r["order"]
            c["ring1"] += r["rings"] == 1
            c["ring2"] += r["rings"] == 2
            c["dash"] += 6 in r["seen"].values()
            c["two wedges"] += sum(v in (5, 6) for v in r["seen"].values()) >= 2
    return c
