"""The oracle of mnx_smiles_pack_symmetric (include/molnextr_hip.h), sharing no code with the kernel:

* the RULE — equal_pair(): two neighbours of one symmetry class (canon_ref.ranks), both on bridges; a bridge is found with the
  bond taken out of the graph and its other end searched for (bridges()), not with the walk's tree;
* the STRING — smiles(): the molecule renumbered by its ranks (as canon_ref.smiles does). A dropped centre gets the symbol
  without its mark, [C] or [CH], and goes through stereo_ref's writer as the plain bracket atom it then is: no mark, no bit 9,
  its wedge counted by bit 6. The double bonds are ez_ref's rule restated with one hook (marked()): the symmetric candidates
  are set aside BEFORE the flips are taken, so the flip rule runs over the remaining candidates — no edit of a written string;
* pack() as the other reference modules have it, with `atom_marks`;
* generate(): molecules on which the rule fires — two copies of one random branch at a marked carbon or at a C= end, alone or
  grafted onto a molecule of the older generators — and coverage(): what a set of molecules covers."""
import numpy as np

import canon_ref as K
import ez_ref as E
import molfile_ref as M
import smiles_ref as S
import stereo_ref as T

FLAG_SYM = 32768
ATOM_CW, ATOM_CCW, ATOM_SYM, ATOM_EZ, ATOM_EZ_SYM = 1, 2, 4, 8, 16
NO_MARKS = 0xFF
UNMARKED = {b"[C@]": b"[C]", b"[C@@]": b"[C]", b"[C@H]": b"[CH]", b"[C@@H]": b"[CH]"}
KEPT_BITS = 0b0110000010111111         # flag bits 0-5, 7, 13, 14: invariant 1


# ---------------------------------------------------------------------------------------------------------------- the rule
def bridges(n, bonds):
    """is_bridge(u, v) for a bond u - v: with that bond taken out, v cannot be reached from u. Answers are kept."""
    around = [set() for _ in range(n)]
    for b in bonds:
        around[b[0]].add(b[1])
        around[b[1]].add(b[0])
    known = {}

    def is_bridge(u, v):
        key = frozenset((u, v))
        if key not in known:
            seen, todo = {u}, [u]
            while todo and v not in seen:
                a = todo.pop()
                for nb in around[a]:
                    if nb not in seen and {a, nb} != {u, v}:
                        seen.add(nb)
                        todo.append(nb)
            known[key] = v not in seen
        return known[key]
    return is_bridge


def equal_pair(u, nbrs, cls, is_bridge):
    """two of `nbrs` (atoms bonded to u) share a class and both their bonds to u are bridges"""
    free = [cls[s] for s in nbrs if is_bridge(u, s)]
    return len(set(free)) < len(free)


def class_pair(nbrs, cls):
    """two of `nbrs` share a class, whatever their bonds"""
    return len({cls[s] for s in nbrs}) < len(nbrs)


# ---------------------------------------------------------------------------------------------------------------- the string
def marked(symbols, xy, bonds, marks, tables, symmetric):
    """ez_ref.smiles (mnx_smiles_pack_marks) restated with one hook: symmetric(a, b, subs) -> a candidate that is set aside. The
    walk, the ring numbers, the sides and the flips are written anew here after the header; atom texts, bond symbols, the plain
    and the tetrahedral writer are the modules' own. Returns (text, pos, flags, n_rings, what) as ez_ref.smiles does, what with
    'symmetric': [(a, b)] and 'centres': stereo_ref's records."""
    n = len(symbols)
    what = {"candidates": {}, "directed": {}, "symmetric": [], "centres": {}}
    if marks & 1:
        *base, what["centres"] = T.smiles(symbols, xy, bonds, tables)
    else:
        base = list(S.smiles(symbols, bonds, tables))
    if base[0] is None or not marks & 2:
        return (*base, what)
    flags, n_rings = base[2], base[3]
    at_marks = {c: r["mark"] for c, r in what["centres"].items()}
    atoms = [S.atom_text(s, tables) for s in symbols]
    around = [[] for _ in range(n)]
    for b in bonds:                                         # (a bond is written with the `type` of its record)
        around[b[0]].append((b[1], b[2]))
        around[b[1]].append((b[0], b[2]))
    for a in around:
        a.sort()
    is_bridge = bridges(n, bonds)

    pos, parent, children, rings, written, roots = {}, {}, [[] for _ in range(n)], [[] for _ in range(n)], [], []
    for root in range(n):                                   # depth-first, neighbours in ascending index, an explicit stack
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
            nb, ty = around[a][k]
            if nb == parent[a]:
                continue
            if nb in pos:
                rings[a].append((nb, ty))
                continue
            pos[nb], parent[nb] = len(written), a
            written.append(nb)
            children[a].append((nb, ty))
            stack.append([nb, 0])

    in_use, number, items, closed = set(), {}, [""] * n, []
    for p, a in enumerate(written):                         # closures, then openings, each by the other end's position
        in_use -= set(closed)
        closed = []
        ends = sorted(rings[a], key=lambda e: pos[e[0]])
        for nb, ty in ends:
            if pos[nb] < p:
                items[a] += S.ring_digits(number[nb, a])
                closed.append(number[nb, a])
        for nb, ty in ends:
            if pos[nb] > p:
                r = min(set(range(1, 101)) - in_use)
                in_use.add(r)
                number[a, nb] = r
                items[a] += S.bond_text(ty, atoms[a][1] and atoms[nb][1]) + S.ring_digits(r)

    cands = what["candidates"]
    for i, j, ty, _ in bonds:
        if ty != 2 or not is_bridge(i, j) or atoms[i][2] or atoms[j][2]:
            continue
        subs = {u: [(nb, t) for nb, t in around[u] if nb != v] for u, v in ((i, j), (j, i))}
        if not all(1 <= len(s) <= 2 and all(t in E.SINGLE for _, t in s) for s in subs.values()):
            continue
        a, b = (i, j) if pos[i] < pos[j] else (j, i)
        if symmetric(a, b, {u: [x for x, _ in subs[u]] for u in (a, b)}):
            what["symmetric"].append((a, b))
            continue
        sides = {u: {x: E.side(xy, a, b, u, x) for x, _ in subs[u]} for u in (a, b)}
        resolved = all(s != 0 for d in sides.values() for s in d.values()) and all(len(set(d.values())) == len(d) for d in sides.values())
        tree = {a: ([parent[a]] if parent[a] is not None else []) + [c for c, _ in children[a] if c != b], b: [c for c, _ in children[b]]}
        cands[a, b] = {"resolved": resolved, "sides": sides, "tree": tree}

    directed = what["directed"]
    for (a, b), c in sorted(cands.items(), key=lambda e: pos[e[0][0]]):
        if not c["resolved"]:
            continue
        p = parent[a]
        listed = [(p, a)] * (p is not None) + [(a, x) for x in c["tree"][a] if x != p] + [(b, x) for x in c["tree"][b]]

        def symbol(bond, flip):
            if bond == (p, a):
                return "\\" if (c["sides"][a][p] > 0) != flip else "/"
            return "/" if (c["sides"][bond[0]][bond[1]] > 0) != flip else "\\"
        want = directed.get((p, a), "/") if listed[0] == (p, a) else "/"
        flip = symbol(listed[0], False) != want
        for bond in listed:
            directed[bond] = symbol(bond, flip)

    def text_of(a):
        t = atoms[a][0]
        return t[:2] + at_marks[a] + t[2:] if at_marks.get(a) else t
    sub = [None] * n
    for a in reversed(written):
        s = text_of(a) + items[a]
        for k, (c, ty) in enumerate(children[a]):
            t = (directed.get((a, c)) or S.bond_text(ty, atoms[a][1] and atoms[c][1])) + sub[c]
            s += t if k == len(children[a]) - 1 else "(" + t + ")"
            sub[c] = None
        sub[a] = s
    text = ".".join(sub[r] for r in roots)

    has = {u for bond in directed for u in bond}
    own = {frozenset(k) for k, c in cands.items() if c["resolved"]} | {frozenset(k) for k in what["symmetric"]}
    flags |= E.FLAG_EZ if directed else 0
    flags |= E.FLAG_EZ_UNRESOLVED if any(not c["resolved"] for c in cands.values()) else 0
    flags |= E.FLAG_EZ_IMPLIED if any(ty == 2 and frozenset((i, j)) not in own and i in has and j in has for i, j, ty, _ in bonds) else 0
    return text, [pos[a] for a in range(n)], flags, n_rings, what


def smiles(symbols, xy, bonds, marks=0, tables=None, even_with_pseudo=False):
    """One molecule: (text or None, written position of every atom or None, flags, n_rings, rank, sym_class, atom_marks or None,
    what); rank and sym_class are None for a molecule with the same atom pair in two bond records. what = {'centres' {atom:
    'kept' / 'dropped' / 'ring pair' (kept although two neighbours share a class: a bond on a cycle)}, 'bonds' {(a, b): the
    same}, 'directed' {(parent, child): symbol}, 'pseudo' the rule was off} — atoms by RANK, the numbering the string is
    written in. even_with_pseudo: the rule stays on for a molecule that holds a pseudo-atom (coverage() asks what it would do)."""
    tables = M.name_tables() if tables is None else tables
    n = len(symbols)
    if len({frozenset(b[:2]) for b in bonds}) != len(bonds):
        text, pos, flags, n_rings = E.smiles(symbols, xy, bonds, marks, tables)[:4]
        assert text is None and flags & S.FLAG_DUPLICATE
        return None, None, flags, n_rings, None, None, None, {}
    rank, sym_class, tie = K.ranks(symbols, xy, bonds, tables)
    msym, mxy, mbonds = T.renumber((symbols, xy, bonds), rank, np.random.default_rng(0))
    cls = [0] * n
    for a in range(n):
        cls[rank[a]] = sym_class[a]
    pseudo = any(S.atom_text(s, tables)[2] for s in symbols)
    on = even_with_pseudo or not pseudo
    is_bridge = bridges(n, mbonds)
    nbrs = [[] for _ in range(n)]
    for b in mbonds:
        nbrs[b[0]].append(b[1])
        nbrs[b[1]].append(b[0])
    what = {"centres": {}, "bonds": {}, "directed": {}, "pseudo": pseudo and not even_with_pseudo}

    if marks & 1:                                           # symmetry first: the candidates are stereo_ref's, the drawing is not asked
        for c, r in T.smiles(msym, mxy, mbonds, tables)[4].items():
            if r["candidate"]:
                what["centres"][c] = "dropped" if on and equal_pair(c, nbrs[c], cls, is_bridge) else \
                    "ring pair" if on and class_pair(nbrs[c], cls) else "kept"
    msym = [UNMARKED[s] if what["centres"].get(a) == "dropped" else s for a, s in enumerate(msym)]

    def symmetric(a, b, subs):
        drop = on and any(equal_pair(u, subs[u], cls, is_bridge) for u in (a, b))
        what["bonds"][a, b] = "dropped" if drop else "ring pair" if on and any(class_pair(subs[u], cls) for u in (a, b)) else "kept"
        return drop
    text, pos, flags, n_rings, w = marked(msym, mxy, mbonds, marks, tables, symmetric)
    flags |= tie
    if text is None:
        return None, None, flags, n_rings, rank, sym_class, None, what
    what["directed"] = w["directed"]
    bits = [0] * n
    for c, r in w["centres"].items():
        bits[c] |= {"@": ATOM_CW, "@@": ATOM_CCW, "": 0}[r["mark"]]
    for c, v in what["centres"].items():
        bits[c] |= ATOM_SYM if v == "dropped" else 0
    for (a, b), c in w["candidates"].items():
        if c["resolved"]:
            bits[a] |= ATOM_EZ
            bits[b] |= ATOM_EZ
    for a, b in w["symmetric"]:
        bits[a] |= ATOM_EZ_SYM
        bits[b] |= ATOM_EZ_SYM
    if any(v & (ATOM_SYM | ATOM_EZ_SYM) for v in bits):
        flags |= FLAG_SYM
    return text, [pos[rank[a]] for a in range(n)], flags, n_rings, rank, sym_class, [bits[rank[a]] for a in range(n)], what


def pack(mols, atoms, bonds, text, marks=0, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None,
         order_fill=S.NO_POSITION, marks_fill=NO_MARKS):
    """mnx_smiles_pack_symmetric on host arrays, as canon_ref.pack: {'recs', 'order', 'rank', 'sym_class', 'atom_marks' uint8,
    'out', 'total'}; atom_marks holds NO_MARKS where `order` holds NO_POSITION and marks_fill where the call writes nothing"""
    out = S.pack_with(lambda syms, xy, B, tb: smiles(syms, xy, B, marks, tb)[:7], mols, atoms, bonds, text, tables, n_atom_records,
                      n_bond_records, n_text_bytes, order_fill, extra=("rank", "sym_class", "atom_marks"))
    written = S.pack_with(lambda syms, xy, B, tb: (None, None, 0, 0), mols, atoms, bonds, text, tables, n_atom_records, n_bond_records,
                          n_text_bytes, 0)["order"] != 0           # the entries that lie inside a molecule
    out["atom_marks"] = np.where(written, np.where(out["order"] == S.NO_POSITION, NO_MARKS, out["atom_marks"] & 0xFF), marks_fill).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------- molecules
LEAVES = (b"C", b"C", b"N", b"O", b"F", b"Cl")


def branch(rng, conjugated=False):
    """a small tree that hangs on its atom 0: (symbols, bonds); conjugated: atom 0 = atom 1 is double, so the bond that
    attaches atom 0 stands beside a candidate"""
    k = int(rng.integers(2, 5)) if conjugated else int(rng.integers(1, 5))
    symbols = [b"C" if a < k - 1 else LEAVES[int(rng.integers(len(LEAVES)))] for a in range(k)]
    bonds = [(int(rng.integers(0, a)) if a > 2 and rng.random() < 0.3 else a - 1, a, 1, 1) for a in range(1, k)]
    if conjugated:
        bonds[0] = (0, 1, 2, 2)
    return symbols, bonds


def generate(rng, base=None):
    """One molecule with a symmetric candidate: (symbols, xy, bonds). A new atom u gets two copies of one branch and
      'centre'  becomes [C@H] / [C@] with a wedge seen from it, its other neighbours a further branch or the base molecule;
      'end'     is the end of a double bond u = w, w carrying one or two other substituents;
      'chain'   the same with conjugated branches and w - y = z - leaf behind it: candidates in front of and behind the
                symmetric one, so the flip of the later one can change;
      'ring'    (no symmetric candidate) a marked carbon of a plain carbon ring with one substituent: its ring neighbours
                share a class on ring bonds, and the mark is kept.
    base: a molecule the new part is bonded to (at an atom with fewer than four bonds), or None. A tenth get a pseudo-atom."""
    symbols, xy, bonds = ([], [], []) if base is None else (list(base[0]), list(base[1]), list(base[2]))
    lo = min((min(p) for p in xy), default=900)
    hi = max((max(p) for p in xy), default=1100) + 40

    def atom(sym):
        symbols.append(sym)
        xy.append((int(rng.integers(lo, hi)), int(rng.integers(lo, hi))))
        return len(symbols) - 1

    def hang(u, br, ty=(1, 1)):
        first = len(symbols)
        for s in br[0]:
            atom(s)
        bonds.append((u, first, *ty))
        bonds.extend((first + i, first + j, t, r) for i, j, t, r in br[1])

    degree = [0] * len(symbols)
    for b in bonds:
        degree[b[0]] += 1
        degree[b[1]] += 1
    free = [a for a in range(len(symbols)) if degree[a] < 4 and symbols[a] in (b"C", b"N")]
    anchor = free[int(rng.integers(len(free)))] if free else None
    kind = ("centre", "end", "chain", "ring")[int(rng.integers(4))]
    other = (b"R", b"Ph")[int(rng.integers(2))] if rng.random() < 0.1 else None
    if kind == "ring":
        size = int(rng.integers(3, 7))
        ring = [atom(b"[C@H]")] + [atom(b"C") for _ in range(size - 1)]
        bonds.extend((ring[k], ring[(k + 1) % size], 1, 1) if ring[k] < ring[(k + 1) % size] else (ring[(k + 1) % size], ring[k], 1, 1)
                     for k in range(size))
        if anchor is None:
            hang(ring[0], branch(rng), (5, 6) if rng.random() < 0.5 else (6, 5))
        else:
            bonds.append((anchor, ring[0], 6, 5) if rng.random() < 0.5 else (anchor, ring[0], 5, 6))
        if size > 3 and rng.random() < 0.5:                 # the 1,4-dimethylcyclohexane pattern: a second centre across the ring
            far = ring[size // 2]
            symbols[far] = b"[C@@H]"
            hang(far, ([b"C"], []), (5, 6))
    elif kind == "centre":
        rest = 1 + int(rng.random() < 0.5)                 # neighbours besides the pair: with the H of [C@H] four in all
        u = atom(b"[C@]" if rest == 2 else (b"[C@H]", b"[C@@H]")[int(rng.integers(2))])
        br = branch(rng, conjugated=rng.random() < 0.2)
        wedge = int(rng.integers(2 + rest))                 # which of u's bonds is the wedge as u sees it
        seen = [((5, 6) if rng.random() < 0.6 else (6, 5)) if k == wedge else (1, 1) for k in range(2 + rest)]
        hang(u, br, seen[0])
        hang(u, br, seen[1])
        k = 2
        if anchor is not None:
            bonds.append((anchor, u, seen[k][1], seen[k][0]))
            k += 1
        while k < 2 + rest:
            hang(u, ([other], []) if other else branch(rng), seen[k])
            other = None
            k += 1
    else:
        u, w = atom(b"C"), atom(b"C")
        bonds.append((u, w, 2, 2))
        br = branch(rng, conjugated=kind == "chain" or rng.random() < 0.2)
        hang(u, br)
        hang(u, br)
        if kind == "chain":
            y, z = atom(b"C"), atom(b"C")
            bonds.extend([(w, y, 1, 1), (y, z, 2, 2)])
            hang(z, ([LEAVES[int(rng.integers(len(LEAVES)))]], []))
            if anchor is not None:
                bonds.append((anchor, z, 1, 1))
        else:
            if anchor is not None:
                bonds.append((anchor, w, 1, 1))
            if anchor is None or rng.random() < 0.4:
                hang(w, ([other], []) if other else branch(rng))
    keys = [int(k) for k in rng.permutation(len(bonds))]
    return symbols, xy, [bonds[k] for k in keys]


def generated_set(count=160, seed=41):
    """every second molecule stands alone, the others are grafted onto a molecule of at most 28 atoms of the two older generators;
    at most 40 atoms each"""
    rng = np.random.default_rng(seed)
    bases = [m for m in T.generated_set(120) + E.generated_set(120) if len(m[0]) <= 28]
    out = []
    while len(out) < count:
        mol = generate(rng, bases[int(rng.integers(len(bases)))] if len(out) % 2 else None)
        if len(mol[0]) <= 40:
            out.append(mol)
    return out


def coverage(mols):
    """what the oracle's output over `mols` covers: counts of the situations of the rule (marks 3)"""
    keys = ("dropped centre", "dropped bond", "kept centre", "kept bond", "kept and dropped", "ring pair kept", "pseudo off",
            "flip changed", "all symmetric", "wedge at dropped centre")
    c = dict.fromkeys(keys, 0)
    for mol in mols:
        text, pos, flags, n_rings, rank, sym_class, bits, what = smiles(*mol, 3)
        if text is None:
            continue
        if what["pseudo"]:
            c["pseudo off"] += bool(smiles(*mol, 3, even_with_pseudo=True)[2] & FLAG_SYM)
        verdicts = list(what["centres"].values()) + list(what["bonds"].values())
        c["dropped centre"] += sum(v == "dropped" for v in what["centres"].values())
        c["dropped bond"] += sum(v == "dropped" for v in what["bonds"].values())
        c["kept centre"] += sum((b & 3) != 0 for b in bits)
        c["kept bond"] += sum((b & ATOM_EZ) != 0 for b in bits) // 2
        c["kept and dropped"] += bool(flags & FLAG_SYM) and any(b & (3 | ATOM_EZ) for b in bits)
        ends = {u for bond, v in what["bonds"].items() if v == "ring pair" for u in bond}
        c["ring pair kept"] += any((b & 3 and what["centres"].get(rank[a]) == "ring pair") or (b & ATOM_EZ and rank[a] in ends)
                                   for a, b in enumerate(bits))
        c["all symmetric"] += bool(verdicts) and all(v == "dropped" for v in verdicts)
        c["wedge at dropped centre"] += bool(flags & FLAG_SYM and flags & S.FLAG_WEDGES and not flags & T.FLAG_STEREO)
        if what["bonds"] and "dropped" in what["bonds"].values():
            moved = T.renumber(mol, rank, np.random.default_rng(0))
            before = E.smiles(*moved, 3)[4]["directed"]
            c["flip changed"] += any(before.get(bond, s) != s for bond, s in what["directed"].items())
    return c
