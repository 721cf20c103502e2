"""The oracle of mnx_smiles_pack_marks (include/molnextr_hip.h) in three parts that share no code with the kernel:

* the WRITER — smiles() / pack(): the graph SMILES with '/' and '\\' at double bonds in plain Python. Its own walk (a stack of
  iterators over sorted neighbour lists), its own ring numbers, its own cycle test (take the bond out and search for its other
  end), its own sides (the cross product on the bins), the flip taken from the rule's wording: a list of directed bonds per
  candidate and a table of the symbols given so far. The atoms' texts and the bond symbols are smiles_ref's, the '@' / '@@' of
  mode 3 and the flag bits 0-9 are smiles_ref's and stereo_ref's (each pinned by its own tests);
* the READER — read(text): a written string parsed into atoms and bonds with their symbols; configurations(): for every double
  bond with a directed bond at both ends, cis or trans of one substituent of each end by the OpenSMILES wording ('/' = the atom
  behind it stands above the atom in front of it); drawn_cis(): the same from the drawing through angles in floating point,
  not the cross product;
* the generated molecules that the CPU and the GPU tests share — substituents at drawing-like angles, a share of them moved
  into the degenerate cases — and what they cover (coverage())."""
import math
import re

import numpy as np

import molfile_ref as M
import smiles_ref as S
import stereo_ref as T

FLAG_EZ, FLAG_EZ_UNRESOLVED, FLAG_EZ_IMPLIED = 1024, 2048, 4096
MARK_TETRAHEDRAL, MARK_DOUBLE_BOND = 1, 2
SINGLE = (1, 5, 6)


# ---------------------------------------------------------------------------------------------------------------- writer
def sign(v):
    return (v > 0) - (v < 0)


def side(xy, a, b, u, x):
    """on which side of the axis a -> b the substituent x of the end u lies: +1 left, -1 right, 0 on the line (y up)"""
    ax, ay = xy[b][0] - xy[a][0], xy[a][1] - xy[b][1]
    vx, vy = xy[x][0] - xy[u][0], xy[u][1] - xy[x][1]
    return sign(ax * vy - ay * vx)


def on_cycle(n, bonds, k):
    """is bond record k on a cycle: with the record taken out, can its j still be reached from its i?"""
    around = [[] for _ in range(n)]
    for q, b in enumerate(bonds):
        if q != k:
            around[b[0]].append(b[1])
            around[b[1]].append(b[0])
    seen, todo = {bonds[k][0]}, [bonds[k][0]]
    while todo:
        for nb in around[todo.pop()]:
            if nb not in seen:
                seen.add(nb)
                todo.append(nb)
    return bonds[k][1] in seen


def smiles(symbols, xy, bonds, marks=MARK_DOUBLE_BOND, tables=None):
    """One molecule: symbols [bytes], xy [(x_bin, y_bin)], bonds [(i, j, type, rev)] with valid i != j, marks a set of MARK_* ->
    (text or None, written position of every atom or None, flags, n_rings, what): what = {'candidates': {(a, b): record},
    'directed': {(parent, child): '/' or '\\'}, 'cycle_doubles': the type-2 records on a cycle}; a candidate's record =
    {'resolved', 'why' ('zero' / 'same' when not), 'subs': {end: {substituent: side}}, 'tree': {end: [its tree-bond substituents
    that carry a symbol, the parent first]}, 'root' a has no parent, 'forced' the flip came from an earlier candidate}"""
    tables = M.name_tables() if tables is None else tables
    n = len(symbols)
    base = T.smiles(symbols, xy, bonds, tables)[:4] if marks & MARK_TETRAHEDRAL else S.smiles(symbols, bonds, tables)
    at_marks = {c: r["mark"] for c, r in T.smiles(symbols, xy, bonds, tables)[4].items()} if marks & MARK_TETRAHEDRAL else {}
    what = {"candidates": {}, "directed": {}, "cycle_doubles": []}
    if base[0] is None or not marks & MARK_DOUBLE_BOND:
        return (*base, what)
    flags, n_rings = base[2], base[3]
    atoms = [S.atom_text(s, tables) for s in symbols]
    around = [[] for _ in range(n)]
    for b in bonds:
        around[b[0]].append((b[1], b[2]))
        around[b[1]].append((b[0], b[2]))
    for a in around:
        a.sort()

    # the walk
    written, pos, parent, children, rings, roots = [], {}, {}, [[] for _ in range(n)], [[] for _ in range(n)], []
    for root in range(n):
        if root in pos:
            continue
        roots.append(root)
        pos[root], parent[root] = len(written), None
        written.append(root)
        stack = [(root, iter(around[root]))]
        while stack:
            a, it = stack[-1]
            step = next(it, None)
            if step is None:
                stack.pop()
            elif step[0] == parent[a]:
                pass
            elif step[0] in pos:
                rings[a].append(step)
            else:
                nb = step[0]
                pos[nb], parent[nb] = len(written), a
                written.append(nb)
                children[a].append(step)
                stack.append((nb, iter(around[nb])))

    # ring numbers
    busy, number, items, freed = set(), {}, [""] * n, []
    for p, a in enumerate(written):
        busy.difference_update(freed)
        freed = []
        for nb, ty in sorted(rings[a], key=lambda e: pos[e[0]]):
            if pos[nb] < p:
                items[a] += S.ring_digits(number[nb, a])
                freed.append(number[nb, a])
        for nb, ty in sorted(rings[a], key=lambda e: pos[e[0]]):
            if pos[nb] > p:
                r = min(k for k in range(1, 101) if k not in busy)
                assert r <= 99                           # (base would have refused the molecule)
                busy.add(r)
                number[a, nb] = r
                items[a] += S.bond_text(ty, atoms[a][1] and atoms[nb][1]) + S.ring_digits(r)

    # the candidates
    cands = what["candidates"]
    for k, (i, j, ty, _) in enumerate(bonds):
        if ty != 2:
            continue
        if on_cycle(n, bonds, k):
            what["cycle_doubles"].append((i, j))
            continue
        if atoms[i][2] or atoms[j][2]:
            continue
        others = {u: [(nb, t) for nb, t in around[u] if nb != v] for u, v in ((i, j), (j, i))}
        if not all(1 <= len(o) <= 2 and all(t in SINGLE for _, t in o) for o in others.values()):
            continue
        a, b = (i, j) if pos[i] < pos[j] else (j, i)
        assert parent[b] == a, "a bond on no cycle is a tree bond"
        subs = {u: {x: side(xy, a, b, u, x) for x, _ in others[u]} for u in (a, b)}
        zero = any(s == 0 for d in subs.values() for s in d.values())
        same = any(len(d) == 2 and len(set(d.values())) == 1 for d in subs.values())
        tree = {a: ([parent[a]] if parent[a] is not None else []) + [c for c, _ in children[a] if c != b], b: [c for c, _ in children[b]]}
        assert tree[a] and tree[b], "every end has a tree-bond substituent"
        cands[a, b] = {"resolved": not zero and not same, "why": "zero" if zero else "same" if same else None, "subs": subs,
                       "tree": tree, "root": parent[a] is None, "forced": False}

    # the flips and the symbols, candidates in ascending written position of a
    directed = what["directed"]
    for (a, b), c in sorted(cands.items(), key=lambda e: pos[e[0][0]]):
        if not c["resolved"]:
            continue
        p = parent[a]
        listed = [(p, a)] * (p is not None) + [(a, x) for x in c["tree"][a] if x != p] + [(b, x) for x in c["tree"][b]]

        def symbol(bond, flip):
            if bond == (p, a):
                return "\\" if (c["subs"][a][p] > 0) != flip else "/"
            return "/" if (c["subs"][bond[0]][bond[1]] > 0) != flip else "\\"
        given = [bond for bond in listed if bond in directed]
        assert all(bond == (p, a) for bond in given), "only the bond to a's parent can have a symbol already"
        want = directed[p, a] if given else "/"
        flip = next(f for f in (False, True) if symbol(listed[0], f) == want)
        c["forced"] = bool(given)
        for bond in listed:
            s = symbol(bond, flip)
            assert directed.get(bond, s) == s, "no conflict is possible"
            directed[bond] = s

    # the string, children before their parent
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
    if directed:
        flags |= FLAG_EZ
    if any(not c["resolved"] for c in cands.values()):
        flags |= FLAG_EZ_UNRESOLVED
    resolved = {frozenset(k) for k, c in cands.items() if c["resolved"]}
    if any(ty == 2 and frozenset((i, j)) not in resolved and i in has and j in has for i, j, ty, _ in bonds):
        flags |= FLAG_EZ_IMPLIED
    return text, [pos[a] for a in range(n)], flags, n_rings, what


def pack(mols, atoms, bonds, text, marks=MARK_DOUBLE_BOND, tables=None, n_atom_records=None, n_bond_records=None, n_text_bytes=None,
         order_fill=S.NO_POSITION):
    """mnx_smiles_pack_marks on host arrays, as smiles_ref.pack: {'recs', 'order', 'out', 'total'}"""
    return S.pack_with(lambda syms, xy, B, tb: smiles(syms, xy, B, marks, tb)[:4], mols, atoms, bonds, text, tables, n_atom_records,
                       n_bond_records, n_text_bytes, order_fill)


# ---------------------------------------------------------------------------------------------------------------- reader
ATOM = re.compile(r"\[[^\]]*\]|Cl|Br|[BCNOPSFIbcnops*]")


def read(text):
    """(atom tokens in written order, {(a, b): symbol} with a < b in written order, a written before b; symbol '' for nothing).
    A ring bond takes the symbol in front of its opening digit; '/' or '\\' there is refused: the writer never directs one."""
    atoms, bonds, open_rings, stack = [], {}, {}, []
    prev, pending, k, dot = None, "", 0, True
    while k < len(text):
        m = ATOM.match(text, k)
        if m:
            me, k = len(atoms), m.end()
            atoms.append(m.group())
            if prev is not None and not dot:
                bonds[prev, me] = pending
            else:
                assert not pending
            prev, pending, dot = me, "", False
            continue
        c = text[k]
        k += 1
        if c in "-=#:~/\\":
            assert not pending and prev is not None and not dot
            pending = c
        elif c.isdigit() or c == "%":
            r = int(c) if c != "%" else int(text[k:k + 2])
            k += 0 if c != "%" else 2
            if r in open_rings:
                other, symbol = open_rings.pop(r)
                assert not pending
                bonds[other, prev] = symbol
            else:
                assert pending not in ("/", "\\"), "a directed ring bond"
                open_rings[r] = (prev, pending)
                pending = ""
        elif c == "(":
            assert not pending
            stack.append(prev)
        elif c == ")":
            assert not pending
            prev = stack.pop()
        elif c == ".":
            assert not pending and not stack
            dot = True
        else:
            raise ValueError(f"unexpected {c!r} in {text!r}")
    assert not open_rings and not stack and not pending
    return atoms, bonds


def configurations(text):
    """every double bond of a written string with a directed bond at both its ends, from the string alone: {(u, v): {(x, y):
    cis}} in written positions, u < v, x a directed substituent of u and y one of v. OpenSMILES: in 'x/u' and in 'u/x' the
    atom behind the symbol stands above the atom in front of it, '\\' below. Two directed substituents of one end must stand
    on opposite sides; where they do not the string contradicts itself and the bond's value is None (that can happen only at
    a double bond that is no resolved candidate, between the marks of two others: MNX_SMILES_EZ_IMPLIED covers it)."""
    atoms, bonds = read(text)
    above = {u: {} for u in range(len(atoms))}              # above[u][x]: x stands above u
    for (p, q), s in bonds.items():
        if s in ("/", "\\"):
            above[p][q] = s == "/"
            above[q][p] = s == "\\"
    out = {}
    for (u, v), s in bonds.items():
        if s == "=" and above[u] and above[v]:
            sound = all(len(above[w]) == 1 or len(set(above[w].values())) == 2 for w in (u, v))
            out[u, v] = {(x, y): above[u][x] == above[v][y] for x in above[u] for y in above[v]} if sound else None
    return out


def strip(text):
    """a written string without its '/' and '\\': each is taken out, and the '-' it replaced between two aromatic atoms put back"""
    atoms, bonds = read(text)
    put_back = iter([atoms[p].lstrip("[0123456789")[0].islower() and atoms[q].lstrip("[0123456789")[0].islower()
                     for (p, q), s in sorted(bonds.items(), key=lambda e: e[0][1]) if s in ("/", "\\")])
    return "".join(("-" if next(put_back) else "") if c in "/\\" else c for c in text)


def drawn_cis(xy, u, v, x, y):
    """do x (at u) and y (at v) lie on the same side of the line u - v in the drawing? Through angles, y up; None on the line"""
    def angle(p, q):
        return math.atan2(-(xy[q][1] - xy[p][1]), xy[q][0] - xy[p][0])
    axis = angle(u, v)
    turns = [(angle(u, x) - axis) % (2 * math.pi), (angle(v, y) - axis) % (2 * math.pi)]
    if any(min(abs(t), abs(t - math.pi), abs(t - 2 * math.pi)) < 1e-9 for t in turns):
        return None
    return (turns[0] < math.pi) == (turns[1] < math.pi)


def read_back(text, pos, xy):
    """{frozenset of the two atoms of a marked double bond: [(x, y, cis as the string reads, cis as the drawing shows)]}, atoms
    by index; None for a bond at which the string contradicts itself"""
    atom_at = {p: a for a, p in enumerate(pos)}
    return {frozenset((atom_at[u], atom_at[v])): pairs and [(atom_at[x], atom_at[y], cis, drawn_cis(xy, atom_at[u], atom_at[v], atom_at[x], atom_at[y]))
                                                            for (x, y), cis in pairs.items()]
            for (u, v), pairs in configurations(text).items()}


def named(bonds, bond, pairs):
    """the configuration of one marked double bond carried over to the lowest-numbered substituent of each end (whatever bond
    it hangs on): the sibling of a substituent stands on the other side. Returns (low end, high end, x, y, cis)."""
    u, v = sorted(bond)
    x, y, cis = pairs[0][:3]
    if x not in {b[0] if b[1] == u else b[1] for b in bonds if u in b[:2]}:
        x, y = y, x
    first = {w: min((b[0] if b[1] == w else b[1]) for b in bonds if w in b[:2] and set(b[:2]) != {u, v}) for w in (u, v)}
    return u, v, first[u], first[v], cis ^ (first[u] != x) ^ (first[v] != y)


# ---------------------------------------------------------------------------------------------------------------- molecules
PLAIN = (b"C", b"C", b"C", b"N", b"O", b"c")
PSEUDO = (b"R", b"[R1]", b"Ph")
STEP = 12                               # bins per bond


def generate(rng, n_atoms, ring_bonds, components=1, degenerate=0.25, double=0.45):
    """A forest of `components` trees over n_atoms atoms drawn as a chemist would: a bond of STEP bins, a chain that zigzags by
    60 degrees, a second branch on the other side, a third straight on, each end a bin or two off. Then up to ring_bonds bonds
    from an atom to an ancestor two to five bonds up. A tree bond becomes double with probability `double` where neither end has
    one (so conjugated chains are common), a few become triple or aromatic, a few single ones wedges; a few atoms are
    pseudo-atoms, a few of degree 3 with single bonds marked carbons with a wedge. A share `degenerate` of the double bonds
    then has one substituent moved: onto the line of the double bond, or beside its sibling on the same side.
    Returns (symbols, xy, bonds) with i < j and the records in random order."""
    deg, pairs, up, heading, has_double = [0] * n_atoms, {}, [None] * n_atoms, [None] * n_atoms, [False] * n_atoms
    xy = [None] * n_atoms
    starts = {0} | (set(int(v) for v in rng.choice(np.arange(1, n_atoms), components - 1, replace=False)) if components > 1 else set())
    kids = [0] * n_atoms
    for a in range(n_atoms):
        if a in starts:
            xy[a] = (int(rng.integers(900, 1100)), int(rng.integers(900, 1100)))
            heading[a] = float(rng.integers(0, 12)) * 30.0
            continue
        free = [k for k in range(a) if deg[k] < (3 if rng.random() < 0.9 else 4)] or [k for k in range(a) if deg[k] < 4]
        k = free[int(rng.integers(len(free)))] if rng.random() < 0.4 else free[-1]
        turn = (60.0, -60.0, 0.0, 180.0)[kids[k]] * (1 if up[k] is None or kids[up[k]] % 2 else -1)
        kids[k] += 1
        heading[a] = heading[k] + turn
        r = math.radians(heading[a])
        xy[a] = (xy[k][0] + int(round(STEP * math.cos(r))) + int(rng.integers(-1, 2)), xy[k][1] - int(round(STEP * math.sin(r))) + int(rng.integers(-1, 2)))
        up[a] = k
        ty = 1
        if not has_double[k] and not has_double[a] and rng.random() < double:
            ty = 2
            has_double[k] = has_double[a] = True
        elif rng.random() < 0.04:
            ty = 3 + int(rng.integers(0, 2))
        pairs[k, a] = [ty, ty]
        deg[k] += 1
        deg[a] += 1
    for _ in range(ring_bonds):
        i = j = int(rng.integers(n_atoms))
        for _ in range(int(rng.integers(2, 6))):
            j = up[j] if up[j] is not None else j
        i, j = sorted((i, j))
        if i != j and (i, j) not in pairs and deg[i] < 4 and deg[j] < 4:
            ty = 2 if not has_double[i] and not has_double[j] and rng.random() < 0.2 else 1
            has_double[i] |= ty == 2
            has_double[j] |= ty == 2
            for e, far in ((i, j), (j, i)):                 # an exocyclic double bond at e: the ring's two bonds on either side of it
                w = [p[0] if p[1] == e else p[1] for p, v in pairs.items() if e in p and v[0] == 2]
                near = [p[0] if p[1] == e else p[1] for p, v in pairs.items() if e in p and v[0] != 2]
                if ty == 1 and len(w) == 1 and len(near) == 1 and rng.random() < 0.8:
                    dx, dy, vx, vy = xy[w[0]][0] - xy[e][0], xy[w[0]][1] - xy[e][1], xy[near[0]][0] - xy[e][0], xy[near[0]][1] - xy[e][1]
                    along = 2.0 * (vx * dx + vy * dy) / (dx * dx + dy * dy)
                    xy[far] = (xy[e][0] + int(round(along * dx - vx)), xy[e][1] + int(round(along * dy - vy)))
            pairs[i, j] = [ty, ty]
            deg[i] += 1
            deg[j] += 1
    symbols =[PLAIN[int(rng.integers(len(PLAIN)))] if rng.random() < 0.97 else PSEUDO[int(rng.integers(len(PSEUDO)))] for _ in range(n_atoms)]
    for c in range(n_atoms):
        mine = [p for p in pairs if c in p]
        if deg[c] == 3 and all(pairs[p] == [1, 1] for p in mine) and rng.random() < 0.4:
            symbols[c] = (b"[C@H]", b"[C@@H]")[int(rng.integers(2))]
            p = mine[int(rng.integers(3))]
            cls = 5 if rng.random() < 0.6 else 6
            pairs[p] = [cls, T.MIRROR[cls]] if c == p[0] else [T.MIRROR[cls], cls]
    for p, v in pairs.items():
        if v == [1, 1] and rng.random() < 0.05:
            pairs[p] = [5, 6] if rng.random() < 0.5 else [6, 5]
    for (i, j), v in list(pairs.items()):
        if v[0] != 2 or rng.random() >= degenerate:
            continue
        u, w = (i, j) if rng.random() < 0.5 else (j, i)
        subs = [(p[0] if p[1] == u else p[1]) for p in pairs if u in p and w not in p]
        if not subs:
            continue
        d = (xy[w][0] - xy[u][0], xy[w][1] - xy[u][1])
        if len(subs) == 2 and rng.random() < 0.5:           # beside its sibling, on the same side
            xy[subs[1]] = (xy[subs[0]][0] + d[0], xy[subs[0]][1] + d[1])
        else:                                               # onto the line of the double bond
            xy[subs[0]] = (xy[u][0] - d[0], xy[u][1] - d[1])
    keys = list(pairs)
    return symbols, [(int(x), int(y)) for x, y in xy], [(i, j, *pairs[i, j]) for i, j in (keys[k] for k in rng.permutation(len(keys)))]


def generated_set(count=300, seed=31):
    """trees and ring systems of 6-60 atoms, every fourth of two or three components"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(6, 61))
        out.append(generate(rng, n, int(rng.integers(0, n // 4 + 2)) if k % 2 else 0, components=1 + (k % 4 == 3) * int(rng.integers(1, 3))))
    return out


def coverage(mols):
    """what the oracle's output over `mols` covers: counts of the situations of the rule"""
    keys = ("resolved", "root", "forced", "exocyclic", "one substituent", "two substituents", "in parentheses", "last child", "/", "\\",
            "zero side", "same side", "cycle double", "implied", "tetrahedral")
    c = dict.fromkeys(keys, 0)
    for symbols, xy, bonds in mols:
        text, pos, flags, n_rings, what = smiles(symbols, xy, bonds, 3)
        if text is None:
            continue
        c["cycle double"] += len(what["cycle_doubles"])
        c["implied"] += bool(flags & FLAG_EZ_IMPLIED)
        c["tetrahedral"] += text.count("@")
        c["/"] += text.count("/")
        c["\\"] += text.count("\\")
        c["in parentheses"] += text.count("(/") + text.count("(\\")
        c["last child"] += len(re.findall(r"[^(][/\\]", text))
        for (a, b), r in what["candidates"].items():
            c["zero side"] += r["why"] == "zero"
            c["same side"] += r["why"] == "same"
            if not r["resolved"]:
                continue
            c["resolved"] += 1
            c["root"] += r["root"]
            c["forced"] += r["forced"]
            c["exocyclic"] += any(len(r["tree"][u]) < len(r["subs"][u]) for u in (a, b))
            c["one substituent"] += sum(len(r["subs"][u]) == 1 for u in (a, b))
            c["two substituents"] += sum(len(r["subs"][u]) == 2 for u in (a, b))
    return c
