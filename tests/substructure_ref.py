"""The oracle of mnx_substructure_match (include/molnextr_hip.h, "Substructure search") in plain Python, written from the rule:
atoms compared as tuples of what molfile_ref.interpret reads, plain recursion over sorted neighbour lists with the step count of
the rule, where the kernel compares packed words and walks on a stack in on-chip memory. A second matcher, embeddings_brute, knows
neither an order nor a step: itertools.permutations over the target's atoms. Neither shares code with the kernel."""
import itertools
import sys

import numpy as np

import molfile_ref as M
from molnextr_amd.engine import MATCH_DTYPE

TOO_LARGE, BEYOND, PSEUDO, TRUNCATED, BAD_BOND = 1, 2, 4, 8, 16
QUERY_TOO_LARGE, QUERY_EMPTY, LIMIT, BAD_PAIR, QUERY_SHIFT = 32, 64, 1 << 16, 1 << 17, 8
SIDE_REFUSED = TOO_LARGE | BEYOND | BAD_BOND
REFUSED = SIDE_REFUSED | SIDE_REFUSED << QUERY_SHIFT | QUERY_TOO_LARGE | QUERY_EMPTY | BAD_PAIR
MAX_QUERY, MAX_QUERY_BONDS, DEFAULT_STEPS, MAX_STEPS, NO_ATOM = 64, 128, 65536, 1 << 20, 0xFFFF
WILD = "*"
ANY = 4                                                # the bond class of every type but 1 .. 6


def atom_key(sym: bytes, tables):
    """WILD for an atom that is no plain atom (a pseudo-atom, a numbered R-group, a '*'), else (element as read, aromatic, charge,
    isotope)"""
    a = M.interpret(sym, tables)
    if a["pseudo"] or a["symbol"] == "R":
        return WILD
    body = sym[1:].lstrip(b"0123456789") if a["bracket"] else sym
    return a["symbol"], body[:1].islower(), a["charge"], a["isotope"]


def atoms_match(q, t) -> bool:
    if q == WILD:
        return True
    return t != WILD and q[:3] == t[:3] and q[3] in (0, t[3])


def bond_class(ty: int) -> int:
    return {1: 0, 5: 0, 6: 0, 2: 1, 3: 2, 4: 3}.get(ty, ANY)


def bonds_match(q: int, t: int) -> bool:
    return q == ANY or q == t


def graph(symbols, bonds, tables=None):
    """(atom keys, {atom: {neighbour: bond class}}) of one molecule with valid bonds, no pair twice"""
    tables = M.name_tables() if tables is None else tables
    around = [{} for _ in symbols]
    for i, j, ty, *_ in bonds:
        around[i][j] = around[j][i] = bond_class(ty)
    return [atom_key(s, tables) for s in symbols], around


def query_order(around):
    """(order, parent): breadth first from the lowest atom not yet placed, neighbours ascending; parent[k] a position or None"""
    order, parent, placed = [], [], set()
    for first in range(len(around)):
        if first in placed:
            continue
        placed.add(first)
        order.append(first)
        parent.append(None)
        head = len(order) - 1
        while head < len(order):
            for b in sorted(around[order[head]]):
                if b not in placed:
                    placed.add(b)
                    order.append(b)
                    parent.append(head)
            head += 1
    return order, parent


class _Stop(Exception):
    pass


def search_root(q, t, root, max_matches, max_steps):
    """the search from one root: (the embeddings as image lists along the order, the steps S(root))"""
    (qk, qa), (tk, ta) = q, t
    order, parent = query_order(qa)
    found, image, steps = [], [None] * len(order), [1]

    def accept(k, cand):
        a = order[k]
        if cand in image[:k] or not atoms_match(qk[a], tk[cand]):
            return False
        return all(image[l] in ta[cand] and bonds_match(c, ta[cand][image[l]]) for l in range(k) for c in [qa[a].get(order[l])] if c is not None)

    def place(k):
        if k == len(order):
            found.append(list(image))
            if len(found) == max_matches:
                raise _Stop
            return
        for cand in (sorted(ta[image[parent[k]]]) if parent[k] is not None else range(len(tk))):
            steps[0] += 1
            if steps[0] > max_steps:
                raise _Stop
            if accept(k, cand):
                image[k] = cand
                place(k + 1)
        image[k] = None

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 400))
    try:
        if accept(0, root):
            image[0] = root
            place(1)
    except _Stop:
        pass
    finally:
        sys.setrecursionlimit(limit)
    return found, steps[0]


def match(q, t, max_matches=1, max_steps=0):
    """one admitted pair of graphs (graph()), the query of 1 .. 64 atoms: (n_matches, steps, limited, the map as a list of target
    atoms in the query's atom order or None)"""
    max_matches, max_steps = max_matches or 1, max_steps or DEFAULT_STEPS
    order, _ = query_order(q[1])
    total, most, broken, first = 0, 0, False, None
    for root in range(len(t[0])):
        found, steps = search_root(q, t, root, max_matches, max_steps)
        total += len(found)
        most = max(most, steps)
        broken |= steps > max_steps
        if found and first is None:
            first = [None] * len(order)
            for k, a in enumerate(order):
                first[a] = found[0][k]
    n = min(total, max_matches)
    return n, most, broken and n < max_matches, first


def embeddings_brute(q, t):
    """every embedding of q in t as a tuple of target atoms in the query's ATOM order, by trying every injective map"""
    (qk, qa), (tk, ta) = q, t
    out = []
    for images in itertools.permutations(range(len(tk)), len(qk)):
        if all(atoms_match(qk[a], tk[images[a]]) for a in range(len(qk))) and \
                all(images[b] in ta[images[a]] and bonds_match(c, ta[images[a]][images[b]]) for a in range(len(qk)) for b, c in qa[a].items()):
            out.append(images)
    return out


def is_embedding(q, t, images) -> bool:
    """the rule checked directly on one map (target atoms in the query's atom order)"""
    (qk, qa), (tk, ta) = q, t
    if len(images) != len(qk) or len(set(images)) != len(images) or any(not 0 <= x < len(tk) for x in images):
        return False
    return all(atoms_match(qk[a], tk[images[a]]) for a in range(len(qk))) and \
        all(images[b] in ta[images[a]] and bonds_match(c, ta[images[a]][images[b]]) for a in range(len(qk)) for b, c in qa[a].items())


def admit(mols, atoms, bonds, text, b, tables, n_a, n_b, n_t):
    """one side as mnx_fingerprint_pack admits a molecule: (bits 0-4, graph() or None when refused, n_atoms, n_bonds)"""
    m = mols[b]
    a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
    flags = TRUNCATED if int(m["flags"]) & 1 else 0
    if na > 999 or nb > 999:
        flags |= TOO_LARGE
    if a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t:
        flags |= BEYOND
    if flags & (TOO_LARGE | BEYOND):
        return flags, None, na, nb
    A, B = atoms[a0:a0 + na], bonds[b0:b0 + nb]
    if any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in A):
        return flags | BEYOND, None, na, nb
    syms = [text[t0 + int(a["sym0"]):t0 + int(a["sym0"]) + int(a["sym_len"])] for a in A]
    if any(M.interpret(s, tables)["pseudo"] for s in syms):
        flags |= PSEUDO
    pairs = [(int(x["i"]), int(x["j"])) for x in B]
    if any(i >= na or j >= na or i == j for i, j in pairs) or len({frozenset(p) for p in pairs}) != len(pairs):
        return flags | BAD_BOND, None, na, nb
    return flags, graph(syms, [(i, j, int(x["type"])) for (i, j), x in zip(pairs, B)], tables), na, nb


def pack(query, target, pairs, max_matches=1, max_steps=0, tables=None, q_sizes=None, t_sizes=None):
    """mnx_substructure_match on host arrays: query and target are (mols, atoms, bonds, text), pairs [n][2]; q_sizes / t_sizes:
    (atom records, bond records, text bytes) where a side is passed as shorter than it is. {'match' MATCH_DTYPE [n], 'map' uint16
    [n, 64], 'most': per pair the largest S(r)}"""
    tables = M.name_tables() if tables is None else tables
    sides = []
    for (mols, atoms, bonds, text), sizes in ((query, q_sizes), (target, t_sizes)):
        text = bytes(text)
        sides.append(((mols, atoms, bonds, text), sizes if sizes is not None else (len(atoms), len(bonds), len(text)), {}))
    recs, maps = np.zeros(len(pairs), MATCH_DTYPE), np.full((len(pairs), MAX_QUERY), NO_ATOM, np.uint16)

    def side(k, b):
        arrays, sizes, seen = sides[k]
        if b not in seen:
            seen[b] = admit(*arrays, b, tables, *sizes)
        return seen[b]

    for p, (qi, ti) in enumerate(np.asarray(pairs, np.uint32).reshape(-1, 2).tolist()):
        if qi >= len(query[0]) or ti >= len(target[0]):
            recs[p] = (BAD_PAIR, 0, 0, 0)
            continue
        (qf, q, nq, nqb), (tf, t, _, _) = side(0, qi), side(1, ti)
        flags = tf | qf << QUERY_SHIFT
        if q is not None:
            flags |= QUERY_EMPTY if nq == 0 else QUERY_TOO_LARGE if nq > MAX_QUERY or nqb > MAX_QUERY_BONDS else 0
        if flags & REFUSED:
            recs[p] = (flags, 0, 0, 0)
            continue
        n, most, limited, first = match(q, t, max_matches, max_steps)
        recs[p] = (flags | (LIMIT if limited else 0), n, most, 0)
        if first is not None:
            maps[p, :nq] = first
    return {"match": recs, "map": maps}
