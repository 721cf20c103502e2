"""The oracle of mnx_main_pack (include/molnextr_hip.h) in plain Python, tables in and tables out: of every molecule the connected
component with the most atoms, among equals the one with the lowest atom — what the reference's _keep_main_molecule keeps
(GetMolFrags lists components by their lowest atom, np.argmax takes the first of the largest). It shares no code with the kernel:
a plain union-find over the bond records where the kernel propagates labels, Python lists where the kernel scans."""
import numpy as np

from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE

KEPT, TIE, REFUSED = 1 << 18, 1 << 19, 1 << 20
MAX_ATOMS = 2047


def components(n, pairs):
    """root[a] of every atom 0..n-1 after joining the pairs: the lowest atom of its component"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return [find(a) for a in range(n)]


def main_component(n, pairs):
    """(keep [bool per atom], flags) of one molecule of n atoms"""
    root = components(n, pairs)
    firsts = sorted(set(root))                                   # the components in GetMolFrags' order
    if len(firsts) <= 1:
        return [True] * n, 0
    sizes = [root.count(r) for r in firsts]
    largest = max(sizes)
    main = firsts[sizes.index(largest)]                          # np.argmax: the first of the largest
    return [r == main for r in root], KEPT | (TIE if sizes.count(largest) > 1 else 0)


def pack(mols, atoms, bonds, text, n_atom_records=None, n_bond_records=None, n_text_bytes=None):
    """mnx_main_pack on host arrays: {'mols', 'atoms', 'bonds', 'text', 'origin', 'totals'}"""
    text = bytes(text)
    n_a = len(atoms) if n_atom_records is None else n_atom_records
    n_b = len(bonds) if n_bond_records is None else n_bond_records
    n_t = len(text) if n_text_bytes is None else n_text_bytes
    out_mols = np.zeros(len(mols), MOL_DTYPE)
    A, B, origin, chunks, at_text = [], [], [], [], 0
    for b, m in enumerate(mols):
        a0, na, b0, nb, t0, tl = (int(m[k]) for k in ("atom0", "n_atoms", "bond0", "n_bonds", "text0", "smiles_len"))
        truncated = int(m["flags"]) & 1
        refused = a0 + na > n_a or b0 + nb > n_b or t0 + tl > n_t or na > MAX_ATOMS
        if not refused:
            ma, mb = atoms[a0:a0 + na], bonds[b0:b0 + nb]
            refused = (any(t0 + int(a["sym0"]) + int(a["sym_len"]) > n_t for a in ma) or
                       any(int(x["i"]) >= na or int(x["j"]) >= na for x in mb))
        if refused:
            out_mols[b] = (len(A), 0, len(B), 0, at_text, 0, truncated | REFUSED, 0, float(m["overall_score"]))
            continue
        keep, flags = main_component(na, [(int(x["i"]), int(x["j"])) for x in mb])
        new, first_atom, first_bond, off = {}, len(A), len(B), 0
        for a, rec in enumerate(ma):
            if keep[a]:
                new[a] = len(new)
                s0, sl = int(rec["sym0"]), int(rec["sym_len"])
                chunks.append(text[t0 + s0:t0 + s0 + sl])
                A.append((off, sl, int(rec["index"]), int(rec["x_bin"]), int(rec["y_bin"]), float(rec["score"])))
                origin.append(a)
                off += sl
        for x in mb:
            if keep[int(x["i"])]:
                B.append((new[int(x["i"])], new[int(x["j"])], int(x["type"]), int(x["rev"]), float(x["score"])))
        out_mols[b] = (first_atom, len(new), first_bond, len(B) - first_bond, at_text, off, truncated | flags, 0, float(m["overall_score"]))
        at_text += off
    return {"mols": out_mols, "atoms": np.array(A, ATOM_DTYPE).reshape(-1), "bonds": np.array(B, BOND_DTYPE).reshape(-1),
            "text": b"".join(chunks), "origin": np.array(origin, np.uint16), "totals": (len(A), len(B), at_text)}
