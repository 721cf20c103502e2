"""The oracle of mnx_graph_pack: the packed molecule records (include/molnextr_hip.h mnx_mol / mnx_atom / mnx_bond, the text
arena and totals) restated in numpy from the DENSE inputs, with CharTokenizer.sequence_to_smiles for the SMILES, symbols,
coordinates and positions and the pair loop of predict_images for the bonds. The tokenizer is pinned on the reference by the
goldens of tests/test_tokenizer.py, so this file, not the kernel, says what the tables hold."""
import numpy as np

from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE


def dense_atoms(tok, toks, lens, kmax):
    """(atom_idx int32 [n,kmax], n_atoms int32 [n]) as the atom scan of mnx_predict writes them: the tokenizer's 'indices',
    cut at kmax."""
    n = len(lens)
    idx = np.zeros((n, kmax), np.int32)
    cnt = np.zeros(n, np.int32)
    for b in range(n):
        ind = tok.sequence_to_smiles(toks[b, :lens[b]].tolist())["indices"][:kmax]
        cnt[b] = len(ind)
        idx[b, :cnt[b]] = ind
    return idx, cnt


def pack(tok, toks, lens, edges, kmax, atom_scores=None, edge_scores=None, overall=None):
    """{'mols', 'atoms', 'bonds' (structured arrays), 'text' (bytes), 'totals' (uint32 [4], totals[3] = 0)} of n rows:
    toks int [n,T], lens [n], edges uint8 [n,kmax,kmax] and optionally the three fp64 score arrays."""
    n = len(lens)
    mols = np.zeros(n, MOL_DTYPE)
    atoms, bonds, text = [], [], bytearray()
    for b in range(n):
        seq = toks[b, :lens[b]].tolist()
        d = tok.sequence_to_smiles(seq)
        smiles = d["smiles"].encode("utf-8")
        # bytes of the SMILES in front of position p: the names of the non-coordinate ids up to the first '<eos>' / '<pad>'
        off = [0]
        for t in seq:
            if t in (0, 2):
                break
            off.append(off[-1] + (len(tok.itos[t].encode("utf-8")) if t < tok.offset else 0))
        assert off[-1] == len(smiles)
        k = min(len(d["indices"]), kmax)
        m = mols[b]
        m["atom0"], m["n_atoms"], m["bond0"], m["text0"], m["smiles_len"] = len(atoms), k, len(bonds), len(text), len(smiles)
        m["flags"] = 1 if len(d["indices"]) > kmax else 0
        m["overall_score"] = 0.0 if overall is None else overall[b]
        for a in range(k):
            sym = d["symbols"][a].encode("utf-8")
            end = off[d["indices"][a] - 2]                  # the symbol's last id sits in front of x, y and the position
            assert smiles[end - len(sym):end] == sym
            x, y = seq[d["indices"][a] - 2] - tok.offset, seq[d["indices"][a] - 1] - tok.offset - tok.maxx
            assert [x / (tok.maxx - 1), y / (tok.maxy - 1)] == d["coords"][a]
            atoms.append((end - len(sym), len(sym), d["indices"][a], x, y, 0.0 if atom_scores is None else atom_scores[b, a]))
        nb = 0
        for i in range(k - 1):                              # reference model.py:135-143
            for j in range(i + 1, k):
                if edges[b, i, j] != 0:
                    bonds.append((i, j, edges[b, i, j], edges[b, j, i], 0.0 if edge_scores is None else edge_scores[b, i, j]))
                    nb += 1
        m["n_bonds"] = nb
        text += smiles
    return {"mols": mols, "atoms": np.array(atoms, ATOM_DTYPE).reshape(-1), "bonds": np.array(bonds, BOND_DTYPE).reshape(-1),
            "text": bytes(text), "totals": np.array([len(atoms), len(bonds), len(text), 0], np.uint32)}


def dense_preds(tok, toks, lens, n_atoms, edges, atom_scores=None, edge_scores=None, overall=None):
    """The per-image dicts as the dense code of predict_pipeline builds them (model.py), on host arrays."""
    preds = []
    for b in range(len(lens)):
        r = tok.sequence_to_smiles(toks[b, :lens[b]].tolist())
        k = int(n_atoms[b])
        assert k == len(r["indices"])
        preds.append({"chartok_coords": r, "edges": edges[b, :k, :k].astype(int).tolist()})
        if overall is not None:
            r["atom_scores"] = atom_scores[b, :k].tolist()
            preds[-1]["edge_scores"] = edge_scores[b, :k, :k].tolist()
            preds[-1]["overall_score"] = float(overall[b])
    return preds


def bonds_of_dense(pred, with_scores):
    """The 'bonds' list unpack_graphs gives for a dense prediction dict: (i, j, type, rev[, score]), i < j ascending."""
    e = pred["edges"]
    k = len(e)
    out = []
    for i in range(k - 1):
        for j in range(i + 1, k):
            if e[i][j] != 0:
                out.append((i, j, e[i][j], e[j][i]) + ((pred["edge_scores"][i][j],) if with_scores else ()))
    return out


def assert_packed_equals_dense(packed, dense, with_scores):
    """Field by field: a prediction of unpack_graphs against the dense dict of the same image (floats bit for bit)."""
    assert len(packed) == len(dense)
    for b, (p, q) in enumerate(zip(packed, dense)):
        assert p["chartok_coords"] == q["chartok_coords"], b
        assert p["bonds"] == bonds_of_dense(q, with_scores), b
        assert set(p) == {"chartok_coords", "bonds"} | ({"overall_score"} if with_scores else set()), b
        if with_scores:
            assert p["overall_score"] == q["overall_score"], b


def fuzz_rows(tok, rng, n_rows, T):
    """n_rows id rows [n_rows, T] (+ lengths) drawn from the whole vocabulary under the decode-time grammar mask
    (get_output_mask: after an x-bin a y-bin, after a y-bin no coordinate), biased towards atoms with coordinates; most rows
    end with '<eos>', some run to T, specials appear inside rows."""
    x0, y0, V = tok.offset, tok.offset + tok.maxx, len(tok)
    atom_ids = [i for i in range(x0) if tok.is_atom(i)]
    toks = np.zeros((n_rows, T), np.int32)
    lens = np.zeros(n_rows, np.int32)
    for b in range(n_rows):
        want = int(rng.integers(1, T + 1)) if rng.random() < 0.9 else T + 1      # T + 1: no '<eos>', the row fills T
        seq, prev = [], 1
        while len(seq) < min(want, T):
            if x0 <= prev < y0:
                t = int(rng.integers(y0, V))
            else:
                r = rng.random()
                if r < 0.35:
                    t = atom_ids[int(rng.integers(len(atom_ids)))]
                elif r < 0.70:
                    t = int(rng.integers(x0, y0)) if prev < x0 else int(rng.integers(5, x0))
                elif r < 0.73:
                    t = int(rng.choice([1, 3, 4] * 5 + [0, 2]))      # specials inside the row; rarely an early end
                else:
                    t = int(rng.integers(5, x0 if prev >= y0 else V))
            seq.append(t)
            prev = t
        if want <= T:
            seq[-1] = 2
        toks[b, :len(seq)] = seq
        lens[b] = len(seq)
        if rng.random() < 0.3:                               # what lies beyond the length is undefined: make it visible
            toks[b, len(seq):] = rng.integers(5, V, T - len(seq))
    return toks, lens


def random_edges(rng, n_atoms, kmax):
    """uint8 [n,kmax,kmax] with a sparsity of its own per image (fully connected and empty ones among them), the two triangles
    independent (rev need not mirror type), the diagonal set, and garbage beyond n_atoms (undefined there)."""
    n = len(n_atoms)
    e = np.full((n, kmax, kmax), 7, np.uint8)
    for b, k in enumerate(n_atoms):
        p = (0.0, 1.0, 0.1, 0.5)[b % 4] if b < 8 else rng.random()
        blk = rng.integers(1, 7, (k, k)).astype(np.uint8) * (rng.random((k, k)) < p)
        np.fill_diagonal(blk, rng.integers(1, 7, k))
        e[b, :k, :k] = blk
    return e
