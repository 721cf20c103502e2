"""What the GPU tests of the two writers of the packed molecule tables (test_gpu_molfile.py, test_gpu_smiles.py) share: the pool
of symbols, random molecules, the tables on the device, and the comparison of one call's records and bytes with an oracle's."""
import ctypes as C

import numpy as np
import torch

import molfile_ref as R

FILL, GUARD = 0x7F, 64
UTF2 = "ŕ".encode("utf-8")              # the vocabulary's two-byte character

# symbols of every class: parsed plain / bracket atoms, the four chiral carbons, table names, unparsable and empty ones
POOL = [b"C", b"N", b"O", b"Cl", b"Br", b"c", b"n", b"s", b"I", b"[nH]", b"[NH3+]", b"[O-]", b"[13C]", b"[C@@H]", b"[C@]", b"[C@H]",
        b"[C@@]", b"[R1]", b"[R12]", b"R", b"[OMe]", b"[Ac]", b"Ph", b"[Xx]", b"[C", b"*", b"[*]", b"[Fe+3]", b"[N++]", b"[se]", b"[2H]",
        b"", b"[]", b"[C:12]", b"[" + UTF2 + b"]", UTF2, b"[[a*]]", b"[a*]", b"R'", b"[2, 4-Cl2C6H3]", b"[Si]", b"[CH12]", b"[U+15]",
        b"[C-16]", b"[999Og]", b"<unk>", b"[\x01\x7f\n]", b"[3,5-[CF3]2C6H3]", b"[3,5-[CF3]2C6H3x]", b"Z", b"[H]", b"[Cn]", b"[C@@H2-]"]


def random_molecule(rng, n_atoms, n_bonds, pool=POOL):
    syms = [pool[k] for k in rng.integers(0, len(pool), n_atoms)]
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (n_atoms, 2))]
    bonds = []
    for _ in range(n_bonds if n_atoms >= 2 else 0):
        i, j = sorted(int(v) for v in rng.choice(n_atoms, 2, replace=False))
        bonds.append((i, j, int(rng.integers(1, 7)), int(rng.integers(0, 7))))
    return syms, xy, bonds


def _up(dev, a):
    raw = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return torch.frombuffer(bytearray(raw) + bytearray(8), dtype=torch.uint8).to(dev)


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


class Tables:
    """packed records on the host and on the device"""

    def __init__(self, dev, molecules=None, arrays=None):
        self.mols, self.atoms, self.bonds, self.text = arrays if arrays is not None else R.build_tables(molecules)
        self.n = len(self.mols)
        self.d = [_up(dev, a) for a in (self.mols, self.atoms, self.bonds, self.text)]
        self.dev = dev


def compare(recs, ref_recs, out, ref_out, total, what):
    """one call at the exact capacity `total` against an oracle: the records field by field, the bytes with the first difference
    shown, and the FILL bytes behind them"""
    for name in recs.dtype.names:
        bad = np.nonzero(recs[name] != ref_recs[name])[0]
        assert bad.size == 0, (name, bad[:5], recs[name][bad[:5]], ref_recs[name][bad[:5]])
    got = out[:total].tobytes()
    if got != ref_out:
        k = next(i for i, (x, y) in enumerate(zip(got, ref_out)) if x != y)
        raise AssertionError(f"first difference at byte {k}: {got[max(k - 80, 0):k + 40]!r} != {ref_out[max(k - 80, 0):k + 40]!r}")
    assert np.all(out[total:] == FILL), f"bytes behind the {what} were overwritten"
