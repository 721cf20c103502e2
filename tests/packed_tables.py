"""The one harness of the GPU tests of the passes over the packed molecule tables (test_gpu_graph, _molfile, _smiles, _stereo, _ez,
_canon, _symmetry, _expand, _normalize, _smiles_read): the `dev` and `eng` fixtures, the pool of symbols and random molecules, the
tables on the device, one call function for the writers of text and one for the writers of tables, and the comparison of a call's
named result with an oracle's dict. This is no test module, so pytest does not rewrite its asserts: each carries its own message."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import molfile_ref as R
from molnextr_amd.engine import ATOM_DTYPE, BOND_DTYPE, MOL_DTYPE, MOLFILE_DTYPE, READ_DTYPE, SMILES_DTYPE, Engine

FILL, GUARD = 0x7F, 64
WORD_FILL = FILL | FILL << 8
UTF2 = "ŕ".encode("utf-8")              # the vocabulary's two-byte character

# symbols of every class: parsed plain / bracket atoms, the four chiral carbons, table names, unparsable and empty ones
POOL = [b"C", b"N", b"O", b"Cl", b"Br", b"c", b"n", b"s", b"I", b"[nH]", b"[NH3+]", b"[O-]", b"[13C]", b"[C@@H]", b"[C@]", b"[C@H]",
        b"[C@@]", b"[R1]", b"[R12]", b"R", b"[OMe]", b"[Ac]", b"Ph", b"[Xx]", b"[C", b"*", b"[*]", b"[Fe+3]", b"[N++]", b"[se]", b"[2H]",
        b"", b"[]", b"[C:12]", b"[" + UTF2 + b"]", UTF2, b"[[a*]]", b"[a*]", b"R'", b"[2, 4-Cl2C6H3]", b"[Si]", b"[CH12]", b"[U+15]",
        b"[C-16]", b"[999Og]", b"<unk>", b"[\x01\x7f\n]", b"[3,5-[CF3]2C6H3]", b"[3,5-[CF3]2C6H3x]", b"Z", b"[H]", b"[Cn]", b"[C@@H2-]"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(synth_ckpt, dev):
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=32, dtype="fp16x3")
    yield e
    e.close()


def random_molecule(rng, n_atoms, n_bonds, pool=POOL):
    syms = [pool[k] for k in rng.integers(0, len(pool), n_atoms)]
    xy = [(int(x), int(y)) for x, y in rng.integers(0, 64, (n_atoms, 2))]
    bonds = []
    for _ in range(n_bonds if n_atoms >= 2 else 0):
        i, j = sorted(int(v) for v in rng.choice(n_atoms, 2, replace=False))
        bonds.append((i, j, int(rng.integers(1, 7)), int(rng.integers(0, 7))))
    return syms, xy, bonds


def mol(symbols, bonds=(), flat=False):
    """a molecule from its symbols and bonds, the atoms on a scattered lattice or (flat) all at (0, 0)"""
    return list(symbols), [(0, 0) if flat else (3 * k % 64, 5 * k % 64) for k in range(len(symbols))], [tuple(b) for b in bonds]


def path(n, ty=1, first=0):
    return [(first + k, first + k + 1, ty, ty) for k in range(n - 1)]


def clean(a):
    """the records of a structured array as the device writes them: padding bytes as zeros"""
    z = np.zeros(len(a), a.dtype)
    for name in a.dtype.names:
        z[name] = a[name]
    return z.tobytes()


def texts(ref):
    """the strings of an oracle's result"""
    return [ref["out"][r["text0"]:r["text0"] + r["len"]].decode() for r in ref["recs"]]


def device_texts(recs, out):
    return [out[r["text0"]:r["text0"] + r["len"]].tobytes().decode() for r in recs]


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

    def head(self, sizes=None):
        """the arguments `mols, n, atoms, na, bonds, nb, text, nt` every pass over the tables begins with (behind the handle)"""
        na, nb, nt = sizes if sizes is not None else (len(self.atoms), len(self.bonds), len(self.text))
        return {"mols": _p(self.d[0]), "n": self.n, "atoms": _p(self.d[1]), "na": na, "bonds": _p(self.d[2]), "nb": nb,
                "text": _p(self.d[3]), "nt": nt}


# the caller's own input side of a writer of tables: the device, the number of molecules, the arguments by name in the header's order
Inputs = collections.namedtuple("Inputs", "dev n args")

# the arguments behind the input side, in the header's order (the handle goes first, the stream last)
TEXT_ARGS = {"mnx_smiles_pack": "recs order out out_cap totals",
             "mnx_smiles_pack_stereo": "recs order out out_cap totals",
             "mnx_smiles_pack_marks": "recs order out out_cap totals marks",
             "mnx_smiles_pack_canonical": "recs order rank sym_class out out_cap totals marks",
             "mnx_smiles_pack_symmetric": "recs order rank sym_class atom_marks out out_cap totals marks",
             "mnx_molfile_pack": "scale files out out_cap totals"}
TABLE_ARGS = {"mnx_expand_pack": "mols_out atoms_out atom_cap bonds_out bond_cap text_out text_cap origin totals",
              "mnx_normalize_pack": "mols_out atoms_out atom_cap bonds_out bond_cap text_out text_cap atom_notes totals",
              # a step limit goes in as step_cap: the harness sizes no output for a name that ends in _cap, and a limit is a capacity of steps
              "mnx_kekulize_pack": "mols_out atoms_out atom_cap bonds_out bond_cap text_out text_cap atom_notes totals step_cap",
              "mnx_formula_pack": "mols_out atoms_out atom_cap bonds_out bond_cap text_out text_cap origin totals step_cap",
              "mnx_smiles_read": "mols recs atoms atom_cap bonds bond_cap text text_cap totals",
              "mnx_graph_pack": "mols atoms atom_cap bonds bond_cap text text_cap totals"}
SIDES = ("origin", "atom_notes", "recs")

TextResult = collections.namedtuple("TextResult", "rc recs order rank sym_class atom_marks out totals error", defaults=(None,) * 8)
TablesResult = collections.namedtuple("TablesResult", "rc mols atoms bonds text side totals error", defaults=(None,) * 7)


def _call(eng, fn, dev, args, sizes, over):
    """eng.lib.<fn>(h, *args.values(), stream): each argument named in `sizes` is an output of that many bytes, FILL-filled and with
    GUARD bytes behind it; `over` replaces arguments by name (None: a null pointer). Returns rc, the handle's error text and the
    outputs on the host, guard bytes included and found untouched."""
    bufs = {k: torch.full((s + GUARD,), FILL, dtype=torch.uint8, device=dev) for k, s in sizes.items()}
    a = {"h": eng.h, **args, **{k: _p(b) for k, b in bufs.items()}, "stream": C.c_void_p(torch.cuda.current_stream().cuda_stream)}
    assert set(sizes) | set(over) <= set(a), f"{fn} has no argument {sorted((set(sizes) | set(over)) - set(a))}"
    a.update(over)
    rc = getattr(eng.lib, fn)(*a.values())
    torch.cuda.synchronize()
    error = eng.lib.mnx_last_error(a["h"]).decode(errors="replace")
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, h in host.items():
        assert np.all(h[sizes[k]:] == FILL), f"{fn}: bytes behind {k} were overwritten: {h[sizes[k]:].tolist()}"
    return rc, error, host


def call_text(fn, eng, t, out_cap, sizes=None, **over):
    """One call of a writer of text (a key of TEXT_ARGS) on the tables t, every output the entry point has FILL-filled with GUARD
    bytes behind it: a TextResult, `recs` being mnx_molfile_pack's `files`, `out` the whole arena, the fields of outputs the entry
    point does not have None. sizes: (na, nb, nt) where the tables are passed as shorter than they are, the outputs sized to match;
    over: arguments by name — None for a null pointer, a skewed pointer, another `h`, `marks`, `na`; `scale` may be an int array."""
    names = TEXT_ARGS[fn].split()
    args = {**t.head(sizes), **dict.fromkeys(names), "out_cap": out_cap}
    if "marks" in names:
        args["marks"] = 0
    if isinstance(over.get("scale"), np.ndarray):
        scale = torch.from_numpy(np.ascontiguousarray(over["scale"], dtype=np.int32)).to(t.dev)
        over["scale"] = _p(scale)
    na, rec = args["na"], "files" if "files" in names else "recs"
    size_of = {rec: t.n * 16, "order": na * 2, "rank": na * 2, "sym_class": na * 2, "atom_marks": na, "out": out_cap, "totals": 8}
    nbytes = {k: size_of[k] for k in names if k in size_of}
    rc, error, host = _call(eng, fn, t.dev, args, nbytes, over)
    dtype = {"files": MOLFILE_DTYPE, "recs": SMILES_DTYPE, "order": np.uint16, "rank": np.uint16, "sym_class": np.uint16, "totals": np.uint32}
    got = {"recs" if k == rec else k: host[k][:nbytes[k]].view(dtype.get(k, np.uint8)) for k in nbytes if k != "out"}
    return TextResult(rc, out=host["out"], error=error, **got)


def call_tables(fn, eng, t, caps, **over):
    """One call of a writer of tables (a key of TABLE_ARGS) at the capacities caps = (atoms, bonds, text bytes), every output
    FILL-filled with GUARD bytes behind its capacity: a TablesResult with `mols` as records, `atoms`, `bonds`, `text` and `side`
    (origin, atom_notes or the reader's recs; None without one) as the bytes up to the capacity, `totals` as four words. t: Tables,
    or Inputs for an entry point with an input side of its own; over: as for call_text."""
    dev, n, head = (t.dev, t.n, t.head()) if isinstance(t, Tables) else t
    names = TABLE_ARGS[fn].split()
    args = {**head, **dict.fromkeys(names), "atom_cap": caps[0], "bond_cap": caps[1], "text_cap": caps[2]}
    size_of = {"mols": n * MOL_DTYPE.itemsize, "atoms": caps[0] * ATOM_DTYPE.itemsize, "bonds": caps[1] * BOND_DTYPE.itemsize, "text": caps[2],
               "origin": caps[0] * 2, "atom_notes": caps[0], "recs": n * READ_DTYPE.itemsize, "totals": 16}
    role = {k: "side" if k in SIDES else k[:-4] if k.endswith("_out") else k for k in names if not k.endswith("_cap")}
    sizes = {k: size_of[r if r != "side" else k] for k, r in role.items()}
    rc, error, host = _call(eng, fn, dev, args, sizes, over)
    got = {r: host[k][:sizes[k]] for k, r in role.items()}
    got.update(mols=got["mols"].view(MOL_DTYPE), totals=got["totals"].view(np.uint32))
    return TablesResult(rc, error=error, **got)


def same_array(got, want, what):
    """two arrays of one shape equal, or the first five differing elements shown"""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, the first at {bad[:5].tolist()}: {got[bad[:5]].tolist()} != {want[bad[:5]].tolist()}"


def same_mols(got, want, what="mols"):
    """two arrays of records (mnx_mol, or any other structured type) field by field"""
    for name in want.dtype.names:
        same_array(got[name], want[name], f"{what}[{name!r}]")


def same_bytes(got, want, what, size=1):
    """two byte strings equal, or the first differing record of `size` bytes shown (size 1: the bytes around the difference)"""
    got, want = (x.tobytes() if isinstance(x, np.ndarray) else bytes(x) for x in (got, want))
    if got != want:
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        lo, hi = (max(k - 80, 0), k + 40) if size == 1 else (k // size * size, k // size * size + size)
        raise AssertionError(f"{what}: first difference at byte {k} (record {k // size}) of {len(got)} / {len(want)}: "
                             f"{got[lo:hi]!r} != {want[lo:hi]!r}")


def same_results(a, b):
    """two results of one call function hold the same rc and the same bytes in every output"""
    assert a.rc == b.rc, f"rc: {a.rc} != {b.rc}"
    for name, x, y in zip(a._fields[1:-1], a[1:-1], b[1:-1]):
        assert (x is None) == (y is None), f"{name}: only one of the two calls has it"
        if x is not None:
            same_bytes(x, y, name)


def compare_text(got, ref, what):
    """a TextResult at the exact capacity ref["total"] against an oracle's dict: rc 0, totals, the records field by field, the bytes
    with the first difference shown, the FILL bytes behind them, and each of order, rank, sym_class, atom_marks the oracle holds"""
    total = ref["total"]
    assert got.rc == 0, f"rc {got.rc}: {got.error}"
    assert got.totals.tolist() == [total, 0], f"totals: {got.totals.tolist()} != {[total, 0]}"
    same_mols(got.recs, ref["files" if "files" in ref else "recs"], "recs")
    same_bytes(got.out[:total], ref["out"], what)
    behind = np.nonzero(got.out[total:] != FILL)[0][:5]
    assert behind.size == 0, f"bytes behind the {what} were overwritten: {behind.tolist()} behind byte {total} hold {got.out[total:][behind].tolist()}"
    for name in ("order", "rank", "sym_class", "atom_marks"):
        if name in ref:
            assert getattr(got, name) is not None, f"the oracle holds {name}, the call has no such output"
            same_array(getattr(got, name), ref[name], name)


def compare_tables(got, ref, side_name=None):
    """a TablesResult at the exact capacities ref["totals"] against an oracle's dict: rc 0, totals, mols field by field and as bytes,
    atoms and bonds as bytes with zeros in the padding and the first differing record shown, the text, and the side output
    ref[side_name] (records field by field and as bytes, anything else element by element in the oracle's type)"""
    assert got.rc == 0, f"rc {got.rc}: {got.error}"
    assert got.totals.tolist() == list(ref["totals"]) + [0], f"totals: {got.totals.tolist()} != {list(ref['totals']) + [0]}"
    same_mols(got.mols, ref["mols"])
    same_bytes(got.mols, clean(ref["mols"]), "mols", MOL_DTYPE.itemsize)
    same_bytes(got.atoms, clean(ref["atoms"]), "atoms", ATOM_DTYPE.itemsize)
    same_bytes(got.bonds, clean(ref["bonds"]), "bonds", BOND_DTYPE.itemsize)
    same_bytes(got.text, ref["text"], "text")
    if side_name is not None:
        want = ref[side_name]
        assert got.side is not None, f"the oracle holds {side_name}, the call has no such output"
        assert got.side.size == want.nbytes, f"{side_name}: {got.side.size} bytes, not {want.nbytes}"
        if want.dtype.names:
            same_mols(got.side.view(want.dtype), want, side_name)
            same_bytes(got.side, want, side_name, want.dtype.itemsize)
        else:
            same_array(got.side.view(want.dtype), want, side_name)


def assert_refused(got, message, fills=None):
    """a refused call: rc == -1, the exact error text, and every output (or those named in `fills`) still FILL — order, rank and
    sym_class as 16-bit words of it"""
    assert got.rc == -1 and got.error == message, f"rc {got.rc} and {got.error!r}, not -1 and {message!r}"
    for name in fills or [f for f in got._fields[1:-1] if getattr(got, f) is not None]:
        x = getattr(got, name)
        ok = np.all(x == WORD_FILL) if x.dtype == np.uint16 else np.all(x.view(np.uint8) == FILL)
        assert ok, f"{name} was written by a call refused with {message!r}: {x.view(np.uint8)[:16].tolist()} ..."
