"""GPU (-m gpu): what the Python side of the packed-table layer calls, pinned where its code paths were merged — which entry
point and which `marks` word Engine.smiles_pack hands to the library for every combination of its flags, and the byte-arena
upload and the scale tensor that smiles_read, molfile_read and molfile_pack share: the refusals' texts, the scale round trip,
the arena of no bytes. Every name used here is older than the split of the binding, so the file passes before and after it."""
import itertools

import numpy as np
import pytest

import molfile_ref as R
from molnextr_amd.engine import MOLREAD_REFUSED, READ_REFUSED, SMILES_MARK_DOUBLE_BOND, SMILES_MARK_TETRAHEDRAL, SMILES_REFUSED
from packed_tables import clean, dev, eng, mol, path, same_mols  # noqa: F401

pytestmark = pytest.mark.gpu

T, D = SMILES_MARK_TETRAHEDRAL, SMILES_MARK_DOUBLE_BOND
# (stereo, double_bonds, canonical, symmetry) -> (entry point, the `marks` word or None where it takes none, values returned):
# written out from the branches of smiles_pack as they stood before they became one path
CALLS = {
    (False, False, False, False): ("mnx_smiles_pack", None, 3),
    (True, False, False, False): ("mnx_smiles_pack_stereo", None, 3),
    (False, True, False, False): ("mnx_smiles_pack_marks", D, 3),
    (True, True, False, False): ("mnx_smiles_pack_marks", D | T, 3),
    (False, False, True, False): ("mnx_smiles_pack_canonical", 0, 5),
    (True, False, True, False): ("mnx_smiles_pack_canonical", T, 5),
    (False, True, True, False): ("mnx_smiles_pack_canonical", D, 5),
    (True, True, True, False): ("mnx_smiles_pack_canonical", T | D, 5),
    (False, False, True, True): ("mnx_smiles_pack_symmetric", 0, 6),
    (True, False, True, True): ("mnx_smiles_pack_symmetric", T, 6),
    (False, True, True, True): ("mnx_smiles_pack_symmetric", D, 6),
    (True, True, True, True): ("mnx_smiles_pack_symmetric", T | D, 6),
}
# the arguments of each entry point, handle and stream included (include/molnextr_hip.h)
N_ARGS = {"mnx_smiles_pack": 15, "mnx_smiles_pack_stereo": 15, "mnx_smiles_pack_marks": 16, "mnx_smiles_pack_canonical": 18,
          "mnx_smiles_pack_symmetric": 19}


class Recording:
    """engine.lib with every call noted as (name, arguments) and forwarded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.fixture(scope="module")
def read(eng):
    rec = eng.smiles_read(["CCO", "c1ccccc1", "F/C=C/F"])
    assert not (rec["read"]["flags"] & READ_REFUSED).any() and rec["mols"]["n_atoms"].tolist() == [3, 6, 4]
    return rec


@pytest.mark.parametrize("flags", sorted(CALLS))
def test_smiles_pack_calls_the_entry_point_of_its_flags(eng, read, flags, monkeypatch):
    assert len(CALLS) == 12 and set(CALLS) == {f for f in itertools.product((False, True), repeat=4) if f[2] or not f[3]}
    stereo, double_bonds, canonical, symmetry = flags
    fn, marks, n_values = CALLS[flags]
    lib = Recording(eng.lib)
    monkeypatch.setattr(eng, "lib", lib)
    got = eng.smiles_pack(read, stereo=stereo, double_bonds=double_bonds, canonical=canonical, symmetry=symmetry)
    monkeypatch.undo()
    assert [name for name, _ in lib.calls] == [fn], lib.calls            # one call: the first capacity holds these strings
    args = lib.calls[0][1]
    assert len(args) == N_ARGS[fn]
    if marks is not None:
        assert args[-2] == marks and isinstance(args[-2], int)           # marks stands in front of the stream
    assert len(got) == n_values
    recs, order, data = got[:3]
    assert not (recs["flags"] & SMILES_REFUSED).any() and len(order) == 13 and sorted(order[:3].tolist()) == [0, 1, 2]
    for per_atom, dtype in zip(got[3:], (np.uint16, np.uint16, np.uint8)):
        assert per_atom.dtype == dtype and per_atom.shape == (13,)
    again = eng.smiles_pack(read, stereo=stereo, double_bonds=double_bonds, canonical=canonical, symmetry=symmetry)
    assert again[2] == data and np.array_equal(again[1], order) and again[0].tobytes() == recs.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(again[3:], got[3:]))


def test_symmetry_without_canonical_is_refused_before_any_call(eng, read, monkeypatch):
    lib = Recording(eng.lib)
    monkeypatch.setattr(eng, "lib", lib)
    for stereo, double_bonds in itertools.product((False, True), repeat=2):
        with pytest.raises(ValueError) as err:
            eng.smiles_pack(read, stereo=stereo, double_bonds=double_bonds, symmetry=True)
        assert str(err.value) == "smiles_pack: symmetry=True needs canonical=True"
    assert lib.calls == []


def test_the_readers_refuse_in_their_own_names(eng):
    for call, message in ((lambda: eng.smiles_read([]), "smiles_read needs at least one string"),
                          (lambda: eng.molfile_read([]), "molfile_read needs at least one file"),
                          (lambda: eng.smiles_read(iter(())), "smiles_read needs at least one string")):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == message


def test_scale_goes_to_the_writer_and_the_reader_alike(eng):
    """one molecule of three atoms and one of none: molfile_pack(scale=S), then molfile_read(scale=S) returns the bins exactly;
    fit=True with a scale is refused in molfile_read's name; a scale as a list and as an array are one tensor"""
    mols, atoms, bonds, text = R.build_tables([mol([b"C", b"C", b"O"], path(3)), mol([])])
    rec = {"mols": mols, "atoms": atoms, "bonds": bonds, "text": text}
    S = np.array([[123457, 98765], [100000, 100000]])
    files, data = eng.molfile_pack(rec, scale=S)
    assert not files["flags"].any() and files["len"].min() > 0
    texts = [data[f["text0"]:f["text0"] + f["len"]] for f in files]
    with pytest.raises(ValueError) as err:
        eng.molfile_read(texts, fit=True, scale=S)
    assert str(err.value) == "molfile_read: fit=True takes no scale"
    for scale in (S, S.tolist(), S.astype(np.int64).reshape(-1)):
        back = eng.molfile_read(texts, scale=scale)
        assert not (back["read"]["flags"] & MOLREAD_REFUSED).any()
        same_mols(back["mols"], mols)
        assert back["atoms"].tobytes() == clean(atoms) and back["bonds"].tobytes() == clean(bonds) and back["text"] == text
        assert back["atoms"]["x_bin"].tolist() == [0, 3, 6] and back["atoms"]["y_bin"].tolist() == [0, 5, 10]
    again = eng.molfile_pack(back, scale=S.tolist())
    assert again[1] == data and again[0].tobytes() == files.tobytes()
    plain_files, plain = eng.molfile_pack(rec)                           # None: 100000 each, another file for the first molecule
    first = plain[int(plain_files[0]["text0"]):int(plain_files[0]["text0"]) + int(plain_files[0]["len"])]
    assert first != texts[0] and eng.molfile_read([first])["atoms"]["x_bin"].tolist() == [0, 3, 6]


def test_an_arena_of_no_bytes_is_read(eng):
    """smiles_read(["", "C"]): the empty molecule, then one atom; and [""] alone, whose arena has no byte at all"""
    rec = eng.smiles_read(["", "C"])
    assert rec["mols"]["n_atoms"].tolist() == [0, 1] and rec["mols"]["n_bonds"].tolist() == [0, 0]
    assert not (rec["read"]["flags"] & READ_REFUSED).any() and rec["text"] == b"C" and len(rec["atoms"]) == 1
    alone = eng.smiles_read([""], keep_device=True)
    assert alone["mols"]["n_atoms"].tolist() == [0] and not (alone["read"]["flags"] & READ_REFUSED).any() and alone["text"] == b""
    recs, order, data = eng.smiles_pack(alone)
    assert recs["len"].tolist() == [0] and len(order) == 0 and data == b""
    assert eng.smiles_read([b"", "C"])["text"] == b"C"                   # bytes and str side by side
