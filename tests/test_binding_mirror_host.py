"""CPU: molnextr_amd/abi.py says what include/molnextr_hip.h says — every declaration's parameter list against its entry of
PROTOTYPES, every numeric #define against its constant, every record struct against its ctypes struct and numpy dtype (one
small C program, as tests/test_abi.py compiles the header) — and the split of the binding into abi / engine / engine_tables /
engine_lab / graphs left every old import path in place: the names of tests/golden/python_surface.json still resolve, and a
moved name is one object under both paths. Nothing here loads the library.

tests/golden/python_surface.json holds the surface of the commit before the split (7f87ae7), written there by
  git archive 7f87ae7 | tar -x -C $T && (cd $T && python -c "import json, molnextr_amd.engine as e, molnextr_amd.model as m; K = ('_ptr', '_stream', '_pipeline', '_same_graph_tables'); s = lambda o: sorted(n for n in dir(o) if not n.startswith('_') or n in K); print(json.dumps({'engine': s(e), 'model': s(m), 'Engine': sorted(dir(e.Engine))}, indent=1))") > tests/golden/python_surface.json
A lab call added since is entered by hand where it sorts ('Engine': dec_linear).
"""
import ctypes
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from molnextr_amd import abi, chain, engine, engine_lab, engine_tables, graphs, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molnextr_hip.h")


def _header():
    """the header without its comments"""
    with open(HEADER) as f:
        text = f.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


SCALARS = {"int32_t": (ctypes.c_int32, ctypes.c_int), "int": (ctypes.c_int32, ctypes.c_int), "uint32_t": (ctypes.c_uint32,),
           "int64_t": (ctypes.c_int64,), "uint64_t": (ctypes.c_uint64,), "float": (ctypes.c_float,), "double": (ctypes.c_double,),
           "size_t": (ctypes.c_size_t,)}


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _kind_matches(c_type: str, t) -> bool:
    """a C parameter or return type (names and const stripped) against a ctypes type (None: void)"""
    if c_type.endswith("*"):
        return t is not None and _is_pointer(t)
    if c_type == "void":
        return t is None
    return any(t is twin for twin in SCALARS[c_type])


def _declarations():
    """{name: (return type, [parameter types])} of every mnx_* function the header declares, types as 'uint32_t' or 'float*'"""
    code = re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\)*", "", _header(), flags=re.M)       # preprocessor lines, continued ones too
    out = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+[\s\*]+)(mnx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        def c_type(decl, named):
            words = decl.replace("*", " * ").split()
            words = [w for w in words if w != "const"]
            if named and words[-1] != "*" and len(words) > 1:
                words = words[:-1]                                                    # the parameter's name
            return "".join(words)
        plist = [p.strip() for p in params.split(",")]
        assert name not in out, f"{name} is declared twice"
        out[name] = (c_type(ret, False), [] if plist == ["void"] else [c_type(p, True) for p in plist])
    return out


def test_every_declaration_matches_its_prototype():
    decl = _declarations()
    assert set(decl) == set(abi.PROTOTYPES), sorted(set(decl) ^ set(abi.PROTOTYPES))
    assert abi.SYMBOLS == tuple(abi.PROTOTYPES) and len(decl) >= 63
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.PROTOTYPES[name]
        assert _kind_matches(ret, restype), f"{name}: the header returns {ret}, the binding {restype}"
        assert len(params) == len(argtypes), f"{name}: {len(params)} parameters in the header, {len(argtypes)} argtypes"
        for k, (p, t) in enumerate(zip(params, argtypes)):
            assert _kind_matches(p, t), f"{name}: parameter {k} is {p} in the header, {t} in the binding"
    assert abi.PROTOTYPES["mnx_abi_version"] == (ctypes.c_int, [])


def test_the_parser_tells_the_kinds_apart():
    """the comparison above can fail: a swapped pair, a missing and a widened argument are each seen"""
    assert _declarations()["mnx_cast16"] == ("int", ["mnx_engine*", "float*", "void*", "int64_t", "int64_t", "float", "void*"])
    assert _declarations()["mnx_last_error"] == ("char*", ["mnx_engine*"])
    assert not _kind_matches("int64_t", ctypes.c_int32) and not _kind_matches("uint32_t", ctypes.c_int32)
    assert not _kind_matches("float*", ctypes.c_float) and not _kind_matches("int32_t", ctypes.c_void_p)
    assert not _kind_matches("void", ctypes.c_int) and not _kind_matches("int", None)
    assert _kind_matches("mnx_config*", ctypes.POINTER(abi.MnxConfig)) and _kind_matches("char*", ctypes.c_char_p)


def test_every_numeric_define_has_its_twin():
    found = re.findall(r"^[ \t]*#define[ \t]+MNX_(\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+|\(\s*1u?\s*<<\s*\d+\s*\))[uU]?[ \t]*$", _header(), flags=re.M)
    assert len(found) >= 87, f"only {len(found)} numeric #define MNX_* lines were recognised"
    for name, literal in found:
        shift = re.fullmatch(r"\(\s*1u?\s*<<\s*(\d+)\s*\)", literal)
        value = 1 << int(shift.group(1)) if shift else int(literal, 0)
        assert hasattr(abi, name), f"MNX_{name} has no twin abi.{name}"
        assert getattr(abi, name) == value, f"abi.{name} = {getattr(abi, name)}, MNX_{name} = {value}"


# the header's struct -> (ctypes struct, numpy dtype) of abi.py, None where the binding has no use for one
RECORDS = {"mnx_mol": (abi.MnxMol, abi.MOL_DTYPE), "mnx_atom": (abi.MnxAtom, abi.ATOM_DTYPE), "mnx_bond": (abi.MnxBond, abi.BOND_DTYPE),
           "mnx_molfile": (abi.MnxMolfile, abi.MOLFILE_DTYPE), "mnx_smiles": (abi.MnxSmiles, abi.SMILES_DTYPE),
           "mnx_read": (None, abi.READ_DTYPE), "mnx_molread": (None, abi.MOLREAD_DTYPE), "mnx_fp": (None, abi.FP_DTYPE),
           "mnx_match": (None, abi.MATCH_DTYPE), "mnx_page": (abi.MnxPage, None), "mnx_config": (abi.MnxConfig, None),
           "mnx_weight_desc": (abi.MnxWeightDesc, None)}


def _struct_fields():
    """{struct: [field names]} as the header declares them, in order"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _header()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")
            fields += [re.sub(r"\[\d+\]", "", x).replace("*", " ").split()[-1] for x in [first] + rest]
        out[name] = fields
    return out


def test_every_record_struct_matches_its_dtypes(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = _struct_fields()
    assert set(RECORDS) <= set(fields), sorted(set(RECORDS) - set(fields))
    lines = [f'    printf("{s} %zu\\n", sizeof({s}));' for s in RECORDS]
    lines += [f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for s in RECORDS for f in fields[s]]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "molnextr_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    measured = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for s, (struct, dtype) in RECORDS.items():
        if struct is not None:
            assert [f[0] for f in struct._fields_] == fields[s], f"{s}: fields of {struct.__name__}"
            assert ctypes.sizeof(struct) == measured[s], f"sizeof({s}) = {measured[s]}, {struct.__name__} has {ctypes.sizeof(struct)}"
            for f in fields[s]:
                assert getattr(struct, f).offset == measured[f"{s}.{f}"], f"{s}.{f}: {struct.__name__}"
        if dtype is not None:
            assert list(dtype.names) == fields[s], f"{s}: fields of the dtype"
            assert dtype.itemsize == measured[s], f"sizeof({s}) = {measured[s]}, the dtype has {dtype.itemsize}"
            for f in fields[s]:
                assert dtype.fields[f][1] == measured[f"{s}.{f}"], f"{s}.{f}: the dtype"
        if struct is not None and dtype is not None:                                  # and the two twins say the same of each field's size
            assert [ctypes.sizeof(t) for _, t in struct._fields_] == [dtype.fields[f][0].itemsize for f in fields[s]], s


def test_the_old_import_paths_reach_the_same_objects():
    with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as f:
        surface = json.load(f)
    assert (len(surface["engine"]), len(surface["model"]), len(surface["Engine"])) == (141, 52, 103)
    for module, names in ((engine, surface["engine"]), (model, surface["model"]), (engine.Engine, surface["Engine"])):
        missing = [n for n in names if not hasattr(module, n)]
        assert not missing, f"{module.__name__} lost {missing}"
    moved = 0
    for old, key, homes in ((engine, "engine", (abi, engine_lab, engine_tables)), (model, "model", (graphs,))):
        for name, home in itertools.product(surface[key], homes):
            there = vars(home).get(name)
            # what a new home defines itself: a function or class by its __module__, anything else that is no module as data
            if there is None or isinstance(there, type(os)) or (callable(there) and there.__module__ != home.__name__):
                continue
            assert getattr(old, name) is there, f"{old.__name__}.{name} is not {home.__name__}.{name}"
            moved += 1
    assert moved > 140, moved
    assert engine.MOL_DTYPE is abi.MOL_DTYPE and engine.MnxError is abi.MnxError and engine.load_library is abi.load_library
    assert engine._ptr is abi._ptr and engine._stream is abi._stream and engine.check_beam_script is engine_lab.check_beam_script
    assert model.canonical_smiles is graphs.canonical_smiles and model._same_graph_tables is graphs._same_graph_tables
    assert model.unpack_graphs is graphs.unpack_graphs and model.page_scale is graphs.page_scale
    # Engine is one class written in three files: the bases bring no state of their own
    assert engine.Engine.__mro__[1:3] == (engine_tables.TableCalls, engine_lab.LabCalls)
    assert "__init__" not in vars(engine_tables.TableCalls) and "__init__" not in vars(engine_lab.LabCalls)
    assert engine.Engine.smiles_read is engine_tables.TableCalls.smiles_read and engine.Engine.gemm16 is engine_lab.LabCalls.gemm16


FLAGS = ("formula", "expand", "keep_main", "kekulize", "normalize")


def test_flags_to_pass_names():
    assert tuple(p.name for p in chain.PASSES) == FLAGS
    for bits in itertools.product((False, True), repeat=5):
        want = [name for name, on in zip(FLAGS, bits) if on]
        assert chain.passes_on(*bits) == want
        assert chain.passes_on(**dict(zip(FLAGS, bits))) == want
        shuffled = dict(reversed(list(zip(FLAGS, bits))))                             # a caller's keyword order does not matter
        assert chain.named_passes("tanimoto", shuffled) == want
        assert chain.named_passes("same_graph", {k: v for k, v in shuffled.items() if v}) == want
    assert chain.passes_on() == [] and chain.named_passes("x", {}) == []
    for who in ("smiles_fingerprints", "molfile_fingerprints", "smiles_substructure", "same_graph"):
        with pytest.raises(TypeError) as err:
            chain.named_passes(who, {"normalize": True, "sanitize": True, "aromatize": False})
        assert str(err.value) == f"{who}: no pass named ['aromatize', 'sanitize']"
