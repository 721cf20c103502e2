"""Writes tests/golden/formula_reference.json: what the reference's condensed-formula search gives for the labels of
tests/golden/formula_corpus.json, as data. Runs in the build container only — it needs the reference's source tree:
    python tools/gen_formula_golden.py /path/to/reference
The reference's abbrs.py and chemical.py are loaded by file with stub toolkit modules (the three functions used here —
_parse_formula, _expand_carbon, _condensed_formula_list_to_smiles — call no toolkit). Per label and per number of start bonds (1, 2,
3) the fixture holds the reference's tokens, whether it succeeded, the bonds it left, its trials, its raw string, and that string
turned into data: the element list in string order and the bond list (a, b, order), with the empty '()' that a token without
atoms leaves removed; both null where the string holds anything but bracket atoms, parentheses and bond symbols (the SMILES of an
abbreviation). The fixture holds data only. tests/test_formula_host.py says which of its cases are a gate and why the others are
a record."""
import importlib.util
import json
import os
import re
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = re.compile(r"\[([A-Za-z0-9]+)\]|([()=#.])")


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(name)

    def __call__(self, *a, **k):
        return None


def load_reference(tree):
    for name in ("rdkit", "rdkit.Chem", "SmilesPE", "SmilesPE.pretokenizer", "MolNexTR"):
        sys.modules[name] = _Stub(name)
    mods = {}
    for name in ("abbrs", "chemical"):
        spec = importlib.util.spec_from_file_location("MolNexTR." + name, os.path.join(tree, "MolNexTR", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["MolNexTR." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["abbrs"], mods["chemical"]


def as_data(raw):
    """(elements, bonds [(a, b, order)]) of a string of bracket atoms, parentheses and bond symbols; (None, None) otherwise"""
    while "()" in raw:
        raw = raw.replace("()", "")
    pieces, at = [], 0
    for m in PIECE.finditer(raw):
        if m.start() != at:
            return None, None
        pieces.append(m.group(1) or m.group(2))
        at = m.end()
    if at != len(raw):
        return None, None
    elements, bonds, prev, stack, order = [], [], None, [], 1
    for p, is_atom in ((m, len(m) > 1 or m.isalnum()) for m in pieces):
        if is_atom:
            elements.append(p)
            if prev is not None and order:
                bonds.append((prev, len(elements) - 1, order))
            prev, order = len(elements) - 1, 1
        elif p == "(":
            stack.append(prev)
        elif p == ")":
            if not stack:
                return None, None
            prev = stack.pop()
        else:
            order = {"=": 2, "#": 3, ".": 0}[p]
    return elements, bonds


def main(tree):
    abbrs, chemical = load_reference(tree)
    with open(os.path.join(ROOT, "tests", "golden", "formula_corpus.json")) as f:
        labels = json.load(f)["labels"]
    cases = []
    for label in labels:
        tokens = abbrs.FORMULA_REGEX.findall(label)
        for start in (1, 2, 3):
            case = {"label": label, "start": start, "tokens": tokens, "success": False, "bonds_left": None, "trials": None,
                    "raw": None, "elements": None, "bonds": None}
            try:
                flat = chemical._expand_carbon(chemical._parse_formula(label))
                raw, left, trials, success = chemical._condensed_formula_list_to_smiles(flat, start, None)
                case.update(success=bool(success), bonds_left=left, trials=trials, raw=raw)
                if success:
                    case["elements"], case["bonds"] = as_data(raw)
            except Exception as e:      # the reference fails on a label: a record of that
                case["raw"] = None
                case["error"] = type(e).__name__
            cases.append(case)
    out = os.path.join(ROOT, "tests", "golden", "formula_reference.json")
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=0)
    print(f"{len(cases)} cases of {len(labels)} labels -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
