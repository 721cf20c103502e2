"""The passes that take packed molecule tables to packed molecule tables, in the one order they run in (the rule:
include/molnextr_hip.h — formula in front of expand, keep_main behind it, kekulize in front of normalize), and the one function
that runs them, with the two that turn a caller's options into its `on` list (passes_on: the five keyword flags; named_passes:
**passes, with the TypeError for a name that is no pass). predict_pipeline (model.py), canonical_smiles and the other
caller-facing table functions (graphs.py), the facade and evaluate's --graph_match read the order, the keys and the error
clauses here; a new pass is one row here, one method of engine_tables.TableCalls, its prototype and flags in abi.py and one
paragraph in the docstrings. What reads the last record without writing tables again — the molfile and
SMILES writers, the path fingerprint (Engine.fingerprint_pack) — is a sink, not a row: it runs behind run_chain's last record,
which keep_last keeps on the device for it."""
import collections

# name: the option's name everywhere (graph_<name> on the facade); method: the Engine method; key: where a prediction dict
# holds the stage; flags_key: where canonical_smiles' items hold its mols['flags'] (None: not reported); side: the per-atom
# output — 'origin' for a pass that adds or drops atoms, 'atom_notes' for one that respells them; packed_why ends
# "<name>=True needs packed=True: ", written goes into "graph_<name>=True needs graph_smiles=True or graph_molfile=True: ..."
Pass = collections.namedtuple("Pass", "name method key flags_key side packed_why written")

PASSES = (
    Pass("formula", "formula_pack", "formula", "formula_flags", "origin",
         "the labels are replaced in the packed tables", "the molecule with its formulas replaced"),
    Pass("expand", "expand_pack", "expanded", None, "origin",
         "the labels are replaced in the packed tables", "the expanded molecule"),
    Pass("keep_main", "main_pack", "main", "main_flags", "origin",
         "the atoms are dropped from the packed tables", "the main molecule"),
    Pass("kekulize", "kekulize_pack", "kekulized", "kekulize_flags", "atom_notes",
         "the aromatic systems are rewritten in the packed tables", "the kekulised molecule"),
    Pass("normalize", "normalize_pack", "normalized", "normalize_flags", "atom_notes",
         "the atoms are respelled in the packed tables", "the normalised molecule"),
)
BY_NAME = {p.name: p for p in PASSES}


def run_chain(engine, rec, on, keep_last: bool):
    """The passes named in `on` (any collection of Pass.name), in the order of PASSES, each on the record the one before it
    returned, the first on rec: ({name: the record that pass returned}, the last record — rec itself when none ran). A stage
    keeps its device tables exactly when something reads them there: a later stage, or, behind the last one, a writer
    (keep_last). Whoever made rec applies the same rule to it: keep_device = keep_last or bool(on)."""
    todo = [p for p in PASSES if p.name in on]
    stages = {}
    for k, p in enumerate(todo):
        rec = stages[p.name] = getattr(engine, p.method)(rec, keep_device=bool(keep_last) or k + 1 < len(todo))
    return stages, rec


def passes_on(formula=False, expand=False, keep_main=False, kekulize=False, normalize=False):
    """The five keyword flags of predict_pipeline, canonical_smiles and canonical_molfiles -> the names that are on, in the
    order of PASSES: run_chain's `on`."""
    given = {"formula": formula, "expand": expand, "keep_main": keep_main, "kekulize": kekulize, "normalize": normalize}
    return [p.name for p in PASSES if given[p.name]]


def named_passes(who: str, passes: dict):
    """A caller's **passes (smiles_fingerprints, molfile_fingerprints, smiles_substructure, same_graph) -> the names that are
    on, in the order of PASSES; TypeError in the name of `who` for a key that is no pass."""
    unknown = set(passes) - set(BY_NAME)
    if unknown:
        raise TypeError(f"{who}: no pass named {sorted(unknown)}")
    return passes_on(**passes)
