"""Public predict API: `get_predictions`, `MolNexTRSingleton` (mirrors reference MolNexTR/molnextr.py:42-309).

Same names, arguments and result keys. Differences, on purpose:
  * the model runs on an MI355X through libmolnextr_hip.so only — there is no MPS / CPU detection and NO CPU
    fallback on error (reference molnextr.py:179-189,256-268): errors propagate;
  * the checkpoint is taken from $MOLNEXTR_CHECKPOINT (reference `.pth` or our `.safetensors`); the reference downloads
    molnextr_best.pth at run time (molnextr.py:129-143), which is impossible offline. Without the variable the call
    raises — MOLNEXTR_CHECKPOINT=synthetic opts into the deterministic hash-generated weights (tests only);
  * `bond_sets` IS returned with atoms_bonds=True (the reference computes it but drops it).
"""
import logging
import os

import torch

logger = logging.getLogger("molnextr")
logger.setLevel(os.environ.get("MOLNEXTR_DEBUG", "INFO").upper() if os.environ.get("MOLNEXTR_DEBUG") else logging.INFO)


class MolNexTRSingleton:
    _instance = None
    _device = None
    _device_name = None

    @classmethod
    def get_instance(cls):
        """Get or create the singleton model instance."""
        if cls._instance is None:
            cls._detect_hardware()
            from .model import molnextr
            path = os.environ.get("MOLNEXTR_CHECKPOINT")
            if not path:
                raise RuntimeError("set MOLNEXTR_CHECKPOINT to a MolNexTR checkpoint (reference .pth or .safetensors); "
                                   "MOLNEXTR_CHECKPOINT=synthetic selects the deterministic test weights")
            logger.info("Initializing MolNexTR (%s) on %s", path, cls._device_name)
            cls._instance = molnextr(path, cls._device)
        return cls._instance

    @classmethod
    def get_device(cls):
        if cls._device is None:
            cls._detect_hardware()
        return cls._device, cls._device_name

    @classmethod
    def _detect_hardware(cls):
        if not torch.cuda.is_available():
            raise RuntimeError("molnextr_amd needs an AMD Instinct MI355X (no CPU path in this engine)")
        cls._device = torch.device("cuda", torch.cuda.current_device())
        cls._device_name = f"ROCm GPU: {torch.cuda.get_device_name(cls._device)}"


def canonical_smiles(smiles_list, expand: bool = False, normalize: bool = False, kekulize: bool = False, keep_main: bool = False):
    """The caller's own SMILES in the canonical form the device writes (no reference counterpart; model.canonical_smiles): per
    item {'smiles' (None where refused), 'read_flags', 'err_pos', 'smiles_flags'}. Not a toolkit's canonical SMILES.
    keep_main: only the largest connected component is written (the reference's _keep_main_molecule)."""
    return MolNexTRSingleton.get_instance().canonical_smiles(smiles_list, expand=expand, normalize=normalize, kekulize=kekulize,
                                                             **({"keep_main": True} if keep_main else {}))


def canonical_molfiles(molfiles, **options):
    """The caller's own V2000 molfiles (model.split_sdf cuts an SDF) in the canonical form the device writes (no reference
    counterpart; model.canonical_molfiles, whose options these are — stereo=True and double_bonds=True write the marks that the
    files' wedges and coordinates resolve): per item {'smiles' (None where refused), 'read_flags', 'err_line', 'smiles_flags'}.
    This library's own reading of a molfile, not a toolkit's."""
    return MolNexTRSingleton.get_instance().canonical_molfiles(molfiles, **options)


def tanimoto(smiles_a, smiles_b, **passes):
    """The similarity of two lists of SMILES, item by item, as a list of floats (no reference counterpart; model.tanimoto): the
    Tanimoto similarity of this library's own path fingerprints, NOT RDKit's. passes: canonical_smiles' pass options; kekulize=True
    and normalize=True make aromatic and Kekule spellings agree. A refused or limited side scores 0.0."""
    return MolNexTRSingleton.get_instance().tanimoto(smiles_a, smiles_b, **passes)


def nearest(smiles_list, library_smiles, k: int = 1, **passes):
    """Per string of smiles_list the k strings of library_smiles nearest to it, as a list of {'index', 'smiles', 'similarity'} (no
    reference counterpart; model.nearest_smiles): by the Tanimoto similarity of this library's own path fingerprints, NOT RDKit's;
    k <= 64. passes: canonical_smiles' pass options; kekulize=True and normalize=True make aromatic and Kekule spellings agree. A
    string that was not read or has no fingerprint gets []."""
    return MolNexTRSingleton.get_instance().nearest(smiles_list, library_smiles, k=k, **passes)


def has_substructure(smiles_list, query, **passes):
    """Per string of smiles_list whether it holds the query SMILES as a substructure: True, False, or None where a string was not
    read or the search gave no answer (no reference counterpart; model.smiles_substructure). passes: canonical_smiles' pass options;
    kekulize=True and normalize=True make aromatic and Kekule spellings agree. This library's own rule, NOT RDKit's
    HasSubstructMatch and not SMARTS: H counts and stereo are not compared."""
    return MolNexTRSingleton.get_instance().has_substructure(smiles_list, query, **passes)


def get_predictions(imagepath: str, atoms_bonds: bool = False, smiles: bool = True, predicted_molfile: bool = False):
    """Predictions for one chemical-structure image (reference molnextr.py:214-309)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    model = MolNexTRSingleton.get_instance()
    start.record()
    predictions = model.predict_final_results(imagepath, return_atoms_bonds=atoms_bonds)
    result = {}
    if smiles:
        result["predicted_smiles"] = predictions["predicted_smiles"]
    if atoms_bonds:
        result["atom_sets"] = predictions["atom_sets"]
        result["bond_sets"] = predictions["bond_sets"]
    if predicted_molfile:
        result["predicted_molfile"] = predictions["predicted_molfile"]
    result["device_info"] = MolNexTRSingleton.get_device()[1]
    end.record()
    torch.cuda.synchronize()
    result["prediction_time_seconds"] = start.elapsed_time(end) / 1000.0
    if not (smiles or atoms_bonds or predicted_molfile):
        return predictions
    return result
