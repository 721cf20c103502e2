"""GPU (-m gpu): evaluate's --graph_match on the synthetic checkpoint — predictions and a gold column compared as this library's
canonical SMILES on the device. Gold is the device's own canonical string of every prediction, written again under another atom
numbering by the host writer (so the bytes differ and only the graph is the same): the score must be 1.0; one gold string
altered: (n - 1) / n; one made unreadable: gold_unreadable = 1. Without the flag nothing changes."""
import numpy as np
import pytest
import torch

import molfile_ref as M
import smiles_read_ref as R
import smiles_ref as S
import stereo_ref as T
from molnextr_amd import evaluate as E
from molnextr_amd import weights as W
from molnextr_amd.engine import SMILES_REFUSED, Engine
from molnextr_amd.model import canonical_smiles
from molnextr_amd.shard import MAX_LEN

pytestmark = pytest.mark.gpu
PAGES, N = 30, 6            # pages decoded; predictions the test scores (the first N that the canonical writer accepts)


def page(i):
    return W.synthetic_page(i % 15)


@pytest.fixture(scope="module")
def eng(synth_ckpt):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    e = Engine(synth_ckpt["encoder"], synth_ckpt["decoder"], device=0, max_batch=8, dtype="fp16x3")
    yield e
    e.close()


def own_strings(eng, records):
    """the canonical strings (marks 0) of the gathered records, None where the writer refuses"""
    n, kmax = len(records), eng.max_atoms
    r = torch.from_numpy(records).to(torch.device("cuda", 0))
    edges = r[:, 2 + MAX_LEN + kmax:].contiguous().view(torch.uint8)[:, :kmax * kmax].reshape(n, kmax, kmax).contiguous()
    pack = eng.graph_pack({"lengths": r[:, 0].contiguous(), "n_atoms": r[:, 1].contiguous(), "tokens": r[:, 2:2 + MAX_LEN].contiguous(),
                           "atom_idx": r[:, 2 + MAX_LEN:2 + MAX_LEN + kmax].contiguous(), "edges": edges})
    recs, _, data, _, _ = eng.smiles_pack(pack, canonical=True)
    return [None if int(x["flags"]) & SMILES_REFUSED else data[int(x["text0"]):int(x["text0"]) + int(x["len"])] for x in recs]


@pytest.fixture(scope="module")
def job(eng):
    """PAGES pages through run_inference as main() calls it under --graph_match. The synthetic checkpoint predicts near-complete
    graphs, most of which the SMILES writers refuse (more than 999 bonds or 99 ring numbers): the records of the first N
    predictions that get a canonical string are what the scores are tested on, the refused ones are counted below."""
    kept = {}
    preds = E.run_inference(eng, page, PAGES, batch_size=2, keep_records=kept)
    assert E.run_inference(eng, page, 4, batch_size=2) == {i: preds[i] for i in range(4)}      # keeping the records changes no prediction
    records = kept["records"]
    assert records.shape[0] == PAGES
    own = own_strings(eng, records)
    written = [b for b, t in enumerate(own) if t]
    assert len(written) >= N, (len(written), PAGES)
    return preds, records, own, written[:N]


def renumbered(text: bytes, rng) -> str:
    """the same graph as another string: read on the host, atoms permuted, written by the plain host writer"""
    atoms, bonds, flags, n_rings = R.read(text)
    mol = ([text[p:p + ln] for p, ln in atoms], [(0, 0)] * len(atoms), [(i, j, ty, ty) for i, j, ty in bonds])
    perm = [int(p) for p in rng.permutation(len(atoms))]
    symbols, _, moved = T.renumber(mol, perm, rng)
    out = S.smiles(symbols, moved, M.name_tables())[0]
    assert out is not None
    return out


def test_graph_match_scores(eng, job):
    preds, records, own, picked = job
    rng = np.random.default_rng(3)
    gold = [renumbered(own[b], rng) for b in picked]
    assert sum(g.encode() != own[b] for g, b in zip(gold, picked)) >= N // 2       # other bytes, the same graphs
    rows = records[picked]
    got = E.graph_match_scores(eng, rows, gold, chunk=4)                           # two chunks
    assert got == {"graph_match_device": 1.0, "gold_unreadable": 0, "pred_refused": 0}, got
    altered = list(gold)
    altered[2] = altered[2] + "F"                                                  # one more atom
    assert E.graph_match_scores(eng, rows, altered) == {"graph_match_device": (N - 1) / N, "gold_unreadable": 0, "pred_refused": 0}
    broken = list(gold)
    broken[4] = broken[4] + "("
    assert E.graph_match_scores(eng, rows, broken) == {"graph_match_device": (N - 1) / N, "gold_unreadable": 1, "pred_refused": 0}
    # every page: a refused prediction is a mismatch whatever the gold says
    everything = E.graph_match_scores(eng, records, [(t or b"C").decode() for t in own], chunk=16)
    refused = sum(t is None for t in own)
    assert everything == {"graph_match_device": (PAGES - refused) / PAGES, "gold_unreadable": 0, "pred_refused": refused} and refused > 0
    # model.canonical_smiles, what a caller without the harness uses
    theirs = canonical_smiles(eng, gold + ["C(", "[Ph]C"])
    assert [t["smiles"] for t in theirs[:N]] == [own[b].decode() for b in picked]
    assert theirs[N] == {"smiles": None, "read_flags": 1, "err_pos": 1, "smiles_flags": 0}
    assert canonical_smiles(eng, ["[Ph]C"], expand=True)[0]["smiles"] == canonical_smiles(eng, ["Cc1ccccc1"])[0]["smiles"] != theirs[N + 1]["smiles"]


def test_without_the_flag_the_scores_are_the_parents(job):
    preds = job[0]
    table = E.predictions_table([f"id{i}" for i in range(PAGES)], preds)
    scores = E.smiles_scores(table["SMILES"][:3] + ["no SMILES"] * (PAGES - 3), table["SMILES"])
    assert scores == {"raw_string_match": 3 / PAGES}                                   # RDKit is absent: one key, as before
    ap = E.build_parser()
    assert ap.parse_args(["--test_file", "x.csv", "--load_path", "synthetic"]).graph_match is False
