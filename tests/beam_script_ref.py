"""Scripted log-prob tables for the beam strategy kernels and what the strategy must make of them (CPU).

A table is fp32 [max_len, B, K, V]: row (t, b, j) is what hypothesis j of ORIGINAL image b sees at step t (the layout of
tests/golden/beam_strategy.npz and of mnx_beam_scripted). `expectation(case)` returns the table and an `Expect`: per step
the parent, id and score of every new hypothesis, the images that stay, the rows the step ran on, and the final n-best
lists. The golden cases take all of that from the arrays the reference's BeamSearch class left in the .npz; every other
case runs the table through oracle.beam.BeamStrategy, whose agreement with that class the golden test pins. Ties and -inf
follow the project's written rule on both sides: lowest flat index (a stable descending sort), stable pool.

`(lp + cum) / len` and `score * len` are single correctly rounded fp32 operations in torch and on the device, so every
number here is compared as an fp32 word.

tests/test_beam_script_host.py checks that each case reaches what it is meant to reach; tests/test_gpu_beam_script.py runs
the device against it."""
import functools
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from molnextr_amd import weights as W
from oracle.beam import BeamStrategy

EOS = 2
FILL = -7                   # what the caller fills the trace with: rows of images that did not enter a step keep it
LOW = -30.0                 # "everything else" of the hand-written tables
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_strategy.npz")
CFG_MAX_LEN = 480           # cfg.max_len of a default Engine: the longest search there is

CASES = ("golden_a", "golden_b", "golden_c", "golden_d", "ties_small", "ties_full", "ties_spread", "boundaries", "pool_quant", "pool_hand",
         "maxlen", "neg_inf")

# boundaries: image -> the flat indices (parent * V + id, K = 8, V = 229) of the tied maxima of step 1
BOUNDARY_TIES = ((0, 1), (63, 64), (255, 256), (228, 229), (1830, 1831),
                 (1 * 229 + 7, 5 * 229 + 7),            # one id under two parents
                 (63, 256, 1831))                       # a triple: the last lane of wave 0, the second candidate of thread 0, the last


@dataclass
class Expect:
    B: int
    K: int
    n_best: int
    max_len: int
    V: int
    steps_run: int = 0
    parent: np.ndarray = None        # [max_len, B, K] int32, FILL where the image did not enter the step
    token: np.ndarray = None
    score: np.ndarray = None         # [max_len, B, K] float32
    entered: np.ndarray = None       # [max_len, B] bool: the image was alive at the start of the step (scores, alive known)
    known: np.ndarray = None         # [max_len, B] bool: parents and ids known (the golden holds them for the images that stay)
    alive: np.ndarray = None         # [max_len, B] int32: 1 the image stays after the step, 0 it leaves, FILL did not enter
    n_active: np.ndarray = None      # [max_len] int32: rows of the step, FILL for the steps not run
    final_ids: List[List[List[int]]] = None      # [B][n_best] ids without <sos>, <eos> included when emitted
    final_scores: np.ndarray = None  # [B, n_best] float32
    stats: dict = field(default_factory=dict)

    def alloc(self):
        ML, B, K = self.max_len, self.B, self.K
        self.parent = np.full((ML, B, K), FILL, np.int32)
        self.token = np.full((ML, B, K), FILL, np.int32)
        self.score = np.full((ML, B, K), float(FILL), np.float32)
        self.entered = np.zeros((ML, B), bool)
        self.known = np.zeros((ML, B), bool)
        self.alive = np.full((ML, B), FILL, np.int32)
        self.n_active = np.full((ML,), FILL, np.int32)
        return self


# ---- tables ----------------------------------------------------------------------------------------------------------
def golden_table(case):
    """Exactly the table of test_oracle_golden.py::test_beam_strategy_vs_reference_class."""
    g = np.load(GOLDEN)
    B, K, NB, ML, V = g[case + "_cfg"].tolist()
    z = W.hash_normal("beam_script_" + case, (ML, B, K, V), 1.0).clone()
    z[..., 2] += float(g[case + "_boost"][0])
    return torch.log_softmax(z, dim=-1), NB


def quantised_table(seed, B, K, max_len, V):
    """-0.25 * {0, 1, 2, 3}: every cumulative sum is exact, and with four values among K x V candidates every step ties"""
    g = torch.Generator().manual_seed(seed)
    return -0.25 * torch.randint(0, 4, (max_len, B, K, V), generator=g).float()


def spread_table(seed, B, K, max_len, V, peaks=2):
    """Quantised too, but a row offers only `peaks` good ids (0, -0.25 or -0.5) among -1 .. -2.75, and <eos> is one of the
    good ones in a quarter of the rows: where the full quantised table finds its best K + 1 candidates at log-prob 0 under
    parent 0 at every step, here the parents' cumulative sums drift apart and the ties are between sums, across parents,
    and at rank K - 1 / K."""
    g = torch.Generator().manual_seed(seed)
    t = -0.25 * torch.randint(4, 12, (max_len, B, K, V), generator=g).float()
    pos = torch.randint(0, V, (max_len, B, K, peaks), generator=g)
    t.scatter_(3, pos, -0.25 * torch.randint(0, 3, (max_len, B, K, peaks), generator=g).float())
    good_eos = torch.rand(max_len, B, K, generator=g) < 0.25
    t[..., EOS] = torch.where(good_eos, -0.25 * torch.randint(0, 3, (max_len, B, K), generator=g).float(), t[..., EOS])
    return t


def boundaries_table():
    K, V, ML = 8, 229, 3
    B = len(BOUNDARY_TIES)
    t = torch.full((ML, B, K, V), LOW)
    t[0, :, 0, 3:3 + K] = 0.0               # step 0: ids 3..10 of the only finite parent tie at 0 -> K parents, all with cum 0
    for b, flats in enumerate(BOUNDARY_TIES):
        for f in flats:
            t[1, b, f // V, f % V] = 0.0    # step 1: the tied maxima; everything else ties at (LOW + 0) / 3
    t[2] = quantised_table(11, B, K, 1, V)[0]
    return t


def pool_hand_table():
    """B, K, n_best, max_len, V = 3, 3, 2, 10, 8. Scores are (lp + cum) / (t + 2).
    image 0: the top beam finishes at step 1 with nothing stored before (1 < n_best: the image stays), a rank-1 hypothesis
             finishes at step 2 -> the image leaves at step 2.
    image 2: the same start, nobody finishes at step 2, a rank-2 hypothesis finishes at step 3 -> it leaves at step 3.
    image 1: hypothesis 0 goes on with id 3 at log-prob 0 (score 0, always on top); <eos> under it finishes at rank 1 or 2
             with the scores below, so the top beam never finishes before step 7 and the pool (n_best = 2) sees
             step 1: -1     stored                                  pool [-1(1)]
             step 2: -1     equal to a kept one, goes behind it     pool [-1(1), -1(2)]
             step 3: -2     worse than a full pool: dropped
             step 4: -0.5   better: the worst, -1(2), drops out     pool [-0.5(4), -1(1)]
             step 5: -1     equal to the worst of a full pool: dropped (the earlier one stays)
             step 6: -0.5   equal to the best: behind it, -1(1) out pool [-0.5(4), -0.5(6)]
             step 7: the top beam finishes with score 0             pool [0(7), -0.5(4)], the image leaves."""
    B, K, V, ML = 3, 3, 8, 10
    t = torch.full((ML, B, K, V), LOW)
    t[0, :, 0, 3], t[0, :, 0, 4], t[0, :, 0, 5] = 0.0, -1.0, -2.0     # three hypotheses with cum 0, -1, -2
    for b in (0, 2):
        t[1, b, 0, EOS] = 0.0       # the top beam finishes: score 0
        t[1, b, 1, 3] = 0.0         # cum -1
        t[1, b, 2, 3] = 0.0         # cum -2
    t[2, 0, 1, 3], t[2, 0, 1, EOS], t[2, 0, 2, 4] = 0.0, -1.0, 0.0    # -1/4; <eos> -2/4 ties with (2, id 4) -2/4: <eos> first
    t[2, 2, 1, 3], t[2, 2, 1, 4], t[2, 2, 2, 3] = 0.0, -1.0, 0.0      # nobody finishes: cum -1, -2, -2
    t[3, 2, 0, 3], t[3, 2, 1, 3], t[3, 2, 2, EOS] = 0.0, 0.0, 0.0     # -1/5, then (1, id 3) and (2, <eos>) tie at -2/5
    fin = {1: -1.0, 2: -1.0, 3: -2.0, 4: -0.5, 5: -1.0, 6: -0.5}
    for s in range(1, 8):
        ln = float(s + 2)
        t[s, 1, 0, 3] = 0.0 if s < 7 else -1.0
        t[s, 1, 0, 4] = -3.0 * ln                   # a third hypothesis that never matters
        t[s, 1, 0, EOS] = fin[s] * ln if s < 7 else 0.0
    return t


def maxlen_table():
    z = W.hash_normal("beam_script_maxlen", (CFG_MAX_LEN, 2, 8, 229), 1.0).clone()
    z[..., EOS] -= 50.0
    return torch.log_softmax(z, dim=-1)


def neg_inf_table():
    """B, K, V, max_len = 2, 3, 4, 6: a quantised table with more than half of its entries -inf; at step 0 image 0 has ONE
    finite id besides the banned <eos> (which is finite, -1e20: it is picked second and finishes), so the third pick is an
    -inf candidate — the lowest flat index among them."""
    B, K, V, ML = 2, 3, 4, 6
    t = quantised_table(5, B, K, ML, V)
    g = torch.Generator().manual_seed(6)
    t[torch.rand(ML, B, K, V, generator=g) < 0.55] = float("-inf")
    t[0, 0, 0] = torch.tensor([float("-inf"), -1.0, -0.5, float("-inf")])
    return t


@functools.lru_cache(maxsize=None)
def table_of(case):
    """(table, n_best) of a case; built once"""
    if case.startswith("golden_"):
        return golden_table(case[-1])
    if case == "ties_small":
        return quantised_table(1, 4, 3, 12, 24), 2
    if case == "ties_full":
        return quantised_table(2, 32, 8, 8, 229), 3
    if case == "ties_spread":
        return spread_table(4, 16, 8, 12, 229), 3
    if case == "boundaries":
        return boundaries_table(), 2
    if case == "pool_quant":
        return quantised_table(3, 2, 5, 10, 8), 5
    if case == "pool_hand":
        return pool_hand_table(), 2
    if case == "maxlen":
        return maxlen_table(), 2
    if case == "neg_inf":
        return neg_inf_table(), 2
    raise KeyError(case)


# ---- expectations ----------------------------------------------------------------------------------------------------
def run_strategy(table, n_best):
    """The table through oracle.beam.BeamStrategy. Besides the expectation, `stats` holds what the host tests count:
    min_gap [image][step]; per step and image the sorted best K + 1 values / flat indices ('top'); the finished hypotheses
    in the order the strategy stored them, per image (step, rank, score) ('finished'); the step every image left at."""
    ML, B, K, V = table.shape
    ex = Expect(B, K, n_best, ML, V).alloc()
    st = BeamStrategy(B, K, n_best, ML, eos=EOS)
    seqs = [[] for _ in range(B * K)]
    top, finished, left = {}, [[] for _ in range(B)], [None] * B
    step = 0
    while not st.done:
        origin = list(st.origin)
        lp = torch.stack([table[step, b, j] for b in origin for j in range(K)])
        sel, tok, scores, fin, keep = st.advance(lp, lambda row, pt, seqs=seqs: seqs[pt[0]] + [pt[1]])
        last = st.last
        assert last["origin"] == origin
        ex.n_active[step] = len(origin) * K
        for i, b in enumerate(origin):
            ex.entered[step, b] = ex.known[step, b] = True
            ex.parent[step, b] = last["parent"][i].numpy()
            ex.token[step, b] = last["tokens"][i].numpy()
            ex.score[step, b] = last["scores"][i].numpy()
            ex.alive[step, b] = int(i in keep)
            top[(step, b)] = (last["top_values"][i].numpy().copy(), last["top_index"][i].numpy().copy())
            for j in range(K):
                if bool(fin[i, j]):
                    finished[b].append((step, j, float(scores[i, j])))
            if i not in keep:
                left[b] = step
        seqs = [seqs[p] + [t] for p, t in zip(sel.tolist(), tok.tolist())]
        step += 1
    ex.steps_run = step
    ex.final_ids = [[list(st.results[b][r][1]) for r in range(n_best)] for b in range(B)]
    ex.final_scores = np.array([[st.results[b][r][0] for r in range(n_best)] for b in range(B)], np.float32)
    for b in range(B):      # the strategy keeps every finished hypothesis: the stored ones are the finished ones, in order
        assert [s for _, _, s in finished[b]] == [h[0] for h in st.hyps[b]]
    ex.stats = {"min_gap": st.min_gap, "top": top, "finished": finished, "left": left}
    return ex


def golden_expectation(case):
    """From the arrays of the .npz alone. The golden keeps back-pointers and ids only of the images that stay after a step
    (`known`); scores it keeps for every image that entered it."""
    g = np.load(GOLDEN)
    B, K, NB, ML, V = g[case + "_cfg"].tolist()
    ex = Expect(B, K, NB, ML, V).alloc()
    origin = list(range(B))
    nsteps = int(g[case + "_nsteps"][0])
    for s in range(nsteps):
        sc = np.asarray(g[f"{case}_score{s}"], np.float32).reshape(len(origin), K)
        after = g[f"{case}_origin{s}"].tolist()
        sel = g[f"{case}_sel{s}"].reshape(len(after), K)
        tok = g[f"{case}_tok{s}"].reshape(len(after), K)
        ex.n_active[s] = len(origin) * K
        for i, b in enumerate(origin):
            ex.entered[s, b] = True
            ex.score[s, b] = sc[i]
            ex.alive[s, b] = int(b in after)
        for i, b in enumerate(after):
            assert (sel[i] // K == origin.index(b)).all()       # back-pointers stay inside the image
            ex.known[s, b] = True
            ex.parent[s, b] = sel[i] % K
            ex.token[s, b] = tok[i]
        origin = after
    assert not origin
    ex.steps_run = nsteps
    ex.final_ids = [[g[f"{case}_pred{b}_{r}"].tolist() for r in range(NB)] for b in range(B)]
    ex.final_scores = np.array([[float(g[f"{case}_final{b}_{r}"][0]) for r in range(NB)] for b in range(B)], np.float32)
    return ex


def coverage(case):
    """What a strategy-driven case reaches, as counts (tests/test_beam_script_host.py asserts them):
    image_steps / tied_steps (min_gap == 0); in_out_ties: steps where rank K - 1 and rank K tie (the tie decides who is in);
    cross_parent_ties: steps where two of the best K + 1 candidates tie under different parents; leave_steps: the distinct
    steps images leave at; short_of_k: steps with fewer than K finite candidates; moved_steps: steps with a hypothesis
    whose parent is not its own row; finish_steps: the distinct steps hypotheses finish at; and the pool's events
    equal_insert, displaced, dropped, top_short (the top beam has finished, fewer than n_best are stored, the image stays
    and leaves later), leaves_while_other_stays."""
    _, ex = expectation(case)
    s, K, V, NB = ex.stats, ex.K, ex.V, ex.n_best
    c = {"image_steps": 0, "tied_steps": 0, "in_out_ties": 0, "cross_parent_ties": 0, "short_of_k": 0,
         "equal_insert": 0, "displaced": 0, "dropped": 0, "top_short": 0, "leaves_while_other_stays": 0}
    for gaps in s["min_gap"]:
        c["image_steps"] += len(gaps)
        c["tied_steps"] += sum(1 for g in gaps if g == 0.0)
    for (step, b), (v, i) in s["top"].items():
        c["in_out_ties"] += int(v[K - 1] == v[K])
        c["cross_parent_ties"] += int(any(v[a] == v[e] and i[a] // V != i[e] // V for a in range(K + 1) for e in range(a)))
        c["short_of_k"] += int(np.isfinite(v[:K]).sum() < K)
    c["leave_steps"] = sorted(set(s["left"]))
    c["moved_steps"] = sum(1 for t in range(ex.steps_run)
                           if any((ex.parent[t, b] != np.arange(K)).any() for b in range(ex.B) if ex.entered[t, b]))
    c["finish_steps"] = sorted({f[0] for fin in s["finished"] for f in fin})
    for b, fin in enumerate(s["finished"]):
        stored, top_done, short_seen = [], False, False     # the pool as the strategy keeps it: everything, sorted at the end
        for t in range(ex.steps_run):
            for (step, rank, sc) in fin:
                if step != t:
                    continue
                kept = sorted(stored, reverse=True)[:NB]
                pos = sum(1 for x in stored if x >= sc)         # stable: behind everything not worse
                if pos < NB and sc in kept:
                    c["equal_insert"] += 1
                if len(kept) == NB and pos < NB and sc > kept[-1]:
                    c["displaced"] += 1
                if len(kept) == NB and pos >= NB:
                    c["dropped"] += 1
                top_done = top_done or rank == 0
                stored.append(sc)
            if top_done and len(stored) < NB and ex.alive[t, b] == 1 and s["left"][b] > t and not short_seen:
                c["top_short"] += 1             # once per image
                short_seen = True
    for t in range(ex.steps_run):
        c["leaves_while_other_stays"] += int((ex.alive[t] == 0).any() and (ex.alive[t] == 1).any())
    return c


@functools.lru_cache(maxsize=None)
def expectation(case):
    """(table, Expect) of a case; computed once and shared — callers do not modify either"""
    table, n_best = table_of(case)
    if case.startswith("golden_"):
        return table, golden_expectation(case[-1])
    return table, run_strategy(table, n_best)
