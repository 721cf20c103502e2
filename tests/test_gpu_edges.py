"""GPU (-m gpu): the bond head by itself — edge_gather_kernel, the 512-column sgemm_tn_kernel launch, edge_pair_kernel and
edge_sym_kernel through mnx_edges and the test aid mnx_edge_probs (mnx_edges plus a copy of the seven class probabilities
the pair kernel leaves on the device). The float64 reference, the inputs, the crafted checkpoints and the derivation of the
tolerance are in tests/edges_ref.py; tests/test_edges_host.py shows on the CPU that the tolerance leaves an honest fp32
evaluation a factor of two, that it catches each named wrong variant tenfold, and that the inputs cover what they claim.

Three comparisons per case:
  1. the probabilities against probs64: every class of every pair i, j < k within the derived tolerance;
  2. edges and scores against symmetrise_exact of the DEVICE'S OWN probabilities: every pair, classes exact, scores as 64-bit
     words — no tolerance, no exclusions (every step of get_edge_prediction is one IEEE double operation);
  3. end to end: edges against the float64 winner of probs64 + symmetrise on every pair whose float64 margin exceeds twice
     the tolerance; the share left out is at most 1 % (random cases; on the crafted ones the margin is zero by design and
     the tie rule is asserted in its place).
Every output lies between two 64-element guards and is filled with 0x7F bytes before the call: guards, the rows and columns
at and beyond n_atoms[b], and everything after a refused call are compared with that fill byte for byte.
Each case prints its largest error / tolerance ratio ("ratio edges_prob <value>": pytest -s shows them;
profiles/edges_tolerances.json records a run). Measured on an MI355X: 0.33 at most on the random cases, 0.41 on the
crafted equal-class checkpoint (whose logits start at a bias of 5).
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import edges_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    """engine(ckpt kind, max_atoms): tiny encoder dims, made on first use — the bond head uses nothing of the encoder"""
    from molnextr_amd.engine import Engine
    made = {}

    def get(kind="synthetic", max_atoms=160):
        if (kind, max_atoms) not in made:
            ck = R.checkpoint(kind)
            made[kind, max_atoms] = Engine(ck["encoder"], ck["decoder"], max_batch=2, enc=R.TINY, dec=R.DEC, dec_slots=64,
                                           max_atoms=max_atoms)
        return made[kind, max_atoms]
    yield get
    for e in made.values():
        e.close()
    print("edges ratios " + json.dumps({k: round(v, 4) for k, v in sorted(RATIOS.items())}))


class Guarded:
    """n elements of dtype td on the device between two guards of 64 elements, every byte 0x7F before the call"""

    def __init__(self, shape, td, dev):
        n = int(np.prod(shape))
        self.size = torch.empty((), dtype=td).element_size()
        self.raw = torch.full(((n + 2 * GUARD) * self.size,), 0x7F, dtype=torch.uint8, device=dev)
        self.t = self.raw[GUARD * self.size:(GUARD + n) * self.size].view(td).view(*shape)
        self._bytes = None

    def guards_intact(self):
        g = GUARD * self.size
        return bool((self.raw[:g] == 0x7F).all()) and bool((self.raw[-g:] == 0x7F).all())

    def all_fill(self):
        return bool((self.raw == 0x7F).all())

    def bytes(self):
        """the payload as numpy uint8 [..., element size] (fetched once: call it after the last launch into the buffer)"""
        if self._bytes is None:
            self._bytes = self.t.contiguous().view(torch.uint8).cpu().numpy().reshape(*self.t.shape, self.size)
        return self._bytes


class Out:
    def __init__(self, B, kmax, dev, scores=True):
        self.edges = Guarded((B, kmax, kmax), torch.uint8, dev)
        self.scores = Guarded((B, kmax, kmax), torch.float64, dev) if scores else None
        self.probs = Guarded((B, kmax, kmax, 8), torch.float32, dev)

    def buffers(self):
        return [g for g in (self.edges, self.scores, self.probs) if g is not None]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def launch(e, c, dev, n_atoms=None, aid=True, scores=True):
    """one call of mnx_edge_probs (aid) or mnx_edges on case c -> Out, synchronised"""
    out = Out(c.B, c.kmax, dev, scores)
    hidden = c.hidden.to(dev)
    ai = c.idx.to(dev)
    na = torch.tensor(c.ks if n_atoms is None else n_atoms, dtype=torch.int32, device=dev)
    args = [e.h, _p(hidden), _p(ai), _p(na), c.B, c.kmax, c.max_len, _p(out.edges.t), _p(out.scores.t) if scores else None]
    rc = e.lib.mnx_edge_probs(*args, _p(out.probs.t), None) if aid else e.lib.mnx_edges(*args, None)
    assert rc == 0, e.lib.mnx_last_error(e.h)
    torch.cuda.synchronize()
    return out


def _words(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def check_case(e, c, dev):
    """the three comparisons, the guards and the untouched remainder; -> Out"""
    ref = R.reference(c.name)
    out = launch(e, c, dev)
    edges, scores, probs = out.edges.t.cpu().numpy(), out.scores.t.cpu().numpy(), out.probs.t.cpu().numpy()
    worst, pairs, excluded = 0.0, 0, 0
    for b, k in enumerate(c.ks):
        p = probs[b, :k, :k, :7]
        if k:                                                                   # 1. probabilities against float64
            ratio = np.abs(p.astype(np.float64) - ref.p64[b]) / ref.tol[b]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (c.name, b, k, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        cls, sc = R.symmetrise_exact(p)                                         # 2. the symmetrisation, exactly
        assert np.array_equal(edges[b, :k, :k], cls), (c.name, b, k, int((edges[b, :k, :k] != cls).sum()))
        assert np.array_equal(_words(scores[b, :k, :k]), _words(sc)), (c.name, b, k)
        if c.random:                                                            # 3. end to end, where float64 decides
            dec = ref.decided(b)
            pairs, excluded = pairs + dec.size, excluded + int((~dec).sum())
            assert np.array_equal(edges[b, :k, :k][dec], ref.cls[b][dec]), (c.name, b, k)
        rest = np.ones((c.kmax, c.kmax), dtype=bool)
        rest[:k, :k] = False
        assert (edges[b][rest] == 0x7F).all() and (out.scores.bytes()[b][rest] == 0x7F).all(), (c.name, b, k)
    assert excluded <= 0.01 * pairs, (c.name, excluded, pairs)
    assert all(g.guards_intact() for g in out.buffers()), c.name
    RATIOS[c.name] = max(RATIOS.get(c.name, 0.0), worst)
    print(f"ratio edges_prob {worst:.4f}   ({c.name}: {pairs} pairs, {excluded} left out of the end-to-end comparison)")
    return out


def same_molecule(a, ba, b, bb, k):
    """edges, score words and probability words of molecule ba of Out a and molecule bb of Out b, over the pairs i, j < k"""
    return all(np.array_equal(x.bytes()[ba, :k, :k], y.bytes()[bb, :k, :k])
               for x, y in ((a.edges, b.edges), (a.scores, b.scores))) and \
        np.array_equal(a.probs.bytes()[ba, :k, :k, :7], b.probs.bytes()[bb, :k, :k, :7])


@pytest.mark.parametrize("name", [n for n in R.RANDOM_CASES if n != "b32"])
def test_bond_head_against_float64_and_exact_symmetrisation(engines, dev, name):
    check_case(engines(), R.case(name), dev)


def test_batch_of_32_equals_every_molecule_alone_bit_for_bit(engines, dev):
    """B = 32 (the call's limit), ragged, max_len 96: the SGEMM's per-row K order does not depend on M and the pair kernel
    works per (b, i), so every molecule's classes, score words and probability words are those of the B = 1 call"""
    e, c = engines(), R.case("b32")
    assert c.B == 32 and {0, 1, 160} <= set(c.ks)
    out = check_case(e, c, dev)
    for b, k in enumerate(c.ks):
        one = launch(e, c.single(b), dev)
        assert same_molecule(out, b, one, 0, k), (b, k)


def test_max_atoms_256_engine(engines, dev):
    """cfg.max_atoms = 256: the pair kernel's j loop uses all 256 lanes, the symmetrisation 4 blocks per row; and a kmax = 160
    call on this engine gives the words of the 160-engine"""
    big = engines("synthetic", 256)
    check_case(big, R.case("m256"), dev)
    c = R.case("k160")
    assert same_molecule(launch(big, c, dev), 0, launch(engines(), c, dev), 0, 160)


def test_positions_out_of_range_are_read_as_clamped(engines, dev):
    e, c = engines(), R.case("clamp")
    assert int(c.idx.min()) < 0 and int(c.idx.max()) >= c.max_len
    out = check_case(e, c, dev)                                  # the reference clamps on the host
    ref = launch(e, R.clamped(c), dev)
    for b, k in enumerate(c.ks):
        assert same_molecule(out, b, ref, b, k), b


def test_n_atoms_out_of_range_is_read_as_clamped(engines, dev):
    """n_atoms = kmax + 5 on the LAST molecule (whose overrun would leave the buffers) and -1: the bytes of n_atoms = kmax and 0"""
    e, c = engines(), R.case("natoms")
    assert c.ks[-1] == c.kmax
    for aid in (True, False):
        got = launch(e, c, dev, n_atoms=[7, -1, c.kmax + 5], aid=aid)
        want = launch(e, c, dev, n_atoms=[7, 0, c.kmax], aid=aid)
        assert all(g.guards_intact() for g in got.buffers())
        assert torch.equal(got.edges.raw, want.edges.raw) and torch.equal(got.scores.raw, want.scores.raw)
        assert (got.edges.t[1] == 0x7F).all() and (got.scores.bytes()[1] == 0x7F).all()
        if aid:
            assert same_molecule(got, 0, want, 0, 7) and same_molecule(got, 2, want, 2, c.kmax)
        else:
            assert got.probs.all_fill()                          # mnx_edges itself copies no probabilities
    check_case(e, c, dev)


def test_equal_classes_tie_everywhere_and_the_first_wins(engines, dev):
    """crafted (a): o[1] == o[3] bit for bit, so p1 == p3 as words on every pair and class 1 — never 3 — wins the tie"""
    c = R.case("equal")
    out = check_case(engines("equal"), c, dev)
    for b, k in enumerate(c.ks):
        p = out.probs.bytes()[b, :k, :k]
        assert np.array_equal(p[:, :, 1], p[:, :, 3]), b
        edges = out.edges.t[b, :k, :k].cpu().numpy()
        assert (edges != 3).all() and (edges == 1).mean() > 0.9, (b, np.bincount(edges.ravel(), minlength=7))


def test_wedge_tie_at_repeated_positions_gives_class_5_in_both_triangles(engines, dev):
    """crafted (b): atoms at one decoder position gather the same row, p_ij == p_ji word for word, e5 == e6 in both
    triangles: class 5 at (i, j) and at (j, i)"""
    from test_edges_host import wedge_pairs
    c = R.case("wedges")
    out = check_case(engines("wedges"), c, dev)
    same, tied = wedge_pairs(c, R.reference("wedges"), 0)
    p = out.probs.bytes()[0, :66, :66, :7]
    assert np.array_equal(p[same], p.transpose(1, 0, 2, 3)[same])
    edges, scores = out.edges.t[0, :66, :66].cpu().numpy(), out.scores.bytes()[0, :66, :66]
    assert tied.sum() >= 20 and (edges[tied] == 5).all() and (edges.T[tied] == 5).all()
    assert np.array_equal(scores[tied], scores.transpose(1, 0, 2)[tied])


def test_same_call_twice_and_without_scores(engines, dev):
    e, c = engines(), R.case("b3_kmax72")
    a, b = launch(e, c, dev), launch(e, c, dev)
    assert all(torch.equal(x.raw, y.raw) for x, y in zip(a.buffers(), b.buffers()))
    for aid in (True, False):
        n = launch(e, c, dev, aid=aid, scores=False)
        assert torch.equal(n.edges.raw, a.edges.raw), aid
    plain = launch(e, c, dev, aid=False)
    assert torch.equal(plain.edges.raw, a.edges.raw) and torch.equal(plain.scores.raw, a.scores.raw)


def test_engine_edge_probs_wrapper(engines, dev):
    e, c = engines(), R.case("k5_kmax8")
    edges, scores, probs = e.edge_probs(c.hidden.to(dev), c.idx, torch.tensor(c.ks))
    ref = launch(e, c, dev)
    assert torch.equal(edges[0, :5, :5], ref.edges.t[0, :5, :5]) and torch.equal(scores[0, :5, :5], ref.scores.t[0, :5, :5])
    assert torch.equal(probs[0, :5, :5, :7], ref.probs.t[0, :5, :5, :7])


@pytest.mark.parametrize("fn", ["mnx_edges", "mnx_edge_probs"])
def test_refusals_launch_nothing(engines, dev, fn):
    e, c = engines(), R.case("k5_kmax8")
    hidden, ai = c.hidden.to(dev), c.idx.to(dev)
    na = torch.tensor(c.ks, dtype=torch.int32, device=dev)
    out = Out(c.B, c.kmax, dev)
    good = dict(hidden=_p(hidden), idx=_p(ai), n=_p(na), B=c.B, kmax=c.kmax, max_len=c.max_len, edges=_p(out.edges.t),
                scores=_p(out.scores.t), probs=_p(out.probs.t))
    bad = [dict(hidden=None), dict(idx=None), dict(n=None), dict(edges=None), dict(B=0), dict(B=33), dict(kmax=0),
           dict(kmax=e.max_atoms + 1), dict(max_len=0)]
    if fn == "mnx_edge_probs":
        bad.append(dict(probs=None))
    for change in bad:
        a = dict(good, **change)
        args = [e.h, a["hidden"], a["idx"], a["n"], a["B"], a["kmax"], a["max_len"], a["edges"], a["scores"]]
        rc = getattr(e.lib, fn)(*args, *([a["probs"]] if fn == "mnx_edge_probs" else []), None)
        torch.cuda.synchronize()
        msg = e.lib.mnx_last_error(e.h)
        assert rc != 0 and msg.startswith(fn.encode() + b": "), (change, rc, msg)
        assert all(g.all_fill() for g in out.buffers()), change
    assert getattr(e.lib, fn)(None, *args[1:], *([good["probs"]] if fn == "mnx_edge_probs" else []), None) == -1
    assert all(g.all_fill() for g in out.buffers())
