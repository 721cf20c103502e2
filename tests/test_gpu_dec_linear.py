"""GPU (-m gpu): dec_linear_kernel<PRO, EPI> (csrc/decoder.hip), the linear of the 8-launches-per-layer decode tick, one launch
at a time on caller buffers under a scripted tick state (mnx_dec_linear), in all six instantiated forms. The references, the
inputs and the derivation of every tolerance are in tests/dec_linear_ref.py; tests/test_dec_linear_host.py shows on the CPU
that each tolerance passes an honest fp32 evaluation and refuses each named wrong variant.

What is compared how:
  * every form against a float64 reference within the derived per-element tolerance, at the production (N, K) and at ticks of
    1, 31, 32, 33, 64 and 65 alive rows (capacity 96 with 33 alive: a full, a partial and an idle tile). The K / V columns of
    EPI 0 are read back from the engine's layer-0 cache with mnx_kv_block.
  * word for word: integer operands (random and single-k probes over every residue mod 256 and every 256-chunk) on <0,1> at
    K = 256 and 1024 and on every plane of <0,4>; the two x_write streams; the hand-over <0,4> -> part -> <1,0>.
  * idle rows: every output lies between two guards and is filled with 0x7F bytes; rows >= n_alive of out, x_write and every
    part plane, the gaps between planes and the guards keep the fill, and a tick with idle rows leaves all sixteen layer-0
    cache blocks of slot 0 (the dummy row view's slot) bit-identical while alive slots change in row t alone.
  * row independence: the bits of one row's outputs at row 0 alone, at row 37 among random neighbours, and beside neighbours
    made of NaN and Inf.
  * every refusal of mnx_dec_linear, and a greedy decode on the same engine before and after the lab calls.
Scripts put row index, slot and PE rank apart (dec_linear_ref.script). Each test prints its largest error / tolerance ratio
("ratio <form> <value>"; pytest -s shows them).

Measured on the MI355X (largest |error| / tolerance per form; the tolerances are worst-case bounds and were not tuned to these):
  <2,0> 0.0045 (k/v 0.0055)   <1,0> 0.0052 (k/v 0.0086)   <1,0> with part 0.0064 (k/v 0.0086)   <0,1> 0.0055, K = 1024 0.0013
  <1,2> 0.0047   <1,3> 0.0045   <0,4> 0.0058   the <0,4> -> <1,0> chain 0.0056 / 0.0041
The bounds charge every one of the K + 2 roundings of a chain at its worst and in one direction; the kernel's four 64-term
partial chains err as a random walk, hence ratios of a few thousandths. What the bounds still refuse is shown on the CPU.
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dec_linear_ref as L
from encoder_ops_ref import words
from molnextr_amd import weights as W
from oracle import kvq as KQ
from test_gpu_encoder_ops import Guarded, _refusals, _sync

pytestmark = pytest.mark.gpu

TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
NK = KQ.rows(L.MAX_LEN)
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rig(dev):
    """One small fp32 engine (128 slots, max_len 16) and the embedding / PE tables it uploaded"""
    from molnextr_amd.engine import Engine
    dec = W.DecoderDims(enc_dim=TINY.num_features)
    ck = W.synthetic_checkpoint(0, enc=TINY, dec=dec)
    e = Engine(ck["encoder"], ck["decoder"], max_batch=2, enc=TINY, dec=dec, dtype="fp32", dec_slots=L.DEC_SLOTS,
               max_len=L.MAX_LEN)
    p = "decoder.chartok_coords.embeddings.make_embedding."
    yield SimpleNamespace(e=e, vocab=dec.vocab, emb=ck["decoder"][p + "emb_luts.0.weight"].numpy(),
                          pe=ck["decoder"][p + "pe.pe"].numpy().reshape(-1, L.D))
    e.close()
    print("dec_linear ratios " + json.dumps({k: round(v, 4) for k, v in sorted(RATIOS.items())}))


def _note(family, got, ref, tol):
    r = L.ratio(got, ref, tol)
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"ratio {family} {r:.4f}")
    return r


def _same_words(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(words(a.contiguous()), words(b.contiguous()))


class Launch:
    """One mnx_dec_linear call with guarded outputs. x / res / part are CPU tensors in ROW order ([capacity, ...])."""

    def __init__(self, rig, dev, pro, epi, N, K, capacity, rows, Wt, bias, x=None, gamma=None, beta=None, part=None, res=None,
                 part_dev=None, part_stride=0):
        self.epi, self.N, self.capacity, self.n_alive = epi, N, capacity, len(rows)
        self.planes = K // 256 if epi == 4 else 1
        self.width = L.D if epi == 0 else N
        self.stride = capacity * N + 64 if epi == 4 else 0          # a gap of 64 floats between two planes
        self.out = Guarded((self.planes - 1) * self.stride + capacity * self.width, torch.float32, dev)
        if epi == 1:
            self.out.t.copy_(res.reshape(-1))
        self.xw = Guarded(capacity * L.D, torch.float32, dev)
        self.writes_xw = pro == 2 or (pro == 1 and (part is not None or part_dev is not None))

        def d(t):
            return None if t is None else t.to(dev).contiguous()
        n_part = 0
        if part is not None:
            part_dev, n_part, part_stride = d(part), part.shape[0], capacity * L.D
        elif part_dev is not None:
            n_part = 4
        self.keep = [d(x), d(Wt), d(bias), d(gamma), d(beta), part_dev]     # alive until the call has returned
        rig.e.dec_linear(pro, epi, self.keep[0], self.keep[1], self.keep[2], self.out.t, rows, capacity, N, K,
                         gamma=self.keep[3], beta=self.keep[4], part=part_dev, n_part=n_part,
                         part_stride=self.stride if epi == 4 else part_stride, x_write=self.xw.t)
        _sync()

    def plane(self, z=0):
        """[capacity, width] of plane z on the CPU"""
        return self.out.t[z * self.stride:z * self.stride + self.capacity * self.width].cpu().reshape(self.capacity, self.width)

    def check_untouched(self, res=None):
        """live rows written, everything else as it was: idle rows, the gaps between planes, the guards, and x_write beyond the
        live rows (all of it when the form writes no stream)"""
        n, what = self.n_alive, f"epi {self.epi} capacity {self.capacity} alive {self.n_alive}"
        if self.epi == 1:
            assert self.out.untouched((0, self.capacity * self.N)), f"{what}: a guard of out changed"
            assert _same_words(self.plane()[n:], res[n:]), f"{what}: an idle row of the in-place stream changed"
        else:
            live = [(z * self.stride, n * self.width) for z in range(self.planes)]
            assert self.out.untouched(*live), f"{what}: out changed outside the live rows"
            assert all(self.out.written(s, m) for s, m in live), f"{what}: a live row of out was not written"
        if self.writes_xw:
            assert self.xw.untouched((0, n * L.D)), f"{what}: x_write changed outside the live rows"
            assert self.xw.written(0, n * L.D), f"{what}: a live row of x_write was not written"
        else:
            assert self.xw.untouched(), f"{what}: x_write changed in a form that writes no stream"

    def stream(self):
        return self.xw.t[:self.n_alive * L.D].cpu().reshape(self.n_alive, L.D)


def _cache_raw(rig, dev, slots):
    """raw layer-0 blocks of the given slots: uint8 numpy [len(slots), K|V, head, NK * 100]"""
    buf = torch.empty(len(slots), 2, L.HEADS, NK * KQ.ROW_BYTES, dtype=torch.uint8, device=dev)
    for i, s in enumerate(slots):
        for w, which in enumerate(("self_k", "self_v")):
            for hd in range(L.HEADS):
                rig.e.kv_block(which, 0, int(s), hd, out=buf[i, w, hd])
    _sync()
    return buf.cpu().numpy()


def _cache_rows(raw, ts):
    """row ts[i] of every block of slot i as a reader sees it: float32 [n, 512], columns as EPI 0's columns 256..767"""
    vals = np.empty((raw.shape[0], 2 * L.D), np.float32)
    for i, t in enumerate(ts):
        for w in range(2):
            for hd in range(L.HEADS):
                vals[i, w * L.D + hd * 32:w * L.D + hd * 32 + 32] = L.cache_values(raw[i, w, hd], NK, int(t))
    return torch.from_numpy(vals)


def _live_stream(rig, pro, rows, capacity, with_part, seed=0):
    """(x, part, stream): the fp32 rows the call is given and, word for word, what its LayerNorm reads (live rows)"""
    ent, rank = L.row_view(rows)
    n = len(rows)
    if pro == 2:
        return None, None, torch.from_numpy(L.embed_stream(rig.emb, rig.pe, ent[:, 2], rank))
    x = L.stream_rows(capacity, seed)
    if not with_part:
        return x, None, x[:n]
    part = L.part_rows(capacity, seed=seed)
    return x, part, torch.from_numpy(L.handover_chain(part.numpy(), x.numpy()))[:n]


# ---- every form against float64 ---------------------------------------------------------------------------------------------
FLOAT_CASES = [(p, e, n, k, wp) for (p, e) in L.FORMS for (n, k) in L.FORM_SHAPES[(p, e)]
               for wp in ((False, True) if (p, e) == (1, 0) else (False,))]


@pytest.mark.parametrize("capacity,n_alive", L.TICKS)
@pytest.mark.parametrize("pro,epi,N,K,with_part", FLOAT_CASES)
def test_every_form_vs_float64(rig, dev, pro, epi, N, K, with_part, capacity, n_alive):
    """<PRO, EPI> at its production (N, K) within the derived tolerance of float64; the streams word for word; idle rows,
    plane gaps and guards untouched"""
    rows = L.script(n_alive, rig.vocab, seed=capacity + n_alive)
    ent, _ = L.row_view(rows)
    Wt, bias, gamma, beta = L.weights(N, K)
    fam = f"<{pro},{epi}>" + (" K=1024" if (pro, epi) == (0, 1) and K > 256 else "") + (" +part" if with_part else "")
    res = None
    if pro == 0:
        x, res = L.plain_rows(capacity, K)
        res, part, stream = res[:, :N].contiguous(), None, x[:n_alive]
    else:
        x, part, stream = _live_stream(rig, pro, rows, capacity, with_part)
    run = Launch(rig, dev, pro, epi, N, K, capacity, rows, Wt, bias, x=x, gamma=gamma, beta=beta, part=part, res=res)
    run.check_untouched(res)
    if run.writes_xw:
        assert _same_words(run.stream(), stream), f"{fam}: x_write is not the stream word for word"
    if epi == 4:
        ref, tol = L.slice_ref(stream, Wt, bias)
        got = torch.stack([run.plane(z)[:n_alive] for z in range(run.planes)])
    else:
        z, tz = L.product_ref(pro, stream, Wt, bias, gamma, beta)
        got = run.plane()[:n_alive]
        if epi == 0:
            ref, tol, kv, tkv = L.qkv_ref(z, tz)
            cached = _cache_rows(_cache_raw(rig, dev, ent[:, 0]), ent[:, 1])
            r = _note(fam + " k/v", cached, kv, tkv)
            assert r <= 1.0, f"{fam}: cached K / V rows {r:.3f} tolerances from float64 (capacity {capacity}, {n_alive} alive)"
        else:
            ref, tol = L.epilogue_ref(epi, z, tz, None if res is None else res[:n_alive])
    r = _note(fam, got, ref, tol)
    assert r <= 1.0, f"{fam}: {r:.3f} tolerances from float64 (capacity {capacity}, {n_alive} alive)"


# ---- exact families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,n_alive", [(96, 33), (64, 64), (96, 65)])
@pytest.mark.parametrize("K", [256, 1024])
def test_integer_operands_in_place_word_for_word(rig, dev, K, capacity, n_alive):
    """<0,1>: integers in [-7, 7] (residual in [-1000, 1000]) give the int64 result exactly, whatever the order; K = 1024 runs
    the double-buffered chunk loop"""
    N = 256
    rows = L.script(n_alive, rig.vocab, seed=K)
    Wt, bias = L.int_weights(N, K)
    x, res = L.int_rows(capacity, K, N)
    run = Launch(rig, dev, 0, 1, N, K, capacity, rows, Wt, bias, x=x, res=res)
    run.check_untouched(res)
    want = L.int_product(x, Wt, bias) + res
    bad = (words(run.plane()[:n_alive]) != words(want[:n_alive])).nonzero()
    assert len(bad) == 0, f"K = {K}: {len(bad)} words differ from the integer result, first (row, column) {bad[:4].tolist()}"


@pytest.mark.parametrize("base", L.PROBE_BASES)
@pytest.mark.parametrize("pro,epi,K", [(0, 1, 256), (0, 1, 1024), (0, 4, 1024)])
def test_single_k_probes_word_for_word(rig, dev, pro, epi, K, base):
    """row r is non-zero at one k: over the four bases every residue mod 256 and every 256-chunk is probed. <0,4>: the product
    shows in the plane of its chunk alone, the bias in plane 0 alone"""
    N, capacity = 256, 64
    rows = L.script(capacity, rig.vocab, seed=base)
    Wt, bias = L.int_weights(N, K, seed=1)
    x = L.probe_rows(capacity, K, base)
    res = L.int_rows(capacity, K, N)[1] if epi == 1 else None
    run = Launch(rig, dev, pro, epi, N, K, capacity, rows, Wt, bias, x=x, res=res)
    run.check_untouched(res)
    if epi == 1:
        assert _same_words(run.plane(), L.int_product(x, Wt, bias) + res), f"K = {K} base {base}: a probe row differs"
    else:
        want = L.int_slices(x, Wt, bias)
        for z in range(run.planes):
            bad = (words(run.plane(z)) != words(want[z])).nonzero()
            assert len(bad) == 0, f"plane {z} base {base}: {len(bad)} words differ, first (row, column) {bad[:4].tolist()}"


@pytest.mark.parametrize("capacity,n_alive", [(96, 33), (64, 64), (32, 1)])
def test_integer_slices_word_for_word(rig, dev, capacity, n_alive):
    """<0,4> on random integers: each of the four planes is exact, the bias sits in plane 0 only"""
    N, K = 256, 1024
    rows = L.script(n_alive, rig.vocab, seed=3)
    Wt, bias = L.int_weights(N, K)
    x, _ = L.int_rows(capacity, K, N)
    run = Launch(rig, dev, 0, 4, N, K, capacity, rows, Wt, bias, x=x)
    run.check_untouched()
    want = L.int_slices(x, Wt, bias)
    for z in range(4):
        bad = (words(run.plane(z)[:n_alive]) != words(want[z, :n_alive])).nonzero()
        assert len(bad) == 0, f"plane {z}: {len(bad)} words differ, first (row, column) {bad[:4].tolist()}"


@pytest.mark.parametrize("capacity,n_alive", [(96, 33), (64, 64), (96, 65), (32, 1)])
@pytest.mark.parametrize("epi,N", [(0, 768), (2, 256), (3, 1024)])
def test_handover_stream_is_summed_in_the_fixed_order(rig, dev, epi, N, capacity, n_alive):
    """PRO 1 with part: x_write = (((p0 + p1) + p2) + p3) + x word for word, on partials whose pairwise, reversed and x-first
    sums all differ (tests/test_dec_linear_host.py), written for the live rows and nothing else"""
    rows = L.script(n_alive, rig.vocab, seed=epi)
    Wt, bias, gamma, beta = L.weights(N, 256)
    parts, x = L.handover_crafted(capacity, seed=n_alive)
    run = Launch(rig, dev, 1, epi, N, 256, capacity, rows, Wt, bias, x=torch.from_numpy(x), gamma=gamma, beta=beta,
                 part=torch.from_numpy(parts))
    run.check_untouched()
    want = torch.from_numpy(L.handover_chain(parts, x))[:n_alive]
    bad = (words(run.stream()) != words(want)).nonzero()
    assert len(bad) == 0, f"<1,{epi}>: {len(bad)} words of x_write are not the fixed-order sum, first {bad[:4].tolist()}"


@pytest.mark.parametrize("capacity,n_alive", [(96, 33), (64, 64)])
def test_embed_stream_word_for_word(rig, dev, capacity, n_alive):
    """PRO 2: x_write = emb[prev_tok] * 16 + pe[rank] with the row's OWN token and rank (neither its row index nor its slot)"""
    rows = L.script(n_alive, rig.vocab, seed=9)
    ent, rank = L.row_view(rows)
    Wt, bias, gamma, beta = L.weights(768, 256)
    run = Launch(rig, dev, 2, 0, 768, 256, capacity, rows, Wt, bias, gamma=gamma, beta=beta)
    run.check_untouched()
    assert _same_words(run.stream(), torch.from_numpy(L.embed_stream(rig.emb, rig.pe, ent[:, 2], rank)))
    # the test can tell: with the row index for the rank, or the slot's order of installation for the row, words differ
    assert not _same_words(run.stream(), torch.from_numpy(L.embed_stream(rig.emb, rig.pe, ent[:, 2], np.arange(n_alive))))
    assert not _same_words(run.stream(), torch.from_numpy(L.embed_stream(rig.emb, rig.pe, rows[:, 2], rank)))


@pytest.mark.parametrize("capacity,n_alive", [(96, 33), (64, 64)])
def test_w2_handover_chain(rig, dev, capacity, n_alive):
    """<0,4> writes the K-slice partials, <1,0> reads those very planes (same buffer, same stride): its x_write equals the numpy
    fp32 chain over the planes the device holds, and both launches stay within their float64 tolerances"""
    rows = L.script(n_alive, rig.vocab, seed=21)
    h, _ = L.plain_rows(capacity, 1024, seed=2)
    W2, b2, _, _ = L.weights(256, 1024, seed=2)
    first = Launch(rig, dev, 0, 4, 256, 1024, capacity, rows, W2, b2, x=h)
    first.check_untouched()
    planes = torch.stack([first.plane(z) for z in range(4)])
    ref, tol = L.slice_ref(h[:n_alive], W2, b2)
    assert _note("<0,4> chain", planes[:, :n_alive], ref, tol) <= 1.0
    x = L.stream_rows(capacity, seed=5)
    Wt, bias, gamma, beta = L.weights(768, 256)
    nxt = Launch(rig, dev, 1, 0, 768, 256, capacity, rows, Wt, bias, x=x, gamma=gamma, beta=beta, part_dev=first.out.t,
                 part_stride=first.stride)
    nxt.check_untouched()
    assert first.out.untouched(*[(z * first.stride, n_alive * 256) for z in range(4)]), "the reader wrote to the partials"
    want = torch.from_numpy(L.handover_chain(planes.numpy()[:, :n_alive], x.numpy()[:n_alive]))     # (idle rows hold the fill)
    assert _same_words(nxt.stream(), want), "x_write is not (((p0 + p1) + p2) + p3) + x of the planes <0,4> wrote"
    z, tz = L.product_ref(1, want, Wt, bias, gamma, beta)
    q, tq, _, _ = L.qkv_ref(z, tz)
    assert _note("<1,0> chain", nxt.plane()[:n_alive], q, tq) <= 1.0


# ---- idle rows and slot 0 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro", [2, 1])
def test_idle_rows_leave_slot0_cache_alone(rig, dev, pro):
    """An idle row carries the dummy row view (slot 0, position 0): after a tick that put slot 0 at position 0, a tick with idle
    rows and slot 0 NOT alive leaves all sixteen layer-0 blocks of slot 0 bit-identical, and the blocks of its alive slots
    change in row t of each head and nowhere else"""
    Wt, bias, gamma, beta = L.weights(768, 256)
    rows1 = L.script(33, rig.vocab, seed=1, with_slot0=True)
    ent1, _ = L.row_view(rows1)
    assert ent1[0, 0] == 0 and ent1[0, 1] == 0
    x, part, stream = _live_stream(rig, pro, rows1, 64, False)
    Launch(rig, dev, pro, 0, 768, 256, 64, rows1, Wt, bias, x=x, gamma=gamma, beta=beta).check_untouched()
    z, tz = L.product_ref(pro, stream, Wt, bias, gamma, beta)
    _, _, kv, tkv = L.qkv_ref(z, tz)
    slot0 = _cache_raw(rig, dev, [0])
    r = _note(f"<{pro},0> slot 0", _cache_rows(slot0, [0]), kv[:1], tkv[:1])
    assert r <= 1.0, "the first call did not write slot 0 at position 0"
    # second tick: other tokens and positions (other values for every row), 33 alive of 96: a full, a partial and an idle tile
    rows2 = L.script(33, rig.vocab, seed=4)
    ent2, _ = L.row_view(rows2)
    assert 0 not in ent2[:, 0]
    before = _cache_raw(rig, dev, ent2[:, 0])
    x, part, stream = _live_stream(rig, pro, rows2, 96, False, seed=8)
    Launch(rig, dev, pro, 0, 768, 256, 96, rows2, Wt, bias, x=x, gamma=gamma, beta=beta).check_untouched()
    assert np.array_equal(_cache_raw(rig, dev, [0]), slot0), "an idle row wrote to slot 0's cache"
    after = _cache_raw(rig, dev, ent2[:, 0])
    z, tz = L.product_ref(pro, stream, Wt, bias, gamma, beta)
    _, _, kv, tkv = L.qkv_ref(z, tz)
    assert _note(f"<{pro},0> k/v", _cache_rows(after, ent2[:, 1]), kv, tkv) <= 1.0
    for i, t in enumerate(ent2[:, 1]):
        for w in range(2):
            for hd in range(L.HEADS):
                qa, sa = KQ.parse_block(after[i, w, hd], NK)
                qb, sb = KQ.parse_block(before[i, w, hd], NK)
                keep = np.arange(NK) != t
                assert np.array_equal(qa[keep], qb[keep]) and np.array_equal(sa[keep].view(np.int32), sb[keep].view(np.int32)), \
                    f"slot {ent2[i, 0]} {'KV'[w]} head {hd}: a row other than t = {t} changed"


# ---- row independence ---------------------------------------------------------------------------------------------------------
def _subject_run(rig, dev, pro, epi, N, K, neighbours_below, neighbours_above, poison):
    """the subject (slot 50, t 5, token 17, rowc 0: PE rank 0 in any company) with its fixed input row, among neighbours in
    slots below / above it; -> the bits of everything the launch stored for it"""
    subject = [50, 5, 17, 0]
    rows = [[2 + i, (2 * i) % L.MAX_LEN, (11 * i + 1) % rig.vocab, 1 + i] for i in range(neighbours_below)] + [subject] + \
           [[60 + i, (3 * i) % L.MAX_LEN, (13 * i + 2) % rig.vocab, 100 + i] for i in range(neighbours_above)]
    rows = np.asarray(rows[::-1], np.int32)                    # installed in descending slot order: the begin kernel sorts
    n, r = len(rows), neighbours_below
    capacity = (n + 31) // 32 * 32
    g = torch.Generator().manual_seed(1234)
    xs, ress, parts = torch.randn(K, generator=g), torch.randn(N, generator=g), 0.5 * torch.randn(4, L.D, generator=g)
    fill = torch.Generator().manual_seed(n)
    x, res, part = torch.randn(capacity, K, generator=fill), torch.randn(capacity, N, generator=fill), None
    if poison:
        x[0::2], x[1::2], res[0::2], res[1::2] = float("nan"), float("inf"), float("-inf"), float("nan")
    x[r], res[r] = xs, ress
    if pro == 1 and epi != 2:                                  # production reads partials in <1,0>; <1,3> takes them as well
        part = 0.5 * torch.randn(4, capacity, L.D, generator=fill)
        if poison:
            part[:, 0::2], part[:, 1::2] = float("inf"), float("nan")
        part[:, r] = parts
    Wt, bias, gamma, beta = L.weights(N, K)
    run = Launch(rig, dev, pro, epi, N, K, capacity, rows, Wt, bias, x=None if pro == 2 else x, gamma=gamma if pro else None,
                 beta=beta if pro else None, part=part, res=res if epi == 1 else None)
    got = [words(run.plane(z)[r]) for z in range(run.planes)]
    if run.writes_xw:
        got.append(words(run.stream()[r]))
    if epi == 0:
        raw = _cache_raw(rig, dev, [50])[0]
        for w in range(2):
            for hd in range(L.HEADS):
                q, s = KQ.parse_block(raw[w, hd], NK)
                got += [torch.from_numpy(q[5].copy()), torch.from_numpy(s[5:6].view(np.int32).copy())]
    return got


@pytest.mark.parametrize("pro,epi,N,K", [(p, e, n, k) for (p, e) in L.FORMS for (n, k) in L.FORM_SHAPES[(p, e)]])
def test_a_rows_bits_do_not_depend_on_its_place_or_company(rig, dev, pro, epi, N, K):
    """The chain of every (row, column) is fixed and reads nothing of the other rows (tests/test_gpu_predict_scale.py relies on
    it): the same row alone at row 0, at row 37 (tile 1, lane 5) among 47 random neighbours, and at row 0 beside neighbours
    whose inputs are NaN and Inf — the weight contract takes any float; every index and size stays in range"""
    alone = _subject_run(rig, dev, pro, epi, N, K, 0, 0, False)
    assert all(torch.isfinite(t.view(torch.float32)).all() for t in alone[:1])
    for what, args in (("at row 37 among neighbours", (37, 10, False)), ("beside NaN / Inf neighbours", (0, 40, True))):
        other = _subject_run(rig, dev, pro, epi, N, K, *args)
        assert len(other) == len(alone)
        for i, (a, b) in enumerate(zip(alone, other)):
            assert torch.equal(a, b), f"<{pro},{epi}> {what}: output {i} of the row differs in {(a != b).sum().item()} words"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_dec_linear_rejects_bad_arguments_and_leaves_the_engine_usable(rig, dev):
    e = rig.e
    feats = W.hash_normal("dec_linear_features", (2, e.n_mem, e.n_feat), 1.0).to(dev)
    words_before = e.decode_greedy(feats, max_len=L.MAX_LEN, stop_on_eos=False)     # every position of every row is written
    before = (words_before["tokens"].cpu(), words(words_before["token_logp"]).cpu())
    capacity, n_alive, N, K = 64, 33, 768, 256
    rows = np.ascontiguousarray(L.script(n_alive, rig.vocab, with_slot0=True))
    Wt, bias, gamma, beta = (t.to(dev) for t in L.weights(N, 1024))
    x = torch.zeros(capacity, 1024, device=dev)
    part = torch.zeros(4, capacity, L.D, device=dev)
    out, xw = Guarded(capacity * 1024, torch.float32, dev), Guarded(capacity * L.D, torch.float32, dev)
    good = dict(pro=1, epi=0, x=x.data_ptr(), W=Wt.data_ptr(), bias=bias.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                part=part.data_ptr(), n_part=4, part_stride=capacity * L.D, out=out.t.data_ptr(), x_write=xw.t.data_ptr(), N=N, K=K,
                capacity=capacity, n_alive=n_alive, rows=rows.ctypes.data, stream=None)

    def script_with(i, col, value):
        bad = rows.copy()
        bad[i, col] = value
        script_with.keep.append(bad)
        return dict(rows=bad.ctypes.data)
    script_with.keep = []
    plain = dict(pro=0, epi=1, part=None, N=256)                      # <0,1>, the form that takes any K
    cases = [(dict(pro=0), "instantiated"), (dict(pro=2, epi=1), "instantiated"), (dict(epi=4), "instantiated"),
             (dict(pro=3), "instantiated"), (dict(epi=5), "instantiated"), (dict(pro=-1), "instantiated"),
             (dict(pro=0, epi=2, part=None), "instantiated"), (dict(pro=2, epi=3), "instantiated"),
             (dict(x=None), "null"), (dict(W=None), "null"), (dict(bias=None), "null"), (dict(gamma=None), "null"),
             (dict(beta=None), "null"), (dict(out=None), "null"), (dict(rows=None), "null"), (dict(x_write=None), "null"),
             (dict(pro=2, part=None, x_write=None), "null"), (dict(**plain, x=None), "null"),
             (dict(pro=0, epi=1, N=256), "part is read"),
             (dict(x=x.data_ptr() + 4), "aligned"), (dict(W=Wt.data_ptr() + 8), "aligned"), (dict(bias=bias.data_ptr() + 4), "aligned"),
             (dict(gamma=gamma.data_ptr() + 4), "aligned"), (dict(beta=beta.data_ptr() + 12), "aligned"),
             (dict(part=part.data_ptr() + 4), "aligned"), (dict(out=out.t.data_ptr() + 4), "aligned"),
             (dict(x_write=xw.t.data_ptr() + 8), "aligned"),
             (dict(capacity=48), "capacity"), (dict(capacity=0), "capacity"), (dict(capacity=-32), "capacity"),
             (dict(capacity=L.DEC_SLOTS + 32), "capacity"), (dict(capacity=33), "capacity"),
             (dict(n_alive=0), "n_alive"), (dict(n_alive=-1), "n_alive"), (dict(n_alive=capacity + 1), "n_alive"),
             (dict(capacity=32), "n_alive"),
             ({**plain, "N": 40}, "N must"), ({**plain, "N": 0}, "N must"), ({**plain, "N": -32}, "N must"),
             (dict(**plain, K=300), "K must"), (dict(**plain, K=0), "K must"), (dict(**plain, K=128), "K must"),
             (dict(K=512), "K must be 256"), (dict(pro=2, part=None, K=1024), "K must be 256"), (dict(pro=1, epi=3, N=1024, K=1024), "K must be 256"),
             (dict(N=256), "N must be 768"), (dict(pro=2, part=None, N=1024), "N must be 768"),
             (dict(n_part=0), "n_part"), (dict(n_part=17), "n_part"),
             (dict(part_stride=capacity * L.D - 4), "part_stride"), (dict(part_stride=capacity * L.D + 2), "part_stride"),
             (dict(part_stride=0), "part_stride"),
             (dict(pro=0, epi=4, part=None, N=256, K=1024, part_stride=capacity * 256 - 4), "part_stride"),
             (script_with(3, 0, L.DEC_SLOTS), "slot"), (script_with(0, 0, -1), "slot"),
             (script_with(5, 0, int(rows[2, 0])), "repeated"), (script_with(n_alive - 1, 0, int(rows[0, 0])), "repeated"),
             (script_with(1, 1, L.MAX_LEN), f": t {L.MAX_LEN} is"), (script_with(1, 1, -1), ": t -1 is"),
             (script_with(2, 2, rig.vocab), "prev_tok"), (script_with(2, 2, -1), "prev_tok"),
             (script_with(4, 3, 512), "rowc"), (script_with(4, 3, -1), "rowc")]
    slot0 = _cache_raw(rig, dev, [0])
    _refusals(e, "mnx_dec_linear", good, cases, [out, xw])
    assert np.array_equal(_cache_raw(rig, dev, [0]), slot0), "a refused call wrote to the cache"
    assert e.lib.mnx_dec_linear(e.h, *good.values()) == 0, e.lib.mnx_last_error(e.h)          # and the valid call is one
    _sync()
    assert out.written(0, n_alive * L.D) and xw.written(0, n_alive * L.D)
    words_after = e.decode_greedy(feats, max_len=L.MAX_LEN, stop_on_eos=False)
    assert torch.equal(words_after["tokens"].cpu(), before[0]) and torch.equal(words(words_after["token_logp"]).cpu(), before[1]), \
        "a greedy decode after the lab calls differs from the one before them"
