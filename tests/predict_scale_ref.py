"""Jobs, expectations and trace reading for the large-engine greedy predict tests (tests/test_gpu_predict_scale.py; the
builders and the comparison are themselves tested on the CPU in tests/test_predict_scale_host.py).

A job is a list of reference batches ("chunks") of `rb` images taken from a POOL of K = 7 distinct batches: chunk c holds pool
batch c % K, and the last chunk is ragged (the first n_img % rb rows of its pool batch). The expected output of a job is put
together from K + 1 LONE calls — predict() on one pool batch, which the engine decodes in tile 0 with a one-pass scan and the
smallest tick capacity, the regime the rest of the suite pins against the reference and the oracle — so the large regimes of
the code under test cannot have produced it.

Why K = 7: duplicated chunks hide a mix-up between two chunks that hold the same batch. The plausible mix-ups alias slots a
power-of-two number of tiles apart (an index cut to 10 or 11 bits, a wrapped 32-bit offset), and 2^k mod 7 is never 0: two
chunks 1, 2, 4, ..., 64 tiles apart always hold different batches. With chunks of three tiles (rb = 96) a row and the row
32 * 2^k slots further sit at different rows of their chunks (32 * 2^k mod 96 is never 0), hence hold different images too."""
import re

import torch

from molnextr_amd import weights as W

K = 7                     # pool batches
ROW_TILE = 32             # slots per tile (csrc/dec_types.h)
TINY = W.EncoderDims(img_size=96, patch=4, embed_dim=32, depths=(2, 2), heads=(1, 2), window=12)
DEC = W.DecoderDims(enc_dim=TINY.num_features)
KEYS = ("tokens", "lengths", "token_logp", "n_atoms", "atom_idx", "edges", "edge_scores", "atom_scores", "overall_score")


def job_images(dec_slots):
    """(ref_batch, n_img) of the two jobs run on an engine of dec_slots slots. A: chunks of one tile, as many as the engine
    has tiles, then a second wave of seven and a ragged one of 20 rows. B: chunks of three tiles, a second wave of one, and
    a ragged one (52, 20 and 84 rows at 1088, 3072 and 4096 slots)."""
    return {"A": (32, dec_slots + 7 * 32 + 20), "B": (96, dec_slots + 96 + 20)}


def job_chunks(n_img, rb, k=K):
    """[(pool batch, rows)] of the job's chunks in image order; only the last one may hold fewer than rb rows."""
    n_chunks = (n_img + rb - 1) // rb
    return [(c % k, min(rb, n_img - c * rb)) for c in range(n_chunks)]


def job_index(n_img, rb, k=K):
    """int64 [n_img]: the pool image (pool batch * rb + row) that job row i holds."""
    i = torch.arange(n_img)
    return (i // rb) % k * rb + i % rb


def lone_calls(n_img, rb, k=K):
    """The distinct (pool batch, rows) a job's expectation is made of: the full batches it uses and its ragged tail."""
    return sorted(set(job_chunks(n_img, rb, k)))


def expectation(lone, n_img, rb, k=K):
    """lone: {(pool batch, rows): result dict of that lone call} -> the job's expected result dict, chunk by chunk."""
    parts = [lone[c] for c in job_chunks(n_img, rb, k)]
    return {key: torch.cat([p[key] for p in parts]) for key in parts[0]}


def _words(t):
    """A float tensor as its integer words (the comparison is bit for bit: -0.0 is not 0.0, a NaN equals itself)."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def compare(got, want, rb, what=""):
    """Every key of `want` word for word; AssertionError names the first differing job row, its chunk and row in the chunk
    (a first-wave chunk of job A sits in the tile of its own index), the key and how many rows differ."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        a, b = _words(got[key]), _words(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, tuple(a.shape), tuple(b.shape), a.dtype, b.dtype)
        if torch.equal(a, b):
            continue
        rows = (a != b).reshape(a.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
        r = rows[0]
        raise AssertionError(f"{what}: '{key}' differs in {len(rows)} of {a.shape[0]} rows, first job row {r} = chunk {r // rb} "
                             f"(pool batch {r // rb % K}) row {r % rb}; differing chunks {sorted({q // rb for q in rows})[:16]}")


_POLL = re.compile(r"^(?P<ms>[0-9.]+) seq (?P<seq>\d+) live (?P<live>\d+) next (?P<next>\d+) next_enc (?P<next_enc>\d+) "
                   r"done (?P<done>\d+) free_tiles (?P<free_tiles>\d+) scan (?P<scan>\d+) rows_cap (?P<rows_cap>\d+)$")
_END = re.compile(r"^(?P<ms>[0-9.]+) end host_wait_ms (?P<host_wait_ms>[0-9.]+)$")


def parse_trace(text):
    """The MNX_TRACE lines of predict calls (csrc/engine.hip predict_impl) -> (polls, ends): one dict per poll line (ms a
    float, the other fields ints) and one per 'end' line. A line of neither form raises ValueError."""
    polls, ends = [], []
    for line in text.splitlines():
        if not line.strip():
            continue
        m = _POLL.match(line)
        if m:
            polls.append({k: float(v) if k == "ms" else int(v) for k, v in m.groupdict().items()})
            continue
        m = _END.match(line)
        if not m:
            raise ValueError(f"not a predict trace line: {line!r}")
        ends.append({k: float(v) for k, v in m.groupdict().items()})
    return polls, ends


def cap_step(bound):
    """The step of the tick capacity for an alive-row bound (predict_impl: one tick graph per capacity)."""
    return 64 if bound <= 1024 else 128 if bound <= 2048 else 256


def rows_cap_of(bound, dec_slots):
    """The tick capacity predict_impl launches for an alive-row bound: the bound rounded up to its step, at most dec_slots."""
    s = cap_step(max(bound, 1))
    return min(dec_slots, (max(bound, 1) + s - 1) // s * s)


def allowed_rows_caps(dec_slots):
    """{capacity: set of the steps that lead to it} over every bound 1 .. dec_slots."""
    out = {}
    for b in range(1, dec_slots + 1):
        out.setdefault(rows_cap_of(b, dec_slots), set()).add(cap_step(b))
    return out
