"""The scripts of tests/test_gpu_beam_forced.py (mnx_decode_beam_forced against oracle.beam.scripted_decode) and what
tests/test_beam_forced_host.py checks about them on the CPU. Not a test module.

A script is (parent, token) int64 [max_len][B][beam]: new hypothesis j of original image b at step t descends from
hypothesis parent[t][b][j] and emits id token[t][b][j]. A hypothesis' slot is b * beam + j; key tau of a row lives in the slot
of its ancestor at step tau, so every change of parent moves where dec_attn_kernel<true> has to read its past from. The
cases are the smallest at which that kernel takes another turn: 32-key value blocks, VPRE = 5 prefetched blocks (160 keys),
the second key per thread from 256 keys, the `#pragma unroll 4` body of the value loop complete at 288 keys, its remainder
from 289."""
from dataclasses import dataclass

import numpy as np
import torch

from molnextr_amd import weights as W

EOS, VOCAB = 2, 229
KEY_RANGES = ((0, 32), (32, 160), (160, 256), (256, 288), (288, 330))
SEAM_SWAPS = (31, 32, 159, 160, 255, 256, 287, 288, 328)
SEAM_CHANGES = (32, 33, 160, 161, 256, 257, 288, 289)      # key indices at which the owning slot changes (and 329, by step 328)


@dataclass
class Case:
    name: str
    B: int
    beam: int
    n_best: int
    max_len: int
    parent: torch.Tensor
    token: torch.Tensor

    @property
    def features(self):
        return W.hash_normal(f"beam_forced_{self.name}", (self.B, 144, 1024), 0.5)


def rotation_parent(t, b, j, K):
    """even images: every hypothesis takes its neighbour's place at every step; odd images: by 1, 2, 3, 1, ... places"""
    return (j + 1 + (t % 3 if b % 2 else 0)) % K


def _tokens(name, max_len, B, K):
    """seeded ids other than <eos> (3 .. VOCAB - 1; the grammar mask only lowers a forced id's log-prob). With one id
    per (step, image, hypothesis) drawn independently a (parent, token) pair could repeat inside an image: hypothesis j
    draws from the ids congruent to j modulo K, so the K ids of an image at a step are distinct."""
    g = np.random.default_rng(sum(name.encode()) + 1000 * max_len)
    base = g.integers(0, (VOCAB - 3) // K, size=(max_len, B, K))
    return torch.from_numpy(3 + base * K + np.arange(K)[None, None, :]).long()


def _rotation(name, B, K, n_best, max_len):
    parent = torch.tensor([[[rotation_parent(t, b, j, K) for j in range(K)] for b in range(B)] for t in range(max_len)])
    return Case(name, B, K, n_best, max_len, parent, _tokens(name, max_len, B, K))


def case(name) -> Case:
    if name == "rotation":
        return _rotation(name, 2, 4, 4, 330)
    if name == "seams":
        c = Case(name, 1, 2, 2, 330, torch.arange(2).repeat(330, 1, 1), _tokens(name, 330, 1, 2))
        for t in SEAM_SWAPS:
            c.parent[t, 0] = torch.tensor([1, 0])
        return c
    if name == "leaving":       # hypothesis 0 of image 1 ends at step 3, that of image 3 at step 40: both images leave at once
        c = _rotation(name, 5, 3, 1, 48)
        c.token[3, 1, 0] = EOS
        c.token[40, 3, 0] = EOS
        return c
    if name == "two_tiles":     # 40 rows: the ancestors' slots reach into the second 32-row tile
        return _rotation(name, 8, 5, 5, 40)
    raise KeyError(name)


CASES = ("rotation", "seams", "leaving", "two_tiles")


def alive_steps(c: Case):
    """[max_len][B] bool: image b is in the batch at step t (top hypothesis finished and n_best stored -> it leaves)"""
    alive = np.ones((c.max_len, c.B), bool)
    for b in range(c.B):
        top, n = False, 0
        for t in range(c.max_len):
            fin = (c.token[t, b] == EOS) | (t + 1 == c.max_len)
            top, n = top or bool(fin[0]), n + int(fin.sum())
            if top and n >= c.n_best:
                alive[t + 1:, b] = False
                break
    return alive
