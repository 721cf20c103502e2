"""CPU: the bond head's float64 reference, its derived tolerance and its inputs (tests/edges_ref.py) judged without a
kernel — what tests/test_gpu_edges.py relies on when it judges the kernels with them.

  * the tolerance is not tight: the fp32 CPU restatement (oracle/edges.edge_logits + softmax) stays within HALF of it on every
    case, on every probability;
  * it is not vacuous: each named wrong variant of the probabilities, written as a small fp32 restatement, exceeds it TENFOLD
    on at least one case;
  * the exact comparison behind edge_sym_kernel is not vacuous: each named wrong variant of the symmetrisation changes at
    least one class or one score word against symmetrise_exact on the same fp32 probabilities;
  * coverage, asserted: on every random case with a molecule of 63 atoms or more the float64 winner takes every class 0..6
    among the compared pairs (the cases of 1, 2 and 5 atoms are there for the seams and strides; 1, 4 and 25 pairs cannot
    hold seven classes and are not asked to); on EVERY random case at most 1 % of the pairs have a float64 margin below
    twice the tolerance (the pairs the end-to-end comparison leaves out); the crafted checkpoints tie where they were made to.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edges_ref as R

ALL_CASES = R.RANDOM_CASES + R.BIG_CASES + R.CRAFTED_CASES + ("clamp", "natoms")
VARIANT_CASES = ("k65", "k5_kmax8", "wedges")
PROB_VARIANTS = ("w1_halves_swapped", "b1_twice", "b1_dropped", "tanh_gelu", "w2_transposed", "w2_stride_7", "softmax_8_stale",
                 "b2_dropped")
SYM_VARIANTS = ("no_cross_average", "mirror_in_wrong_triangle", "no_mirror_below", "average_in_fp32", "last_maximum",
                "diagonal_averaged")
SYM_CASES = ("k65", "b3_kmax72", "equal", "wedges")


def _molecules(name):
    c, ref = R.case(name), R.reference(name)
    sd = R.checkpoint(c.ckpt)["decoder"]
    for b, k in enumerate(c.ks):
        if k:
            yield c, ref, sd, b, k, c.idx[b, :k].clamp(0, c.max_len - 1)


@pytest.mark.parametrize("name", ALL_CASES)
def test_fp32_restatement_stays_within_half_the_tolerance(name):
    worst = 0.0
    for c, ref, sd, b, k, idx in _molecules(name):
        err = np.abs(R.probs32(c.hidden[b], idx, sd).numpy() - ref.p64[b])
        worst = max(worst, float((err / ref.tol[b]).max()))
        assert (ref.tol[b] > 0).all()
    print(f"ratio edges_prob_fp32_restatement {name} {worst:.4f}")
    assert worst <= 0.5, (name, worst)


def test_the_largest_tolerance_is_a_small_multiple_of_the_fp32_error():
    """4.5e-7 is what the fp32 restatement measures on the k = 57 / 159 rows of test_bond_head_ragged_batch_and_empty: the
    largest tolerance of the synthetic-checkpoint cases leaves it a factor of two and is not ten times it"""
    top = max(float(t.max()) for n in R.RANDOM_CASES for t in R.reference(n).tol if t.size)
    print(f"largest tolerance {top:.3e}")
    assert 2 * 4.5e-7 <= top <= 10 * 4.5e-7, top


@torch.no_grad()
def wrong_probs(hidden, idx, sd, variant):
    """the head in fp32 with one named mistake -> float64 [k, k, 7]"""
    W1, b1, W2, b2 = R.head_weights(sd, torch.float32)
    h = hidden[torch.as_tensor(idx, dtype=torch.long)]
    k = h.shape[0]
    hi, hj = h[:, None, :].expand(k, k, R.D), h[None, :, :].expand(k, k, R.D)
    hh = torch.cat([hj, hi] if variant == "w1_halves_swapped" else [hi, hj], dim=-1)
    a = F.linear(hh, W1, None if variant == "b1_dropped" else b1)
    if variant == "b1_twice":
        a = a + b1
    z = F.gelu(a, approximate="tanh" if variant == "tanh_gelu" else "none")
    if variant == "w2_transposed":                      # element (c, t) read at t * 7 + c
        W2 = W2.reshape(R.D, 7).T
    elif variant == "w2_stride_7":                      # element (c, t) read at c * 7 + t
        flat = W2.reshape(-1)
        W2 = torch.stack([flat[c * 7:c * 7 + R.D] for c in range(7)])
    o = F.linear(z, W2, None if variant == "b2_dropped" else b2)
    if variant == "softmax_8_stale":                    # the eighth slot of a pair holds what a zeroed buffer does
        return torch.softmax(torch.cat([o, torch.zeros(k, k, 1)], dim=-1), dim=-1)[..., :7].double()
    return torch.softmax(o, dim=-1).double()


@pytest.mark.parametrize("variant", PROB_VARIANTS)
def test_each_wrong_probability_variant_exceeds_the_tolerance_tenfold(variant):
    worst = 0.0
    for name in VARIANT_CASES:
        for c, ref, sd, b, k, idx in _molecules(name):
            err = np.abs(wrong_probs(c.hidden[b], idx, sd, variant).numpy() - ref.p64[b])
            worst = max(worst, float((err / ref.tol[b]).max()))
    print(f"{variant}: {worst:.1f} tolerances")
    assert worst >= 10.0, (variant, worst)


def wrong_symmetrise(p32, variant):
    """get_edge_prediction with one named mistake, on fp32 probabilities [k, k, 7] -> (class, score)
    no_cross_average          classes 5 and 6 averaged with themselves: e5 = (p_ij5 + p_ji5) / 2
    mirror_in_wrong_triangle  the 5 <-> 6 exchange lands on the pairs i < j and not on the pairs i > j
    no_mirror_below           the pairs i > j copy the pair above the diagonal without exchanging 5 and 6
    average_in_fp32           (p_ij + p_ji) * 0.5f, then widened
    last_maximum              >= in the scan for the maximum: the last of equal maxima
    diagonal_averaged         the diagonal goes through the same averages, e5 = e6 = (p_ii5 + p_ii6) / 2"""
    p = np.asarray(p32, dtype=np.float32)
    k = p.shape[0]
    t = p.transpose(1, 0, 2)
    if variant == "average_in_fp32":
        e = ((p + t) * np.float32(0.5)).astype(np.float64)
        e[..., 5] = ((p[..., 5] + t[..., 6]) * np.float32(0.5)).astype(np.float64)
        e[..., 6] = ((p[..., 6] + t[..., 5]) * np.float32(0.5)).astype(np.float64)
    else:
        p64, t64 = p.astype(np.float64), t.astype(np.float64)
        e = (p64 + t64) / 2
        if variant != "no_cross_average":
            e[..., 5] = (p64[..., 5] + t64[..., 6]) / 2
            e[..., 6] = (p64[..., 6] + t64[..., 5]) / 2
    ii, jj = np.indices((k, k))
    exchange = {"mirror_in_wrong_triangle": ii != jj, "no_mirror_below": ii > jj}.get(variant)
    if exchange is not None:
        e[exchange] = e[exchange][:, [0, 1, 2, 3, 4, 6, 5]]
    if variant != "diagonal_averaged":
        e[ii == jj] = p[ii == jj].astype(np.float64)
    if variant == "last_maximum":
        return 6 - np.argmax(e[..., ::-1], axis=2), np.max(e, axis=2)
    return np.argmax(e, axis=2), np.max(e, axis=2)


def _fp32_probs(name):
    for c, ref, sd, b, k, idx in _molecules(name):
        yield R.probs32(c.hidden[b], idx, sd).numpy().astype(np.float32)


def test_wrong_symmetrise_restates_the_exact_one_when_nothing_is_wrong():
    for name in SYM_CASES:
        for p in _fp32_probs(name):
            cls, sc = R.symmetrise_exact(p)
            c2, s2 = wrong_symmetrise(p, "none")
            assert np.array_equal(cls, c2) and np.array_equal(sc.view(np.int64), s2.view(np.int64)), name


@pytest.mark.parametrize("variant", SYM_VARIANTS)
def test_each_wrong_symmetrisation_changes_a_class_or_a_score_word(variant):
    caught = {}
    for name in SYM_CASES:
        n = 0
        for p in _fp32_probs(name):
            cls, sc = R.symmetrise_exact(p)
            c2, s2 = wrong_symmetrise(p, variant)
            n += int(((cls != c2) | (sc.view(np.int64) != s2.view(np.int64))).sum())
        caught[name] = n
    print(f"{variant}: pairs that differ {caught}")
    assert any(caught.values()), (variant, caught)
    if variant == "last_maximum":                       # only an exact tie separates > from >=
        assert caught["equal"] and caught["wedges"], caught
    if variant in ("no_cross_average", "no_mirror_below", "mirror_in_wrong_triangle", "average_in_fp32"):
        assert caught["k65"], caught                    # the random inputs alone catch these


@pytest.mark.parametrize("name", R.RANDOM_CASES + R.BIG_CASES)
def test_random_cases_cover_the_classes_and_leave_few_pairs_undecided(name):
    c, ref = R.case(name), R.reference(name)
    pairs = excluded = 0
    seen = np.zeros(7, dtype=np.int64)
    for b, k in enumerate(c.ks):
        dec = ref.decided(b)
        pairs += dec.size
        excluded += int((~dec).sum())
        seen += np.bincount(ref.cls[b][dec].ravel(), minlength=7)
    print(f"{name}: {pairs} pairs, {excluded} below twice the tolerance, winners per class {seen.tolist()}")
    assert excluded <= 0.01 * pairs, (name, excluded, pairs)
    if max(c.ks) >= 63:
        assert (seen > 0).all(), (name, seen.tolist())


def test_crafted_equal_classes_tie_on_nearly_every_pair():
    """p1 and p3 are the same function of the same numbers; they win (together) on more than 90 % of the pairs"""
    c, ref = R.case("equal"), R.reference("equal")
    for b, k in enumerate(c.ks):
        e = R.symmetrise(ref.p64[b])
        assert np.abs(e[..., 1] - e[..., 3]).max() < 1e-15
        share = float((np.maximum(e[..., 1], e[..., 3]) >= e.max(axis=2)).mean())
        print(f"equal[{b}]: classes 1 / 3 hold the maximum on {100 * share:.1f} % of {k * k} pairs")
        assert share > 0.9, (b, share)
    for p in _fp32_probs("equal"):                      # and the rule: the first of the two
        cls, _ = R.symmetrise_exact(np.concatenate([p[..., :3], p[..., 1:2], p[..., 4:]], axis=-1))
        assert (cls != 3).all() and (cls == 1).mean() > 0.9


def wedge_pairs(c, ref, b):
    """the pairs i != j of molecule b at one decoder position whose (equal) classes 5 and 6 hold the float64 maximum"""
    idx = c.idx[b, :c.ks[b]].numpy()
    e = R.symmetrise(ref.p64[b])
    same = (idx[:, None] == idx[None, :]) & ~np.eye(len(idx), dtype=bool)
    wins = np.minimum(e[..., 5], e[..., 6]) > e[..., :5].max(axis=2) + 1e-6
    assert np.abs(e[..., 5] - e[..., 6])[same].max() < 1e-15
    return same, same & wins


def test_crafted_wedges_tie_at_repeated_positions():
    c, ref = R.case("wedges"), R.reference("wedges")
    same, tied = wedge_pairs(c, ref, 0)
    print(f"wedges: {int(same.sum())} ordered pairs at a shared position, {int(tied.sum())} with 5 = 6 as the maximum")
    assert same.sum() == 66 * (R.WEDGE_REPEAT - 1) and tied.sum() >= 2 * 10
    assert np.array_equal(tied, tied.T)
