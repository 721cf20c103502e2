"""CPU: the scripted beam cases (tests/beam_script_ref.py) reach what they are meant to reach. These are conditions on the
INPUTS of tests/test_gpu_beam_script.py, checked with oracle.beam.BeamStrategy alone, so that the device agreeing with the
expectation means the tie rule, the pool and the bookkeeping were exercised — not that a case happened to avoid them."""
import numpy as np
import pytest

import beam_script_ref as R


@pytest.mark.parametrize("case", ["ties_small", "ties_full", "ties_spread", "pool_quant"])
def test_quantised_tables_tie_at_every_step(case):
    c = R.coverage(case)
    print(case, c)
    assert c["image_steps"] > 0 and c["tied_steps"] == c["image_steps"]


def test_tie_cases_decide_membership_and_cross_parents():
    """Together: a tie between rank K - 1 and rank K (who is in), and a tie between candidates of different parents. The
    full quantised table finds K + 1 zeros under parent 0 at every step (its ties are all inside one row); ties_spread is
    there so that the 256-row shape also ties ACROSS parents."""
    small, full, spread = R.coverage("ties_small"), R.coverage("ties_full"), R.coverage("ties_spread")
    assert small["in_out_ties"] + full["in_out_ties"] >= 1
    assert small["cross_parent_ties"] + full["cross_parent_ties"] >= 1
    assert spread["in_out_ties"] >= 1 and spread["cross_parent_ties"] >= 1


def test_ties_full_uses_every_candidate_slot_and_images_leave_apart():
    table, ex = R.expectation("ties_full")
    assert ex.B * ex.K == 256 and ex.K * ex.V - 1 == 1831 > 7 * 256       # the eighth candidate of a thread is in use
    assert len(R.coverage("ties_full")["leave_steps"]) >= 3


def test_ties_spread_moves_parents_and_scores():
    _, ex = R.expectation("ties_spread")
    c = R.coverage("ties_spread")
    assert c["moved_steps"] >= ex.steps_run // 2
    assert len(np.unique(ex.final_scores)) > 3 and len(c["leave_steps"]) >= 3


def test_boundaries_are_the_tied_maxima():
    _, ex = R.expectation("boundaries")
    assert ex.B == len(R.BOUNDARY_TIES) and (ex.K, ex.V) == (8, 229)
    assert (ex.score[0] == 0.0).all() and (ex.parent[0] == 0).all()        # step 0: K parents with equal cum
    for b, flats in enumerate(R.BOUNDARY_TIES):
        v, i = ex.stats["top"][(1, b)]
        n = len(flats)
        assert i[:n].tolist() == list(flats), f"image {b}"
        assert (v[:n] == v[0]).all() and v[n] < v[0], f"image {b}"
        assert (ex.parent[1, b, :n] * ex.V + ex.token[1, b, :n]).tolist() == list(flats)


def test_pool_events_all_occur():
    c = R.coverage("pool_hand")
    print("pool_hand", c, "pool_quant", R.coverage("pool_quant"))
    for event in ("equal_insert", "displaced", "dropped", "top_short", "leaves_while_other_stays"):
        assert c[event] >= 1, event
    _, ex = R.expectation("pool_hand")
    # image 1, as the table's docstring walks through it: the earlier of two equal scores stays ahead
    assert ex.final_scores[1].tolist() == [0.0, -0.5] and [len(x) for x in ex.final_ids[1]] == [8, 5]
    assert ex.stats["left"] == [2, 7, 3]


def test_maxlen_runs_to_the_last_step_with_moving_parents():
    _, ex = R.expectation("maxlen")
    c = R.coverage("maxlen")
    assert ex.max_len == R.CFG_MAX_LEN and ex.steps_run == ex.max_len and ex.K == 8
    assert c["finish_steps"] == [ex.max_len - 1]
    assert all(len(f) == ex.K for f in ex.stats["finished"])               # every hypothesis finishes at it
    assert c["moved_steps"] >= ex.max_len // 2
    assert all(len(ids) == ex.max_len for row in ex.final_ids for ids in row)


def test_neg_inf_runs_short_of_finite_candidates_without_nan():
    table, ex = R.expectation("neg_inf")
    c = R.coverage("neg_inf")
    assert torch_isinf_count(table) > table.numel() // 2
    assert c["short_of_k"] >= 1
    assert np.isneginf(ex.score[ex.entered]).any()                         # an -inf candidate was picked
    assert not np.isnan(ex.score).any() and not np.isnan(ex.final_scores).any()
    v, i = ex.stats["top"][(0, 0)]                                         # step 0 of image 0: one finite id, the banned <eos>, then
    assert i[:3].tolist() == [1, R.EOS, 0] and np.isneginf(v[2])           # the lowest flat index among the -inf candidates


def torch_isinf_count(t):
    return int(t.isinf().sum())


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_golden_expectation_is_the_golden(case):
    """The expectation of a golden case holds what the .npz holds (that the rebuilt table reproduces those scores exactly
    through BeamStrategy is test_oracle_golden.py::test_beam_strategy_vs_reference_class); here: BeamStrategy on the
    rebuilt table gives the same expectation wherever the golden knows it."""
    table, ex = R.expectation("golden_" + case)
    st = R.run_strategy(table, ex.n_best)
    assert st.steps_run == ex.steps_run
    assert np.array_equal(st.entered, ex.entered) and np.array_equal(st.alive, ex.alive)
    assert np.array_equal(st.n_active, ex.n_active)
    assert np.array_equal(st.score.view(np.int32), ex.score.view(np.int32))
    assert np.array_equal(st.parent[ex.known], ex.parent[ex.known]) and np.array_equal(st.token[ex.known], ex.token[ex.known])
    assert st.final_ids == ex.final_ids and np.array_equal(st.final_scores.view(np.int32), ex.final_scores.view(np.int32))
    assert ex.known.sum() < ex.entered.sum()        # the golden does hide the images that leave
