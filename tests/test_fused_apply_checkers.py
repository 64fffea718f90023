"""tests/fused_apply_ref.py without a GPU: ``table_violations`` accepts the
right table and rejects each wrong one it exists for, an optimizer applied
twice to a hot key, a skipped long-role uid and a changed bystander row."""

import pytest
import torch

import fused_apply_ref as fref
import sparse_core_ref as ref


def _case(variant, dim=9, n=17):
    """(case, slots, live, table before, table after one right step): the
    uid at position 0 stands for the hot key."""
    case = ref.OptCase(variant, dim, n)
    slots, grads, counts = case.step(0)
    live = n - 3                      # the last uids lie beyond u_dev
    assert int(slots[0]) >= 0 and int((slots[:live] < 0).sum()) >= 1
    w1, s1 = ref.step_reference(case.opt, case.weights, case.state, slots,
                                grads, counts, torch.float32, live)
    return case, slots, grads, counts, live, w1, s1


VARIANTS = ["default", "adagrad", "adam", "test"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_right_table_passes(variant):
    case, slots, _, _, live, w1, s1 = _case(variant)
    assert fref.table_violations(case.weights, case.state, w1.clone(),
                                 s1.clone(), w1, s1, slots, live) == []
    # and the step is visible: an unapplied table is not "right"
    assert fref.table_violations(case.weights, case.state, case.weights,
                                 case.state, w1, s1, slots, live) \
        == ["a live row was not applied"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_optimizer_applied_twice_to_a_hot_key(variant):
    case, slots, grads, counts, live, w1, s1 = _case(variant)
    hot = torch.full_like(slots, -1)
    hot[0] = slots[0]
    w2, s2 = ref.step_reference(case.opt, w1, s1, hot, grads, counts,
                                torch.float32, live)
    assert not ref.bits_equal(w2[slots[0]], w1[slots[0]])
    bad = fref.table_violations(case.weights, case.state, w2, s2, w1, s1,
                                slots, live)
    assert bad == ["a live row differs from the two-launch result"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_skipped_long_role_uid(variant):
    case, slots, _, _, live, w1, s1 = _case(variant)
    w2, s2 = w1.clone(), s1.clone()
    w2[slots[0]] = case.weights[slots[0]]
    s2[slots[0]] = case.state[slots[0]]
    bad = fref.table_violations(case.weights, case.state, w2, s2, w1, s1,
                                slots, live)
    assert bad == ["a live row was not applied"]


def test_bystander_rows():
    """A canary row, the row behind a uid at or beyond the live count, and
    a state entry count as changed on a single flipped bit."""
    case, slots, _, _, live, w1, s1 = _case("adagrad")
    keep = ref.untouched_rows(case.R, slots, live)
    tail_row = int(slots[live:][slots[live:] >= 0][0])
    assert bool(keep[tail_row])
    canary = int(keep.nonzero()[0])
    for row, in_state in [(canary, False), (tail_row, False),
                          (canary, True)]:
        w2, s2 = w1.clone(), s1.clone()
        t = (s2 if in_state else w2)[row]
        t.view(torch.int32)[0] ^= 1
        bad = fref.table_violations(case.weights, case.state, w2, s2, w1,
                                    s1, slots, live)
        assert bad == ["a row that no live uid names changed"], (row, bad)


def test_pair_keys_lists_hold_at_most_two():
    g = torch.Generator().manual_seed(0)
    keys = fref.pair_keys(301, g)
    cnt = torch.unique(keys, return_counts=True)[1]
    assert keys.numel() == 451 and int(cnt.max()) == 2
    assert int((cnt == 2).sum()) == 150 and int((cnt == 1).sum()) == 151
