"""tests/fused_pull_ref.py without a GPU: each checker accepts the right
result and rejects the wrong one it exists for: a row initialised although
not new, a duplicate's ``out`` differing from its first occurrence, ``valid``
left unset, and a changed bystander."""

import torch

import fused_pull_ref as pref


def _scene():
    """A 12-row table, rows 0..5 live; the batch names slots 2, 3 (live)
    and 7, 8 (new). Returns (before, right after, touched)."""
    g = torch.Generator().manual_seed(1)
    w0 = torch.randn(12, 5, generator=g)
    s0 = torch.rand(12, 3, generator=g)
    v0 = torch.zeros(12, dtype=torch.uint8)
    v0[:6] = 1
    w1, s1, v1 = w0.clone(), s0.clone(), v0.clone()
    for r in (7, 8):
        w1[r] = torch.randn(5, generator=g)
        s1[r] = 0.3
        v1[r] = 1
    return (w0, s0, v0), (w1, s1, v1), torch.tensor([2, 7, 3, 8, 7])


def _clone(t):
    return tuple(x.clone() for x in t)


def test_right_table_passes():
    before, after, touched = _scene()
    assert pref.table_violations(before, _clone(after), after, touched) == []


def test_row_initialised_although_not_new():
    before, after, touched = _scene()
    got = _clone(after)
    got[0][2] = 0.25            # live row 2 re-initialised
    assert pref.table_violations(before, got, after, touched) \
        == ["a row that was not new was written"]
    got = _clone(after)
    got[1][3, 1] = 0.3          # its state row alone
    assert pref.table_violations(before, got, after, touched) \
        == ["a row that was not new was written"]


def test_valid_left_unset():
    before, after, touched = _scene()
    got = _clone(after)
    got[2][8] = 0
    assert pref.table_violations(before, got, after, touched) \
        == ["valid left unset for a touched slot"]


def test_bystanders_and_new_rows():
    before, after, touched = _scene()
    got = _clone(after)
    got[0][10].view(torch.int32)[0] ^= 1          # canary row, one bit
    assert pref.table_violations(before, got, after, touched) \
        == ["a row outside the batch changed"]
    got = _clone(after)
    got[2][11] = 1
    assert pref.table_violations(before, got, after, touched) \
        == ["the bitmap changed outside the touched slots"]
    got = _clone(after)
    got[0][7, 4] += 1.0                            # wrong init value
    assert pref.table_violations(before, got, after, touched) \
        == ["a new row differs from the unfused pull's"]
    got = _clone(after)
    got[1][8] = 0.0                                # state row not initialised
    assert pref.table_violations(before, got, after, touched) \
        == ["a new row differs from the unfused pull's"]


def test_duplicate_out_differs_from_first_occurrence():
    keys = torch.tensor([5, 9, 5, -1, 9, 5, -1])
    g = torch.Generator().manual_seed(2)
    rows = {5: torch.randn(4, generator=g), 9: torch.randn(4, generator=g),
            -1: torch.zeros(4)}
    out = torch.stack([rows[int(k)] for k in keys])
    assert pref.duplicate_violations(keys, out) == []
    bad = out.clone()
    bad[5, 3] += 1e-3
    assert pref.duplicate_violations(keys, bad) \
        == ["a duplicate's row differs from its first occurrence's"]
    bad = out.clone()
    bad[0, 0] = 7.0             # the first occurrence itself is the odd one
    assert pref.duplicate_violations(keys, bad) != []


def test_expected_slots_guards():
    keys = torch.tensor([0, 1, 2, 3, 29, 30, -1, -7, 1 << 40])
    assert pref.expected_slots(keys, 1, 30).tolist() \
        == [0, 1, 2, 3, 29, -1, -1, -1, -1]
    assert pref.expected_slots(keys, 3, 10).tolist() \
        == [0, 0, 0, 1, 9, -1, -1, -1, -1]
