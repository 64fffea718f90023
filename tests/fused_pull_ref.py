"""Reference side of tests/test_gpu_fused_pull.py: plain torch, no GPU.

The fused pull (array touch inside the dedup's assign kernel, then
k_pull_merged) is held against the unfused launches run from the same table
snapshot. uids are not reproducible from run to run, so everything is
compared through keys:

  - ``expected_slots``: key // shard_num with k_array_touch's guards;
  - ``duplicate_violations``: every occurrence of a key reads the row its
    first occurrence reads;
  - ``table_violations``: the table after the pull against the snapshot
    before it and the unfused result: a row that was live is never written
    (it would have been initialised although not new), every touched slot
    is marked valid, rows and bitmap outside the touched slots are bit for
    bit what they were, new rows hold what the unfused pull put there.

The checkers are themselves tested in tests/test_fused_pull_checkers.py.
"""

from __future__ import annotations

import torch


def expected_slots(keys, shard_num, cap):
    """int64 [n]: the array-table slot of every key, -1 for a negative key
    (the reserved -1 among them) and for a slot at or beyond ``cap``."""
    s = torch.div(keys.clamp(min=0), shard_num, rounding_mode="floor")
    return torch.where((keys < 0) | (s >= cap), torch.full_like(s, -1), s)


def _rows_differ(a, b):
    if a.dim() == 1:
        return a != b
    if a.shape[1] == 0:
        return torch.zeros(a.shape[0], dtype=torch.bool)
    return (a.contiguous().view(torch.int32)
            != b.contiguous().view(torch.int32)).any(dim=1)


def duplicate_violations(keys, out):
    """``out`` [n, dim] of a pull of ``keys`` [n]."""
    n = keys.numel()
    uniq, inv = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64)
    first.scatter_reduce_(0, inv, torch.arange(n), reduce="amin")
    if bool(_rows_differ(out, out[first[inv]]).any()):
        return ["a duplicate's row differs from its first occurrence's"]
    return []


def table_violations(before, after, want, touched):
    """before / after / want: (weights [R, dim], state [R, sd], valid uint8
    [R]) snapshots; ``touched``: the slots >= 0 the batch names."""
    w0, s0, v0 = before
    w1, s1, v1 = after
    ww, ws, wv = want
    R = w0.shape[0]
    named = torch.zeros(R, dtype=torch.bool)
    named[touched] = True
    moved = _rows_differ(w1, w0) | _rows_differ(s1, s0)
    bad = []
    if bool((moved & (v0 != 0)).any()):
        bad.append("a row that was not new was written")
    if bool((moved & ~named).any()):
        bad.append("a row outside the batch changed")
    if bool((v1[named] == 0).any()):
        bad.append("valid left unset for a touched slot")
    if bool(((v1 != v0) & ~named).any()):
        bad.append("the bitmap changed outside the touched slots")
    fresh = named & (v0 == 0)
    if bool(((_rows_differ(w1, ww) | _rows_differ(s1, ws)) & fresh).any()):
        bad.append("a new row differs from the unfused pull's")
    if not torch.equal(v1, wv) and not bad:
        bad.append("the bitmap differs from the unfused pull's")
    return bad
