"""Reference side of tests/test_gpu_fused_apply.py: plain torch, no GPU.

  - ``table_violations``: holds a table after ``reduce_apply_by_index``
    against the table the two launches (``reduce_by_index`` then
    ``apply_optimizer``) leave on a clone, row by row and bit by bit, and
    names what went wrong: a row that no live uid names changed, a live row
    was left as it was, a live row holds something else (a sum applied
    twice, a wrong sum, a wrong count);
  - ``pair_keys``: keys whose lists hold at most two elements, so that a
    float32 sum of random gradients does not depend on the order;
  - ``seq_child_main``: the child process of the switch test.

The checker is itself tested in tests/test_fused_apply_checkers.py.
"""

from __future__ import annotations

import torch

import sparse_core_ref as ref


def _row_bits_differ(a, b):
    """[R] bool: row r of ``a`` and ``b`` (float32 [R, k]) differ bitwise."""
    if a.shape[1] == 0:
        return torch.zeros(a.shape[0], dtype=torch.bool)
    return (a.contiguous().view(torch.int32)
            != b.contiguous().view(torch.int32)).any(dim=1)


def table_violations(w0, s0, got_w, got_s, want_w, want_s, slots, live):
    """(w0, s0): the table before the step; got: after the fused launch;
    want: after the two launches on a clone; ``slots`` int64 [n] with -1
    entries, ``live`` the unique count. Returns the violated properties
    (empty = the tables agree)."""
    bad = []
    R = w0.shape[0]
    keep = ref.untouched_rows(R, slots, live)
    moved = _row_bits_differ(got_w, w0) | _row_bits_differ(got_s, s0)
    if bool((moved & keep).any()):
        bad.append("a row that no live uid names changed")
    differs = (_row_bits_differ(got_w, want_w)
               | _row_bits_differ(got_s, want_s)) & ~keep
    stepped = (_row_bits_differ(want_w, w0)
               | _row_bits_differ(want_s, s0)) & ~keep
    if bool((differs & ~moved & stepped).any()):
        bad.append("a live row was not applied")
    if bool((differs & moved).any()):
        bad.append("a live row differs from the two-launch result")
    return bad


def pair_keys(m, g):
    """m distinct keys, the first m // 2 of them twice, shuffled."""
    keys = torch.cat([torch.arange(m), torch.arange(m // 2)]) * 7919 + 3
    return keys[torch.randperm(keys.numel(), generator=g)].to(torch.int64)


def seq_child_main(out_path):
    """Entry of the child process of the switch test (OEAMD_FUSED_PULL=0
    and OEAMD_FUSED_APPLY=0): the eager sequence of segreduce_ref for both
    table kinds on the unfused launches."""
    import segreduce_ref as sref
    from openembedding_amd.parallel import sharded
    assert sharded._FUSED_APPLY is False and sharded._FUSED_PULL is False
    assert sharded._SEG_REDUCE is True
    out = {}
    for hash_mode in (False, True):
        table, h = sref.seq_eager_table("cuda:0", hash_mode)
        assert h.index is not None
        out[hash_mode] = table
    sref.seq_reset()
    torch.save(out, out_path)
