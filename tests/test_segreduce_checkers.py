"""The reference side of the segmented-reduce GPU tests, tested without a
GPU: the index checker must accept a valid index and reject each wrong
result it exists for, and the torch form of reduce_by_index must equal a
plain index_add."""

import pytest
import torch

import segreduce_ref as sref
from openembedding_amd.ops import dispatch as ops

T = 4


def _case(seed=0, n=300, u_keys=40):
    g = torch.Generator().manual_seed(seed)
    keys = torch.randint(0, u_keys, (n,), generator=g)
    keys[::3] = 7                      # one long list
    _, inverse = torch.unique(keys, return_inverse=True)
    u = int(inverse.max()) + 1
    return g, inverse, u


def _index(seed=0):
    g, inverse, u = _case(seed)
    idx = [t.clone() for t in sref.build_index(inverse, u, T, g)]
    return inverse, u, idx


def _bad(inverse, u, idx):
    return sref.index_violations(inverse, u, *idx, T)


def _two_lists(idx, u, same_len=False):
    """Two different uids; with ``same_len`` of equal count >= 2."""
    cnt = idx[1][:u]
    for a in range(u):
        for b in range(a + 1, u):
            if same_len and not (cnt[a] == cnt[b] and cnt[a] >= 2):
                continue
            return a, b
    raise AssertionError("case has no such pair")


def test_valid_index_passes():
    for seed in range(3):
        inverse, u, idx = _index(seed)
        assert _bad(inverse, u, idx) == []
        assert int(idx[4]) >= 1 and int((idx[1][:u] <= T).sum()) >= 1


def test_empty_batch():
    e = torch.empty(0, dtype=torch.int64)
    idx = sref.build_index(e, 0, T)
    assert sref.index_violations(e, 0, *idx, T) == []


def test_rejects_overlapping_lists():
    inverse, u, idx = _index()
    a, b = _two_lists(idx, u, same_len=True)
    idx[0][b] = idx[0][a]              # b's list laid over a's
    bad = _bad(inverse, u, idx)
    assert any("overlap" in s for s in bad), bad


def test_rejects_element_under_another_uid():
    inverse, u, idx = _index()
    a, b = _two_lists(idx, u)
    pa, pb = int(idx[0][a]), int(idx[0][b])
    idx[2][[pa, pb]] = idx[2][[pb, pa]]
    bad = _bad(inverse, u, idx)
    assert bad == ["an element is filed under another uid"], bad


def test_rejects_missing_element():
    inverse, u, idx = _index()
    # the second element of a list of >= 2 replaced by a copy of the first:
    # same uid, so only the coverage properties can notice
    a = int((idx[1][:u] >= 2).nonzero()[0])
    p = int(idx[0][a])
    idx[2][p + 1] = idx[2][p]
    bad = _bad(inverse, u, idx)
    assert "an element is in no list" in bad, bad


def test_rejects_count_off_by_one():
    for delta in (-1, 1):
        inverse, u, idx = _index()
        a = int((idx[1][:u] >= 2).nonzero()[0])
        if delta > 0:   # keep the longer list inside [0, n)
            a = int(torch.argmin(idx[0][:u]))
        idx[1][a] += delta
        bad = _bad(inverse, u, idx)
        assert "seg_cnt != bincount(inverse)" in bad, (delta, bad)


def test_rejects_long_uid_missing():
    inverse, u, idx = _index()
    assert int(idx[4]) >= 1
    idx[4][0] -= 1                     # drop the last long uid
    bad = _bad(inverse, u, idx)
    assert bad == ["a long uid is missing from long_list"], bad


def test_rejects_short_uid_in_long_list():
    inverse, u, idx = _index()
    short = int((idx[1][:u] <= T).nonzero()[0])
    k = int(idx[4])
    idx[3][k] = short
    idx[4][0] = k + 1
    bad = _bad(inverse, u, idx)
    assert bad == ["long_list names a uid that is not long"], bad


def test_rejects_uid_twice_in_long_list():
    inverse, u, idx = _index()
    k = int(idx[4])
    idx[3][k] = idx[3][0]
    idx[4][0] = k + 1
    bad = _bad(inverse, u, idx)
    assert bad == ["a uid is in long_list twice"], bad


def test_rejects_out_of_range():
    inverse, u, idx = _index()
    idx[2][5] = inverse.numel()
    assert _bad(inverse, u, idx) == ["a perm entry outside [0, n)"]
    inverse, u, idx = _index()
    idx[0][3] = inverse.numel()
    assert _bad(inverse, u, idx) == ["a list leaves [0, n)"]


@pytest.mark.parametrize("dim", [1, 10, 65])
def test_torch_reduce_by_index_equals_index_add(dim):
    g, inverse, u = _case(seed=dim)
    n = inverse.numel()
    idx = sref.build_index(inverse, u, T, g)
    grads = torch.randint(-8, 9, (n, dim), generator=g).float()
    ugrads, counts = ops.reduce_by_index(idx, grads, u)
    want = torch.zeros(n, dim).index_add_(0, inverse, grads)
    assert ugrads.shape == (n, dim) and counts.shape == (n,)
    assert counts.dtype == torch.int64
    assert torch.equal(ugrads, want)
    assert torch.equal(counts, torch.bincount(inverse, minlength=n))
    assert not bool(ugrads[u:].any()) and not bool(counts[u:].any())
    # float64 goes the same way
    u64, _ = ops.reduce_by_index(idx, grads.double(), u)
    assert torch.equal(u64, want.double())


def test_sum_bound_holds_for_float32_index_add():
    g, inverse, u = _case(seed=9, n=4000, u_keys=30)
    n = inverse.numel()
    grads = torch.randn(n, 10, generator=g)
    ref64 = torch.zeros(n, 10, dtype=torch.float64).index_add_(
        0, inverse, grads.double())
    got32 = torch.zeros(n, 10).index_add_(0, inverse, grads)
    bound = sref.sum_bound(inverse, grads, u)
    assert bool(((got32.double() - ref64).abs() <= bound).all())
    # and it is no blanket: half a percent of a hot row's magnitude fails
    hot = int(torch.bincount(inverse).argmax())
    worse = got32.clone()
    worse[hot] *= 1.005
    assert not bool(((worse.double() - ref64).abs() <= bound).all())
