"""Read-only pooled lookup on the torch engine (no GPU): the oracle form
``VariableShard.pull_pooled_readonly`` against pooling the flat read-only
rows, EmbeddingBag evaluation against its training-mode forward, and the
guarantee that a lookup inserts nothing."""

import pytest
import torch

from openembedding_amd.core.variable import (HASH_VOCAB_THRESHOLD,
                                             VariableMeta, VariableShard)
from openembedding_amd.ops.dispatch import pool_rows

MODES = ["sum", "mean", "sqrtn"]
DIM = 5
VOCAB = 64
TAIL = 3
LENS = [0, 1, 4, 0, 7, 2, 0]            # empty first, in the middle, last


def _shard(hash_mode: bool) -> VariableShard:
    meta = VariableMeta(variable_id=3, embedding_dim=DIM,
                        vocabulary_size=(HASH_VOCAB_THRESHOLD if hash_mode
                                         else VOCAB))
    sh = VariableShard(meta)
    sh.set_initializer("uniform", minval=-1.0, maxval=1.0)
    sh.pull(torch.arange(0, VOCAB, 2, dtype=torch.int64))   # even keys live
    return sh


def _problem():
    """values with absent (odd) keys, a repeated key, a key shared by bags
    and a -1 tail behind offsets[-1]."""
    g = torch.Generator().manual_seed(1)
    nnz = sum(LENS)
    vals = torch.randint(0, VOCAB, (nnz,), dtype=torch.int64, generator=g)
    vals[::4] = 6
    vals[2:4] = vals[1]
    assert bool((vals % 2 == 1).any()) and bool((vals % 2 == 0).any())
    vals = torch.cat([vals, torch.full((TAIL,), -1, dtype=torch.int64)])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64),
                         torch.tensor(LENS).cumsum(0)])
    w = torch.randn(vals.numel(), generator=g)
    return vals, offsets, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hash_mode", [True, False])
def test_shard_equals_pooling_the_readonly_rows(hash_mode, mode, weighted):
    sh = _shard(hash_mode)
    vals, offsets, w = _problem()
    w = w if weighted else None
    n0 = sh.num_rows
    got = sh.pull_pooled_readonly(vals, offsets, mode, w)
    rows = sh.pull_readonly(vals)
    assert bool((rows[vals % 2 == 1] == 0).all())   # the misses are zeros
    want = pool_rows(rows, offsets, mode, weights=w)[0]
    assert got.shape == (len(LENS), DIM)
    assert torch.equal(got, want)
    assert bool((got[0] == 0).all()) and bool((got[-1] == 0).all())
    assert sh.num_rows == n0


def test_missed_elements_count_toward_the_bag_length():
    sh = _shard(True)
    vals = torch.tensor([2, 3, 5, 7], dtype=torch.int64)    # one hit in four
    offsets = torch.tensor([0, 4], dtype=torch.int64)
    got = sh.pull_pooled_readonly(vals, offsets, "mean")
    assert torch.equal(got[0], sh.pull_readonly(vals[:1])[0] / 4)


def test_unknown_mode_is_rejected():
    sh = _shard(True)
    vals, offsets, _ = _problem()
    with pytest.raises(ValueError):
        sh.pull_pooled_readonly(vals, offsets, "max")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hash_mode", [True, False])
def test_embedding_bag_no_grad_equals_training_forward(hash_mode, weighted):
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    get_context("cpu")
    emb = embed.EmbeddingBag(-1 if hash_mode else VOCAB, DIM, mode="mean")
    vals, offsets, w = _problem()
    vals = vals.clamp(min=0)[:-TAIL]    # the torch engine takes no -1 key
    w = w[:-TAIL]
    args = (vals, offsets) + ((w,) if weighted else ())
    emb(*args)                          # creates the rows
    train = emb(*args)
    assert train.requires_grad
    rows0 = emb.variable.sharded.shard.num_rows
    with torch.no_grad():
        ev = emb(*args)
        unseen = emb(vals + 10_000 if hash_mode else vals, offsets)
    assert not ev.requires_grad
    assert torch.equal(ev, train.detach())
    assert emb.variable.sharded.shard.num_rows == rows0     # nothing inserted
    if hash_mode:
        assert bool((unseen == 0).all())
