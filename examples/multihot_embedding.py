#!/usr/bin/env python3
"""A multi-hot (variable-length) categorical field with ``EmbeddingBag``.

CTR models routinely carry fields such as "tags" or "recently viewed items":
a ragged list of ids per sample, pooled into one vector with a sum or mean
combiner (the reference took these as ``tf.RaggedTensor`` in sparse_read).
``EmbeddingBag`` takes the ragged batch as flat ``values`` plus ``offsets``
row splits and pools inside the pull, so neither the [nnz, dim] rows nor
their gradient are ever materialised.

The batch below uses a FIXED ``values`` capacity padded with the reserved
key -1 — the shape a hipGraph-captured train step needs.
"""

import torch
import torch.nn as nn

import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed

BATCH, DIM, VOCAB, CAPACITY = 64, 8, 10_000, 64 * 12


class TagModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.tags = embed.EmbeddingBag(VOCAB, DIM, mode="mean")
        self.head = nn.Linear(DIM, 1)

    def forward(self, values, offsets):
        return self.head(self.tags(values, offsets)).squeeze(-1)


def ragged_batch(g, device):
    """A batch of BATCH tag lists (0..11 tags each; some are empty)."""
    lens = torch.randint(0, 12, (BATCH,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    nnz = int(offsets[-1])
    values = torch.full((CAPACITY,), -1, dtype=torch.int64)   # -1 = padding
    values[:nnz] = torch.randint(0, VOCAB, (nnz,), generator=g)
    # the label depends on the tags, so there is something to learn
    first = values[offsets[:-1].clamp(max=CAPACITY - 1)]
    labels = ((lens > 0) & (first % 2 == 0)).float()
    return values.to(device), offsets.to(device), labels.to(device)


def main():
    ctx = embed.get_context()
    torch.manual_seed(0)
    model = TagModel().to(ctx.device)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.05))
    lossf = nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(0)
    for step in range(20):
        values, offsets, labels = ragged_batch(g, ctx.device)
        opt.zero_grad()
        loss = lossf(model(values, offsets), labels)
        loss.backward()
        opt.step()
        if ctx.rank == 0 and (step + 1) % 5 == 0:
            print(f"step {step + 1}: loss={loss.item():.4f}")
    with torch.no_grad():       # read-only pooled lookup (serving-style)
        values, offsets, _ = ragged_batch(g, ctx.device)
        pooled = model.tags(values, offsets)
    if ctx.rank == 0:
        rows = model.tags.variable.sharded.shard.num_rows
        print(f"pooled {tuple(pooled.shape)}; tag rows materialized: {rows}")


if __name__ == "__main__":
    main()
