#!/usr/bin/env python3
"""Attention pooling over a behaviour sequence: a weighted ``EmbeddingBag``.

A "recently viewed items" field is a ragged list of ids per sample. Instead
of a plain mean, each element gets a LEARNED weight — here a sigmoid over a
small ``nn.Linear`` of a per-element feature (dwell time, recency), the
DIN-style attention pool — and the bag is the weighted mean of its rows:

    out[b] = sum_j w_j * row(values[j]) / sum_j w_j

``per_sample_weights`` pools inside the pull like the unweighted bag, so the
[nnz, dim] rows never exist, and because the weights require a gradient the
backward also returns d loss / d w, which trains the gate. Data weights
(TF-IDF and the like) are the same call with a tensor that needs no
gradient.
"""

import torch
import torch.nn as nn

import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed

BATCH, DIM, VOCAB, CAPACITY, NFEAT = 64, 8, 10_000, 64 * 12, 2


class AttentionPooled(nn.Module):
    def __init__(self):
        super().__init__()
        self.items = embed.EmbeddingBag(VOCAB, DIM, mode="mean")
        self.gate = nn.Linear(NFEAT, 1)
        self.head = nn.Linear(DIM, 1)

    def forward(self, values, offsets, feats):
        w = torch.sigmoid(self.gate(feats)).squeeze(-1)     # [CAPACITY]
        pooled = self.items(values, offsets, per_sample_weights=w)
        return self.head(pooled).squeeze(-1)


def ragged_batch(g, device):
    """BATCH item lists (0..11 items each) in a fixed-capacity buffer padded
    with the reserved key -1, plus one feature vector per element."""
    lens = torch.randint(0, 12, (BATCH,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    nnz = int(offsets[-1])
    values = torch.full((CAPACITY,), -1, dtype=torch.int64)
    values[:nnz] = torch.randint(0, VOCAB, (nnz,), generator=g)
    feats = torch.randn(CAPACITY, NFEAT, generator=g)
    # the label depends on the first item, so there is something to learn
    first = values[offsets[:-1].clamp(max=CAPACITY - 1)]
    labels = ((lens > 0) & (first % 2 == 0)).float()
    return (values.to(device), offsets.to(device), feats.to(device),
            labels.to(device))


def main():
    ctx = embed.get_context()
    torch.manual_seed(0)
    model = AttentionPooled().to(ctx.device)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.05))
    lossf = nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(0)
    for step in range(20):
        values, offsets, feats, labels = ragged_batch(g, ctx.device)
        opt.zero_grad()
        loss = lossf(model(values, offsets, feats), labels)
        loss.backward()
        gate_grad = model.gate.weight.grad.norm().item()
        opt.step()
        if ctx.rank == 0 and (step + 1) % 5 == 0:
            print(f"step {step + 1}: loss={loss.item():.4f} "
                  f"gate weight grad norm={gate_grad:.3e}")
    assert gate_grad > 0, "the gate received no gradient"
    if ctx.rank == 0:
        rows = model.items.variable.sharded.shard.num_rows
        print(f"item rows materialized: {rows}")


if __name__ == "__main__":
    main()
