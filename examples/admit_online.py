#!/usr/bin/env python3
"""Online learning with feature admission: on a long-tailed id stream most ids
occur once or twice and never again. With ``admission={"min_count": 3}`` an id
earns its row only after it was seen in three training steps; until then it
reads as a zero row and its gradient is dropped.

1. trains the same small model twice on the same Zipf-shaped stream, once
   with a plain hashed ``Embedding`` and once behind an admission filter of
   ``--min-count``, and compares the table sizes;
2. expires the rows that went stale (``expire_server_model``) and ages the
   filter (``age_admission_filters``), the pair that keeps table and sketch
   bounded on an endless stream;
3. prints the filter's statistics.

Run: python examples/admit_online.py [--min-count N] [--steps N]
"""

import argparse
import os as _os
import sys as _sys
import tempfile

import torch

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed

IDS, BATCH, DIM = 200_000, 512, 16


def stream(steps, seed=0):
    """Batches of ids with probability ~ 1 / (rank + 1), scattered over the
    int64 key space."""
    g = torch.Generator().manual_seed(seed)
    p = 1.0 / (torch.arange(IDS, dtype=torch.float64) + 1)
    for _ in range(steps):
        ranks = torch.multinomial(p, BATCH, replacement=True, generator=g)
        yield (ranks * 2654435761) % (1 << 40) + 1


def run(ctx, admission, steps):
    torch.manual_seed(0)
    emb = embed.Embedding(-1, DIM, admission=admission)
    head = torch.nn.Linear(DIM, 1).to(ctx.device)
    opt = embed.distributed_optimizer(torch.optim.Adagrad(
        list(emb.parameters()) + list(head.parameters()), lr=0.05))
    lossf = torch.nn.BCEWithLogitsLoss()

    def train(n, seed=0):
        for ids in stream(n, seed):
            ids = ids.to(ctx.device)
            labels = (ids % 2).to(torch.float32)
            opt.zero_grad()
            lossf(head(emb(ids)).squeeze(1), labels).backward()
            opt.step()

    train(steps)
    return emb, train


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--min-count", type=int, default=3)
    p.add_argument("--steps", type=int, default=40)
    args = p.parse_args()

    ctx = embed.get_context()
    embed.track_server_model_changes()      # expiry reads the row stamps
    plain, _ = run(ctx, None, args.steps)
    gated, train_gated = run(ctx, {"min_count": args.min_count,
                                   "width": 1 << 18}, args.steps)
    rows_plain = plain.variable.sharded.shard.num_rows
    shard = gated.variable.sharded.shard
    rows_gated = shard.num_rows
    st = shard.admission_stats()
    print(f"{args.steps} steps of {BATCH} ids: {rows_plain} rows without "
          f"admission, {rows_gated} with min_count={args.min_count}")
    print(f"filter: admitted {st['admitted']}, turned away "
          f"{st['turned_away']} sightings, sketch fill {st['fill']:.3f}")
    assert st["admitted"] == rows_gated
    assert rows_gated * 2 < rows_plain, (rows_gated, rows_plain)

    # the housekeeping pair of an endless stream: stale rows go, and the
    # counters halve so that ids of long ago have to earn their row again
    embed.save_server_model(tempfile.mkdtemp(prefix="oe_admit_"))
    train_gated(4, seed=1)                  # a new save interval
    gone = embed.expire_server_model(max_age=0)
    embed.age_admission_filters(1)
    st2 = shard.admission_stats()
    print(f"expired {gone['rows']} rows, aged the filter: fill "
          f"{st['fill']:.3f} -> {st2['fill']:.3f}, table at "
          f"{shard.num_rows} rows")
    assert st2["fill"] < st["fill"] and shard.num_rows < rows_gated
    print("admission kept the table small: OK")


if __name__ == "__main__":
    main()
