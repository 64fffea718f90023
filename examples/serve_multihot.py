#!/usr/bin/env python3
"""Train a multi-hot (EmbeddingBag) model -> dump -> serve pooled lookups:

1. trains a weighted-mean EmbeddingBag + linear head a few steps on
   synthetic ragged data;
2. dumps the server model and loads it into the serving ModelController;
3. asks the replica for POOLED rows — POST .../pull_pooled with the ragged
   ids, the row splits, the combiner and the per-sample weights — so the
   client receives [B, dim] floats instead of fetching nnz rows over
   ``/pull`` and redoing the combiner itself;
4. checks the served pooled rows equal the live model's evaluation forward.

Run: python examples/serve_multihot.py
"""

import argparse
import tempfile

import torch

import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed
from openembedding_amd.serving import ModelController, make_app


def ragged_batch(n_bags, vocab, max_len, gen, device):
    lens = torch.randint(0, max_len + 1, (n_bags,), generator=gen)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    nnz = int(offsets[-1])
    values = torch.randint(0, vocab, (nnz,), generator=gen)
    weights = torch.rand(nnz, generator=gen) + 0.5
    labels = torch.randint(0, 2, (n_bags,), generator=gen).float()
    return (values.to(device), offsets.to(device), weights.to(device),
            labels.to(device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bags", type=int, default=64)
    ap.add_argument("--dim", type=int, default=8)
    args = ap.parse_args()

    ctx = embed.get_context()
    dev = str(ctx.device)
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    vocab = 500
    bag = embed.EmbeddingBag(-1, args.dim, mode="mean")     # hash table
    head = torch.nn.Linear(args.dim, 1).to(ctx.device)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(head.parameters(), lr=0.05))
    lossf = torch.nn.BCEWithLogitsLoss()
    for _ in range(args.steps):
        values, offsets, weights, labels = ragged_batch(
            args.bags, vocab, 12, gen, dev)
        opt.zero_grad()
        pooled = bag(values, offsets, per_sample_weights=weights)
        loss = lossf(head(pooled).squeeze(1), labels)
        loss.backward()
        opt.step()
    print(f"trained: loss={loss.item():.4f}")

    uri = tempfile.mkdtemp(prefix="oe_bag_dump_")
    embed.save_server_model(uri)
    sign = f"{ctx.model_uuid}-{ctx.model_version}"
    print(f"dumped to {uri} sign={sign}")

    controller = ModelController(device=dev)
    controller.create_model(uri)
    from fastapi.testclient import TestClient
    client = TestClient(make_app(controller))

    # a query with ids the model never saw: they pool as zero rows
    values, offsets, weights, _ = ragged_batch(8, 2 * vocab, 12, gen, dev)
    bag.eval()
    with torch.no_grad():
        live = bag(values, offsets, per_sample_weights=weights)
    r = client.post(f"/models/{sign}/variables/0/pull_pooled",
                    json={"values": values.cpu().tolist(),
                          "offsets": offsets.cpu().tolist(),
                          "mode": "mean",
                          "per_sample_weights": weights.cpu().tolist()})
    assert r.status_code == 200, r.text
    served = torch.tensor(r.json()["pooled"], device=live.device)
    print(f"pooled reply: {tuple(served.shape)} for nnz={values.numel()}")
    assert torch.allclose(live, served, atol=1e-6), "served pooled rows differ!"

    # malformed bags are refused before any lookup runs
    bad = client.post(f"/models/{sign}/variables/0/pull_pooled",
                      json={"values": [1, 2, 3], "offsets": [0, 2, 1]})
    assert bad.status_code == 422
    print("pooled serving matches evaluation: OK")


if __name__ == "__main__":
    main()
