#!/usr/bin/env python3
"""Online learning: keep a live serving model fresh with delta checkpoints.

1. turns change tracking on and trains DeepFM a few steps;
2. writes a full dump (the base) and serves it;
3. trains on, then writes a DELTA: only the rows those steps changed;
4. applies the delta to the live model over REST, in place;
5. checks the updated model answers exactly like a fresh load of a new full
   dump, and like the trainer's own table.

Run: python examples/online_update.py [--quantize int8|fp16]
"""

import argparse
import os as _os
import sys as _sys
import tempfile

import torch

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed
from openembedding_amd.models import DeepFM, synthetic_batch
from openembedding_amd.serving import ModelController, make_app


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quantize", choices=["int8", "fp16"], default=None)
    args = p.parse_args()

    ctx = embed.get_context()
    embed.track_server_model_changes()      # before the variables train
    torch.manual_seed(0)
    fv = [1000] * 26
    model = DeepFM(field_vocabs=fv, dim=9).to(ctx.device)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01))
    lossf = torch.nn.BCEWithLogitsLoss()

    def train(steps):
        for _ in range(steps):
            dense, sparse, labels = synthetic_batch(
                256, field_vocabs=fv, device=str(ctx.device))
            opt.zero_grad()
            lossf(model(dense, sparse), labels).backward()
            opt.step()
        return sparse

    train(5)
    base = tempfile.mkdtemp(prefix="oe_base_")
    embed.save_server_model(base)

    controller = ModelController(device=str(ctx.device))
    from fastapi.testclient import TestClient
    client = TestClient(make_app(controller))
    r = client.post("/models", json={"model_uri": base, "sign": "ctr",
                                     "quantize": args.quantize})
    assert r.status_code == 200, r.text
    print(f"serving the base at epoch {r.json()['epoch']}")

    sparse = train(3)
    delta = tempfile.mkdtemp(prefix="oe_delta_")
    info = embed.save_server_model_delta(delta)
    total = sum(v.shard.num_rows for v in ctx.variables.values())
    print(f"delta of epoch {info['epoch']}: {info['rows']} of {total} rows")
    assert 0 < info["rows"] < total

    r = client.post("/models/ctr/deltas", json={"model_uri": delta})
    assert r.status_code == 200, r.text
    print(f"live model now at epoch {r.json()['epoch']}")

    # a fresh load of a new full dump is what the update must equal
    full = tempfile.mkdtemp(prefix="oe_full_")
    embed.save_server_model(full)
    fresh = ModelController(device=str(ctx.device)).create_model(
        full, sign="fresh", quantize=args.quantize)
    emb = model.embedding
    probe = (sparse[:8] + emb.field_offsets).cpu()
    body = {"indices": probe.tolist()}
    for vid in sorted(fresh.variables):
        served = torch.tensor(client.post(
            f"/models/ctr/variables/{vid}/pull", json=body).json()["weights"])
        want = fresh.variables[vid].pull_weights(probe).cpu()
        assert torch.equal(served, want), "updated rows differ!"
    if args.quantize is None:
        live = emb.variable.sparse_read(probe.to(ctx.device)).cpu()
        vid = emb.variable.sharded.variable_id
        assert torch.equal(fresh.variables[vid].pull_weights(probe).cpu(),
                           live)
    print("updated model equals a fresh load: OK")


if __name__ == "__main__":
    main()
