#!/usr/bin/env python3
"""Online learning with feature expiry: a table fed from a drifting id stream
gives the rows of ids that stopped occurring back, and its serving replica
follows through the tombstones of the delta checkpoints.

1. turns change tracking on, trains DeepFM on period 0 of the stream, writes
   a full dump (the base) and serves it;
2. per period: trains on that period's ids (the id window slides), drops the
   rows not seen for ``--max-age`` save intervals with
   ``expire_server_model``, writes a DELTA and applies it to the live
   replica over REST;
3. checks that the table stopped growing, that the replica shrank with it,
   and that it answers exactly like a fresh load of a new full dump.

Run: python examples/expire_online.py [--quantize int8|fp16] [--max-age N]
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

VOCAB, WINDOW, SLIDE = 1000, 300, 100


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quantize", choices=["int8", "fp16"], default=None)
    p.add_argument("--max-age", type=int, default=1)
    p.add_argument("--periods", type=int, default=5)
    args = p.parse_args()

    ctx = embed.get_context()
    embed.track_server_model_changes()      # expiry reads the row stamps
    torch.manual_seed(0)
    fv = [VOCAB] * 26
    model = DeepFM(field_vocabs=fv, dim=9).to(ctx.device)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01))
    lossf = torch.nn.BCEWithLogitsLoss()

    def train(period, steps=4):
        """The ids of a period lie in a window that slides with it."""
        for _ in range(steps):
            dense, sparse, labels = synthetic_batch(
                256, field_vocabs=fv, device=str(ctx.device))
            sparse = (sparse % WINDOW + SLIDE * period) % VOCAB
            opt.zero_grad()
            lossf(model(dense, sparse), labels).backward()
            opt.step()
        return sparse

    def table_rows():
        return sum(v.shard.num_rows for v in ctx.variables.values())

    train(0)
    base = tempfile.mkdtemp(prefix="oe_base_")
    embed.save_server_model(base)
    controller = ModelController(device=str(ctx.device))
    from fastapi.testclient import TestClient
    client = TestClient(make_app(controller))
    r = client.post("/models", json={"model_uri": base, "sign": "ctr",
                                     "quantize": args.quantize})
    assert r.status_code == 200, r.text
    print(f"serving the base at epoch {r.json()['epoch']}: "
          f"{table_rows()} rows")

    sizes = []
    for period in range(1, args.periods + 1):
        sparse = train(period)
        # between opt.step() and the next forward: no pull handle is live
        gone = embed.expire_server_model(max_age=args.max_age)
        delta = tempfile.mkdtemp(prefix="oe_delta_")
        info = embed.save_server_model_delta(delta)
        r = client.post("/models/ctr/deltas", json={"model_uri": delta})
        assert r.status_code == 200, r.text
        assert r.json().get("removed", 0) == gone["rows"], r.json()
        sizes.append(table_rows())
        print(f"period {period}: expired {gone['rows']} rows last written "
              f"before epoch {gone['before']}, delta of {info['rows']} rows, "
              f"table at {sizes[-1]} rows, replica at epoch "
              f"{r.json()['epoch']}")

    # the window slides, the table does not grow with the stream
    assert max(sizes[args.max_age:]) <= sizes[args.max_age] * 1.2, sizes
    served_rows = sum(v.shard.num_rows for v in
                      controller.manager.get("ctr").variables.values())
    assert served_rows == table_rows(), (served_rows, table_rows())

    # a fresh load of a new full dump is what the replica must equal
    full = tempfile.mkdtemp(prefix="oe_full_")
    embed.save_server_model(full)
    fresh = ModelController(device=str(ctx.device)).create_model(
        full, sign="fresh", quantize=args.quantize)
    emb = model.embedding
    live_ids = (sparse[:8] + emb.field_offsets).cpu()
    stale_ids = (torch.arange(8).unsqueeze(1) % WINDOW
                 + emb.field_offsets.cpu())           # period 0 only
    for ids, expired in ((live_ids, False), (stale_ids, True)):
        body = {"indices": ids.tolist()}
        for vid in sorted(fresh.variables):
            served = torch.tensor(client.post(
                f"/models/ctr/variables/{vid}/pull",
                json=body).json()["weights"])
            want = fresh.variables[vid].pull_weights(ids).cpu()
            assert torch.equal(served, want), "replica rows differ!"
            if expired:
                assert not served.any(), "an expired id still has a row"
    print("replica after expiry equals a fresh load: OK")


if __name__ == "__main__":
    main()
