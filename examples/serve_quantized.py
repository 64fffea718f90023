#!/usr/bin/env python3
"""Serve one dump from fp32 and from int8 tables, side by side:

1. trains an EmbeddingBag + linear head a few steps on the CPU;
2. dumps the server model;
3. loads the dump twice into one serving controller — once as it is, once
   with ``"quantize": "int8"`` in the POST /models body, which packs every
   row into 8-bit codes with a per-row fp32 scale and offset at load time;
4. sends the same /pull and /pull_pooled requests to both models and prints
   the largest difference of the answers next to both tables' sizes.

Run: python examples/serve_quantized.py
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


def ragged_batch(n_bags, vocab, max_len, gen):
    lens = torch.randint(0, max_len + 1, (n_bags,), generator=gen)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    values = torch.randint(0, vocab, (int(offsets[-1]),), generator=gen)
    labels = torch.randint(0, 2, (n_bags,), generator=gen).float()
    return values, offsets, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bags", type=int, default=64)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--quantize", default="int8", choices=["int8", "fp16"])
    args = ap.parse_args()

    ctx = embed.get_context("cpu")
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    vocab = 2000
    bag = embed.EmbeddingBag(-1, args.dim, mode="mean")     # hash table
    bag.variable.set_initializer("uniform", minval=-0.1, maxval=0.1)
    head = torch.nn.Linear(args.dim, 1)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(head.parameters(), lr=0.05))
    lossf = torch.nn.BCEWithLogitsLoss()
    for _ in range(args.steps):
        values, offsets, labels = ragged_batch(args.bags, vocab, 12, gen)
        opt.zero_grad()
        loss = lossf(head(bag(values, offsets)).squeeze(1), labels)
        loss.backward()
        opt.step()
    print(f"trained: loss={loss.item():.4f}")

    uri = tempfile.mkdtemp(prefix="oe_quant_dump_")
    embed.save_server_model(uri)
    print(f"dumped to {uri}")

    from fastapi.testclient import TestClient
    client = TestClient(make_app(ModelController(device="cpu")))
    info = {}
    for sign, body in (("fp32", {}), ("packed", {"quantize": args.quantize})):
        r = client.post("/models", json={"model_uri": uri, "sign": sign,
                                         **body})
        assert r.status_code == 200, r.text
        info[sign] = r.json()["variables"][0]
        print(f"model {sign!r}: storage={info[sign]['storage']} "
              f"table_bytes={info[sign]['table_bytes']}")
    assert info["packed"]["storage"] == args.quantize
    bad = client.post("/models", json={"model_uri": uri, "sign": "x",
                                       "quantize": "int3"})
    assert bad.status_code == 422

    values, offsets, _ = ragged_batch(16, vocab, 12, gen)
    worst = 0.0
    for route, body, field in (
            ("pull", {"indices": values.tolist()}, "weights"),
            ("pull_pooled", {"values": values.tolist(),
                             "offsets": offsets.tolist(), "mode": "mean"},
             "pooled")):
        got = {}
        for sign in info:
            r = client.post(f"/models/{sign}/variables/0/{route}", json=body)
            assert r.status_code == 200, r.text
            got[sign] = torch.tensor(r.json()[field])
        diff = float((got["fp32"] - got["packed"]).abs().max())
        print(f"{route}: largest |fp32 - {args.quantize}| = {diff:.3e} "
              f"(largest |fp32| = {float(got['fp32'].abs().max()):.3e})")
        worst = max(worst, diff)
    rows = torch.tensor(client.post("/models/fp32/variables/0/pull",
                                    json={"indices": values.tolist()}
                                    ).json()["weights"])
    span = float((rows.amax(1) - rows.amin(1)).max())
    step = (span / 255 if args.quantize == "int8"     # fp16: an ulp of max
            else float(rows.abs().max()) * 2.0 ** -10)
    assert 0 < worst <= 0.51 * step + 1e-6, (worst, step)
    print(f"largest difference {worst:.3e} is within half a step "
          f"({step / 2:.3e}) of the widest row")
    print(f"table bytes: fp32 {info['fp32']['table_bytes']} -> "
          f"{args.quantize} {info['packed']['table_bytes']}")
    print("quantized serving: OK")


if __name__ == "__main__":
    main()
