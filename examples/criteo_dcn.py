#!/usr/bin/env python3
"""Train DCN-v2 on Criteo-shaped synthetic data.

The cross network runs as ``ops.cross_network``: with ``--bf16`` on a GPU
all cross layers are one HIP launch each way (ops/csrc/cross.hip), else
torch ops.

Single GPU / CPU:
    python examples/criteo_dcn.py --steps 100 [--structure stacked] [--bf16]
"""

import argparse
import time

import torch

import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(
    _os.path.abspath(__file__))))  # run from a source checkout

import openembedding_amd.torch as embed
from openembedding_amd.models import DCN, synthetic_batch
from openembedding_amd.models.ctr import convert_mlp_bf16


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--structure", default="parallel",
                   choices=["parallel", "stacked"])
    p.add_argument("--cross-layers", type=int, default=3)
    p.add_argument("--dim", type=int, default=9)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--lr", type=float, default=0.005)
    p.add_argument("--bf16", action="store_true",
                   help="native-bf16 towers: fused MLP and cross kernels")
    args = p.parse_args()

    ctx = embed.get_context()
    torch.manual_seed(1234)
    model = DCN(dim=args.dim, cross_layers=args.cross_layers,
                structure=args.structure).to(ctx.device)
    if args.bf16:
        model = convert_mlp_bf16(model)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=args.lr))
    lossf = torch.nn.BCEWithLogitsLoss()
    gen = torch.Generator().manual_seed(1 + ctx.rank)

    t0 = time.perf_counter()
    for step in range(args.steps):
        dense, sparse, labels = (t.to(ctx.device) for t in synthetic_batch(
            args.batch, generator=gen))
        opt.zero_grad()
        loss = lossf(model(dense, sparse), labels)
        loss.backward()
        opt.step()
        if ctx.rank == 0 and (step + 1) % 20 == 0:
            sps = (args.batch * ctx.world_size * (step + 1)
                   / (time.perf_counter() - t0))
            print(f"step {step + 1}: loss={loss.item():.4f} "
                  f"{sps:,.0f} samples/s")
    if ctx.rank == 0:
        print(f"done: {args.steps} steps, final loss={loss.item():.4f}")


if __name__ == "__main__":
    main()
