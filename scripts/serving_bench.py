#!/usr/bin/env python3
"""Serving read-path microbenchmark: batched pulls/s from a loaded model
(GPU HIP tables or CPU), the serving-side analogue of the training bench.

Without arguments: the flat pull of a briefly trained DeepFM (dim 9).

With ``--quantize int8|fp16``: the same keys are served from an fp32 table
and from a quantized table of ``--rows`` random rows of ``--dim`` columns,
alternating the two in one process, flat (``pull_weights``) and pooled
(``pull_pooled``-shaped bags straight at the shard, so that host-side
validation is not what is timed). Every call is timed by itself (host clock
around a device synchronise); reported are the median with p10-p90, the
pulls/s of the median and each table's ``table_bytes``. One JSON line per
route and storage goes to stdout."""

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def deepfm_flat():
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DeepFM, synthetic_batch
    from openembedding_amd.serving import ModelController

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    torch.manual_seed(0)
    model = DeepFM(dim=9).to(dev)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01))
    lossf = torch.nn.BCEWithLogitsLoss()
    for _ in range(3):
        dense, sparse, labels = synthetic_batch(4096, device=dev)
        opt.zero_grad()
        loss = lossf(model(dense, sparse), labels)
        loss.backward()
        opt.step()
    uri = tempfile.mkdtemp(prefix="oe_srv_bench_")
    embed.save_server_model(uri)
    ctx = embed.get_context()
    sign = f"{ctx.model_uuid}-{ctx.model_version}"
    c = ModelController(device=dev)
    c.create_model(uri)
    var = c.manager.find_model_variable(sign, 0)

    batch, steps, warmup = 4096, 200, 20
    emb = model.embedding
    gen = torch.Generator().manual_seed(9)
    probes = []
    for _ in range(8):
        _, sp, _ = synthetic_batch(batch, generator=gen)
        probes.append((sp.to(dev) + emb.field_offsets))
    for i in range(warmup):
        var.pull_weights(probes[i % 8])
    if dev.startswith("cuda"):
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        var.pull_weights(probes[i % 8])
    if dev.startswith("cuda"):
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = batch * 26
    print(f"serving pull: {dev} batch {batch}x26 keys: "
          f"{steps / dt:,.0f} pulls/s, {steps * n / dt / 1e6:,.1f}M "
          f"keys/s, {dt / steps * 1e6:.0f} us/pull "
          f"(shard={type(var.shard).__name__})")


def _quantiles(ts):
    t = torch.tensor(ts, dtype=torch.float64) * 1e6
    q = torch.quantile(t, torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64))
    return [float(v) for v in q]


def quantized(args):
    from openembedding_amd.core.quantized import QuantizedShard
    from openembedding_amd.core.variable import VariableMeta, VariableShard
    from openembedding_amd.serving import ServedVariable

    dev = args.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    cuda = dev.startswith("cuda")
    meta = VariableMeta(variable_id=0, embedding_dim=args.dim)   # hash table
    if cuda:
        from openembedding_amd.core.variable_gpu import HipVariableShard
        plain = HipVariableShard(meta, device=dev)
    else:
        plain = VariableShard(meta, device=dev)
    packed = QuantizedShard(meta, args.quantize, device=dev)
    if cuda:
        plain.reserve_rows(args.rows)
    packed.reserve_rows(args.rows)
    gen = torch.Generator().manual_seed(0)
    blk = 1 << 16
    for s in range(0, args.rows, blk):
        n = min(blk, args.rows - s)
        keys = torch.arange(s, s + n, dtype=torch.int64) * 2654435761 + 7
        rows = torch.randn(n, args.dim, generator=gen) * 0.05
        plain.import_rows(keys.to(dev), rows.to(dev))
        packed.import_rows(keys.to(dev), rows.to(dev))
    tables = {"fp32": ServedVariable(plain), args.quantize:
              ServedVariable(packed)}

    # 8 request batches; one key in 16 is absent from the table
    flat, bags = [], []
    for _ in range(8):
        ids = torch.randint(0, args.rows + args.rows // 16,
                            (args.batch * args.bag,), generator=gen)
        keys = (ids * 2654435761 + 7).to(dev)
        offsets = (torch.arange(args.batch + 1) * args.bag).to(dev)
        flat.append(keys[:args.batch * min(26, args.bag)].contiguous())
        bags.append((keys, offsets))
    routes = {
        "flat": lambda v, i: v.shard.pull_readonly(flat[i % 8]),
        "pooled": lambda v, i: v.shard.pull_pooled_readonly(
            *bags[i % 8], "mean"),
    }

    def sync():
        if cuda:
            torch.cuda.synchronize()

    print(f"# {dev} rows={args.rows} dim={args.dim} flat batch "
          f"{args.batch}x26 keys, pooled {args.batch} bags x {args.bag} "
          f"keys, {args.steps} timed calls each after {args.warmup} warm-up")
    for route, call in routes.items():
        times = {name: [] for name in tables}
        for i in range(args.warmup + args.steps):
            for name, var in tables.items():    # alternate the storages
                sync()
                t0 = time.perf_counter()
                call(var, i)
                sync()
                if i >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        a = routes[route](tables["fp32"], 0)
        b = routes[route](tables[args.quantize], 0)
        worst = float((a - b).abs().max())
        for name, var in tables.items():
            p10, p50, p90 = _quantiles(times[name])
            print(json.dumps({
                "route": route, "storage": name, "dim": args.dim,
                "rows": args.rows, "pulls_per_s": round(1e6 / p50, 1),
                "us_per_pull_median": round(p50, 1),
                "us_per_pull_p10": round(p10, 1),
                "us_per_pull_p90": round(p90, 1),
                "table_bytes": var.table_bytes,
                "max_abs_diff_vs_fp32": worst if name != "fp32" else 0.0,
                "shard": type(var.shard).__name__}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--quantize", choices=["int8", "fp16"], default=None,
                    help="compare a quantized table with the fp32 table")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--bag", type=int, default=32,
                    help="keys per bag of the pooled route")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--device", default=None)
    args = ap.parse_args()
    if args.quantize is None:
        deepfm_flat()
    else:
        quantized(args)


if __name__ == "__main__":
    main()
