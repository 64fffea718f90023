#!/usr/bin/env python
"""DCN-v2 cross network: the HIP route (ops/csrc/cross.hip) against the
operator's torch route, in one process.

    python scripts/bench_dcn.py [--block 20 --blocks 15] [--out FILE.md]

Per embedding dim (9: d = 247, dp 256; 16: d = 429, dp 448), batch 4096,
F = 26, L = 3, native bf16, parallel structure:

  step  the captured training step (forward, fused BCE, backward, sparse
        commit, flat Adagrad). One model and one optimizer, captured twice:
        once on the HIP route, once with ``ops.dispatch._CROSS`` off (what
        ``OEAMD_CROSS=0`` selects at import), so both graphs hold the same
        weights and see the same batches.
  pair  forward + backward of the operator alone (logit form, fresh
        gradients), both routes as captured graphs on the same operands.
  bm    the two kernels alone at BM = 16 and 32 over M, the table behind
        the launcher's rule (eager launches between device events).

Timing is in alternating blocks: every round times each variant for
``--block`` replays between device events over ``--blocks`` rounds; reported
is the per-replay median and the p10-p90 spread over blocks. Needs a GPU."""

import argparse
import json
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(_HERE), _HERE]
from bench_dlrm import capture  # noqa: E402
from bench_multihot import summarize, time_blocks  # noqa: E402

B = 4096
N_BATCHES = 8
L = 3


def operands(M, d, device, seed=1):
    g = torch.Generator(device).manual_seed(seed)
    bf = torch.bfloat16
    dp = (d + 31) // 32 * 32

    def rn(*s, k=1.0):
        return (torch.randn(*s, device=device, generator=g) * k).to(bf)
    x0 = torch.nn.functional.pad(rn(M, d), (0, dp - d)).contiguous()
    return (x0, rn(L, d, d, k=d ** -0.5), rn(L, d, k=0.1),
            rn(d, k=d ** -0.5), rn(1),
            torch.randn(M, device=device, generator=g),
            torch.randn(M, device=device, generator=g))


def run_dim(dim, device, block, blocks, warmup):
    import openembedding_amd.context as cm
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DCN, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16
    from openembedding_amd.ops import dispatch
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    embed._tracked.clear()
    assert dispatch._CROSS, "run without OEAMD_CROSS=0"

    torch.manual_seed(1234)
    model = convert_mlp_bf16(DCN(dim=dim, cross_layers=L).to(device))
    assert model.fused_mlp and model.fused_cross
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.005), flatten_dense=True)
    gen = torch.Generator().manual_seed(0)
    batches = [tuple(t.to(device) for t in synthetic_batch(B, generator=gen))
               for _ in range(N_BATCHES)]
    static = tuple(t.clone() for t in batches[0])
    seed_one = torch.ones((), device=device)

    def step():
        opt.zero_grad(set_to_none=False)
        loss = dispatch.bce_with_logits(model(static[0], static[1]).float(),
                                        static[2])
        loss.backward(gradient=seed_one)
        opt.step()

    def on_torch_route(fn):
        dispatch._CROSS = False
        try:
            return fn()
        finally:
            dispatch._CROSS = True

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graphs = {"hip": capture(step),
              "torch": on_torch_route(lambda: capture(step))}

    def replay(graph):
        def run(i):
            for s, t in zip(static, batches[i % N_BATCHES]):
                s.copy_(t)
            graph.replay()
        return run

    # the operator alone, on operands of the step's shape
    d = 26 * dim + 13
    x0, W, b, wo, bo, partial, dout = operands(B, d, device)
    leaves = [t.requires_grad_() for t in (x0, W, b, wo, bo)]

    def pair():
        out = dispatch.cross_network(*leaves, partial=partial)
        torch.autograd.grad(out, leaves, dout)

    # faster and different is not faster
    got = dispatch.cross_network(*leaves, partial=partial).detach()
    want = on_torch_route(
        lambda: dispatch.cross_network(*leaves, partial=partial).detach())
    torch.testing.assert_close(got, want, rtol=2 ** -5, atol=2 ** -4)

    pairs = {"hip": capture(pair),
             "torch": on_torch_route(lambda: capture(pair))}
    res = {}
    for key, gs in (("step", {k: replay(v) for k, v in graphs.items()}),
                    ("pair", {k: (lambda i, v=v: v.replay())
                              for k, v in pairs.items()})):
        for i in range(warmup):
            for fn in gs.values():
                fn(i)
        torch.cuda.synchronize()
        res[key] = summarize(time_blocks(gs, batches, block, blocks))
        res[key]["torch_over_hip"] = (res[key]["torch"]["median_us"]
                                      / res[key]["hip"]["median_us"])
    return res


def bm_table(d, device, reps=200):
    """us per launch (best of 3 x reps) of each kernel at BM 16 / 32."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    rows = {}
    for M in (1024, 2048, 4096, 8192, 16384):
        x0, W, b, wo, bo, partial, dout = operands(M, d, device)
        dp = x0.shape[1]
        bufs = dispatch._cross_images(W, dp, True, ext)
        xs, us, qs = (torch.empty(L, M, dp, dtype=x0.dtype, device=device)
                      for _ in range(3))
        out, dx0 = torch.empty(M, device=device), torch.empty_like(x0)
        cell = {}
        for bm in (16, 32):
            fns = {
                "fwd": lambda: ext.cross_fwd(x0, bufs["w"], b, xs, us, wo,
                                             bo, partial, out, bm),
                "bwd": lambda: ext.cross_bwd(x0, us, bufs["wt"], b, dout,
                                             wo, None, qs, dx0, bm)}
            for name, fn in fns.items():
                best = float("inf")
                for _ in range(3):
                    fn()
                    t0, t1 = (torch.cuda.Event(enable_timing=True)
                              for _ in range(2))
                    t0.record()
                    for _ in range(reps):
                        fn()
                    t1.record()
                    torch.cuda.synchronize()
                    best = min(best, t0.elapsed_time(t1) * 1e3 / reps)
                cell[f"{name}{bm}"] = best
        cell["picked"] = int(ext.cross_bm(M))
        rows[M] = cell
    return rows


def to_markdown(results, tables, args):
    lines = [
        "# DCN-v2 cross network: HIP route vs the operator's torch route",
        "",
        f"`scripts/bench_dcn.py --block {args.block} --blocks {args.blocks}`"
        f" on {torch.cuda.get_device_name(0)}. Batch {B}, F = 26, L = {L}, "
        "native bf16, parallel structure. `step` is the captured training "
        "step, `pair` the captured forward + backward of the operator alone "
        "(fresh gradients); one process, the torch route selected as "
        "`OEAMD_CROSS=0` does. Median us per replay, p10-p90 over blocks.",
        "",
        "| dim | dp | what | HIP | torch | torch / HIP |",
        "|---|---|---|---|---|---|"]
    for dim, r in results.items():
        dp = (26 * dim + 13 + 31) // 32 * 32
        for key in ("step", "pair"):
            h, t = r[key]["hip"], r[key]["torch"]
            lines.append(
                f"| {dim} | {dp} | {key} | {h['median_us']:.1f} "
                f"({h['p10_us']:.1f}-{h['p90_us']:.1f}) | "
                f"{t['median_us']:.1f} ({t['p10_us']:.1f}-{t['p90_us']:.1f})"
                f" | {r[key]['torch_over_hip']:.2f} |")
    lines += ["", "Kernels alone, us per launch (best of 3 x 200 back-to-back "
              "launches), logit form with mirrors; `rule` is the launcher's "
              "choice.", ""]
    for dim, rows in tables.items():
        lines += [f"dim {dim}:", "",
                  "| M | fwd 16 | fwd 32 | bwd 16 | bwd 32 | rule |",
                  "|---|---|---|---|---|---|"]
        for M, c in rows.items():
            lines.append(f"| {M} | {c['fwd16']:.1f} | {c['fwd32']:.1f} | "
                         f"{c['bwd16']:.1f} | {c['bwd32']:.1f} | "
                         f"{c['picked']} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dims", type=int, nargs="+", default=[9, 16])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dcn.py needs a GPU"
    device = "cuda:0"
    results = {dim: run_dim(dim, device, args.block, args.blocks,
                            args.warmup) for dim in args.dims}
    tables = {dim: bm_table(26 * dim + 13, device) for dim in args.dims}
    md = to_markdown(results, tables, args)
    print(md)
    print(json.dumps({"results": results, "bm": tables}))
    if args.out:
        with open(args.out, "w") as f:
            f.write(md + "\n")


if __name__ == "__main__":
    main()
