"""DLRM dot interaction: the HIP kernels against the torch route.

    python scripts/bench_dlrm.py [--out profiles/dlrm_dot.md]

step  : the captured DLRM training step (forward, BCE, backward, sparse
        commit, flat Adagrad) at batch 4096, F = 26, bf16 MLPs, dim 16 and
        64. One model and one optimizer, captured twice: once with
        ``ops.dot_interact`` on k_dot_interact_fwd / k_dot_interact_bwd, once
        on its torch route (what ``OEAMD_DLRM_DOT=0`` selects at import; here
        the same switch is flipped around the second capture, so both graphs
        are of one build, one process and one set of weights).
pair  : the two kernels back to back (bf16 padded out, bf16 d_out) against
        the torch ops they replace (cat, rounding, bmm, triangle gather, cat,
        cast, pad, and autograd's way back), both as captured graphs on the
        same [4096, 26, dim] operands.

Method: everything is warmed up, then timed in alternating blocks of
``--block`` replays between device events over ``--blocks`` rounds;
reported is the per-replay median and the p10-p90 spread over blocks. Before
timing, the two routes' deep_in are compared at the timed size. Needs a GPU:
there is no CPU fallback for a timing."""

import argparse
import json
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(_HERE), _HERE]
from bench_multihot import summarize, time_blocks  # noqa: E402

B = 4096
N_BATCHES = 8


def capture(fn, warm=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def run_dim(dim, device, block, blocks, warmup):
    import openembedding_amd.context as cm
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DLRM, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16
    from openembedding_amd.ops import dispatch, require_hip
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    embed._tracked.clear()
    ext = require_hip()
    assert dispatch._DLRM_DOT, "run without OEAMD_DLRM_DOT=0"

    torch.manual_seed(1234)
    model = convert_mlp_bf16(DLRM(dim=dim).to(device))
    assert model.fused_mlp
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

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graphs = {"hip": capture(step)}
    dispatch._DLRM_DOT = False
    try:
        for _ in range(3):
            step()
        graphs["torch"] = capture(step)
    finally:
        dispatch._DLRM_DOT = True

    def replay(graph):
        def run(i):
            for s, t in zip(static, batches[i % N_BATCHES]):
                s.copy_(t)
            graph.replay()
        return run

    # the operator alone, on operands of the step's shape
    g = torch.Generator(device).manual_seed(1)
    e = torch.randn(B, 26, dim, device=device, generator=g).requires_grad_()
    x = torch.randn(B, dim, device=device, generator=g).requires_grad_()
    d_out = torch.randn(ext.dot_interact_fwd(e, x, True, True).shape,
                        device=device, generator=g).to(torch.bfloat16)

    def hip_pair():
        ext.dot_interact_fwd(e, x, True, True)
        ext.dot_interact_bwd(e, x, d_out, True)

    def torch_pair():
        out = dispatch._dot_interact_torch(e, x, True, True)
        torch.autograd.grad(out, [e, x], d_out)

    # faster and different is not faster: one bf16 ulp of the larger dots
    got = ext.dot_interact_fwd(e, x, True, True).float()
    want = dispatch._dot_interact_torch(e, x, True, True).detach().float()
    torch.testing.assert_close(got, want, rtol=2 ** -7, atol=1e-6)

    pairs = {"hip": capture(hip_pair), "torch": capture(torch_pair)}
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


def to_markdown(results, args):
    cell = lambda r: (f"{r['median_us']:.1f} ({r['p10_us']:.1f}-"  # noqa: E731
                      f"{r['p90_us']:.1f})")
    lines = [
        "# DLRM dot interaction: HIP kernels vs the torch route (MI355X)",
        "",
        f"`scripts/bench_dlrm.py`: batch {B}, F = 26, bf16 MLPs, Criteo "
        "cardinalities, Adagrad. `step` is the captured training step with "
        "`ops.dot_interact` on the HIP kernels or on its torch route "
        "(`OEAMD_DLRM_DOT=0`), one model captured twice; `pair` is forward "
        "+ backward of the operator alone (bf16 padded out), both captured. "
        f"Device events around alternating blocks of {args.block} replays, "
        f"{args.blocks} blocks per path after {args.warmup} warm-up "
        "replays, one process; median (p10-p90) in microseconds.",
        "",
        "| dim | what | HIP | torch | torch / HIP |",
        "|---|---|---|---|---|",
    ]
    for dim, r in results.items():
        for key in ("step", "pair"):
            lines.append(f"| {dim} | {key} | {cell(r[key]['hip'])} | "
                         f"{cell(r[key]['torch'])} | "
                         f"{r[key]['torch_over_hip']:.2f}x |")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dims", default="16,64")
    # 200 replays: 80-160 ms per timed block of the step, 1-2 s per path
    p.add_argument("--block", type=int, default=200)
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--out", default="")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dlrm.py needs a GPU")
    device = torch.device("cuda:0")
    results = {}
    for dim in (int(d) for d in args.dims.split(",")):
        results[dim] = run_dim(dim, device, args.block, args.blocks,
                               args.warmup)
        print(json.dumps({"dim": dim, **results[dim]}), flush=True)
    md = to_markdown(results, args)
    print(md)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(md)


if __name__ == "__main__":
    main()
