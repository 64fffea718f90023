#!/usr/bin/env python
"""DCN-v2 low-rank cross network (ops/csrc/cross_lr.hip), dp = 256, L = 3:

  kern  k_cross_lr_fwd / bwd alone at BM = 16, 32 and the launcher's choice
        (logit form with mirrors), next to the full-rank k_cross_fwd / bwd
        on W = U V;
  pair  forward + backward of ``ops.cross_network_lr`` (fresh gradients of
        every parameter, weight packs and library wgrads included) on the
        HIP route and on the torch route (``ops.dispatch._CROSS_LR`` off:
        what ``OEAMD_CROSS_LR=0`` selects at import), both as captured
        graphs on the same operands.

    python scripts/bench_dcn_lr.py [--reps 200 --blocks 7] [--out FILE.md]

us per call: median over ``--blocks`` blocks of ``--reps`` back-to-back
calls between device events, after one warm-up block. The clocks the run
starts under are read with rocm-smi and printed. Needs a GPU."""

import argparse
import os
import statistics
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(_HERE), _HERE]
from bench_dlrm import capture  # noqa: E402

L, D = 3, 247


def timed(fn, reps, blocks):
    meds = []
    for i in range(blocks + 1):
        t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        if i:
            meds.append(t0.elapsed_time(t1) * 1e3 / reps)
    return statistics.median(meds)


def row(M, r, reps, blocks, device="cuda:0"):
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    bf = torch.bfloat16
    g = torch.Generator(device).manual_seed(M + r)
    rn = lambda *s, k=1.0: (torch.randn(  # noqa: E731
        *s, device=device, generator=g) * k).to(bf)
    dp, rp = (D + 31) // 32 * 32, (r + 31) // 32 * 32
    x0 = torch.nn.functional.pad(rn(M, D), (0, dp - D)).contiguous()
    U, V, b = rn(L, D, r, k=r ** -0.5), rn(L, r, D, k=D ** -0.5), rn(L, D, k=.1)
    wo, bo = rn(D, k=D ** -0.5), rn(1)
    partial, dout = (torch.randn(M, device=device, generator=g)
                     for _ in range(2))
    W = (U.float() @ V.float()).to(bf)
    lb = dispatch._cross_lr_images(U, V, dp, rp, True, ext)
    fb = dispatch._cross_images(W, dp, True, ext)
    new = lambda n: torch.empty(L, M, n, dtype=bf, device=device)  # noqa: E731
    xs, us, qs, ps, ss = new(dp), new(dp), new(dp), new(rp), new(rp)
    out, dx0 = torch.empty(M, device=device), torch.empty_like(x0)
    res = {}
    for bm in (16, 32, 0):
        res[f"lr_fwd{bm}"] = timed(lambda: ext.cross_lr_fwd(
            x0, lb["v"], lb["u"], b, r, xs, us, ps, wo, bo, partial, out,
            bm), reps, blocks)
        res[f"lr_bwd{bm}"] = timed(lambda: ext.cross_lr_bwd(
            x0, us, lb["ut"], lb["vt"], b, r, dout, wo, None, qs, ss, dx0,
            bm), reps, blocks)
    res["full_fwd"] = timed(lambda: ext.cross_fwd(
        x0, fb["w"], b, xs, us, wo, bo, partial, out, 0), reps, blocks)
    res["full_bwd"] = timed(lambda: ext.cross_bwd(
        x0, us, fb["wt"], b, dout, wo, None, qs, dx0, 0), reps, blocks)
    res["rule"] = int(ext.cross_lr_bm(M))
    leaves = [t.requires_grad_() for t in (x0, U, V, b, wo, bo)]

    def pair():
        o = dispatch.cross_network_lr(*leaves, partial=partial)
        torch.autograd.grad(o, leaves, dout)
    graphs = {"pair_hip": capture(pair)}
    dispatch._CROSS_LR = False
    try:
        graphs["pair_torch"] = capture(pair)
    finally:
        dispatch._CROSS_LR = True
    for key, graph in graphs.items():
        res[key] = timed(graph.replay, reps // 4, blocks)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dcn_lr.py needs a GPU"
    keys = ["lr_fwd16", "lr_fwd32", "lr_fwd0", "lr_bwd16", "lr_bwd32",
            "lr_bwd0", "rule", "full_fwd", "full_bwd", "pair_hip",
            "pair_torch"]
    try:
        clk = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"],
                             capture_output=True, text=True,
                             timeout=30).stdout
    except (OSError, subprocess.TimeoutExpired):
        clk = ""
    clocks = "; ".join(ln.split(":", 1)[1].strip() for ln in clk.splitlines()
                       if "clock level" in ln) or "not readable"
    lines = [f"`scripts/bench_dcn_lr.py --reps {args.reps} --blocks "
             f"{args.blocks}` on {torch.cuda.get_device_name(0)}; d = {D}, "
             f"L = {L}, us per call. Clocks at the start: {clocks}.", "",
             "| M | r | " + " | ".join(keys) + " |",
             "|---" * (len(keys) + 2) + "|"]
    for M in (4096, 8192):
        for r in (32, 64):
            c = row(M, r, args.reps, args.blocks)
            lines.append(f"| {M} | {r} | " + " | ".join(
                str(c[k]) if k == "rule" else f"{c[k]:.1f}" for k in keys)
                + " |")
            print(lines[-1], flush=True)
    md = "\n".join(lines)
    print(md)
    if args.out:
        with open(args.out, "w") as f:
            f.write(md + "\n")


if __name__ == "__main__":
    main()
