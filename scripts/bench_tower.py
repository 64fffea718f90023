#!/usr/bin/env python
"""Fused MLP tower (ops/csrc/tower.hip), K0 = 247, widths (512, 256, 128,
32) and (256, 128, 64):

  kern  k_tower_fwd / k_tower_bwd alone at BM = 16, 32 and the launcher's
        choice (with mirrors), per launch;
  wg    k_tower_wgrad + k_tower_wgrad_fold alone (fresh gradients) at the
        launcher's m_split, per pair of launches;
  pair  forward + backward of ``ops.mlp_tower`` (fresh gradients of every
        parameter, weight packs and wgrads included) on the HIP route with
        the fused wgrad (pair_hip), with the library wgrads
        (``ops.dispatch._TOWER_WGRAD`` off: what ``OEAMD_TOWER_WGRAD=0``
        selects at import; pair_lib) and on the torch route
        (``ops.dispatch._TOWER`` off; pair_torch), all as captured graphs on
        the same operands, their blocks alternated;
  --sweep: the wgrad pair alone at m_split 1, 2, 4, 8, 16 and the rule's,
        M = 1024 .. 8192, instead of the table above.

    python scripts/bench_tower.py [--reps 200 --blocks 7] [--sweep]
                                  [--out FILE.md]

us per call: median (min-max) over ``--blocks`` blocks of ``--reps``
back-to-back calls between device events, after one warm-up block. The
clocks the run starts under are read with rocm-smi and printed. Needs a
GPU."""

import argparse
import os
import statistics
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(_HERE), _HERE]
from bench_dlrm import capture  # noqa: E402

K0 = 247
TOWERS = [(512, 256, 128, 32), (256, 128, 64)]


def timed(fn, reps, blocks):
    """(median, min, max) us per call over the blocks."""
    us = []
    for i in range(blocks + 1):
        t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        if i:
            us.append(t0.elapsed_time(t1) * 1e3 / reps)
    return statistics.median(us), min(us), max(us)


def timed_alternating(fns, reps, blocks):
    """``timed`` for several callables, one block of each in turn, so that
    drift of the clocks falls on all of them alike."""
    us = {k: [] for k in fns}
    for i in range(blocks + 1):
        for k, fn in fns.items():
            t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if i:
                us[k].append(t0.elapsed_time(t1) * 1e3 / reps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def wgrad_call(ext, M, widths, x0, acts, dzs, dout, m_split):
    """The wgrad pair on fresh gradients, as a callable."""
    dims = (K0,) + tuple(widths)
    shapes = [(h, k) for k, h in zip(dims, widths)] \
        + [(h,) for h in widths] + [(widths[-1],), (1,)]
    grads = [torch.empty(s, dtype=torch.bfloat16, device=x0.device)
             for s in shapes]
    scratch = torch.empty(ext.tower_wgrad_plan(M, K0, list(widths),
                                               m_split)[1], device=x0.device)
    return lambda: ext.tower_wgrad(x0, K0, acts, dzs, dout, grads, False,
                                   scratch, m_split)


def row(M, widths, reps, blocks, device="cuda:0", sweep=False):
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    bf = torch.bfloat16
    g = torch.Generator(device).manual_seed(M + len(widths))
    rn = lambda *s, k=1.0: (torch.randn(  # noqa: E731
        *s, device=device, generator=g) * k).to(bf)
    K0p = (K0 + 31) // 32 * 32
    x0 = torch.nn.functional.pad(rn(M, K0), (0, K0p - K0)).contiguous()
    dims = (K0,) + tuple(widths)
    W = [rn(h, k, k=k ** -0.5) for k, h in zip(dims, widths)]
    b = [rn(h, k=.1) for h in widths]
    wo, bo = rn(widths[-1], k=widths[-1] ** -0.5), rn(1)
    partial, dout = (torch.randn(M, device=device, generator=g)
                     for _ in range(2))
    bufs = dispatch._tower_images(W, K0p, True, ext)
    new = lambda: [torch.empty(M, h, dtype=bf, device=device)  # noqa: E731
                   for h in widths]
    acts, dzs = new(), new()
    out, dx0 = torch.empty(M, device=device), torch.empty_like(x0)
    res = {}
    if sweep:
        ext.tower_fwd(x0, K0, bufs["w"], b, acts, wo, bo, partial, out, 0)
        ext.tower_bwd(K0, acts, bufs["wt"], dout, wo, dzs, dx0, 0)
        for ms in (1, 2, 4, 8, 16, 0):
            res[f"wg{ms}"] = timed(wgrad_call(ext, M, widths, x0, acts, dzs,
                                              dout, ms), reps, blocks)
        res["S"] = int(ext.tower_wgrad_plan(M, K0, list(widths), 0)[0])
        return res
    for bm in (16, 32, 0):
        res[f"fwd{bm}"] = timed(lambda: ext.tower_fwd(
            x0, K0, bufs["w"], b, acts, wo, bo, partial, out, bm),
            reps, blocks)
        res[f"bwd{bm}"] = timed(lambda: ext.tower_bwd(
            K0, acts, bufs["wt"], dout, wo, dzs, dx0, bm), reps, blocks)
    res["rule"] = int(ext.tower_bm(M))
    res["wg"] = timed(wgrad_call(ext, M, widths, x0, acts, dzs, dout, 0),
                      reps, blocks)
    res["S"] = int(ext.tower_wgrad_plan(M, K0, list(widths), 0)[0])
    leaves = [t.requires_grad_() for t in [x0] + W + b + [wo, bo]]
    L = len(widths)

    def pair():
        o = dispatch.mlp_tower(leaves[0], leaves[1:1 + L],
                               leaves[1 + L:1 + 2 * L], leaves[-2],
                               leaves[-1], partial)
        torch.autograd.grad(o, leaves, dout)
    graphs = {"pair_hip": capture(pair)}
    dispatch._TOWER_WGRAD = False
    try:
        graphs["pair_lib"] = capture(pair)
    finally:
        dispatch._TOWER_WGRAD = True
    dispatch._TOWER = False
    try:
        graphs["pair_torch"] = capture(pair)
    finally:
        dispatch._TOWER = True
    res.update(timed_alternating({k: g.replay for k, g in graphs.items()},
                                 reps // 4, blocks))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tower.py needs a GPU"
    keys = ["fwd16", "fwd32", "fwd0", "bwd16", "bwd32", "bwd0", "rule",
            "wg", "S", "pair_hip", "pair_lib", "pair_torch"]
    if args.sweep:
        keys = ["wg1", "wg2", "wg4", "wg8", "wg16", "wg0", "S"]
    try:
        clk = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"],
                             capture_output=True, text=True,
                             timeout=30).stdout
    except (OSError, subprocess.TimeoutExpired):
        clk = ""
    clocks = "; ".join(ln.split(":", 1)[1].strip() for ln in clk.splitlines()
                       if "clock level" in ln) or "not readable"
    lines = [f"`scripts/bench_tower.py --reps {args.reps} --blocks "
             f"{args.blocks}{' --sweep' if args.sweep else ''}` on "
             f"{torch.cuda.get_device_name(0)}; K0 = {K0}, "
             "us per call, median (min-max) over the blocks. Clocks at the "
             f"start: {clocks}.", "",
             "| M | widths | " + " | ".join(keys) + " |",
             "|---" * (len(keys) + 2) + "|"]
    for M in (1024, 2048, 4096, 8192) if args.sweep else (4096, 8192):
        for widths in TOWERS:
            c = row(M, widths, args.reps, args.blocks, sweep=args.sweep)
            lines.append(f"| {M} | {'-'.join(map(str, widths))} | "
                         + " | ".join(
                             str(c[k]) if k in ("rule", "S") else
                             "{:.1f} ({:.1f}-{:.1f})".format(*c[k])
                             for k in keys) + " |")
            print(lines[-1], flush=True)
    md = "\n".join(lines)
    print(md)
    if args.out:
        with open(args.out, "w") as f:
            f.write(md + "\n")


if __name__ == "__main__":
    main()
