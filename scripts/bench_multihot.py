"""Fused multi-hot pooled step vs the same step composed from flat ops.

    python scripts/bench_multihot.py [--out profiles/multihot_pool.md]
    python scripts/bench_multihot.py --weighted \
        [--out profiles/multihot_pool_weighted.md]
    python scripts/bench_multihot.py --readonly \
        [--out profiles/multihot_pool_readonly.md]

fused    : EmbeddingBag forward (pooled pull) + backward (pooled push) +
           commit — no [nnz, dim] tensor in either direction.
composed : what a user wrote before EmbeddingBag existed — flat Embedding
           pull of the values, torch segment pooling (bag ids from the
           offsets, index_add, scale), autograd expansion back to
           [nnz, dim], flat push, commit.

``--weighted`` times the per-sample-weight step instead: fused is
EmbeddingBag(values, offsets, per_sample_weights=w), composed multiplies the
flat rows by w before the same torch pooling (weighted mean: divided by the
bag's sum of w). Both are timed with data weights (no gradient) and with
weights that require a gradient (``_wg``: the fused step adds k_pool_wgrad,
the composed step autograd's [nnz, dim] product backward), and the unweighted
fused step runs in the same alternating blocks for reference.

``--readonly`` times evaluation instead of training (see
``run_dim_readonly``): the fused read-only pooled lookup against the flat
read-only pull plus ``ops.pool_fwd``, both eager, and the fused lookup as a
captured hipGraph.

Workload: batch 4096 bags, mean length 8 with a long tail (lengths drawn
multinomially from log-normal weights, so every batch has the same nnz and
both steps can also be timed as captured hipGraphs), 20% of the values on
64 hot keys, array table of 2M rows, Adagrad, mode mean; dim 9 and 64.

Method: both steps are warmed up, then timed in alternating blocks of
``--block`` steps between device events over ``--blocks`` rounds (same
process, same batches); reported is the per-step median and the p10-p90
spread over blocks. Needs a GPU: there is no CPU fallback for a timing."""

import argparse
import json
import os
import statistics
import sys

import torch

B = 4096
MEAN_LEN = 8
VOCAB = 2_000_000
N_BATCHES = 8


def make_batches(device):
    g = torch.Generator().manual_seed(0)
    nnz = B * MEAN_LEN
    out = []
    for _ in range(N_BATCHES):
        weights = torch.exp(1.2 * torch.randn(B, generator=g))
        picks = torch.multinomial(weights, nnz, replacement=True, generator=g)
        lens = torch.bincount(picks, minlength=B)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64),
                             lens.cumsum(0)])
        vals = torch.randint(0, VOCAB, (nnz,), dtype=torch.int64, generator=g)
        hot = torch.rand(nnz, generator=g) < 0.2
        vals[hot] = torch.randint(0, 64, (int(hot.sum()),), generator=g)
        out.append((vals.to(device), offsets.to(device), int(lens.max())))
    return out


def build(dim, device):
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    ctx = get_context(device)
    bag = embed.EmbeddingBag(VOCAB, dim, mode="mean")
    flat = embed.Embedding(VOCAB, dim)
    for e in (bag, flat):
        e.variable.set_optimizer("adagrad", learning_rate=0.01,
                                 initial_accumulator_value=0.1,
                                 epsilon=1e-10)
    w = torch.randn(B, dim, device=device,
                    generator=torch.Generator(device).manual_seed(1))
    pos = torch.arange(B * MEAN_LEN, device=device)

    def fused(vals, offsets):
        out = bag(vals, offsets)
        (out * w).sum().backward()
        ctx.update_all_weights()
        return out

    def composed(vals, offsets):
        rows = flat(vals)                                   # [nnz, dim]
        bag_of = torch.bucketize(pos, offsets[1:], right=True)
        lens = (offsets[1:] - offsets[:-1]).to(rows.dtype)
        out = torch.zeros(B, dim, device=device).index_add(0, bag_of, rows)
        out = out / lens.clamp(min=1).unsqueeze(1)
        (out * w).sum().backward()
        ctx.update_all_weights()
        return out

    return fused, composed, bag, flat


def build_weighted(dim, device):
    """{name: step(vals, offsets, w)}; w is [nnz] in [0.25, 2], a leaf that
    requires grad for the ``_wg`` steps."""
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    ctx = get_context(device)
    bag = embed.EmbeddingBag(VOCAB, dim, mode="mean")
    flat = embed.Embedding(VOCAB, dim)
    for e in (bag, flat):
        e.variable.set_optimizer("adagrad", learning_rate=0.01,
                                 initial_accumulator_value=0.1,
                                 epsilon=1e-10)
    t = torch.randn(B, dim, device=device,
                    generator=torch.Generator(device).manual_seed(1))
    pos = torch.arange(B * MEAN_LEN, device=device)

    def finish(out, w):
        if w is not None:
            w.grad = None
        (out * t).sum().backward()
        ctx.update_all_weights()
        return out

    def fused(vals, offsets, w):
        return finish(bag(vals, offsets, per_sample_weights=w), w)

    def unweighted(vals, offsets, w):
        return finish(bag(vals, offsets), None)

    def composed(vals, offsets, w):
        rows = flat(vals) * w.unsqueeze(1)                  # [nnz, dim]
        bag_of = torch.bucketize(pos, offsets[1:], right=True)
        out = torch.zeros(B, dim, device=device).index_add(0, bag_of, rows)
        den = torch.zeros(B, device=device).index_add(0, bag_of, w)
        out = out / torch.where(den != 0, den,
                                torch.ones_like(den)).unsqueeze(1)
        return finish(out, w)

    return {"fused": fused, "composed": composed,
            "unweighted_fused": unweighted}, bag


def run_dim_weighted(dim, device, block, blocks, warmup):
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()
    batches = make_batches(device)
    g = torch.Generator().manual_seed(2)
    ws = [(torch.rand(B * MEAN_LEN, generator=g) * 1.75 + 0.25).to(device)
          for _ in batches]
    fns, bag = build_weighted(dim, device)

    # the fused weighted forward must equal torch pooling of the same rows
    vals, offsets, _ = batches[0]
    got = bag(vals, offsets, per_sample_weights=ws[0]).detach()
    rows = bag.variable.sparse_read(vals) * ws[0].unsqueeze(1)
    bag_of = torch.bucketize(torch.arange(vals.numel(), device=device),
                             offsets[1:], right=True)
    den = torch.zeros(B, device=device).index_add(0, bag_of, ws[0])
    want = torch.zeros_like(got).index_add(0, bag_of, rows) \
        / torch.where(den != 0, den, torch.ones_like(den)).unsqueeze(1)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)

    # (step name, function, weights require grad)
    plan = [("fused", "fused", False), ("composed", "composed", False),
            ("fused_wg", "fused", True), ("composed_wg", "composed", True),
            ("unweighted_fused", "unweighted_fused", False)]
    wg = [w.clone().requires_grad_() for w in ws]

    def eager_step(fn, grad):
        def run(i):
            vals, offsets, _ = batches[i % N_BATCHES]
            fn(vals, offsets, (wg if grad else ws)[i % N_BATCHES])
        return run

    eager = {name: eager_step(fns[f], grad) for name, f, grad in plan}
    for i in range(warmup):
        for fn in eager.values():
            fn(i)
    torch.cuda.synchronize()
    res = {"eager": summarize(time_blocks(eager, batches, block, blocks))}

    s_vals = batches[0][0].clone()
    s_off = batches[0][1].clone()
    s_w = {False: ws[0].clone(), True: ws[0].clone().requires_grad_()}
    graphs = {}
    for name, f, grad in plan:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fns[f](s_vals, s_off, s_w[grad])
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fns[f](s_vals, s_off, s_w[grad])
        graphs[name] = (gr, grad)

    def replay(name):
        gr, grad = graphs[name]

        def run(i):
            vals, offsets, _ = batches[i % N_BATCHES]
            s_vals.copy_(vals)
            s_off.copy_(offsets)
            with torch.no_grad():
                s_w[grad].copy_(ws[i % N_BATCHES])
            gr.replay()
        return run

    captured = {k: replay(k) for k in graphs}
    for i in range(warmup):
        for fn in captured.values():
            fn(i)
    torch.cuda.synchronize()
    res["graph"] = summarize(time_blocks(captured, batches, block, blocks))
    res["max_bag_len"] = max(b[2] for b in batches)
    for mode in ("eager", "graph"):
        for suf in ("", "_wg"):
            res[mode]["composed_over_fused" + suf] = (
                res[mode]["composed" + suf]["median_us"]
                / res[mode]["fused" + suf]["median_us"])
    return res


def to_markdown_weighted(results, args):
    cell = lambda r: (f"{r['median_us']:.1f} ({r['p10_us']:.1f}-"
                      f"{r['p90_us']:.1f})")
    lines = [
        "# Weighted multi-hot pooled step: fused vs composed (MI355X)",
        "",
        f"`scripts/bench_multihot.py --weighted`: batch {B} bags, nnz "
        f"{B * MEAN_LEN} (mean length {MEAN_LEN}, long tail), array table "
        f"of {VOCAB} rows, Adagrad, mode mean, weights uniform in "
        "[0.25, 2]. Per-step time from device events around alternating "
        f"blocks of {args.block} steps, {args.blocks} blocks per path after "
        f"{args.warmup} warm-up steps, all paths in one process on the same "
        "batches; median (p10-p90) in microseconds. `w` = data weights (no "
        "gradient), `w+dw` = weights that require a gradient; `unweighted` "
        "is the unweighted fused step in the same alternating blocks.",
        "",
        "| dim | mode | weights | fused | composed | composed / fused | "
        "unweighted fused |",
        "|---|---|---|---|---|---|---|",
    ]
    for dim, r in results.items():
        for mode in ("eager", "graph"):
            for suf, label in (("", "w"), ("_wg", "w+dw")):
                lines.append(
                    f"| {dim} | {mode} | {label} | "
                    f"{cell(r[mode]['fused' + suf])} | "
                    f"{cell(r[mode]['composed' + suf])} | "
                    f"{r[mode]['composed_over_fused' + suf]:.2f}x | "
                    f"{cell(r[mode]['unweighted_fused'])} |")
    lines.append("")
    lines.append("Longest bag over the batches: "
                 f"{max(r['max_bag_len'] for r in results.values())}.")
    return "\n".join(lines) + "\n"


def run_dim_readonly(dim, device, block, blocks, warmup):
    """Evaluation (no_grad) lookup of the same workload: the fused
    read-only pooled lookup against the route evaluation took before it —
    flat ``pull(readonly=True)`` (exact unique with its host sync, row
    gather, index_select to [nnz, dim]) plus ``ops.pool_fwd``. Both eager;
    the fused lookup also as a captured hipGraph (the flat route syncs the
    host and cannot be captured)."""
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    from openembedding_amd.ops import dispatch as ops
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()
    batches = make_batches(device)
    fused_step, _, bag, _ = build(dim, device)
    for vals, offsets, _ in batches:        # every timed key gets a row
        fused_step(vals, offsets)
    bag.eval()
    sharded = bag.variable.sharded

    def fused(vals, offsets):
        with torch.no_grad():
            return bag(vals, offsets)

    def flat_route(vals, offsets):
        with torch.no_grad():
            rows, _ = sharded.pull(vals, readonly=True)
            return ops.pool_fwd(rows.reshape(-1, dim), None, None, offsets,
                                "mean")[0]

    for vals, offsets, _ in batches:        # same rows, same order: same bits
        assert torch.equal(fused(vals, offsets), flat_route(vals, offsets))

    eager = {"fused": lambda i: fused(*batches[i % N_BATCHES][:2]),
             "flat": lambda i: flat_route(*batches[i % N_BATCHES][:2])}
    for i in range(warmup):
        for fn in eager.values():
            fn(i)
    torch.cuda.synchronize()
    res = {"eager": summarize(time_blocks(eager, batches, block, blocks))}

    s_vals = batches[0][0].clone()
    s_off = batches[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fused(s_vals, s_off)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fused(s_vals, s_off)

    def replay(i):
        vals, offsets, _ = batches[i % N_BATCHES]
        s_vals.copy_(vals)
        s_off.copy_(offsets)
        graph.replay()

    replay(1)
    assert torch.equal(out, fused(*batches[1][:2]))
    for i in range(warmup):
        replay(i)
    torch.cuda.synchronize()
    res["graph"] = summarize(time_blocks({"fused": replay}, batches, block,
                                         blocks))
    res["max_bag_len"] = max(b[2] for b in batches)
    res["flat_over_fused_eager"] = (res["eager"]["flat"]["median_us"]
                                    / res["eager"]["fused"]["median_us"])
    res["flat_eager_over_fused_graph"] = (
        res["eager"]["flat"]["median_us"]
        / res["graph"]["fused"]["median_us"])
    return res


def to_markdown_readonly(results, args):
    cell = lambda r: (f"{r['median_us']:.1f} ({r['p10_us']:.1f}-"
                      f"{r['p90_us']:.1f})")
    lines = [
        "# Read-only pooled lookup: fused vs flat pull + pool (MI355X)",
        "",
        f"`scripts/bench_multihot.py --readonly --block {args.block} "
        f"--blocks {args.blocks}`: batch {B} bags, nnz "
        f"{B * MEAN_LEN} (mean length {MEAN_LEN}, long tail), array table "
        f"of {VOCAB} rows trained one step per batch first (every looked-up "
        "key has a row), mode mean, under `torch.no_grad()`. `fused` is "
        "EmbeddingBag evaluation (one `k_pool_lookup` launch); `flat` is "
        "the route evaluation took before: `pull(readonly=True)` (exact "
        "unique with a host sync, row gather, index_select to [nnz, dim]) "
        "then `ops.pool_fwd`. Per-call time from device events around "
        f"alternating blocks of {args.block} calls, {args.blocks} blocks per "
        f"path after {args.warmup} warm-up calls, same process, same "
        "batches; median (p10-p90) in microseconds. `fused graph` replays "
        "one captured hipGraph (plus the two input copies); the flat route "
        "syncs the host and cannot be captured. Outputs of the two routes "
        "are checked bit-equal before timing.",
        "",
        "| dim | fused eager | flat eager | flat / fused (eager) | "
        "fused graph | flat eager / fused graph |",
        "|---|---|---|---|---|---|",
    ]
    for dim, r in results.items():
        lines.append(
            f"| {dim} | {cell(r['eager']['fused'])} | "
            f"{cell(r['eager']['flat'])} | "
            f"{r['flat_over_fused_eager']:.2f}x | "
            f"{cell(r['graph']['fused'])} | "
            f"{r['flat_eager_over_fused_graph']:.2f}x |")
    lines.append("")
    lines.append("Longest bag over the batches: "
                 f"{max(r['max_bag_len'] for r in results.values())}.")
    return "\n".join(lines) + "\n"


def time_blocks(steps, batches, block, blocks):
    """steps: {name: callable(i)} timed in alternating blocks."""
    ms = {k: [] for k in steps}
    i = 0
    for _ in range(blocks):
        for name, fn in steps.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(block):
                fn(i)
                i += 1
            stop.record()
            stop.synchronize()
            ms[name].append(start.elapsed_time(stop) / block)
    return ms


def summarize(ms):
    out = {}
    for k, v in ms.items():
        q = statistics.quantiles(v, n=10)
        out[k] = {"median_us": 1e3 * statistics.median(v),
                  "p10_us": 1e3 * q[0], "p90_us": 1e3 * q[-1]}
    return out


def run_dim(dim, device, block, blocks, warmup):
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()
    batches = make_batches(device)
    fused, composed, bag, flat = build(dim, device)

    # faster and different is not faster: at the timed size the fused
    # forward must equal torch pooling of the same table's rows (the two
    # variables draw different init rows, so each is checked on its own)
    vals, offsets, _ = batches[0]
    got = bag(vals, offsets).detach()
    rows = bag.variable.sparse_read(vals)
    bag_of = torch.bucketize(torch.arange(vals.numel(), device=device),
                             offsets[1:], right=True)
    lens = (offsets[1:] - offsets[:-1]).float().clamp(min=1).unsqueeze(1)
    want = torch.zeros_like(got).index_add(0, bag_of, rows) / lens
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)

    eager = {"fused": lambda i: fused(*batches[i % N_BATCHES][:2]),
             "composed": lambda i: composed(*batches[i % N_BATCHES][:2])}
    for i in range(warmup):
        for fn in eager.values():
            fn(i)
    torch.cuda.synchronize()
    res = {"eager": summarize(time_blocks(eager, batches, block, blocks))}

    # captured: one graph per path over static input buffers
    s_vals = batches[0][0].clone()
    s_off = batches[0][1].clone()
    graphs = {}
    for name, fn in (("fused", fused), ("composed", composed)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn(s_vals, s_off)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(s_vals, s_off)
        graphs[name] = g

    def replay(name):
        def run(i):
            vals, offsets, _ = batches[i % N_BATCHES]
            s_vals.copy_(vals)
            s_off.copy_(offsets)
            graphs[name].replay()
        return run

    captured = {k: replay(k) for k in graphs}
    for i in range(warmup):
        for fn in captured.values():
            fn(i)
    torch.cuda.synchronize()
    res["graph"] = summarize(time_blocks(captured, batches, block, blocks))
    res["max_bag_len"] = max(b[2] for b in batches)
    for mode in ("eager", "graph"):
        res[mode]["composed_over_fused"] = (
            res[mode]["composed"]["median_us"]
            / res[mode]["fused"]["median_us"])
    return res


def to_markdown(results, args):
    lines = [
        "# Multi-hot pooled step: fused vs composed (MI355X)",
        "",
        f"`scripts/bench_multihot.py`: batch {B} bags, nnz {B * MEAN_LEN} "
        f"(mean length {MEAN_LEN}, long tail), array table of {VOCAB} rows, "
        "Adagrad, mode mean. Per-step time from device events around "
        f"alternating blocks of {args.block} steps, {args.blocks} blocks per "
        f"path after {args.warmup} warm-up steps; median (p10-p90) in "
        "microseconds. `eager` includes the host launch path, `graph` "
        "replays one captured hipGraph per path (plus the two input "
        "copies).",
        "",
        "| dim | mode | fused | composed | composed / fused |",
        "|---|---|---|---|---|",
    ]
    for dim, r in results.items():
        for mode in ("eager", "graph"):
            f, c = r[mode]["fused"], r[mode]["composed"]
            lines.append(
                f"| {dim} | {mode} | {f['median_us']:.1f} "
                f"({f['p10_us']:.1f}-{f['p90_us']:.1f}) | "
                f"{c['median_us']:.1f} ({c['p10_us']:.1f}-"
                f"{c['p90_us']:.1f}) | "
                f"{r[mode]['composed_over_fused']:.2f}x |")
    lines.append("")
    lines.append("Longest bag over the batches: "
                 f"{max(r['max_bag_len'] for r in results.values())}.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[9, 64])
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="write a markdown table")
    ap.add_argument("--weighted", action="store_true",
                    help="time the per-sample-weight step (with and "
                         "without a gradient for the weights)")
    ap.add_argument("--readonly", action="store_true",
                    help="time the evaluation lookup: fused read-only "
                         "pooled lookup vs flat pull(readonly) + pool_fwd")
    args = ap.parse_args()
    if args.weighted and args.readonly:
        sys.exit("--weighted and --readonly are separate measurements")
    if not torch.cuda.is_available():
        sys.exit("bench_multihot.py needs a GPU (no CPU fallback)")
    from openembedding_amd.ops import require_hip
    require_hip()
    name, run, md = "multihot_pool", run_dim, to_markdown
    if args.weighted:
        name, run, md = ("multihot_pool_weighted", run_dim_weighted,
                         to_markdown_weighted)
    elif args.readonly:
        name, run, md = ("multihot_pool_readonly", run_dim_readonly,
                         to_markdown_readonly)
    results = {d: run(d, "cuda:0", args.block, args.blocks, args.warmup)
               for d in args.dims}
    if args.out:
        with open(args.out, "w") as f:
            f.write(md(results, args))
    print(json.dumps({"bench": name, "results": results}))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    main()
