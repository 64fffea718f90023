#!/usr/bin/env python3
"""Cost and gain of the admission filter on one GPU.

A Zipf-shaped hashed id stream (ids drawn with probability ~ 1 / (rank + 1)
out of ``--pool``, batch 4096 x 26 ids a step) trains an adagrad table of dim
64 twice through the flat bounded route (``ShardedVariable.pull`` ->
``push`` -> ``update_weights``): with ``min_count`` 1, which admits every id
at first sight and so holds the rows a table without a filter holds, and with
``min_count`` 3. Recorded per run: the rows and bytes in the table after
``--steps`` steps, the milliseconds per pull + push + commit (host clock
around the step and a device synchronise, after ``--warmup`` untimed steps)
and the sketch's fill. A third, unfiltered run gives the time without the
two admission launches.

Asserted:
  - ``min_count`` 3 holds no more rows than ``min_count`` 1;
  - admission delays a row's creation and changes nothing else about it: on
    a pull-only replay of the first ``--check-steps`` steps both filters
    return bit-identical rows for the keys admitted in both, and the keys
    admitted at 3 are exactly those seen in three steps. That needs a width
    at which the sketch admits nothing early, which the CPU emulation
    (tests/admission_ref.py) establishes first.

Prints one JSON line. Needs a GPU; there is no CPU fall-back.
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import admission_ref as ar  # noqa: E402
from openembedding_amd.core.variable import VariableMeta  # noqa: E402
from openembedding_amd.core.variable_gpu import HipVariableShard  # noqa: E402
from openembedding_amd.parallel.sharded import ShardedVariable  # noqa: E402

DEV = "cuda:0"
BATCH, FIELDS, DIM, DEPTH, SEED = 4096, 26, 64, 4, 7


def stream(steps: int, pool: int):
    """``steps`` batches [BATCH, FIELDS] of ids on the device."""
    g = torch.Generator(device=DEV).manual_seed(0)
    p = 1.0 / (torch.arange(pool, dtype=torch.float32, device=DEV) + 1)
    out = []
    for _ in range(steps):
        ranks = torch.multinomial(p, BATCH * FIELDS, replacement=True,
                                  generator=g)
        out.append(((ranks * 2654435761) % (1 << 40) + 1)
                   .reshape(BATCH, FIELDS))
    return out


def shard(min_count, width: int, rows: int):
    sh = HipVariableShard(VariableMeta(0, DIM), device=DEV)
    sh.set_initializer("uniform", minval=-0.1, maxval=0.1)
    sh.set_optimizer("adagrad", learning_rate=0.05)
    sh.reserve_rows(rows)
    if min_count:
        sh.set_admission(min_count, width=width, depth=DEPTH, seed=SEED)
    return sh


def train(min_count, batches, warmup: int, width: int, rows: int):
    sh = shard(min_count, width, rows)
    var = ShardedVariable(sh)
    grads = torch.randn(BATCH, FIELDS, DIM, device=DEV,
                        generator=torch.Generator(device=DEV).manual_seed(1))
    times = []
    for i, ids in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, h = var.pull(ids)
        var.push(h, grads)
        var.update_weights()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    n = sh.num_rows
    res = {"rows": n,
           "table_bytes": n * (4 * (DIM + sh.state_dim) + 8),
           "median_ms": round(1e3 * times[len(times) // 2], 3),
           "min_ms": round(1e3 * times[0], 3),
           "max_ms": round(1e3 * times[-1], 3)}
    if min_count:
        st = sh.admission_stats()
        res.update(fill=round(st["fill"], 5), admitted=st["admitted"],
                   turned_away=st["turned_away"],
                   sketch_bytes=4 * sh.admit_sketch.numel())
    return res


def check_rows(batches, width: int, rows: int):
    """The pull-only replay (module docstring); returns the figures."""
    uniq = [torch.unique(b).cpu() for b in batches]
    ref = ar.RefAdmission(width, DEPTH, SEED, 3)
    seen = {}
    for u in uniq:
        ref.call(u)
        for k in u.tolist():
            seen[k] = seen.get(k, 0) + 1
    exact = {k for k, c in seen.items() if c >= 3}
    early = len(set(ref.index) - exact)
    assert early == 0 and set(ref.index) == exact, \
        f"width {width} admits {early} ids early: the check needs a wider " \
        "sketch"
    a, b = shard(1, width, rows), shard(3, width, rows)
    for u in uniq:
        a.pull(u.to(DEV))
        b.pull(u.to(DEV))
    kb = b.export_rows()[0].sort().values
    assert torch.equal(kb.cpu(), ref.keys()), \
        "min_count=3 did not admit exactly the ids seen in three steps"
    assert torch.equal(a.pull_readonly(kb), b.pull_readonly(kb)), \
        "the two filters return different rows for ids admitted in both"
    assert bool(a.pull_readonly(kb).abs().sum(1).min() > 0)
    return {"steps": len(batches), "ids_seen": len(seen),
            "admitted_at_3": int(kb.numel()), "early": early}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--pool", type=int, default=4_000_000)
    p.add_argument("--width", type=int, default=1 << 22)
    p.add_argument("--check-steps", type=int, default=6)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_admission.py needs a GPU")
    batches = stream(args.steps, args.pool)
    rows = args.steps * BATCH * FIELDS // 2
    check = check_rows(batches[:args.check_steps], args.width, rows)
    runs = {name: train(mc, batches, args.warmup, args.width, rows)
            for name, mc in (("off", None), ("min_count_1", 1),
                             ("min_count_3", 3))}
    assert runs["min_count_3"]["rows"] <= runs["min_count_1"]["rows"]
    assert runs["min_count_1"]["rows"] == runs["off"]["rows"]
    print(json.dumps({
        "bench": "admission", "dim": DIM, "batch": [BATCH, FIELDS],
        "steps": args.steps, "warmup": args.warmup, "pool": args.pool,
        "width": args.width, "depth": DEPTH, "identity_check": check,
        **runs}))


if __name__ == "__main__":
    main()
