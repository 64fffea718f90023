#!/usr/bin/env python3
"""Row expiry against the rebuild it replaces, on one GPU.

Times ``expire_rows`` removing half of a hashed adagrad table (default 4M
rows, dim 64) and, beside it, the only route the table had before:
``export_rows`` -> ``clear`` -> ``import_rows`` of the survivors. Both start
from the same table (same keys, same stamps); a removal destroys its input,
so every repeat rebuilds the table first, outside the timed window, and the
two variants alternate. A time is a host clock around the call and a device
synchronise. Peak extra device memory is the rise of
``torch.cuda.max_memory_allocated`` over the allocation before the call.

Acceptance (asserted): the expiry's extra memory does not scale with
rows x dim — its rise at dim 9 and at dim 64 is equal up to allocator
rounding — and both variants leave the same key -> row mapping.

Prints one JSON line. Needs a GPU; there is no CPU fall-back.
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openembedding_amd.core.variable import VariableMeta  # noqa: E402
from openembedding_amd.core.variable_gpu import HipVariableShard  # noqa: E402

DEV = "cuda:0"
BLOCK = 1 << 18


def build(rows: int, dim: int):
    """A tracked table of ``rows`` rows; the even keys are seen again in
    epoch 2, so ``expire_rows(2)`` removes the odd half."""
    sh = HipVariableShard(VariableMeta(0, dim), device=DEV)
    sh.set_optimizer("adagrad", learning_rate=0.1)
    sh.reserve_rows(rows)
    sh.track_changes()
    g = torch.Generator(device=DEV).manual_seed(dim)
    for start in range(0, rows, BLOCK):
        keys = torch.arange(start, min(start + BLOCK, rows), device=DEV)
        sh.import_rows(keys, torch.randn(keys.numel(), dim, device=DEV,
                                         generator=g))
    sh.set_epoch(2)
    for start in range(0, rows, 2 * BLOCK):
        keys = torch.arange(start, min(start + 2 * BLOCK, rows), 2,
                            device=DEV)
        sh.ext.mark_rows(sh._lookup_readonly(keys), None, None, sh.epoch_dev,
                         sh.row_epoch)
    torch.cuda.synchronize()
    return sh


def run_expire(sh):
    return sh.expire_rows(2)


def run_rebuild(sh):
    """What a user of the table could do before expiry existed."""
    keys, w, s = sh.export_rows()
    keep = sh.row_epoch[:keys.numel()] >= 2
    keys, w, s = keys[keep], w[keep], s[keep]
    sh.clear()
    sh.import_rows(keys, w, s)


def measure(fn, rows: int, dim: int):
    sh = build(rows, dim)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    fn(sh)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rise = torch.cuda.max_memory_allocated() - base
    return dt, rise, sh


def mapping(sh):
    keys, w, s = sh.export_rows()
    order = torch.argsort(keys)
    return keys[order], w[order], s[order]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expire.py needs a GPU")

    # warm-up at the timed shapes: code objects, allocator pools
    for fn in (run_expire, run_rebuild):
        measure(fn, args.rows, args.dim)
    times = {"expire": [], "rebuild": []}
    rises = {"expire": [], "rebuild": []}
    last = {}
    for _ in range(args.repeats):
        for name, fn in (("expire", run_expire), ("rebuild", run_rebuild)):
            last.pop(name, None)        # one spare table at a time
            dt, rise, sh = measure(fn, args.rows, args.dim)
            times[name].append(dt)
            rises[name].append(rise)
            last[name] = sh
    a, b = mapping(last["expire"]), mapping(last["rebuild"])
    assert all(torch.equal(x, y) for x, y in zip(a, b)), \
        "expiry and rebuild disagree"
    assert a[0].numel() == (args.rows + 1) // 2
    last.clear()

    # the memory condition: the rise must not depend on dim
    _, rise9, sh9 = measure(run_expire, args.rows, 9)
    slab9 = sh9.weights.numel() * 4 + sh9.state.numel() * 4
    del sh9
    _, rise64, sh64 = measure(run_expire, args.rows, 64)
    slab64 = sh64.weights.numel() * 4 + sh64.state.numel() * 4
    del sh64
    rounding = 32 * 512         # < 32 temporaries, each rounded to 512 B
    assert abs(rise9 - rise64) <= rounding, (rise9, rise64)
    assert rise64 < slab64 // 16, (rise64, slab64)

    def stats(v):
        v = sorted(v)
        return {"median_ms": round(1e3 * v[len(v) // 2], 3),
                "min_ms": round(1e3 * v[0], 3),
                "max_ms": round(1e3 * v[-1], 3)}

    print(json.dumps({
        "bench": "expire", "rows": args.rows, "dim": args.dim,
        "removed": args.rows // 2, "repeats": args.repeats,
        "expire": {**stats(times["expire"]),
                   "peak_extra_bytes": max(rises["expire"])},
        "rebuild": {**stats(times["rebuild"]),
                    "peak_extra_bytes": max(rises["rebuild"])},
        "expire_extra_bytes_dim9": rise9,
        "expire_extra_bytes_dim64": rise64,
        "slab_bytes_dim9": slab9, "slab_bytes_dim64": slab64,
    }))


if __name__ == "__main__":
    main()
