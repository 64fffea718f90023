"""Delta checkpoints across shard counts (gloo): a world-2 trainer writes a
full dump and two deltas; reloaded at world 1 and at world 3, base + deltas
equal the world-2 final state key by key, exactly."""

import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

DIM = 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method=f"tcp://127.0.0.1:{port}")


def _make(table, track):
    from openembedding_amd.context import Context
    ctx = Context(device="cpu")
    st = ctx.create_storage()
    var = st.create_variable(1500 if table == "array" else -1, DIM)
    var.set_initializer("uniform", minval=-1, maxval=1)
    var.set_optimizer("adam", learning_rate=0.05)
    if track:
        var.shard.track_changes()
    return ctx, st, var


def _step(st, var, rank, phase, lo, hi):
    g = torch.Generator().manual_seed(1000 * phase + rank)
    keys = torch.randint(lo, hi, (600,), generator=g, dtype=torch.int64)
    _, h = var.pull(keys)
    var.push(h, torch.randn(600, DIM, generator=g))
    st.update_weights()


def _owned_rows(var):
    keys, w, s = var.shard.export_rows(include_state=True)
    return {int(k): (w[i].clone(), s[i].clone())
            for i, k in enumerate(keys.tolist())}


def _trainer(rank, world, port, tmp, table):
    from openembedding_amd import checkpoint
    _init(rank, world, port)
    ctx, st, var = _make(table, track=True)
    _step(st, var, rank, 1, 0, 1000)
    checkpoint.dump_model(ctx, os.path.join(tmp, "A"))
    _step(st, var, rank, 2, 200, 400)
    d1 = checkpoint.dump_delta(ctx, os.path.join(tmp, "D1"))
    _step(st, var, rank, 3, 900, 1300)
    d2 = checkpoint.dump_delta(ctx, os.path.join(tmp, "D2"))
    assert (d1["since"], d1["epoch"]) == (2, 2)
    assert (d2["since"], d2["epoch"]) == (3, 3)
    torch.save({"rows": _owned_rows(var), "d1": d1["rows"],
                "d2": d2["rows"]}, os.path.join(tmp, f"final_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _consumer(rank, world, port, tmp, table):
    from openembedding_amd import checkpoint
    if world > 1:
        _init(rank, world, port)
    ctx, st, var = _make(table, track=False)
    checkpoint.load_model(ctx, os.path.join(tmp, "A"))
    checkpoint.apply_delta(ctx, os.path.join(tmp, "D1"))
    checkpoint.apply_delta(ctx, os.path.join(tmp, "D2"))
    assert ctx.loaded_epoch == 3
    torch.save(_owned_rows(var),
               os.path.join(tmp, f"w{world}_{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.finalize()


def _clear_env():
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
              "MASTER_PORT"):
        os.environ.pop(v, None)


def _merged(tmp, pattern, n):
    rows = {}
    for r in range(n):
        part = torch.load(os.path.join(tmp, pattern.format(r)),
                          weights_only=True)
        part = part["rows"] if "rows" in part else part
        assert not set(part) & set(rows)       # every key has one owner
        rows.update(part)
    return rows


@pytest.mark.timeout(240)
@pytest.mark.parametrize("table", ("hash", "array"))
def test_world2_chain_reloads_at_world1_and_world3(tmp_path, table):
    from openembedding_amd import checkpoint
    tmp = str(tmp_path)
    try:
        mp.spawn(_trainer, args=(2, _free_port(), tmp, table), nprocs=2,
                 join=True)
        mp.spawn(_consumer, args=(3, _free_port(), tmp, table), nprocs=3,
                 join=True)
    finally:
        _clear_env()
    _consumer(0, 1, 0, tmp, table)

    want = _merged(tmp, "final_{}.pt", 2)
    # the deltas are partial: fewer rows than the table, summed over ranks
    finals = [torch.load(os.path.join(tmp, f"final_{r}.pt"),
                         weights_only=True) for r in range(2)]
    for name, key in (("D1", "d1"), ("D2", "d2")):
        n = sum(len(k) for _, k, _, _ in checkpoint.iter_blocks(
            os.path.join(tmp, name)))
        assert n == finals[0][key] + finals[1][key]
        assert 0 < n < len(want) // 2
    for world in (1, 3):
        got = _merged(tmp, f"w{world}_{{}}.pt", world)
        assert set(got) == set(want) and len(want) > 600
        for k, (w, s) in want.items():
            assert torch.equal(got[k][0], w), k
            assert torch.equal(got[k][1], s), k
