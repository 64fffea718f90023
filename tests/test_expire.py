"""Row expiry on the CPU: the torch form of ``expire_rows`` / ``remove_rows``
against a dict model written here (layout rule, returned keys, misses,
re-creation), the preconditions, array tables, tombstones in delta chains
(base + deltas == full dump as a mapping), the pruned removal log, a gloo
world-2 chain reloaded at world 1, serving replicas in every row format, the
public entry point and the example. Rows are copied, never computed: every
comparison is exact."""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from fastapi.testclient import TestClient

import delta_ref as dr
from openembedding_amd import checkpoint
from openembedding_amd.core.quantized import QuantizedShard
from openembedding_amd.core.variable import VariableMeta, VariableShard
from openembedding_amd.serving import (ModelController, ServedModel,
                                       make_app)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 5


def _t(*a):
    return torch.tensor(a, dtype=torch.int64)


# ------------------------------------------------------------ the dict model

class DictTable:
    """The layout rule of the issue over plain lists: ``rows[slot]`` is
    (key, weights, state, stamp)."""

    def __init__(self, rows):
        self.rows = list(rows)

    def remove(self, dead_slots):
        n, dead = len(self.rows), sorted(set(dead_slots))
        n2 = n - len(dead)
        removed = [self.rows[s][0] for s in dead]
        holes = [s for s in dead if s < n2]
        movers = [s for s in range(n2, n) if s not in set(dead)]
        assert len(holes) == len(movers)
        for h, m in zip(holes, movers):
            self.rows[h] = self.rows[m]
        del self.rows[n2:]
        return removed


def _shard(opt="adagrad", vocab=None, dim=DIM, track=True):
    meta = VariableMeta(0, dim) if vocab is None \
        else VariableMeta(0, dim, vocabulary_size=vocab)
    sh = VariableShard(meta)
    sh.set_initializer("normal", mean=0.0, stddev=0.1)
    sh.set_optimizer(opt, learning_rate=0.05)
    if track:
        sh.track_changes()
    return sh


def _train(sh, keys, seed):
    keys = torch.as_tensor(keys, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    sh.pull(keys)
    sh.push(keys, torch.randn(keys.numel(), sh.dim, generator=g),
            torch.ones(keys.numel(), dtype=torch.int64))
    sh.update_weights()


def _model_of(sh):
    n = sh._nrows
    sk = sh._slot_key_list().tolist()
    return DictTable((sk[s], sh.weights[s].clone(), sh.state[s].clone(),
                      int(sh.row_epoch[s]) if sh.tracking else 0)
                     for s in range(n))


def _assert_matches(sh, model):
    n = len(model.rows)
    assert sh._nrows == sh.num_rows == n
    assert sh._slot_key_list().tolist() == [r[0] for r in model.rows]
    assert sh._index == {r[0]: s for s, r in enumerate(model.rows)}
    for s, (_k, w, st, ep) in enumerate(model.rows):
        assert torch.equal(sh.weights[s], w)
        assert torch.equal(sh.state[s], st)
        if sh.tracking:
            assert int(sh.row_epoch[s]) == ep


PATTERNS = {
    "none": lambda n, g: [],
    "all": lambda n, g: list(range(n)),
    "first": lambda n, g: [0],
    "last": lambda n, g: [n - 1],
    "tail": lambda n, g: list(range(n - max(1, n // 3), n)),
    "head": lambda n, g: list(range(n // 2 + 1)),
    "alternating": lambda n, g: list(range(1, n, 2)),
    "random": lambda n, g: (torch.rand(n, generator=g) < 0.5).nonzero()
    .flatten().tolist(),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("opt", ("sgd", "adagrad", "adam"))
@pytest.mark.parametrize("n", (1, 2, 7, 100))
def test_layout_rule_against_the_dict_model(n, opt, pattern):
    g = torch.Generator().manual_seed(n)
    keys = (torch.randperm(10 * n, generator=g)[:n] * 7 + 3)
    dead = PATTERNS[pattern](n, g)
    for by_age in (True, False):
        sh = _shard(opt)
        _train(sh, keys, 1)
        first = {int(k): sh.initializer(sh.seed, _t(int(k)), DIM,
                                        sh.dtype)[0] for k in keys}
        sh.set_epoch(2)
        keep = [s for s in range(n) if s not in set(dead)]
        if keep:
            _train(sh, keys[keep], 2)        # survivors are seen again
        model = _model_of(sh)
        assert [r[0] for r in model.rows] == keys.tolist()
        want = model.remove(dead)
        if by_age:
            got = sh.expire_rows(2)
        else:
            dk = keys[dead] if dead else keys[:0]
            got = sh.remove_rows(torch.cat([dk, dk[:3], _t(-1, 10 ** 12)]))
        assert got.dtype == torch.int64 and got.tolist() == want
        assert want == keys[sorted(dead)].tolist() if dead else want == []
        _assert_matches(sh, model)
        # removed keys miss; survivors read their rows
        out = sh.pull_readonly(keys)
        for i, k in enumerate(keys.tolist()):
            if i in set(dead):
                assert not out[i].any()
            else:
                assert torch.equal(out[i], sh.weights[sh._index[k]])
        # a training pull re-creates a removed key as its first-ever row
        if dead:
            k = int(keys[dead[0]])
            again = sh.pull(_t(k))[0]
            assert torch.equal(again, first[k])
            assert sh._index[k] == n - len(dead)
            assert torch.equal(sh.state[sh._index[k]],
                               sh._state_init_row[0])
        assert sh.removed_since(1).tolist() == want
        assert sh.removed_since(3).tolist() == []


def test_reset_stamps_are_the_oldest():
    sh = _shard()
    _train(sh, [1, 2, 3], 1)
    sh.set_epoch(4, reset=True)
    _train(sh, [2], 2)
    assert sh.expire_rows(1).tolist() == [1, 3]
    assert sh.expire_rows(4).tolist() == []
    assert sh.expire_rows(5).tolist() == [2]


def test_preconditions():
    sh = _shard()
    _train(sh, [1, 2, 3], 1)
    sh.push(_t(1), torch.ones(1, DIM), _t(1))
    for call in (lambda: sh.expire_rows(5), lambda: sh.remove_rows(_t(1))):
        with pytest.raises(RuntimeError, match="queued"):
            call()
    sh.update_weights()
    assert sh.num_rows == 3
    off = _shard(track=False)
    _train(off, [1, 2, 3], 1)
    with pytest.raises(RuntimeError, match="tracking"):
        off.expire_rows(5)
    assert off.remove_rows(_t(2, 2, 9)).tolist() == [2]    # works untracked
    assert off.num_rows == 2 and not hasattr(off, "_removed_log")
    from openembedding_amd.core.tiered import TieredVariableShard
    tier = TieredVariableShard(VariableMeta(0, DIM), cache_rows=1024)
    with pytest.raises(NotImplementedError):
        tier.expire_rows(1)
    with pytest.raises(NotImplementedError):
        tier.remove_rows(_t(1))
    q = QuantizedShard(VariableMeta(0, DIM), "int8")
    assert not hasattr(q, "expire_rows")


def test_array_mode_clears_valid_and_moves_nothing():
    sh = VariableShard(VariableMeta(0, DIM, vocabulary_size=100),
                       shard_id=1, shard_num=3)
    sh.set_initializer("normal", mean=0.0, stddev=0.1)
    sh.set_optimizer("adagrad", learning_rate=0.05)
    sh.track_changes()
    keys = _t(1, 4, 31, 97, 64)
    _train(sh, keys, 1)
    sh.set_epoch(2)
    _train(sh, _t(4, 97), 2)
    w = sh.weights.clone()
    assert sh.expire_rows(2).tolist() == [1, 31, 64]       # ascending slot
    assert torch.equal(sh.weights, w) and sh.num_rows == 2
    assert sh.valid.nonzero().flatten().tolist() == [1, 32]
    out = sh.pull_readonly(keys)
    assert not out[[0, 2, 4]].any() and out[[1, 3]].any()
    # keys of another shard, out of range, negative, duplicates: ignored
    assert sh.remove_rows(_t(97, 97, 0, 2, 5, -1, -2, 1000)).tolist() == [97]
    assert sh.num_rows == 1
    assert sh.removed_since(1).tolist() == [1, 31, 64, 97]
    first = sh.initializer(sh.seed, _t(31), DIM, sh.dtype)
    assert torch.equal(sh.pull(_t(31)), first)


# --------------------------------------------------------- tombstone chains

def _removed_keys(uri):
    return [k for _h, keys in checkpoint.iter_removed(uri)
            for k in keys.tolist()]


def _removed_files(uri):
    return sorted(f for f in dr.all_files(uri) if "removed_" in f)


@pytest.mark.parametrize("opt", ("adagrad", "adam"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_chain_with_tombstones_equals_full_dump(tmp_path, table, opt):
    ctx, st, var = dr.make_trainer("cpu", table, opt)
    uri = {n: str(tmp_path / n) for n in ("A", "D1", "D2", "D3", "B")}
    dr.train(st, var, list(range(300)), 1)
    checkpoint.dump_model(ctx, uri["A"])                      # epoch 1
    dr.train(st, var, list(range(100, 300)), 2)
    d1 = checkpoint.dump_delta(ctx, uri["D1"])                # epoch 2
    assert _removed_files(uri["D1"]) == []    # no removals, no file
    # epoch 3: keys 0..99 expire; 10..19 come back in the same interval
    with pytest.raises(ValueError):
        checkpoint.expire_rows(ctx)
    with pytest.raises(ValueError):
        checkpoint.expire_rows(ctx, max_age=1, before=2)
    r = checkpoint.expire_rows(ctx, max_age=1)
    assert r == {"before": 2, "rows": 100}
    dr.train(st, var, list(range(10, 20)) + [500], 3)
    d2 = checkpoint.dump_delta(ctx, uri["D2"])
    assert sorted(_removed_keys(uri["D2"])) == list(range(100))
    assert _removed_files(uri["D2"]) == ["0/removed_0"]
    hdr = next(checkpoint.iter_removed(uri["D2"]))[0]
    assert hdr == {"variable_id": 0, "num_items": 100, "removed": True}
    # epoch 4: key 15 is removed a second time, 500 for the first time
    assert checkpoint.expire_rows(ctx, before=3)["rows"] == 200
    assert var.shard.remove_rows(_t(15, 500, 15)).numel() == 2
    dr.train(st, var, [600], 4)
    checkpoint.dump_delta(ctx, uri["D3"])
    checkpoint.dump_model(ctx, uri["B"])
    assert (d1["rows"], d2["rows"]) == (200, 11)
    want = dr.rows_by_key(var.shard)
    assert want[0].tolist() == [10, 11, 12, 13, 14, 16, 17, 18, 19, 600]

    c1, _, v1 = dr.make_consumer("cpu", table, opt)
    checkpoint.load_model(c1, uri["A"])
    for d in ("D1", "D2", "D3"):
        checkpoint.apply_delta(c1, uri[d])
    c2, _, v2 = dr.make_consumer("cpu", table, opt)
    checkpoint.load_model(c2, uri["B"])
    assert want[2] is not None
    dr.assert_same_rows(dr.rows_by_key(v1.shard), want)
    dr.assert_same_rows(dr.rows_by_key(v2.shard), want)
    # the intermediate state, against the files merged by hand
    ctx2, st2, var2 = dr.make_trainer("cpu", table, opt)
    checkpoint.load_model(ctx2, uri["A"])
    checkpoint.apply_delta(ctx2, uri["D1"])
    checkpoint.apply_delta(ctx2, uri["D2"])
    assert ctx2.loaded_epoch == 3
    dr.assert_same_rows(
        dr.rows_by_key(var2.shard),
        _expected_after_d2(uri))


def _expected_after_d2(uri):
    """Base A + D1 + D2 by hand: A's and the deltas' rows, later winning,
    minus D2's tombstones unless D2 upserts the key again."""
    rows = {}
    for name in ("A", "D1"):
        rows.update(dr.dump_rows(uri[name])[0])
    for k in _removed_keys(uri["D2"]):
        rows.pop(k, None)
    rows.update(dr.dump_rows(uri["D2"])[0])
    keys = sorted(rows)
    w = torch.from_numpy(np.stack(
        [np.frombuffer(rows[k][0], dtype="<f4") for k in keys]).copy())
    s = torch.from_numpy(np.stack(
        [np.frombuffer(rows[k][1], dtype="<f4") for k in keys]).copy())
    return torch.tensor(keys), w, s


def test_removals_are_applied_before_upserts(tmp_path):
    """Key 7 expires and is re-created inside one interval: it is in the
    delta's tombstones and in its rows, and the consumer keeps it."""
    ctx, st, var = dr.make_trainer()
    dr.train(st, var, [1, 7], 1)
    base, delta = str(tmp_path / "base"), str(tmp_path / "delta")
    checkpoint.dump_model(ctx, base)
    assert checkpoint.expire_rows(ctx, before=2)["rows"] == 2
    dr.train(st, var, [7], 2)
    checkpoint.dump_delta(ctx, delta)
    assert sorted(_removed_keys(delta)) == [1, 7]
    assert dr.dump_rows(delta)[1] == [7]
    c, _, v = dr.make_consumer()
    checkpoint.load_model(c, base)
    checkpoint.apply_delta(c, delta)
    dr.assert_same_rows(dr.rows_by_key(v.shard), dr.rows_by_key(var.shard))
    assert dr.rows_by_key(v.shard)[0].tolist() == [7]


def test_delta_without_removals_is_unchanged(tmp_path):
    """No removal, no file: the delta's files are those of the rows alone,
    and a later removal adds exactly one file."""
    ctx, st, var = dr.make_trainer()
    dr.train(st, var, list(range(50)), 1)
    checkpoint.dump_model(ctx, str(tmp_path / "A"))
    dr.train(st, var, list(range(10)), 2)
    checkpoint.dump_delta(ctx, str(tmp_path / "D1"))
    assert sorted(dr.all_files(str(tmp_path / "D1"))) == \
        ["0/model_0_0", "model_meta"]
    assert list(checkpoint.iter_removed(str(tmp_path / "D1"))) == []
    var.shard.remove_rows(_t(3))
    checkpoint.dump_delta(ctx, str(tmp_path / "D2"))
    assert sorted(dr.all_files(str(tmp_path / "D2"))) == \
        ["0/model_0_0", "0/removed_0", "model_meta"]
    # the rows of a delta are still read by iter_blocks alone
    assert dr.dump_rows(str(tmp_path / "D2"))[1] == []


def test_pruned_log_refuses_an_earlier_since(tmp_path):
    ctx, st, var = dr.make_trainer()
    dr.train(st, var, list(range(20)), 1)
    checkpoint.dump_model(ctx, str(tmp_path / "A"))           # epoch 1
    dr.train(st, var, [1], 2)
    checkpoint.dump_delta(ctx, str(tmp_path / "D1"))          # epoch 2
    # nothing was dropped so far: an earlier since is served as before
    checkpoint.dump_delta(ctx, str(tmp_path / "D1b"), since=2)  # epoch 3
    var.shard.remove_rows(_t(5))                              # epoch 4
    checkpoint.dump_model(ctx, str(tmp_path / "B"))           # prunes
    assert var.shard.removed_since(1).numel() == 0
    assert ctx.removals_pruned_epoch == 5
    dr.train(st, var, [2], 3)
    with pytest.raises(ValueError, match="[Rr]eload the base"):
        checkpoint.dump_delta(ctx, str(tmp_path / "bad"), since=4)
    ok = checkpoint.dump_delta(ctx, str(tmp_path / "D2"), since=5)
    assert ok["rows"] == 1
    # a load prunes too
    var.shard.remove_rows(_t(6))
    checkpoint.load_model(ctx, str(tmp_path / "B"))
    assert var.shard.removed_since(1).numel() == 0
    assert ctx.removals_pruned_epoch == var.shard.epoch


# ------------------------------------------------------------- gloo world 2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _owned(var):
    keys, w, s = var.shard.export_rows(include_state=True)
    return {int(k): (w[i].clone(), s[i].clone())
            for i, k in enumerate(keys.tolist())}


def _dist_trainer(rank, world, port, tmp):
    for k, v in (("RANK", rank), ("WORLD_SIZE", world), ("LOCAL_RANK", rank),
                 ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", port)):
        os.environ[k] = str(v)
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method=f"tcp://127.0.0.1:{port}")
    ctx, st, var = dr.make_trainer("cpu", "hash", "adam")

    def step(phase, lo, hi):
        g = torch.Generator().manual_seed(100 * phase + rank)
        keys = torch.randint(lo, hi, (300,), generator=g)
        _, h = var.pull(keys)
        var.push(h, torch.randn(300, dr.DIM, generator=g))
        st.update_weights()

    step(1, 0, 600)
    checkpoint.dump_model(ctx, os.path.join(tmp, "A"))
    step(2, 300, 600)
    r = checkpoint.expire_rows(ctx, max_age=0)      # all not seen in epoch 2
    step(3, 280, 320)                               # some come back
    checkpoint.dump_delta(ctx, os.path.join(tmp, "D1"))
    torch.save({"rows": _owned(var), "expired": r["rows"]},
               os.path.join(tmp, f"final_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_world2_tombstones_reload_at_world1(tmp_path):
    tmp = str(tmp_path)
    try:
        mp.spawn(_dist_trainer, args=(2, _free_port(), tmp), nprocs=2,
                 join=True)
    finally:
        for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
                  "MASTER_PORT"):
            os.environ.pop(v, None)
    finals = [torch.load(os.path.join(tmp, f"final_{r}.pt"),
                         weights_only=True) for r in range(2)]
    want = {**finals[0]["rows"], **finals[1]["rows"]}
    assert all(f["expired"] > 50 for f in finals)
    d1 = os.path.join(tmp, "D1")
    assert _removed_files(d1) == ["0/removed_0", "0/removed_1"]
    assert len(_removed_keys(d1)) == sum(f["expired"] for f in finals)
    ctx, st, var = dr.make_consumer("cpu", "hash", "adam")
    checkpoint.load_model(ctx, os.path.join(tmp, "A"))
    n_base = var.shard.num_rows
    checkpoint.apply_delta(ctx, d1)
    got = _owned(var)
    assert set(got) == set(want) and len(want) < n_base
    for k, (w, s) in want.items():
        assert torch.equal(got[k][0], w) and torch.equal(got[k][1], s), k
    ctx.finalize()


# ------------------------------------------------------------------ serving

@pytest.fixture(scope="module")
def tomb_chain(tmp_path_factory):
    """A: keys 0..199. D1: 0..49 removed, 40..44 re-created, 300 created.
    B: the full dump at that point."""
    out = {}
    for table in ("hash", "array"):
        tmp = tmp_path_factory.mktemp(f"tomb_{table}")
        ctx, st, var = dr.make_trainer("cpu", table, "adagrad")
        uri = {n: str(tmp / n) for n in ("A", "D1", "B")}
        dr.train(st, var, list(range(200)), 1)
        checkpoint.dump_model(ctx, uri["A"])
        dr.train(st, var, list(range(50, 200)), 2)
        assert checkpoint.expire_rows(ctx, before=2)["rows"] == 50
        dr.train(st, var, list(range(40, 45)) + [300], 3)
        checkpoint.dump_delta(ctx, uri["D1"])
        checkpoint.dump_model(ctx, uri["B"])
        ctx.finalize()
        out[table] = uri
    return out


SERVE_PROBE = list(range(200)) + [300, 301]


@pytest.mark.parametrize("fmt", (None, "int8", "fp16"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_served_model_applies_tombstones(tomb_chain, table, fmt):
    uri = tomb_chain[table]
    m = ServedModel("live", uri["A"])
    m.load(device="cpu", quantize=fmt)
    sh = m.variables[0].shard
    assert sh.num_rows == 200
    m.export_block(0, 0, 10)                       # warm the page cache
    r = m.apply_delta(uri["D1"])
    assert r == {"since": 2, "epoch": 2, "rows": 156, "removed": 50}
    assert sh.num_rows == 156
    assert m.export_block(0, 0, 10)["total"] == 156
    fresh = ServedModel("fresh", uri["B"])
    fresh.load(device="cpu", quantize=fmt)
    probe = torch.tensor(SERVE_PROBE)
    got = m.variables[0].pull_weights(probe)
    assert torch.equal(got, fresh.variables[0].pull_weights(probe))
    gone = [k for k in range(50) if not 40 <= k < 45] + [201]  # key 301
    assert not got[gone].any()
    assert got[[40, 44, 50, 199, 200]].abs().sum(1).min() > 0
    for mode in ("sum", "mean"):
        a = m.variables[0].pull_pooled(SERVE_PROBE, [0, 60, 150, 202], mode)
        b = fresh.variables[0].pull_pooled(SERVE_PROBE, [0, 60, 150, 202],
                                           mode)
        assert torch.equal(a, b)


@pytest.mark.parametrize("fmt", ("int8", "fp16"))
def test_quantized_remove_rows_follows_the_layout_rule(fmt):
    g = torch.Generator().manual_seed(3)
    q = QuantizedShard(VariableMeta(0, DIM), fmt)
    keys = torch.randperm(1000, generator=g)[:40]
    q.import_rows(keys, torch.randn(40, DIM, generator=g))
    model = DictTable((int(k), q.slab[s].clone(), None, 0)
                      for s, k in enumerate(keys.tolist()))
    dead = [0, 3, 4, 17, 38, 39]
    want = model.remove(dead)
    ptr = q.slab.data_ptr()
    got = q.remove_rows(torch.cat([keys[dead], keys[dead][:2],
                                   _t(-1, 5000)]))
    assert got.tolist() == want and q.num_rows == 34
    assert q.slab.data_ptr() == ptr
    assert q.slot_keys[:34].tolist() == [r[0] for r in model.rows]
    assert torch.equal(q.slab[:34], torch.stack([r[1] for r in model.rows]))
    assert q._index == {r[0]: s for s, r in enumerate(model.rows)}
    assert not q.pull_readonly(keys[dead]).any()
    assert q.remove_rows(keys[dead]).numel() == 0


def test_rest_route_reports_removed(tomb_chain):
    uri = tomb_chain["hash"]
    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    r = client.post("/models", json={"model_uri": uri["A"], "sign": "m"})
    assert r.status_code == 200
    r = client.post("/models/m/deltas", json={"model_uri": uri["D1"]})
    assert r.status_code == 200, r.text
    assert r.json()["removed"] == 50 and r.json()["epoch"] == 2
    r = client.post("/models/m/variables/0/pull",
                    json={"indices": [0, 41, 60]})
    w = torch.tensor(r.json()["weights"])
    assert not w[0].any() and w[1].any() and w[2].any()
    page = client.get("/models/m/variables/0/rows",
                      params={"start": 0, "count": 1000}).json()
    assert page["total"] == 156 and 0 not in page["keys"]


# ----------------------------------------------------------- public surface

def test_expire_server_model_entry_point():
    import openembedding_amd.torch as embed
    from openembedding_amd import context as ctxmod
    assert "expire_server_model" in embed.__all__
    old = ctxmod._context
    ctxmod._context = None
    os.environ["OEAMD_DEVICE"] = "cpu"
    try:
        embed.track_server_model_changes()
        emb = embed.Embedding(-1, 4)
        opt = embed.distributed_optimizer(
            torch.optim.SGD(list(emb.parameters()), lr=0.1))

        def step(ids):
            opt.zero_grad()
            emb(torch.tensor(ids)).sum().backward()
            opt.step()

        step([1, 2, 3, 4])
        sh = emb.variable.sharded.shard
        sh.set_epoch(2)
        step([2, 3])
        with pytest.raises(ValueError):
            embed.expire_server_model()
        emb.variable.prefetch(torch.tensor([9]))
        with pytest.raises(RuntimeError, match="prefetch"):
            embed.expire_server_model(max_age=0)
        emb.variable._prefetched.clear()
        r = embed.expire_server_model(max_age=0)
        assert r == {"before": 2, "rows": 2}
        assert sorted(sh.export_rows()[0].tolist()) == [2, 3, 9]
    finally:
        os.environ.pop("OEAMD_DEVICE", None)
        if ctxmod._context is not None:
            ctxmod._context.finalize()
        ctxmod._context = old


def test_expire_online_example():
    env = dict(os.environ, OMP_NUM_THREADS="2", OEAMD_DEVICE="cpu")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "expire_online.py")],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "replica after expiry equals a fresh load: OK" in r.stdout
