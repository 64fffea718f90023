"""Delta checkpoints on the CPU engine (the oracle of the HIP path): stamp
rules, the base + deltas == full dump chain, refusals, an explicit
``since``, and the untouched default-off path. Every comparison is exact:
the feature copies rows and does no arithmetic."""

import json
import os

import pytest
import torch

import delta_ref as dr
from openembedding_amd import checkpoint, flags
from openembedding_amd.context import Context
from openembedding_amd.core.variable import (HASH_VOCAB_THRESHOLD,
                                             VariableMeta, VariableShard)

TABLES = ("hash", "array")


def _shard(table, opt="adagrad"):
    vocab = HASH_VOCAB_THRESHOLD if table == "hash" else 500
    sh = VariableShard(VariableMeta(0, 4, vocabulary_size=vocab))
    sh.set_initializer("normal", mean=0.0, stddev=0.1)
    sh.set_optimizer(opt, learning_rate=0.1)
    sh.track_changes()
    return sh


def _changed(sh, since):
    keys = [k for blk in sh.export_changed(since) for k in blk[0].tolist()]
    assert len(keys) == len(set(keys))
    return set(keys)


# ------------------------------------------------------------ 1. stamp rules

@pytest.mark.parametrize("table", TABLES)
def test_stamp_rules(table):
    sh = _shard(table)
    assert sh.epoch == 1 and sh.row_epoch.dtype == torch.int32
    t = lambda *a: torch.tensor(a, dtype=torch.int64)  # noqa: E731

    # a pull of new keys creates (and stamps) them
    sh.pull(t(3, 9, 27, 81))
    assert _changed(sh, 1) == {3, 9, 27, 81}

    # a pull of existing keys with no push adds nothing
    sh.set_epoch(2)
    sh.pull(t(3, 9))
    sh.pull_readonly(t(3, 9, 100))
    sh.pull_pooled_readonly(t(3, 9, 100), t(0, 2, 3), "sum")
    assert _changed(sh, 2) == set()
    assert _changed(sh, 1) == {3, 9, 27, 81}

    # push then update stamps the pushed keys (one of them new)
    sh.push(t(9, 27, 200), torch.ones(3, 4), t(1, 1, 1))
    sh.update_weights()
    assert _changed(sh, 2) == {9, 27, 200}

    # import_rows stamps what it writes, existing or new
    sh.set_epoch(3)
    sh.import_rows(t(81, 300), torch.zeros(2, 4))
    assert _changed(sh, 3) == {81, 300}
    assert _changed(sh, 2) == {9, 27, 200, 81, 300}

    # an optimizer of the same kind keeps the state: nothing stamped
    sh.set_epoch(4)
    sh.set_optimizer("adagrad", learning_rate=0.5)
    assert _changed(sh, 4) == set()
    # another kind rebuilds the state block of every live row
    sh.set_optimizer("adam", learning_rate=0.1)
    assert _changed(sh, 4) == {3, 9, 27, 81, 200, 300}

    # the slab growing keeps the stamps
    if table == "hash":
        sh.set_epoch(5)
        sh.pull(torch.arange(1000, 3000, dtype=torch.int64))
        assert sh.row_epoch.numel() == sh.weights.shape[0]
        assert _changed(sh, 5) == set(range(1000, 3000))
        assert _changed(sh, 4) >= {3, 9, 27, 81, 200, 300}

    sh.clear()
    assert _changed(sh, 0) == set()
    assert int(sh.row_epoch.abs().sum()) == 0
    sh.pull(t(3))
    assert _changed(sh, 1) == {3}


@pytest.mark.parametrize("table", TABLES)
def test_stamp_scenario_matches_the_sets_computed_by_hand(table):
    """The scenario that the GPU shard is held to (tests/test_gpu_delta.py),
    on the oracle."""
    vocab = HASH_VOCAB_THRESHOLD if table == "hash" else 4000
    sh = VariableShard(VariableMeta(0, 4, vocabulary_size=vocab))
    sh.set_optimizer("adagrad", learning_rate=0.1)
    sh.track_changes()
    assert dr.stamp_scenario(sh, 2000) == dr.stamp_scenario_by_hand(2000)


@pytest.mark.parametrize("table", TABLES)
def test_export_changed_blocks_in_slot_order(table, monkeypatch):
    monkeypatch.setattr(checkpoint, "BLOCK_ROWS", 7)
    sh = _shard(table, "adam")
    keys = torch.tensor([40, 2, 33, 8, 21, 5, 13, 1, 34, 3, 55, 89, 144,
                         233, 377, 4, 6, 10, 12, 14], dtype=torch.int64)
    sh.pull(keys)
    blocks = list(sh.export_changed(1))
    assert [b[0].numel() for b in blocks] == [7, 7, 6]
    got = torch.cat([b[0] for b in blocks])
    want = keys if table == "hash" else keys.sort().values   # slot order
    assert torch.equal(got, want)
    assert torch.equal(torch.cat([b[1] for b in blocks]),
                       sh.pull_readonly(want))
    assert all(b[2].shape == (b[0].numel(), sh.state_dim) for b in blocks)
    assert all(b[2] is None
               for b in sh.export_changed(1, include_state=False))


def test_tracking_off_by_default_and_untrackable_shards():
    sh = VariableShard(VariableMeta(0, 4))
    assert not sh.tracking and not hasattr(sh, "row_epoch")
    with pytest.raises(RuntimeError):
        sh.select_changed(1)
    sh.track_changes()
    sh.track_changes(False)
    assert not sh.tracking and not hasattr(sh, "row_epoch")

    from openembedding_amd.core.quantized import QuantizedShard
    from openembedding_amd.core.tiered import TieredVariableShard
    q = QuantizedShard(VariableMeta(0, 4), "int8")
    with pytest.raises(NotImplementedError):
        q.track_changes()
    tiered = TieredVariableShard(VariableMeta(0, 4), cache_rows=1024)
    with pytest.raises(NotImplementedError):
        tiered.track_changes()
    assert not tiered.tracking


# ------------------------------------------------------ 2. chain equivalence

@pytest.mark.parametrize("opt", ("adagrad", "adam"))
@pytest.mark.parametrize("table", TABLES)
def test_chain_equals_full_dump(tmp_path, table, opt):
    ctx, st, var, info = dr.run_chain(tmp_path, "cpu", table, opt)
    uri = info["uri"]
    # exact content of each delta ("dump everything" cannot pass)
    assert info["d1"] == {"since": 2, "epoch": 2, "rows": len(dr.KEYS_B)}
    assert info["d2"] == {"since": 3, "epoch": 3,
                          "rows": len(set(dr.KEYS_C))}
    _, k1 = dr.dump_rows(uri["D1"])
    _, k2 = dr.dump_rows(uri["D2"])
    assert sorted(k1) == sorted(dr.KEYS_B) and len(k1) == 150
    assert sorted(k2) == sorted(set(dr.KEYS_C))
    meta = checkpoint.read_meta(uri["D1"])
    assert meta["delta"] == {"since": 2, "epoch": 2,
                             "model_uuid": ctx.model_uuid}
    hdrs = {json.dumps(h, sort_keys=True)
            for h, *_ in checkpoint.iter_blocks(uri["D1"])}
    assert len(hdrs) == 1
    hdr = json.loads(hdrs.pop())
    assert hdr["delta"] is True and hdr["num_items"] == 150
    assert hdr["state_dim"] == var.shard.state_dim > 0
    base = checkpoint.read_meta(uri["A"])
    assert base["epoch"] == 1 and base["model_uuid"] == ctx.model_uuid
    assert checkpoint.read_meta(uri["B"])["epoch"] == 4
    assert var.shard.epoch == 5

    c1, _, v1 = dr.make_consumer("cpu", table, opt)
    checkpoint.load_model(c1, uri["A"])
    assert c1.loaded_epoch == 1
    checkpoint.apply_delta(c1, uri["D1"])
    assert c1.loaded_epoch == 2
    checkpoint.apply_delta(c1, uri["D2"])
    assert c1.loaded_epoch == 3

    c2, _, v2 = dr.make_consumer("cpu", table, opt)
    checkpoint.load_model(c2, uri["B"])
    got, want = dr.rows_by_key(v1.shard), dr.rows_by_key(v2.shard)
    assert want[2] is not None and want[0].numel() == 1060
    dr.assert_same_rows(got, want)
    dr.assert_same_rows(got, dr.rows_by_key(var.shard))


def test_delta_file_is_reproducible(tmp_path):
    a = dr.run_chain(tmp_path / "r1")[3]["uri"]
    b = dr.run_chain(tmp_path / "r2")[3]["uri"]
    for name in ("D1", "D2"):
        fa, fb = dr.all_files(a[name]), dr.all_files(b[name])
        fa.pop("model_meta"), fb.pop("model_meta")   # holds the random uuid
        assert fa == fb and fa


def test_tracking_trainer_continues_a_loaded_chain(tmp_path):
    """A restarted trainer loads the base, keeps training and cuts a delta
    that a replica of the ORIGINAL base accepts; the loaded base itself is
    not re-emitted."""
    ctx, st, var, info = dr.run_chain(tmp_path)
    uri = info["uri"]
    c, st2, v = dr.make_trainer()
    checkpoint.load_model(c, uri["B"])
    assert v.shard.epoch == 5 and c.model_uuid == ctx.model_uuid
    dr.train(st2, v, [1, 2, 3, 5000], 9)
    d = checkpoint.dump_delta(c, str(tmp_path / "D3"))
    assert d == {"since": 5, "epoch": 5, "rows": 4}
    replica, _, rv = dr.make_consumer()
    checkpoint.load_model(replica, uri["B"])
    checkpoint.apply_delta(replica, str(tmp_path / "D3"))
    dr.assert_same_rows(dr.rows_by_key(rv.shard), dr.rows_by_key(v.shard))


# ------------------------------------------------------------- 3. refusals

def test_refusals_change_nothing(tmp_path):
    ctx, st, var, info = dr.run_chain(tmp_path)
    uri = info["uri"]
    c, _, v = dr.make_consumer()
    checkpoint.load_model(c, uri["A"])
    before = dr.rows_by_key(v.shard)

    def refused(fn, *a):
        with pytest.raises(RuntimeError):
            fn(*a)
        dr.assert_same_rows(dr.rows_by_key(v.shard), before)
        assert c.loaded_epoch == 1

    refused(checkpoint.apply_delta, c, uri["D2"])        # D2 before D1
    refused(checkpoint.apply_delta, c, uri["A"])         # not a delta
    refused(checkpoint.load_model, c, uri["D1"])         # would clear
    # a delta of another model, same epochs
    other = dr.run_chain(tmp_path / "other")[3]["uri"]
    refused(checkpoint.apply_delta, c, other["D1"])

    checkpoint.apply_delta(c, uri["D1"])
    before = dr.rows_by_key(v.shard)
    with pytest.raises(RuntimeError):
        checkpoint.apply_delta(c, uri["D1"])             # twice
    dr.assert_same_rows(dr.rows_by_key(v.shard), before)
    assert c.loaded_epoch == 2

    # a context that loaded nothing, or a base without tracking
    fresh, _, _ = dr.make_consumer()
    with pytest.raises(RuntimeError):
        checkpoint.apply_delta(fresh, uri["D1"])

    # cutting a delta needs tracking
    plain, pst, pvar = dr.make_trainer(track=False)
    dr.train(pst, pvar, [1, 2, 3], 1)
    with pytest.raises(RuntimeError):
        checkpoint.dump_delta(plain, str(tmp_path / "nope"))
    assert not os.path.exists(tmp_path / "nope")
    with pytest.raises(ValueError):
        checkpoint.dump_delta(ctx, str(tmp_path / "nope"), since=99)


# ------------------------------------------------------- 4. explicit since

@pytest.mark.parametrize("table", TABLES)
def test_explicit_since_is_union_of_chain(tmp_path, table):
    ctx, st, var = dr.make_trainer("cpu", table, "adam")
    union = {}
    for i, keys in enumerate((dr.KEYS_A[:300], dr.KEYS_B, dr.KEYS_C)):
        dr.train(st, var, keys, 10 + i)
        uri = str(tmp_path / f"d{i}")
        d = checkpoint.dump_delta(ctx, uri)
        assert d["since"] == d["epoch"] == i + 1
        union.update(dr.dump_rows(uri)[0])     # the last value per key
    big = checkpoint.dump_delta(ctx, str(tmp_path / "big"), since=1)
    assert big == {"since": 1, "epoch": 4, "rows": len(union)}
    rows, order = dr.dump_rows(str(tmp_path / "big"))
    assert len(order) == len(rows)
    assert rows == union
    # a consumer two deltas behind takes it in one go
    c, _, v = dr.make_consumer("cpu", table, "adam")
    ctx0 = checkpoint.read_meta(str(tmp_path / "d0"))["delta"]
    c.loaded_epoch, c.loaded_model_uuid = 0, ctx0["model_uuid"]
    checkpoint.apply_delta(c, str(tmp_path / "big"))
    dr.assert_same_rows(dr.rows_by_key(v.shard), dr.rows_by_key(var.shard))


# ------------------------------------------------ 5. default path untouched

def _seeded_dump(tmp, config):
    old = flags.config
    flags.config = config
    try:
        ctx, st, var = dr.make_trainer(track=False, opt="adam")
    finally:
        flags.config = old
    ctx.model_uuid = "0" * 32
    assert not var.shard.tracking and not hasattr(var.shard, "row_epoch")
    dr.train(st, var, dr.KEYS_A[:200], 4)
    checkpoint.dump_model(ctx, str(tmp))
    return dr.all_files(str(tmp))


def test_tracking_off_dump_is_byte_identical(tmp_path):
    absent = _seeded_dump(tmp_path / "absent", "")
    false = _seeded_dump(tmp_path / "false",
                         '{"server": {"track_changes": false}}')
    assert absent == false and set(absent) == {"model_meta", "0/model_0_0"}
    # and it is the format from before tracking existed: no new field
    meta = json.loads(absent["model_meta"])
    assert list(meta) == ["model_sign", "version", "num_storages",
                          "world_size", "variables"]
    hdr = next(checkpoint.iter_blocks(str(tmp_path / "absent")))[0]
    assert list(hdr) == ["variable_id", "datatype", "embedding_dim",
                         "vocabulary_size", "state_dim", "optimizer",
                         "initializer", "shard_id", "shard_num", "num_items"]


def test_config_knob_and_public_surface(tmp_path):
    import openembedding_amd.torch as embed
    old = flags.config
    flags.config = '{"server": {"track_changes": true}}'
    try:
        e = embed.Embedding(-1, 4)
    finally:
        flags.config = old
    assert e.variable.sharded.shard.tracking
    embed.track_server_model_changes(False)
    assert not e.variable.sharded.shard.tracking
    with pytest.raises(RuntimeError):
        embed.save_server_model_delta(str(tmp_path / "x"))
    embed.track_server_model_changes()
    e2 = embed.Embedding(300, 4)            # created later: tracked too
    assert e2.variable.sharded.shard.tracking
    for emb in (e, e2):
        emb.variable.set_optimizer("sgd", learning_rate=0.1)
    e(torch.tensor([1, 2, 3])).sum().backward()
    embed.get_context().update_all_weights()
    embed.save_server_model(str(tmp_path / "base"))
    e(torch.tensor([2, 50])).sum().backward()
    e2(torch.tensor([7])).sum().backward()
    embed.get_context().update_all_weights()
    want = [e.variable.sparse_read(torch.tensor([1, 2, 3, 50])).clone(),
            e2.variable.sparse_read(torch.tensor([7])).clone()]
    d = embed.save_server_model_delta(str(tmp_path / "d"))
    assert d == {"since": 2, "epoch": 2, "rows": 3}
    embed.load_server_model(str(tmp_path / "base"))
    assert not torch.equal(
        e.variable.sparse_read(torch.tensor([1, 2, 3, 50])), want[0])
    embed.load_server_model_delta(str(tmp_path / "d"))
    assert torch.equal(
        e.variable.sparse_read(torch.tensor([1, 2, 3, 50])), want[0])
    assert torch.equal(e2.variable.sparse_read(torch.tensor([7])), want[1])


def test_config_knob_refuses_tiered_variables():
    old = flags.config
    flags.config = ('{"server": {"track_changes": true, '
                    '"cache_size_mb": 1}}')
    try:
        ctx = Context(device="cpu")
    finally:
        flags.config = old
    with pytest.raises(NotImplementedError):
        ctx.create_storage().create_variable(-1, 4)
