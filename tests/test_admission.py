"""Feature admission on the CPU engine: the count-min filter in front of a
hashed row's creation, against the independent emulation in
admission_ref.py, through the shard, the checkpoint and the public layers."""

import os
import socket
import subprocess
import sys
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import admission_ref as ar
from openembedding_amd import checkpoint
from openembedding_amd.context import Context
from openembedding_amd.core.tiered import TieredVariableShard
from openembedding_amd.core.variable import VariableMeta, VariableShard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 8


def _shard(min_count=None, W=4096, D=4, seed=7, **kw):
    sh = VariableShard(VariableMeta(0, DIM), **kw)
    sh.set_initializer("uniform", minval=-1.0, maxval=1.0)
    sh.set_optimizer("adagrad", learning_rate=0.1)
    if min_count:
        sh.set_admission(min_count, width=W, depth=D, seed=seed)
    return sh


def _step(sh, keys, seed=0):
    """pull + push of a seeded gradient + commit; returns the pulled rows."""
    g = torch.Generator().manual_seed(seed)
    rows = sh.pull(keys)
    sh.push(keys, torch.randn(keys.numel(), DIM, generator=g),
            torch.ones(keys.numel(), dtype=torch.int64))
    sh.update_weights()
    return rows


def _keys_of(sh):
    return sh.export_rows()[0].sort().values


# ------------------------------------------------------- reference stream

def test_reference_stream_figures():
    """The figures the feature was specified with."""
    assert len(ar.exact_counts()) == 2494
    wide, narrow = ar.stream_result(65536), ar.stream_result(4096)
    exact3 = {k for k, c in ar.exact_counts().items() if c >= 3}
    assert wide.admitted == 1174 and wide.turned_away == 4298
    assert set(wide.index) == exact3
    assert narrow.admitted == 1194 and set(narrow.index) > exact3


@pytest.mark.parametrize("W", (65536, 4096))
def test_stream_matches_emulation(W):
    ref = ar.stream_result(W)
    sh = _shard(ar.STREAM_MIN_COUNT, W, ar.STREAM_D, ar.STREAM_SEED)
    for i, ks in enumerate(ar.reference_stream()):
        _step(sh, ks, i)
    assert torch.equal(_keys_of(sh), ref.keys())
    assert torch.equal(sh.export_admission(), torch.from_numpy(ref.sketch))
    st = sh.admission_stats()
    assert (st["admitted"], st["turned_away"]) == (ref.admitted,
                                                   ref.turned_away)
    assert st["min_count"] == 3 and st["width"] == W and st["depth"] == 4
    assert st["fill"] == float((ref.sketch != 0).mean())
    if W == 65536:
        want = sorted(k for k, c in ar.exact_counts().items() if c >= 3)
        assert _keys_of(sh).tolist() == want


# ------------------------------------------------------------- semantics

def test_unadmitted_key_is_a_zero_row_and_leaves_nothing(tmp_path):
    ctx = Context(device="cpu")
    st = ctx.create_storage()
    var = st.create_variable(-1, DIM)
    var.set_initializer("uniform", minval=-1.0, maxval=1.0)
    var.set_optimizer("adagrad", learning_rate=0.1)
    var.set_admission(2, width=4096)
    sh = var.shard
    keys = torch.tensor([5, 9, 11])
    rows = _step(sh, keys)
    assert rows.shape == (3, DIM) and not rows.any()
    assert sh.num_rows == 0 and sh.export_rows()[0].numel() == 0
    checkpoint.dump_model(ctx, str(tmp_path / "A"))
    assert not list(checkpoint.iter_blocks(str(tmp_path / "A")))
    # the second sighting admits: initial row, then it trains
    rows = sh.pull(keys)
    assert sh.num_rows == 3 and rows.abs().sum(1).min() > 0
    before = sh.pull_readonly(keys)
    _step(sh, keys)
    assert not torch.equal(sh.pull_readonly(keys), before)
    # read-only pulls never count
    for _ in range(3):
        assert not sh.pull_readonly(torch.tensor([77])).any()
    assert not sh.pull(torch.tensor([77])).any()
    ctx.finalize()


def test_min_count_1_equals_no_admission_row_for_row():
    a, b = _shard(), _shard(1)
    for i, ks in enumerate(ar.reference_stream()[:4]):
        ra, rb = _step(a, ks, i), _step(b, ks, i)
        assert torch.equal(ra, rb)
    for x, y in zip(a.export_rows(), b.export_rows()):
        assert torch.equal(x, y)          # same keys in the same slots
    assert b.admission_stats()["turned_away"] == 0


def test_push_without_pull_is_dropped():
    sh = _shard(2)
    keys = torch.tensor([1, 2, 3])
    sh.pull(keys[:1])
    sh.pull(keys[:1])                     # key 1 admitted, 2 and 3 unseen
    w0 = sh.pull_readonly(keys)
    sketch0 = sh.export_admission()
    sh.push(keys, torch.ones(3, DIM), torch.ones(3, dtype=torch.int64))
    sh.push(keys[1:], torch.ones(2, DIM), torch.ones(2, dtype=torch.int64))
    sh.update_weights()
    w1 = sh.pull_readonly(keys)
    assert sh.num_rows == 1 and not w1[1:].any()
    assert not torch.equal(w1[0], w0[0])
    assert torch.equal(sh.export_admission(), sketch0)   # no sighting


def test_import_rows_bypasses_admission():
    sh = _shard(5)
    keys = torch.tensor([10, 20, 30])
    w = torch.arange(3 * DIM, dtype=torch.float32).reshape(3, DIM)
    sh.import_rows(keys, w)
    assert sh.num_rows == 3 and torch.equal(sh.pull(keys), w)
    assert not sh.export_admission().any()


@pytest.mark.parametrize("shift", (1, 2, 31, 40))
def test_age_is_a_right_shift(shift):
    sh = _shard(3, W=256)
    for ks in ar.reference_stream()[:6]:
        sh.pull(ks)
    before = sh.export_admission()
    assert int(before.max()) >= 4
    sh.age_admission(shift)
    want = torch.zeros_like(before) if shift >= 31 else before >> shift
    assert torch.equal(sh.export_admission(), want)


def test_off_by_default_and_switching_off_frees_the_sketch():
    sh = _shard()
    assert sh._admit is None and not hasattr(sh, "admit_sketch")
    assert sh.export_admission() is None
    assert sh.admission_stats()["min_count"] == 0
    with pytest.raises(RuntimeError):
        sh.age_admission()
    sh.set_admission(2, width=64)
    assert sh.admit_sketch.numel() == 4 * 64
    assert sh.admit_sketch.dtype == torch.int32
    sh.set_admission(0)
    assert sh._admit is None and not hasattr(sh, "admit_sketch")
    assert sh.pull(torch.tensor([3])).any()      # plain insert again


def test_set_admission_validates():
    sh = _shard()
    for bad in (dict(width=100), dict(depth=0), dict(depth=9)):
        with pytest.raises(ValueError):
            sh.set_admission(2, **bad)
    with pytest.raises(ValueError):
        sh.set_admission(-1)
    arr = VariableShard(VariableMeta(0, DIM, vocabulary_size=100))
    with pytest.raises(ValueError, match="preallocated"):
        arr.set_admission(2)
    tier = TieredVariableShard(VariableMeta(0, DIM), cache_rows=1024)
    with pytest.raises(NotImplementedError):
        tier.set_admission(2)


def test_default_seed_is_the_variables():
    sh = _shard()
    sh.set_admission(2, width=64)
    assert sh._admit["seed"] == sh.seed


# ------------------------------------------------------- expiry and deltas

def test_expired_key_returns_at_once_unless_aged():
    sh = _shard(2, W=65536)
    sh.track_changes()
    keys = torch.tensor([4, 8])
    _step(sh, keys)
    _step(sh, keys)
    assert sh.num_rows == 2
    sh.set_epoch(2)
    assert sorted(sh.expire_rows(2).tolist()) == [4, 8]
    assert sh.num_rows == 0
    assert sh.pull(keys[:1]).any() and sh.num_rows == 1   # counters kept
    sh.age_admission(31)
    assert not sh.pull(keys[1:]).any() and sh.num_rows == 1
    assert sh.pull(keys[1:]).any() and sh.num_rows == 2   # earned again


def test_delta_after_admission_carries_the_new_rows(tmp_path):
    ctx = Context(device="cpu")
    st = ctx.create_storage()
    var = st.create_variable(-1, DIM)
    var.set_initializer("uniform", minval=-1.0, maxval=1.0)
    var.set_optimizer("adagrad", learning_rate=0.1)
    var.shard.track_changes()
    var.set_admission(2, width=65536)
    a, b = torch.tensor([1, 2, 3]), torch.tensor([3, 4, 5])
    _step(var.shard, a, 1)
    _step(var.shard, a, 2)                      # 1 2 3 admitted
    _step(var.shard, b, 3)                      # 4 5 seen once
    checkpoint.dump_model(ctx, str(tmp_path / "A"))
    _step(var.shard, b, 4)                      # 4 5 admitted
    r = checkpoint.dump_delta(ctx, str(tmp_path / "D"))
    assert r["rows"] == 3
    got = {int(k) for _h, ks, _w, _s in
           checkpoint.iter_blocks(str(tmp_path / "D")) for k in ks}
    assert got == {3, 4, 5}
    assert not os.path.exists(tmp_path / "D" / "0" / "admission_0")
    ctx.finalize()


# ---------------------------------------------------------------- checkpoint

def _ctx_var(rank=0, world=1, admission=None):
    """A CPU context posing as ``rank`` of ``world`` (no process group: only
    the shard layer and the checkpoint are driven)."""
    ctx = Context(device="cpu")
    ctx.rank, ctx.world_size = rank, world
    st = ctx.create_storage()
    var = st.create_variable(-1, DIM)
    var.set_initializer("uniform", minval=-1.0, maxval=1.0)
    var.set_optimizer("adagrad", learning_rate=0.1)
    if admission:
        var.set_admission(**admission)
    return ctx, st, var


ADM = {"min_count": 3, "width": 4096, "depth": 4, "seed": 7}


def test_checkpoint_roundtrip_same_shard_count(tmp_path):
    uri = str(tmp_path / "A")
    ctx, st, var = _ctx_var(admission=ADM)
    for i, ks in enumerate(ar.reference_stream()[:6]):
        _step(var.shard, ks, i)
    checkpoint.dump_model(ctx, uri)
    assert os.path.exists(os.path.join(uri, "0", "admission_0"))
    ctx2, st2, var2 = _ctx_var()
    assert var2.shard._admit is None
    checkpoint.load_model(ctx2, uri)
    assert var2.shard._admit == var.shard._admit == ADM
    assert torch.equal(var2.shard.export_admission(),
                       var.shard.export_admission())
    a, b = var.shard.export_rows(), var2.shard.export_rows()
    oa, ob = a[0].argsort(), b[0].argsort()
    for x, y in zip(a, b):
        assert torch.equal(x[oa], y[ob])
    # both continue alike
    ks = ar.reference_stream()[6]
    assert torch.equal(_step(var.shard, ks, 9), _step(var2.shard, ks, 9))
    assert torch.equal(_keys_of(var.shard), _keys_of(var2.shard))
    ctx.finalize()
    ctx2.finalize()


def test_checkpoint_without_admission_loads_as_before(tmp_path):
    uri = str(tmp_path / "A")
    ctx, st, var = _ctx_var()
    _step(var.shard, torch.tensor([1, 2, 3]))
    checkpoint.dump_model(ctx, uri)
    assert os.listdir(os.path.join(uri, "0")) == ["model_0_0"]
    ctx2, st2, var2 = _ctx_var(admission=dict(ADM, min_count=2))
    var2.shard.pull(torch.tensor([50]))
    sketch = var2.shard.export_admission()
    checkpoint.load_model(ctx2, uri)
    assert var2.shard.num_rows == 3 and var2.shard._admit["min_count"] == 2
    assert torch.equal(var2.shard.export_admission(), sketch)
    ctx.finalize()
    ctx2.finalize()


def _two_shard_dump(uri, widths=(4096, 4096), min_count=3):
    """Ranks 0 and 1 of a world-2 run, one after the other: each pulls the
    keys it owns of the stream's first six pulls, then dumps."""
    sketches = []
    for rank in (0, 1):
        ctx, st, var = _ctx_var(rank, 2, dict(ADM, width=widths[rank],
                                              min_count=min_count))
        for ks in ar.reference_stream()[:6]:
            var.shard.pull(ks[ks % 2 == rank])
        checkpoint.dump_model(ctx, uri)
        sketches.append(var.shard.export_admission())
        ctx.finalize()
    return sketches


def test_two_shard_dump_loads_as_the_sum_into_one(tmp_path):
    uri = str(tmp_path / "A")
    s0, s1 = _two_shard_dump(uri)
    ctx, st, var = _ctx_var()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        checkpoint.load_model(ctx, uri)
    assert var.shard._admit == ADM and var.shard.num_rows > 0
    assert s0.any() and s1.any()
    assert torch.equal(var.shard.export_admission(), s0 + s1)
    ctx.finalize()


def test_sum_of_sketches_is_the_sketch_of_the_joined_stream(tmp_path):
    """With nothing admitted on the way (every sighting counts), and from a
    dump that holds no rows at all."""
    uri = str(tmp_path / "A")
    s0, s1 = _two_shard_dump(uri, min_count=100)
    ctx, st, var = _ctx_var()
    checkpoint.load_model(ctx, uri)
    assert var.shard._admit == dict(ADM, min_count=100)
    one = _shard(100, seed=7)
    for ks in ar.reference_stream()[:6]:
        one.pull(ks)
    assert torch.equal(var.shard.export_admission(), one.export_admission())
    ctx.finalize()


def test_mismatched_width_starts_empty_with_a_warning(tmp_path):
    uri = str(tmp_path / "A")
    _two_shard_dump(uri, widths=(4096, 2048))
    ctx, st, var = _ctx_var()
    with pytest.warns(UserWarning, match="cannot be summed"):
        checkpoint.load_model(ctx, uri)
    assert var.shard._admit is not None
    assert not var.shard.export_admission().any()
    assert var.shard.num_rows > 0          # the rows still load
    ctx.finalize()


# ------------------------------------------------------------ public layers

@pytest.fixture
def cpu_context():
    from openembedding_amd import context as ctxmod
    old = ctxmod._context
    ctxmod._context = None
    os.environ["OEAMD_DEVICE"] = "cpu"
    try:
        yield
    finally:
        os.environ.pop("OEAMD_DEVICE", None)
        if ctxmod._context is not None:
            ctxmod._context.finalize()
        ctxmod._context = old


@pytest.mark.parametrize("layer", ("embedding", "bag", "combined"))
def test_layers_end_to_end(cpu_context, layer):
    import openembedding_amd.torch as embed
    adm = {"min_count": 2, "width": 4096}
    if layer == "embedding":
        emb = embed.Embedding(-1, 8, admission=adm)
        args = (torch.tensor([[3, 5], [5, 9]]),)
    elif layer == "bag":
        emb = embed.EmbeddingBag(-1, 8, mode="mean", admission=adm)
        args = (torch.tensor([3, 5, 5, 9]), torch.tensor([0, 1, 4]))
    else:
        emb = embed.CombinedEmbedding([10, 10], 8, hash_mode=True,
                                      admission=adm)
        args = (torch.tensor([[3, 5], [5, 9]]),)
    opt = embed.distributed_optimizer(
        torch.optim.SGD(list(emb.parameters()), lr=0.1))
    sh = emb.variable.sharded.shard

    def step():
        opt.zero_grad()
        out = emb(*args)
        out.sum().backward()
        opt.step()
        return out.detach().clone()

    assert not step().any() and sh.num_rows == 0
    out = step()
    assert out.abs().sum(-1).min() > 0 and sh.num_rows > 0
    rows = sh.export_rows()[1].clone()
    assert not torch.equal(step(), out)               # the rows train
    assert not torch.equal(sh.export_rows()[1], rows)
    st = embed.admission_stats()
    assert list(st) == [sh.meta.variable_id]
    assert st[sh.meta.variable_id]["admitted"] == sh.num_rows
    assert st[sh.meta.variable_id]["turned_away"] == sh.num_rows
    embed.age_admission_filters(31)
    assert not sh.export_admission().any()


def test_array_layer_refuses_admission(cpu_context):
    import openembedding_amd.torch as embed
    with pytest.raises(ValueError):
        embed.Embedding(100, 8, admission={"min_count": 2})


def test_config_key_applies_to_new_hash_variables(cpu_context):
    import openembedding_amd as oe
    import openembedding_amd.torch as embed
    old = oe.flags.config
    oe.flags.config = "server:\n  admission_min_count: 3\n"
    try:
        h = embed.Embedding(-1, 4)
        a = embed.Embedding(50, 4)
        assert h.variable.sharded.shard._admit["min_count"] == 3
        assert a.variable.sharded.shard._admit is None
    finally:
        oe.flags.config = old


def test_metrics_route_reports_admission(cpu_context):
    from fastapi.testclient import TestClient

    import openembedding_amd.torch as embed
    from openembedding_amd.serving import ModelController, make_app
    emb = embed.Embedding(-1, 4, admission={"min_count": 2, "width": 64})
    sh = emb.variable.sharded.shard
    sh.pull(torch.tensor([1, 2, 3]))
    sh.pull(torch.tensor([1, 2]))
    text = TestClient(make_app(ModelController(device="cpu"))).get(
        "/metrics").text
    vid = sh.meta.variable_id
    assert f'openembedding_admission{{variable="{vid}",stat="admitted"}} 2' \
        in text
    assert f'openembedding_admission{{variable="{vid}",' \
        f'stat="turned_away"}} 3' in text


# ------------------------------------------------------------- gloo world 2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_trainer(rank, world, port, tmp):
    for k, v in (("RANK", rank), ("WORLD_SIZE", world), ("LOCAL_RANK", rank),
                 ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", port)):
        os.environ[k] = str(v)
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method=f"tcp://127.0.0.1:{port}")
    ctx = Context(device="cpu")
    st = ctx.create_storage()
    var = st.create_variable(-1, DIM)
    var.set_initializer("uniform", minval=-1.0, maxval=1.0)
    var.set_optimizer("adagrad", learning_rate=0.1)
    var.set_admission(ar.STREAM_MIN_COUNT, width=65536, depth=ar.STREAM_D,
                      seed=ar.STREAM_SEED)
    for ks in ar.reference_stream():
        # every rank feeds the same batch: one sighting per owner and pull
        # needs the batch once, so rank 1 sends an empty one
        mine = ks if rank == 0 else ks[:0]
        out, h = var.pull(mine)
        var.push(h, torch.ones_like(out))
        st.update_weights()
    torch.save({"keys": var.shard.export_rows()[0],
                "stats": var.shard.admission_stats()},
               os.path.join(tmp, f"final_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_world2_admits_what_one_shard_admits(tmp_path):
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
    for r, f in enumerate(finals):
        assert f["keys"].numel() and bool((f["keys"] % 2 == r).all())
    union = torch.cat([f["keys"] for f in finals]).sort().values
    assert torch.equal(union, ar.stream_result(65536).keys())
    assert sum(f["stats"]["admitted"] for f in finals) == 1174
    assert sum(f["stats"]["turned_away"] for f in finals) == 4298


# -------------------------------------------------------------------- example

def test_admit_online_example():
    env = dict(os.environ, OMP_NUM_THREADS="2", OEAMD_DEVICE="cpu")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "admit_online.py")],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "admission kept the table small: OK" in r.stdout
