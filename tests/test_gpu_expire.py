"""Row expiry on the GPU: HipVariableShard against the CPU shard fed the same
operations, slot for slot. The kernels copy rows and do no arithmetic, so
every comparison of a removal is exact (``torch.equal``); only the training
steps after an expiry use the optimizer tolerance of test_gpu_numerics.py.
Shapes sit at the edges of the compaction tile and of the row-move groups."""

import pytest
import torch

import delta_ref as dr
from openembedding_amd import checkpoint
from openembedding_amd.core.quantized import QuantizedShard
from openembedding_amd.core.variable import VariableMeta, VariableShard

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HASH = 1 << 63


@pytest.fixture(scope="module")
def ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _hip(vocab, dim, opt, **kw):
    from openembedding_amd.core.variable_gpu import HipVariableShard
    return _setup(HipVariableShard(VariableMeta(0, dim,
                                                vocabulary_size=vocab),
                                   device=DEV, **kw), opt)


def _cpu(vocab, dim, opt, **kw):
    return _setup(VariableShard(VariableMeta(0, dim, vocabulary_size=vocab),
                                **kw), opt)


def _setup(sh, opt):
    sh.set_initializer("normal", mean=0.0, stddev=0.1)
    sh.set_optimizer(opt, learning_rate=0.05)
    sh.track_changes()
    return sh


def _step(sh, keys, seed):
    """pull -> push -> commit of unique keys with seeded gradients."""
    g = torch.Generator().manual_seed(seed)
    grads = torch.randn(keys.numel(), sh.dim, generator=g)
    dev = sh.device
    out = sh.pull(keys.to(dev))
    sh.push(keys.to(dev), grads.to(dev),
            torch.ones(keys.numel(), dtype=torch.int64, device=dev))
    sh.update_weights()
    return out


def _trained_rows(n, dim, opt):
    """(keys, weights, state or None) of n rows after one training step on
    the GPU, on the CPU."""
    g = torch.Generator().manual_seed(n * 131 + dim)
    keys = torch.randperm(4 * n + 8, generator=g)[:n] * 5 + 1
    gpu = _hip(HASH, dim, opt)
    _step(gpu, keys, 1)
    k, w, s = gpu.export_rows()
    assert k.numel() == n
    return k.cpu(), w.cpu(), s.cpu() if s is not None else None


def _pair(n, dim, opt, rows=None):
    """A GPU and a CPU shard holding the same n trained rows with the same
    slot layout, bit for bit, and the keys in slot order: the GPU imports
    the rows (a hash insert hands out slots in no fixed order), the CPU
    imports them in the order of the GPU's slots."""
    k, w, s = rows if rows is not None else _trained_rows(n, dim, opt)
    gpu, cpu = _hip(HASH, dim, opt), _cpu(HASH, dim, opt)
    gpu.import_rows(k.to(DEV), w.to(DEV), s.to(DEV) if s is not None
                    else None)
    keys = gpu.slot_keys[:n].cpu()
    by_key = torch.argsort(k)
    sel = by_key[torch.searchsorted(k[by_key], keys)]
    assert torch.equal(k[sel], keys)
    cpu.import_rows(keys, w[sel], s[sel] if s is not None else None)
    return gpu, cpu, keys


def _restamp(gpu, cpu, keys, dead):
    """Epoch 2: every survivor is written again (re-imported), on both."""
    for sh in (gpu, cpu):
        sh.set_epoch(2)
    keep = keys[~dead]
    if keep.numel():
        w = gpu.pull_readonly(keep.to(DEV))
        slots = gpu._lookup_readonly(keep.to(DEV))
        s = gpu.state[slots] if gpu.state_dim else None
        gpu.import_rows(keep.to(DEV), w, s)
        cpu.import_rows(keep, w.cpu(), s.cpu() if s is not None else None)


def _assert_same_slab(gpu, cpu):
    n2 = cpu._nrows
    assert int(gpu.nrows_dev.item()) == gpu.num_rows == n2
    assert gpu._nrows_exact == gpu._nrows_upper == n2
    assert torch.equal(gpu.slot_keys[:n2].cpu(), cpu._slot_key_list())
    assert torch.equal(gpu.weights[:n2].cpu(), cpu.weights[:n2])
    assert torch.equal(gpu.state[:n2].cpu(), cpu.state[:n2])
    assert torch.equal(gpu.row_epoch[:n2].cpu(), cpu.row_epoch[:n2])


def _ptrs(sh):
    names = ("weights", "state", "slot_keys", "row_epoch", "tk", "tv",
             "nrows_dev", "slab", "valid_u8")
    return {n: getattr(sh, n).data_ptr() for n in names if hasattr(sh, n)}


def _dead_patterns(n, g):
    idx = torch.arange(n)
    return {
        "none": torch.zeros(n, dtype=torch.bool),
        "all": torch.ones(n, dtype=torch.bool),
        "first": idx == 0,
        "last": idx == n - 1,
        "tail": idx >= n - max(1, n // 3),
        "head": idx <= n // 2,
        "alternating": idx % 2 == 1,
        "random": torch.rand(n, generator=g) < 0.5,
    }


SIZES = ("1", "63", "64", "65", "T-1", "T", "T+1", "2T+17", "5000")
SHAPES = [("sgd", 1), ("sgd", 9), ("sgd", 64), ("adagrad", 1),
          ("adagrad", 9), ("adagrad", 64), ("adam", 1), ("adam", 9),
          ("adam", 64)]


def _size(ext, name):
    tile = int(ext.DELTA_TILE_ROWS)
    return {"T-1": tile - 1, "T": tile, "T+1": tile + 1,
            "2T+17": 2 * tile + 17}.get(name) or int(name)


@pytest.mark.parametrize("opt,dim", SHAPES,
                         ids=[f"{o}-{d}" for o, d in SHAPES])
@pytest.mark.parametrize("size", SIZES)
def test_expire_layout_matches_cpu(ext, size, opt, dim):
    n = _size(ext, size)
    g = torch.Generator().manual_seed(n)
    rows = _trained_rows(n, dim, opt)
    for name, dead in _dead_patterns(n, g).items():
        gpu, cpu, keys = _pair(n, dim, opt, rows)
        _restamp(gpu, cpu, keys, dead)
        ptrs = _ptrs(gpu)
        got = gpu.expire_rows(2)
        want = cpu.expire_rows(2)
        tag = (n, opt, dim, name)
        assert got.is_cuda and got.dtype == torch.int64, tag
        assert torch.equal(got.cpu(), want), tag
        assert torch.equal(want, keys[dead]), tag
        assert cpu._nrows == n - int(dead.sum()), tag
        _assert_same_slab(gpu, cpu)
        assert _ptrs(gpu) == ptrs, tag            # in place: same storage
        a = gpu.pull_readonly(keys.to(DEV)).cpu()
        assert torch.equal(a, cpu.pull_readonly(keys)), tag
        assert not a[dead].any(), tag
        assert torch.equal(gpu.removed_since(1).cpu(), want), tag


def test_remove_rows_unknown_duplicate_reserved(ext):
    n = int(ext.DELTA_TILE_ROWS) + 40
    gpu, cpu, keys = _pair(n, 9, "adagrad")
    gpu.track_changes(False)
    cpu.track_changes(False)                  # works without tracking
    named = torch.cat([keys[::7], keys[:5], keys[::7][:3],
                       torch.tensor([-1, 10 ** 12, 2, -1])])
    ptrs = _ptrs(gpu)
    got, want = gpu.remove_rows(named.to(DEV)), cpu.remove_rows(named)
    assert torch.equal(got.cpu(), want)
    dead = torch.zeros(n, dtype=torch.bool)
    dead[::7] = True
    dead[:5] = True
    assert torch.equal(want, keys[dead])
    n2 = cpu._nrows
    assert int(gpu.nrows_dev.item()) == n2 == n - int(dead.sum())
    assert torch.equal(gpu.slot_keys[:n2].cpu(), cpu._slot_key_list())
    assert torch.equal(gpu.weights[:n2].cpu(), cpu.weights[:n2])
    assert torch.equal(gpu.state[:n2].cpu(), cpu.state[:n2])
    assert _ptrs(gpu) == ptrs
    assert torch.equal(gpu.pull_readonly(keys.to(DEV)).cpu(),
                       cpu.pull_readonly(keys))
    # nothing left to remove: an empty answer, nothing changes
    assert gpu.remove_rows(named.to(DEV)).numel() == 0
    assert gpu.remove_rows(named[:0].to(DEV)).numel() == 0
    assert int(gpu.nrows_dev.item()) == n2


def test_preconditions_on_the_gpu_shard():
    gpu = _hip(HASH, 4, "adagrad")
    keys = torch.arange(10)
    _step(gpu, keys, 1)
    gpu.push(keys[:2].to(DEV), torch.ones(2, 4, device=DEV),
             torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="queued"):
        gpu.expire_rows(5)
    gpu.update_weights()
    gpu.push_slots(keys[:2].to(DEV), torch.tensor([2], dtype=torch.int32,
                                                  device=DEV),
                   gpu._lookup_readonly(keys[:2].to(DEV)),
                   torch.ones(2, 4, device=DEV),
                   torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="queued"):
        gpu.remove_rows(keys[:1].to(DEV))
    gpu.update_weights()
    gpu.track_changes(False)
    with pytest.raises(RuntimeError, match="tracking"):
        gpu.expire_rows(5)
    from openembedding_amd.core.tiered_gpu import HipTieredVariableShard
    tier = HipTieredVariableShard(VariableMeta(0, 4), device=DEV,
                                  cache_rows=1024)
    with pytest.raises(NotImplementedError):
        tier.expire_rows(1)
    with pytest.raises(NotImplementedError):
        tier.remove_rows(keys.to(DEV))


@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_array_mode_matches_cpu(ext, opt):
    tile = int(ext.DELTA_TILE_ROWS)
    vocab, num, sid = 3 * (tile + 70), 3, 1
    gpu = _hip(vocab, 9, opt, shard_id=sid, shard_num=num)
    cpu = _cpu(vocab, 9, opt, shard_id=sid, shard_num=num)
    g = torch.Generator().manual_seed(5)
    slots = torch.randperm(tile + 70, generator=g)[:tile + 9]
    keys = slots * num + sid
    _step(gpu, keys, 1)
    k, w, s = gpu.export_rows()
    cpu.import_rows(k.cpu(), w.cpu(), s.cpu() if s is not None else None)
    seen = keys[torch.rand(keys.numel(), generator=g) < 0.5]
    for sh in (gpu, cpu):
        sh.set_epoch(2)
        sh.import_rows(seen.to(sh.device),
                       torch.ones(seen.numel(), 9, device=sh.device))
    ptrs, wbits = _ptrs(gpu), gpu.weights.clone()
    got, want = gpu.expire_rows(2), cpu.expire_rows(2)
    assert torch.equal(got.cpu(), want) and want.numel() > 100
    assert torch.equal(want, torch.sort(want).values)
    assert torch.equal(gpu.valid_u8.cpu() != 0, cpu.valid)
    assert torch.equal(gpu.weights, wbits) and _ptrs(gpu) == ptrs
    named = torch.cat([seen[:50], seen[:10], keys[:20],
                       torch.tensor([-1, 0, 2, vocab + 1, 10 ** 12])])
    got, want = gpu.remove_rows(named.to(DEV)), cpu.remove_rows(named)
    assert torch.equal(got.cpu(), want) and want.numel() >= 50
    assert torch.equal(gpu.valid_u8.cpu() != 0, cpu.valid)
    assert gpu.num_rows == cpu.num_rows
    assert torch.equal(gpu.pull_readonly(keys.to(DEV)).cpu(),
                       cpu.pull_readonly(keys))
    assert torch.equal(gpu.removed_since(1).cpu(), cpu.removed_since(1))


@pytest.mark.parametrize("opt", ("sgd", "adagrad", "adam"))
def test_training_goes_on_after_an_expiry(opt):
    """Two more steps after an expiry, over survivors, removed keys (which
    start again from their first-ever row) and new keys, match the CPU shard
    under the optimizer tolerance of test_gpu_numerics.py
    (test_optimizer_parity_engine: pulls rtol 2e-5 / atol 1e-5, final rows
    3e-5)."""
    n, dim = 3000, 9
    gpu, cpu, keys = _pair(n, dim, opt)
    g = torch.Generator().manual_seed(1)
    dead = torch.rand(n, generator=g) < 0.5
    first = gpu.initializer(gpu.seed, keys[dead][:50].to(DEV), dim,
                            gpu.dtype)
    _restamp(gpu, cpu, keys, dead)
    assert torch.equal(gpu.expire_rows(2).cpu(), cpu.expire_rows(2))
    again = gpu.pull(keys[dead][:50].to(DEV))
    assert torch.equal(again, first)           # re-created == first init
    cpu.pull(keys[dead][:50])
    for step in (2, 3):
        batch = torch.cat([keys[torch.randperm(n, generator=g)[:800]],
                           torch.arange(800) * 5 + 3 + 10 ** 6 * step])
        a = _step(cpu, batch, step)
        b = _step(gpu, batch, step).cpu()
        torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-5)
    probe = torch.cat([keys, torch.arange(800) * 5 + 3 + 2 * 10 ** 6])
    torch.testing.assert_close(cpu.pull_readonly(probe),
                               gpu.pull_readonly(probe.to(DEV)).cpu(),
                               rtol=3e-5, atol=3e-5)
    assert gpu.num_rows == cpu.num_rows


def test_graph_captured_before_an_expiry_replays_after_it():
    """A step captured on a reserve_rows shard looks slots up on every
    replay and reads nrows_dev through its pointer: after an expiry, which
    reallocates nothing, it replays without recapture to what an eager twin
    computes, exactly (a batch repeats no key, so the sums are order
    free)."""
    def run(captured):
        ctx, st, var = dr.make_trainer(DEV, "hash", "adagrad", reserve=8192)
        sh = var.shard
        k0 = torch.arange(0, 2000, dtype=torch.int64)
        static_k = k0.to(DEV)
        static_g = torch.randn(2000, dr.DIM,
                               generator=torch.Generator().manual_seed(0)
                               ).to(DEV)

        def step():
            _, h = var.pull(static_k)
            var.push(h, static_g)
            st.update_weights()

        step()
        graph = None
        if captured:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
        else:
            step()

        def feed(lo, seed):
            g = torch.Generator().manual_seed(seed)
            static_k.copy_(torch.arange(lo, lo + 2000).to(DEV))
            static_g.copy_(torch.randn(2000, dr.DIM, generator=g).to(DEV))
            graph.replay() if captured else step()

        sh.set_epoch(2)
        feed(1000, 1)                 # 1000..2999 seen in epoch 2
        ptrs = _ptrs(sh)
        gone = sh.expire_rows(2)      # 0..999 go, the tail fills the holes
        assert sorted(gone.tolist()) == list(range(1000))
        assert _ptrs(sh) == ptrs and sh.num_rows == 2000
        feed(500, 2)                  # 500..999 come back, 1000..2499 move on
        feed(2400, 3)
        torch.cuda.synchronize()
        assert sh.num_rows == 3900
        rows = dr.rows_by_key(sh)
        ctx.finalize()
        return rows

    dr.assert_same_rows(run(True), run(False))


def test_expiry_never_copies_a_slab(ext):
    """The extra device memory is O(rows) small integers: the same at dim 9
    and at dim 64, and far below the slab."""
    rows = 200_000

    def rise(dim):
        sh = _hip(HASH, dim, "adagrad")
        sh.reserve_rows(rows)
        keys = torch.arange(rows, device=DEV)
        sh.import_rows(keys, torch.ones(rows, dim, device=DEV))
        sh.set_epoch(2)
        sh.import_rows(keys[::2].contiguous(),
                       torch.ones(rows // 2, dim, device=DEV))
        R = sh.slot_keys.numel()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        gone = sh.expire_rows(2)
        torch.cuda.synchronize()
        out = torch.cuda.max_memory_allocated() - base
        assert gone.numel() == rows // 2 and sh.num_rows == rows // 2
        return out, R, sh.weights.numel() * 4 + sh.state.numel() * 4

    r9, R9, _ = rise(9)
    r64, R64, slab64 = rise(64)
    assert R9 == R64
    # flags (1 B per slab row), hole and mover lists (int32, at most
    # min(m, n') = rows / 2 entries each), the returned keys (8 B each),
    # and per compaction tile counts + scan + the scan's scratch (an 8-byte
    # descriptor per element is an upper bound), three times; fewer than 32
    # temporaries, each rounded up to 512 B by the allocator
    tiles = -(-R64 // int(ext.DELTA_TILE_ROWS))
    bound = (R64 + 2 * 4 * (rows // 2) + 8 * (rows // 2)
             + 3 * tiles * (4 + 4 + 8) + 32 * 512)
    print(f"expire_rows peak rise: dim 9 {r9} B, dim 64 {r64} B, bound "
          f"{bound} B, slab {slab64} B")
    assert abs(r9 - r64) <= 32 * 512
    assert r64 <= bound < slab64 // 16


def test_removal_is_refused_under_capture():
    gpu = _hip(HASH, 4, "adagrad")
    gpu.reserve_rows(1024)
    keys = torch.arange(10, device=DEV)
    gpu.pull(keys)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="capture"):
            gpu.remove_rows(keys)
        gpu.pull_readonly(keys)
    assert gpu.num_rows == 10


# ---------------------------------------------------------------- serving

@pytest.mark.parametrize("fmt", ("int8", "fp16"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_quantized_remove_rows_equals_the_cpu_form(ext, table, fmt):
    n, dim = int(ext.DELTA_TILE_ROWS) + 77, 9
    vocab = HASH if table == "hash" else 4 * n
    g = torch.Generator().manual_seed(9)
    keys = torch.randperm(4 * n, generator=g)[:n]
    w = torch.randn(n, dim, generator=g)
    qg = QuantizedShard(VariableMeta(0, dim, vocabulary_size=vocab), fmt,
                        device=DEV)
    qg.import_rows(keys.to(DEV), w.to(DEV))
    order = qg.slot_keys[:n].cpu() if table == "hash" else keys
    pos = {int(k): i for i, k in enumerate(keys.tolist())}
    sel = torch.tensor([pos[int(k)] for k in order.tolist()])
    qc = QuantizedShard(VariableMeta(0, dim, vocabulary_size=vocab), fmt)
    qc.import_rows(order, w[sel])
    rows = n if table == "hash" else vocab
    assert torch.equal(qg.slab[:rows].cpu(), qc.slab[:rows])
    named = torch.cat([keys[::3], keys[:40], keys[:9],
                       torch.tensor([-1, 10 ** 12, 4 * n + 5])])
    ptrs = _ptrs(qg)
    got, want = qg.remove_rows(named.to(DEV)), qc.remove_rows(named)
    assert torch.equal(got.cpu(), want) and want.numel() > n // 3
    assert qg.num_rows == qc.num_rows == n - want.numel()
    assert _ptrs(qg) == ptrs
    if table == "hash":
        n2 = qc.num_rows
        assert int(qg.nrows_dev.item()) == n2
        assert torch.equal(qg.slot_keys[:n2].cpu(), qc.slot_keys[:n2])
        assert torch.equal(qg.slab[:n2].cpu(), qc.slab[:n2])
    else:
        assert torch.equal(qg.valid_u8.cpu(), qc.valid_u8)
        assert torch.equal(qg.slab.cpu(), qc.slab)
    assert torch.equal(qg.pull_readonly(keys.to(DEV)).cpu(),
                       qc.pull_readonly(keys))
    assert qg.remove_rows(named.to(DEV)).numel() == 0


@pytest.fixture(scope="module")
def tomb_chain(tmp_path_factory):
    """A: keys 0..1999. D1: 0..999 removed, 400..449 re-created, 5000
    created. B: the full dump at that point. Trained on the GPU."""
    out = {}
    for table in ("hash",):
        tmp = tmp_path_factory.mktemp(f"tomb_{table}")
        ctx, st, var = dr.make_trainer(DEV, table, "adagrad")
        uri = {n: str(tmp / n) for n in ("A", "D1", "B")}
        dr.train(st, var, list(range(2000)), 1)
        checkpoint.dump_model(ctx, uri["A"])
        dr.train(st, var, list(range(1000, 2000)), 2)
        assert checkpoint.expire_rows(ctx, before=2) == \
            {"before": 2, "rows": 1000}
        dr.train(st, var, list(range(400, 450)) + [5000], 3)
        checkpoint.dump_delta(ctx, uri["D1"])
        checkpoint.dump_model(ctx, uri["B"])
        out[table] = (uri, dr.rows_by_key(var.shard))
        ctx.finalize()
    return out


def test_gpu_chain_with_tombstones_equals_full_dump(tomb_chain):
    uri, want = tomb_chain["hash"]
    assert want[0].numel() == 1051
    c1, _, v1 = dr.make_consumer(DEV, "hash", "adagrad")
    checkpoint.load_model(c1, uri["A"])
    checkpoint.apply_delta(c1, uri["D1"])
    c2, _, v2 = dr.make_consumer(DEV, "hash", "adagrad")
    checkpoint.load_model(c2, uri["B"])
    dr.assert_same_rows(dr.rows_by_key(v1.shard), want)
    dr.assert_same_rows(dr.rows_by_key(v2.shard), want)
    removed = sorted(k for _h, ks in checkpoint.iter_removed(uri["D1"])
                     for k in ks.tolist())
    assert removed == list(range(1000))


@pytest.mark.parametrize("fmt", (None, "int8", "fp16"))
def test_served_gpu_model_applies_tombstones(tomb_chain, fmt):
    from openembedding_amd.serving import ServedModel
    uri, _ = tomb_chain["hash"]
    m = ServedModel("live", uri["A"])
    m.load(device=DEV, quantize=fmt)
    sh = m.variables[0].shard
    assert sh.device.type == "cuda" and sh.num_rows == 2000
    r = m.apply_delta(uri["D1"])
    assert r == {"since": 2, "epoch": 2, "rows": 1051, "removed": 1000}
    assert sh.num_rows == 1051
    fresh = ServedModel("fresh", uri["B"])
    fresh.load(device=DEV, quantize=fmt)
    probe = torch.tensor(list(range(2000)) + [5000, 5001])
    got = m.variables[0].pull_weights(probe).cpu()
    assert torch.equal(got, fresh.variables[0].pull_weights(probe).cpu())
    gone = torch.ones(2002, dtype=torch.bool)
    gone[400:450] = False
    gone[1000:2001] = False
    assert not got[gone].any() and got[~gone].abs().sum(1).min() > 0
