"""GPU tests of the fused read-only pooled lookup (all @gpu): k_pool_lookup
against the CPU oracle (exact on integer data) and, bit for bit, against the
unfused GPU route (pull_readonly + pool_fwd); no [nnz, dim] tensor;
hipGraph capture of EmbeddingBag evaluation; the table stays untouched;
unsanitised offsets; serving from HBM; and the capacity tier's override.

The shapes are those of tests/test_gpu_ragged.py (67 bags, edge lengths,
a bag over 256 elements, nnz no multiple of 256, a 37-element -1 tail, a
key shared by many bags, a key repeated inside one bag)."""

import functools

import pytest
import torch

import sparse_core_ref as ref
from test_gpu_ragged import (B, DEV, DIMS, MODES, TAIL, VOCAB, _engine_batches,
                             _make, _problem, _reset, _step)

pytestmark = pytest.mark.gpu

TABLES = ["array", "hash", "hash_full_range", "hash_colliding"]
N_COLL = 24


def _classes():
    from openembedding_amd.core.variable import (HASH_VOCAB_THRESHOLD,
                                                 VariableMeta, VariableShard)
    from openembedding_amd.core.variable_gpu import HipVariableShard
    return HASH_VOCAB_THRESHOLD, VariableMeta, VariableShard, HipVariableShard


@functools.lru_cache(maxsize=None)
def _keymap(table: str) -> torch.Tensor:
    """id in [0, VOCAB) -> table key. ``hash_full_range``: keys over the
    whole signed range (negative ones other than -1 included).
    ``hash_colliding``: the first N_COLL ids — the hot key 7 among them —
    share the home bucket cap-2 of the shard's initial probe table, so
    their chain runs past the table end and wraps."""
    g = torch.Generator().manual_seed(77)
    if table == "hash_full_range":
        km = ref.full_range_keys(VOCAB, g)
    elif table == "hash_colliding":
        cap = _classes()[3].INITIAL_TABLE_CAP
        coll = ref.colliding_keys(cap - 1, [cap - 2], N_COLL,
                                  limit=4_000_000)
        km = torch.arange(VOCAB, dtype=torch.int64) + 5_000_000
        km[:N_COLL] = coll
    else:
        km = torch.arange(VOCAB, dtype=torch.int64)
    assert torch.unique(km).numel() == VOCAB and not bool((km == -1).any())
    return km


def _present() -> torch.Tensor:
    """About one id in nine is absent from the table."""
    return torch.arange(VOCAB) % 9 != 4


def _shards(table: str, rows: torch.Tensor, gpu_only: bool = False):
    """(gpu, cpu) shards holding ``rows[i]`` under key _keymap[i] for the
    present ids."""
    hash_vocab, VariableMeta, VariableShard, HipVariableShard = _classes()
    meta = VariableMeta(variable_id=1, embedding_dim=rows.shape[1],
                        vocabulary_size=(VOCAB if table == "array"
                                         else hash_vocab))
    keys = _keymap(table)[_present()]
    live = rows[_present()]
    gpu = HipVariableShard(meta, device=DEV)
    gpu.import_rows(keys.to(DEV), live.to(DEV))
    if table != "array":
        assert gpu._cap == HipVariableShard.INITIAL_TABLE_CAP
    if gpu_only:
        return gpu, None
    cpu = VariableShard(meta)
    cpu.import_rows(keys, live)
    return gpu, cpu


def _keys_of(table: str, vals: torch.Tensor) -> torch.Tensor:
    km = _keymap(table)
    return torch.where(vals >= 0, km[vals.clamp(min=0)], vals)


def _int_weights(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (n,), generator=g).float()


# ------------------------------------------------------ exact, vs CPU oracle

@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_exact_against_cpu_oracle(dim, mode):
    """Small-integer rows (and weights): fp32 sums are exact in any order
    (mean only with power-of-two lengths), so the fused kernel must equal
    the CPU oracle bit for bit on array and hash tables, with absent keys,
    full-range keys and a probe chain that wraps at the table end."""
    vals, offsets = _problem(pow2=(mode == "mean"), seed=dim)
    g = torch.Generator().manual_seed(dim)
    rows = torch.randint(-8, 9, (VOCAB, dim), generator=g).float()
    w = _int_weights(vals.numel(), dim)
    assert bool((vals[-TAIL:] == -1).all())
    for table in TABLES:
        gpu, cpu = _shards(table, rows)
        if table == "hash_colliding":
            cap = gpu._cap          # the chain occupies both table ends
            assert int(gpu.tk[cap - 1]) != -1 and int(gpu.tk[0]) != -1
        keys = _keys_of(table, vals)
        want = cpu.pull_pooled_readonly(keys, offsets, mode)
        got = gpu.pull_pooled_readonly(keys.to(DEV), offsets.to(DEV), mode)
        assert got.shape == (B, dim)
        assert torch.equal(got.cpu(), want), table
        assert bool((want != 0).any())
        if mode == "sum":       # integer weights keep the weighted sum exact
            want_w = cpu.pull_pooled_readonly(keys, offsets, mode, w)
            got_w = gpu.pull_pooled_readonly(keys.to(DEV), offsets.to(DEV),
                                             mode, w.to(DEV))
            assert torch.equal(got_w.cpu(), want_w), table


# ------------------------------------------- bitwise, vs the unfused kernels

@functools.lru_cache(maxsize=None)
def _random_case(dim: int):
    vals, offsets = _problem(pow2=False, seed=100 + dim)
    g = torch.Generator().manual_seed(200 + dim)
    rows = torch.randn(VOCAB, dim, generator=g)
    w = torch.randn(vals.numel(), generator=g)
    return vals, offsets, rows, w


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", MODES)
def test_bitwise_against_unfused_gpu_route(dim, mode):
    """Random fp32 rows: the fused lookup adds the same rows in the same
    order as ``pull_readonly`` + ``pool_fwd`` / ``pool_fwd_weighted`` (the
    route evaluation took before), so the outputs are bit-identical,
    weighted or not, and the same from run to run."""
    from openembedding_amd.ops import dispatch as ops
    vals, offsets, rows, w = _random_case(dim)
    for table in ("array", "hash_full_range"):
        gpu, _ = _shards(table, rows, gpu_only=True)
        keys = _keys_of(table, vals).to(DEV)
        off, wd = offsets.to(DEV), w.to(DEV)
        flat = gpu.pull_readonly(keys)
        assert flat.shape == (vals.numel(), dim)

        got = gpu.pull_pooled_readonly(keys, off, mode)
        want, _ = ops.pool_fwd(flat, None, None, off, mode)
        assert torch.equal(got, want), table
        assert torch.equal(gpu.pull_pooled_readonly(keys, off, mode), got)

        got_w = gpu.pull_pooled_readonly(keys, off, mode, wd)
        want_w, _, _ = ops.pool_fwd_weighted(flat, None, None, off, wd, mode)
        assert torch.equal(got_w, want_w), table
        assert torch.equal(gpu.pull_pooled_readonly(keys, off, mode, wd),
                           got_w)
        assert not torch.equal(got_w, got)


# ------------------------------------------------- EmbeddingBag evaluation

def _trained_bag(hash_mode, dim, mode):
    """An EmbeddingBag on the GPU after one train step per engine batch, so
    every key of those batches has a row."""
    batches = _engine_batches(hash_mode)
    ctx, emb, w = _make(DEV, hash_mode, dim, mode,
                        reserve=16384 if hash_mode else 0)
    for vals, offsets in batches:
        _step(ctx, emb, w, vals.to(DEV), offsets.to(DEV))
    return emb, batches


def _sample_weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g).to(DEV)


@pytest.mark.parametrize("weighted", [False, True])
def test_eval_builds_no_nnz_by_dim_tensor(weighted):
    """One evaluation call at dim 260 may raise the allocator's peak by less
    than half of an [nnz, dim] fp32 tensor; the fused path allocates only
    the [B, dim] output (about 2 % of it)."""
    dim = 260
    emb, batches = _trained_bag(True, dim, "mean")
    vals, offsets = (t.to(DEV) for t in batches[0])
    nnz = int(offsets[-1])
    w = _sample_weights(vals.numel(), 1) if weighted else None
    emb.eval()
    with torch.no_grad():
        emb(vals, offsets, w)                       # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = emb(vals, offsets, w)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    bound = nnz * dim * 4 // 2
    print(f"peak rise {rise} B, bound {bound} B, output "
          f"{out.numel() * 4} B")
    assert out.shape == (B, dim) and bool((out != 0).any())
    assert rise < bound
    _reset()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hash_mode,dim,mode",
                         [(False, 9, "mean"), (True, 64, "sqrtn")])
def test_eval_is_graph_capturable(hash_mode, dim, mode, weighted):
    """EmbeddingBag.eval() forward under no_grad captured as a hipGraph and
    replayed over a second problem written into the same buffers equals the
    eager result on that problem (no host sync on the path)."""
    emb, batches = _trained_bag(hash_mode, dim, mode)
    emb.eval()
    cap = max(v.numel() for v, _ in batches)
    s_vals = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    s_off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    s_w = torch.zeros(cap, device=DEV) if weighted else None
    ws = [_sample_weights(cap, 10 + i) for i in range(len(batches))]

    def load(i):
        vals, offsets = batches[i]
        s_vals.fill_(-1)
        s_vals[:vals.numel()].copy_(vals)
        s_off.copy_(offsets)
        if weighted:
            s_w.copy_(ws[i])

    with torch.no_grad():
        load(0)
        emb(s_vals, s_off, s_w)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                emb(s_vals, s_off, s_w)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = emb(s_vals, s_off, s_w)
        outs = []
        for i in (1, 2):
            load(i)
            graph.replay()
            outs.append(out.clone())
        torch.cuda.synchronize()
        for i, got in zip((1, 2), outs):
            load(i)
            eager = emb(s_vals, s_off, s_w)
            assert bool((eager != 0).any())
            assert torch.equal(got, eager)
    assert not torch.equal(outs[0], outs[1])
    _reset()


def test_frozen_table_learned_weights_stay_on_autograd():
    """Grad enabled, table frozen, weights requiring a gradient: that branch
    pools with torch ops, so the weights still get their gradient."""
    emb, batches = _trained_bag(False, 9, "sum")
    vals, offsets = (t.to(DEV) for t in batches[0])
    emb.grad_hook.requires_grad_(False)
    w = _sample_weights(vals.numel(), 3).requires_grad_(True)
    out = emb(vals, offsets, w)
    assert out.requires_grad
    out.sum().backward()
    assert w.grad is not None and bool((w.grad[:int(offsets[-1])] != 0).any())
    with torch.no_grad():
        fused = emb(vals, offsets, w)
    torch.testing.assert_close(fused, out.detach(), rtol=1e-5, atol=1e-6)
    _reset()


# ------------------------------------------------------------------ read-only

def test_lookup_of_unseen_keys_writes_nothing():
    g = torch.Generator().manual_seed(9)
    rows = torch.randn(VOCAB, 24, generator=g)
    gpu, _ = _shards("hash_colliding", rows, gpu_only=True)
    cap = gpu._cap
    n0, nd0 = gpu.num_rows, gpu.nrows_dev.clone()
    tk0, tv0, w0 = gpu.tk.clone(), gpu.tv.clone(), gpu.weights.clone()
    # unseen: fresh full-range keys, absent members of the colliding chain
    # (probed to its end) and more keys homed at the table's last buckets
    absent = _keymap("hash_colliding")[:N_COLL][~_present()[:N_COLL]]
    more = ref.colliding_keys(cap - 1, [cap - 2, cap - 1], 2 * N_COLL + 8,
                              limit=4_000_000)
    more = more[~torch.isin(more, _keymap("hash_colliding"))]
    unseen = torch.cat([ref.full_range_keys(150, g), absent, more,
                        torch.full((TAIL,), -1, dtype=torch.int64)])
    assert not bool(torch.isin(unseen, _keymap("hash_colliding")
                               [_present()]).any())
    n = unseen.numel() - TAIL
    offsets = torch.tensor([0, 1, 1, 70, n], dtype=torch.int64)
    for w in (None, torch.ones(unseen.numel(), device=DEV)):
        out = gpu.pull_pooled_readonly(unseen.to(DEV), offsets.to(DEV),
                                       "sum", w)
        assert torch.equal(out, torch.zeros(4, 24, device=DEV))
    assert gpu.num_rows == n0 and torch.equal(gpu.nrows_dev, nd0)
    assert int(gpu.tk.sum()) == int(tk0.sum())
    assert torch.equal(gpu.tk, tk0) and torch.equal(gpu.tv, tv0)
    assert torch.equal(gpu.weights, w0)

    # array table: keys below 0 or past the vocabulary are misses too
    arr, _ = _shards("array", rows, gpu_only=True)
    valid0 = arr.valid_u8.clone()
    bad = torch.tensor([-5, VOCAB, VOCAB + 1, 1 << 40, 4, -1],
                       dtype=torch.int64, device=DEV)     # id 4 is absent
    out = arr.pull_pooled_readonly(
        bad, torch.tensor([0, 3, 5], device=DEV), "mean")
    assert torch.equal(out, torch.zeros(2, 24, device=DEV))
    assert torch.equal(arr.valid_u8, valid0)


# ------------------------------------------------------- unsanitised offsets

@pytest.mark.parametrize("table", ["array", "hash"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_unsanitised_offsets_are_clamped(table, mode):
    """offsets below 0 or above nnz_cap are clamped and a decreasing pair is
    an empty bag — the kernel's own guards, below EmbeddingBag's checks.
    Reference: the CPU oracle, one bag at a time, on the clamped bounds
    (integer rows, power-of-two lengths: exact)."""
    dim, nnz = 24, 48
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(-8, 9, (VOCAB, dim), generator=g).float()
    gpu, cpu = _shards(table, rows)
    vals = torch.randint(0, VOCAB, (nnz,), generator=g, dtype=torch.int64)
    keys = _keys_of(table, vals)
    w = _int_weights(nnz, 5)
    offsets = torch.tensor([-3, 4, 12, 8, 16, 80], dtype=torch.int64)
    bounds = [(0, 4), (4, 12), (12, 12), (8, 16), (16, 48)]
    for weights in (None, w):
        if weights is not None and mode != "sum":
            continue
        want = torch.stack([
            cpu.pull_pooled_readonly(
                keys[s:e], torch.tensor([0, e - s]), mode,
                None if weights is None else weights[s:e])[0]
            for s, e in bounds])
        got = gpu.pull_pooled_readonly(
            keys.to(DEV), offsets.to(DEV), mode,
            None if weights is None else weights.to(DEV))
        assert torch.equal(got.cpu(), want)
        assert bool((want[2] == 0).all()) and bool((want[4] != 0).any())


# -------------------------------------------------------------------- serving

@pytest.mark.parametrize("weighted", [False, True])
def test_serve_pooled_from_gpu(tmp_path, weighted):
    import openembedding_amd.torch as embed
    from fastapi.testclient import TestClient
    from openembedding_amd.core.variable_gpu import HipVariableShard
    from openembedding_amd.serving import ModelController, make_app

    emb, batches = _trained_bag(True, 24, "mean")      # three train steps
    uri = str(tmp_path / "dump")
    embed.save_server_model(uri)
    ctx = embed.get_context()
    sign = f"{ctx.model_uuid}-{ctx.model_version}"

    vals, offsets = batches[1]
    w = _sample_weights(vals.numel(), 6) if weighted else None
    emb.eval()
    with torch.no_grad():
        live = emb(vals.to(DEV), offsets.to(DEV), w)
    assert bool((live != 0).any())

    c = ModelController(device=DEV)
    c.create_model(uri)
    var = c.manager.find_model_variable(sign, 0)
    assert isinstance(var.shard, HipVariableShard)
    got = var.pull_pooled(vals, offsets, "mean", w)
    assert got.device.type == "cuda"
    assert torch.allclose(got, live, atol=1e-6)

    body = {"values": vals.tolist(), "offsets": offsets.tolist(),
            "mode": "mean"}
    if weighted:
        body["per_sample_weights"] = w.cpu().tolist()
    r = TestClient(make_app(c)).post(
        f"/models/{sign}/variables/0/pull_pooled", json=body)
    assert r.status_code == 200
    served = torch.tensor(r.json()["pooled"], device=DEV)
    assert torch.allclose(served, live, atol=1e-6)
    _reset()


# ------------------------------------------------------------- capacity tier

def test_tiered_shard_keeps_the_unfused_route():
    """Rows of a tiered shard may sit in host DRAM, where the fused kernel
    cannot see them: ``pull_pooled(readonly=True)`` must still go through
    ``pull_readonly`` and match an untiered shard holding the same rows."""
    from openembedding_amd.parallel.sharded import ShardedVariable
    from test_gpu_tiered import _mk, _step as _tier_step

    t, r = _mk(cache_rows=32)
    gen = torch.Generator().manual_seed(5)
    for _ in range(20):
        keys = torch.randint(0, 256, (48,), generator=gen,
                             dtype=torch.int64).to(DEV)
        _tier_step(t, keys)
        _tier_step(r, keys)
    assert t._host_live
    vals = torch.cat([torch.randint(0, 300, (200,), generator=gen,
                                    dtype=torch.int64),
                      torch.full((5,), -1, dtype=torch.int64)]).to(DEV)
    offsets = torch.tensor([0, 0, 7, 64, 65, 200], device=DEV)
    w = _sample_weights(vals.numel(), 8)
    assert not t.fused_pooled_readonly and r.fused_pooled_readonly
    for weights in (None, w):
        want = r.pull_pooled_readonly(vals, offsets, "sqrtn", weights)
        got, h = ShardedVariable(t).pull_pooled(vals, offsets, "sqrtn",
                                                readonly=True,
                                                weights=weights)
        assert h.inverse is not None            # the unfused route's handle
        assert torch.equal(got, want)
        assert torch.equal(
            t.pull_pooled_readonly(vals, offsets, "sqrtn", weights), want)
        fused, h2 = ShardedVariable(r).pull_pooled(vals, offsets, "sqrtn",
                                                   readonly=True,
                                                   weights=weights)
        assert h2.inverse is None and torch.equal(fused, want)
