"""Multi-hot embedding bags on the CPU engine: the dispatch oracle
(ops.pool_fwd / ops.reduce_bags_by_inverse) against torch, and EmbeddingBag
end to end against a flat Embedding pooled with torch ops."""

import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from openembedding_amd.ops import dispatch as ops

DIM = 5
VOCAB = 200
MODES = ["sum", "mean", "sqrtn"]
# empty bags first, in the middle and last; a long bag; single-element bags
LENS = [0, 3, 1, 0, 7, 2, 40, 1, 0]


def _offsets(lens):
    return torch.cat([torch.zeros(1, dtype=torch.int64),
                      torch.tensor(lens, dtype=torch.int64).cumsum(0)])


def _values(lens, seed, vocab=VOCAB, tail=0):
    g = torch.Generator().manual_seed(seed)
    nnz = int(sum(lens))
    v = torch.randint(0, vocab, (nnz,), dtype=torch.int64, generator=g)
    v[1] = v[0]                 # a key repeated inside one bag
    v[-1] = v[0]                # ... and shared with another bag
    return torch.cat([v, torch.full((tail,), -1, dtype=torch.int64)])


def _pool_loop(elems, offsets, mode):
    """Independent per-bag reference (python loop)."""
    out = torch.zeros(offsets.numel() - 1, elems.shape[1], dtype=elems.dtype)
    for b in range(offsets.numel() - 1):
        s, e = int(offsets[b]), int(offsets[b + 1])
        if e > s:
            out[b] = elems[s:e].sum(0)
            if mode == "mean":
                out[b] = out[b] / (e - s)
            elif mode == "sqrtn":
                out[b] = out[b] / (e - s) ** 0.5
    return out


# ------------------------------------------------------------ dispatch oracle

@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_pool_fwd_matches_torch_embedding_bag(mode):
    rows = torch.randn(VOCAB, DIM, generator=torch.Generator().manual_seed(1))
    offsets = _offsets(LENS)
    vals = _values(LENS, 2)
    out, bag_of = ops.pool_fwd(rows, vals, None, offsets, mode)
    ref = F.embedding_bag(vals, rows, offsets[:-1], mode=mode)
    torch.testing.assert_close(out, ref)
    want = torch.repeat_interleave(torch.arange(len(LENS)),
                                   torch.tensor(LENS))
    assert torch.equal(bag_of.long(), want)


def test_pool_fwd_sqrtn_map_identity_and_tail():
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(VOCAB, DIM, generator=g)
    offsets = _offsets(LENS)
    vals = _values(LENS, 4, tail=6)
    nnz = int(offsets[-1])
    lens = torch.tensor(LENS, dtype=torch.float32).clamp(min=1)
    # sqrtn == sum / sqrt(len); the -1 tail belongs to no bag
    s, bag_of = ops.pool_fwd(rows, vals.clamp(min=0), None, offsets, "sum")
    q, _ = ops.pool_fwd(rows, vals.clamp(min=0), None, offsets, "sqrtn")
    torch.testing.assert_close(q, s / lens.sqrt().unsqueeze(1))
    assert torch.all(bag_of[nnz:] == -1) and torch.all(bag_of[:nnz] >= 0)
    # second-level map: unique id -> row, -1 = zero row
    uniq, inverse = torch.unique(vals, return_inverse=True)
    row_map = uniq.clone()              # the tail key -1 maps to row -1
    row_map[3] = -1                     # one live key resolves to a miss
    for dtype in (torch.int64, torch.int32):
        got, _ = ops.pool_fwd(rows, inverse, row_map.to(dtype), offsets,
                              "mean")
        elems = rows[vals.clamp(min=0)].clone()
        elems[(vals < 0) | (vals == uniq[3])] = 0
        torch.testing.assert_close(got, _pool_loop(elems, offsets, "mean"))
    # identity form pools already-gathered rows
    elems = rows[vals.clamp(min=0)]
    got, _ = ops.pool_fwd(elems, None, None, offsets, "sum")
    torch.testing.assert_close(got, _pool_loop(elems, offsets, "sum"))


@pytest.mark.parametrize("mode", MODES)
def test_reduce_bags_matches_expand_then_reduce(mode):
    offsets = _offsets(LENS)
    vals = _values(LENS, 5, tail=4)
    nnz = int(offsets[-1])
    uniq, inverse = torch.unique(vals, return_inverse=True)
    u = uniq.numel()
    B = len(LENS)
    grad_out = torch.randn(B, DIM, generator=torch.Generator().manual_seed(6))
    _, bag_of = ops.pool_fwd(torch.zeros(u, DIM), inverse, None, offsets,
                             mode)
    ug, cnt = ops.reduce_bags_by_inverse(inverse, grad_out, bag_of, offsets,
                                         mode, u)
    # expand through autograd of the independent loop reference, then the
    # plain reduce over the live elements
    elems = torch.zeros(vals.numel(), DIM, requires_grad=True)
    _pool_loop(elems, offsets, mode).backward(grad_out)
    ref_g, ref_c = ops.reduce_by_inverse(inverse[:nnz], elems.grad[:nnz], u)
    torch.testing.assert_close(ug, ref_g)
    assert torch.equal(cnt, ref_c)
    assert int(cnt[uniq == -1]) == 0    # the tail adds no count


# ----------------------------------------------------------------- end to end

def _reset():
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()


def _batches(n, tail=0):
    out = []
    for i in range(n):
        lens = LENS[i:] + LENS[:i]
        out.append((_values(lens, 10 + i, tail=tail), _offsets(lens)))
    return out


def _train(make, fwd, batches, probe):
    """3 Adagrad steps; returns (first output, table rows of ``probe``)."""
    import openembedding_amd.torch as embed
    _reset()
    emb = make(embed)
    opt = embed.Adagrad(emb.parameters(), lr=0.1)
    w = torch.randn(len(LENS), DIM, generator=torch.Generator().manual_seed(9))
    first = None
    for vals, offsets in batches:
        opt.zero_grad()
        out = fwd(emb, vals, offsets)
        if first is None:
            first = out.detach().clone()
        (out * w).sum().backward()
        opt.step()
    rows = emb.variable.sparse_read(probe)
    n = emb.variable.sharded.shard.num_rows
    _reset()
    return first, rows, n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_embeddings", [VOCAB, -1])
def test_embedding_bag_matches_flat_embedding(num_embeddings, mode):
    batches = _batches(3, tail=5)
    probe = torch.arange(VOCAB)

    def fwd_bag(emb, vals, offsets):
        return emb(vals, offsets)

    def fwd_flat(emb, vals, offsets):
        nnz = int(offsets[-1])
        return _pool_loop(emb(vals[:nnz]), offsets, mode)

    o1, t1, n1 = _train(
        lambda e: e.EmbeddingBag(num_embeddings, DIM, mode=mode),
        fwd_bag, batches, probe)
    o2, t2, n2 = _train(lambda e: e.Embedding(num_embeddings, DIM),
                        fwd_flat, batches, probe)
    torch.testing.assert_close(o1, o2)
    torch.testing.assert_close(t1, t2)
    assert n1 == n2                     # the -1 tail created no row


def test_sparse_as_dense_pools_dense_table():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    nnz = int(offsets[-1])
    emb = embed.EmbeddingBag(VOCAB, DIM, mode="mean", sparse_as_dense=True)
    out = emb(vals, offsets)
    ref = F.embedding_bag(vals[:nnz], emb.dense.weight, offsets[:-1],
                          mode="mean")
    torch.testing.assert_close(out, ref)
    g_out, = torch.autograd.grad(out.sum(), emb.dense.weight)
    g_ref, = torch.autograd.grad(ref.sum(), emb.dense.weight)
    torch.testing.assert_close(g_out, g_ref)


def test_no_grad_is_a_readonly_pooled_read():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    emb = embed.EmbeddingBag(-1, DIM, mode="sum")
    with torch.no_grad():
        out = emb(vals, offsets)
    assert float(out.abs().sum()) == 0.0            # missing rows are zeros
    assert emb.variable.sharded.shard.num_rows == 0  # and stay missing
    trained = emb(vals, offsets).detach()
    with torch.no_grad():
        torch.testing.assert_close(emb(vals, offsets), trained)


def test_prefetched_pull_is_pooled():
    batches = _batches(3)
    probe = torch.arange(VOCAB)

    def fwd_prefetch(emb, vals, offsets):
        emb.prefetch(vals)
        assert len(emb.variable._prefetched) == 1
        out = emb(vals, offsets)
        assert not emb.variable._prefetched      # consumed by the forward
        return out

    o1, t1, _ = _train(lambda e: e.EmbeddingBag(VOCAB, DIM, mode="sqrtn"),
                       fwd_prefetch, batches, probe)
    o2, t2, _ = _train(lambda e: e.EmbeddingBag(VOCAB, DIM, mode="sqrtn"),
                       lambda emb, v, o: emb(v, o), batches, probe)
    torch.testing.assert_close(o1, o2)
    torch.testing.assert_close(t1, t2)


def test_input_checks_and_validate():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1)[0]
    with pytest.raises(ValueError):
        embed.EmbeddingBag(VOCAB, DIM, mode="max")
    emb = embed.EmbeddingBag(VOCAB, DIM, validate=True)
    with pytest.raises(TypeError):
        emb(vals.float(), offsets)
    with pytest.raises(TypeError):
        emb(vals.view(1, -1), offsets)
    with pytest.raises(TypeError):
        emb(vals, offsets.to(torch.int32))
    bad = offsets.clone()
    bad[3] = bad[2] - 1                              # non-monotone
    with pytest.raises(ValueError):
        emb(vals, bad)
    with pytest.raises(ValueError):
        emb(vals[:-1], offsets)                      # offsets[-1] > nnz_cap
    assert emb(vals, offsets).shape == (len(LENS), DIM)
    # without validate a malformed offsets tensor is clamped, never an error
    loose = embed.EmbeddingBag(VOCAB, DIM)
    assert loose(vals, bad).shape == (len(LENS), DIM)


def test_multihot_example_runs():
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OEAMD_DEVICE="cpu")
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(repo, "examples",
                                      "multihot_embedding.py")],
        cwd=repo, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tag rows materialized" in r.stdout


# ------------------------------------------------------------- gloo world 2

def _rank_bags(rank):
    lens = LENS[rank:] + LENS[:rank]
    g = torch.Generator().manual_seed(50 + rank)
    grad = torch.randn(len(LENS), DIM, generator=g)
    return _values(lens, 60 + rank), _offsets(lens), grad


def _make_vars(ctx):
    st = ctx.create_storage()
    out = []
    for padded in (False, True):
        var = st.create_variable(VOCAB, DIM)
        var.set_initializer("uniform", minval=-1, maxval=1)
        var.set_optimizer("adagrad", learning_rate=0.1,
                          initial_accumulator_value=0.1, epsilon=1e-10)
        var._padded = padded
        out.append(var)
    return st, out


def _worker_pooled(rank, world, port, tmp):
    from openembedding_amd.context import Context
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method=f"tcp://127.0.0.1:{port}")
    st, variables = _make_vars(Context(device="cpu"))
    vals, offsets, grad = _rank_bags(rank)
    res = {}
    for name, var in zip(("exact", "padded"), variables):
        out, h = var.pull_pooled(vals, offsets, "mean")
        assert h.padded == (name == "padded")
        var.push_pooled(h, grad, offsets, "mean")
        res[name + "_out"] = out
    st.update_weights()
    for name, var in zip(("exact", "padded"), variables):
        res[name + "_table"], _ = var.pull(torch.arange(VOCAB), readonly=True)
    torch.save(res, os.path.join(tmp, f"pooled_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_pooled_matches_world1(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker_pooled, args=(2, port, str(tmp_path)), nprocs=2,
             join=True)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
              "MASTER_PORT"):
        os.environ.pop(v, None)

    # world 1 over both ranks' bags, committed together
    from openembedding_amd.context import Context
    # (one variable per route: lazy init is seeded by the variable id)
    st, variables = _make_vars(Context(device="cpu"))
    outs = {}
    for name, var in zip(("exact", "padded"), variables):
        for rank in range(2):
            vals, offsets, grad = _rank_bags(rank)
            out, h = var.pull_pooled(vals, offsets, "mean")
            var.push_pooled(h, grad, offsets, "mean")
            outs[name, rank] = out
    st.update_weights()
    for name, var in zip(("exact", "padded"), variables):
        table, _ = var.pull(torch.arange(VOCAB), readonly=True)
        for rank in range(2):
            r = torch.load(tmp_path / f"pooled_{rank}.pt", weights_only=True)
            torch.testing.assert_close(r[name + "_out"], outs[name, rank])
            torch.testing.assert_close(r[name + "_table"], table,
                                       rtol=1e-5, atol=1e-5)
