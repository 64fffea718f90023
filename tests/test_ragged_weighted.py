"""Per-sample weights of the multi-hot pooled pull/push on the CPU engine: the
dispatch oracle (ops.pool_fwd_weighted / reduce_bags_weighted_by_inverse /
pool_wgrad) against a literal loop and against float64 autograd, and the
weighted EmbeddingBag end to end against a flat Embedding pooled by hand."""

import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from openembedding_amd.ops import dispatch as ops

from test_ragged import (DIM, LENS, MODES, VOCAB, _batches, _make_vars,
                         _offsets, _rank_bags, _reset, _values)

TAIL = 6


def _weights(nnz_cap, seed, nnz=None):
    """Mixed-sign weights; NaN behind ``nnz`` (the -1 tail)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(nnz_cap, generator=g) * 1.75 + 0.25
    w[torch.rand(nnz_cap, generator=g) < 0.3] *= -1
    if nnz is not None:
        w[nnz:] = float("nan")
    return w


def _wpool_loop(elems, w, offsets, mode):
    """Literal per-bag reference: (out [B, dim], scale [B])."""
    out, scale = [], []
    for b in range(offsets.numel() - 1):
        s, e = int(offsets[b]), int(offsets[b + 1])
        acc = torch.zeros(elems.shape[1], dtype=elems.dtype)
        den = torch.zeros((), dtype=elems.dtype)
        for j in range(s, e):
            acc = acc + w[j] * elems[j]
            den = den + (w[j] * w[j] if mode == "sqrtn" else w[j])
        sc = torch.zeros((), dtype=elems.dtype)
        if mode == "sum":
            sc = sc + 1.0
        elif den != 0:
            sc = 1.0 / den if mode == "mean" else 1.0 / den.sqrt()
        out.append(acc * sc)
        scale.append(sc)
    return torch.stack(out), torch.stack(scale)


def _edge_problem(mode):
    """Bags with the edge cases of the weighted combiner: a zero-sum bag,
    a bag of all-zero weights, negative weights, empty bags, a NaN tail."""
    lens = [0, 2, 3, 0, 4, 1, 7, 0]
    offsets = _offsets(lens)
    nnz = int(offsets[-1])
    vals = _values(lens, 21, tail=TAIL)
    w = _weights(vals.numel(), 22, nnz)
    w[0:2] = torch.tensor([1.5, -1.5])          # bag 1: sum of w is 0
    w[2:5] = 0.0                                # bag 2: all-zero weights
    w[5:9] = torch.tensor([-2.0, 0.5, -0.25, 1.0])
    return vals, offsets, w, nnz


# ------------------------------------------------------------ dispatch oracle

@pytest.mark.parametrize("mode", MODES)
def test_oracle_matches_literal_loop(mode):
    vals, offsets, w, nnz = _edge_problem(mode)
    rows = torch.randn(VOCAB, DIM, generator=torch.Generator().manual_seed(1))
    uniq, inverse = torch.unique(vals, return_inverse=True)
    row_map = uniq.clone()                      # tail key -1 -> row -1
    row_map[2] = -1                             # one live key misses
    rows_nan = rows.clone()
    rows_nan[uniq[2]] = float("nan")            # the row behind the miss
    elems = rows[vals.clamp(min=0)].clone()
    elems[(vals < 0) | (vals == uniq[2])] = 0
    ref, ref_scale = _wpool_loop(elems, w, offsets, mode)
    assert torch.isfinite(ref).all()
    for dtype in (torch.int64, torch.int32):
        out, bag_of, scale = ops.pool_fwd_weighted(
            rows_nan, inverse, row_map.to(dtype), offsets, w, mode)
        torch.testing.assert_close(out, ref)
        torch.testing.assert_close(scale, ref_scale)
    assert torch.all(bag_of[nnz:] == -1) and torch.all(bag_of[:nnz] >= 0)
    if mode == "mean":
        assert float(scale[1]) == 0.0 and float(out[1].abs().sum()) == 0.0
    if mode != "sum":
        assert float(scale[2]) == 0.0 and float(out[2].abs().sum()) == 0.0
        assert float(scale[0]) == 0.0           # empty bag
    # identity form pools already-gathered rows
    got, _, _ = ops.pool_fwd_weighted(elems, None, None, offsets, w, mode)
    torch.testing.assert_close(got, ref)

    # backward through the same chain: nothing of the NaN tail leaks
    g = torch.randn(len(offsets) - 1, DIM,
                    generator=torch.Generator().manual_seed(2))
    u = uniq.numel()
    ug, cnt = ops.reduce_bags_weighted_by_inverse(inverse, g, bag_of, w,
                                                  scale, u)
    dw = ops.pool_wgrad(rows_nan, inverse, row_map, w, bag_of, scale, out,
                        g, mode)
    assert torch.isfinite(ug).all() and torch.isfinite(dw).all()
    assert torch.all(dw[nnz:] == 0)
    assert int(cnt[uniq == -1]) == 0 and int(cnt.sum()) == nnz
    # counts do not depend on weights: the weight-0 elements still count
    assert torch.equal(cnt, torch.bincount(inverse[:nnz], minlength=u))
    if mode == "mean":
        assert torch.all(dw[0:2] == 0)          # zero-sum bag: zero dw
    if mode == "sqrtn":
        assert torch.all(dw[2:5] == 0)


@pytest.mark.parametrize("mode", MODES)
def test_gradients_match_float64_autograd(mode):
    """dw and the row gradients against autograd of the composed expression
    (rows gathered, multiplied, pooled with torch ops) in float64."""
    lens = LENS
    offsets = _offsets(lens)
    nnz = int(offsets[-1])
    B = len(lens)
    vals = _values(lens, 31, tail=TAIL)
    gen = torch.Generator().manual_seed(32)
    w = _weights(vals.numel(), 33, nnz).double()
    if mode == "mean":
        w = w.abs()                             # keep sum of w away from 0
    uniq, inverse = torch.unique(vals, return_inverse=True)
    u = uniq.numel()
    rows = torch.randn(u, DIM, generator=gen, dtype=torch.float64)
    g = torch.randn(B, DIM, generator=gen, dtype=torch.float64)

    rows_ad = rows.clone().requires_grad_()
    w_ad = w[:nnz].clone().requires_grad_()
    ew = rows_ad[inverse[:nnz]] * w_ad.unsqueeze(1)
    seg = torch.repeat_interleave(torch.arange(B), torch.tensor(lens))
    pooled = torch.zeros(B, DIM, dtype=torch.float64).index_add(0, seg, ew)
    if mode != "sum":
        den = torch.zeros(B, dtype=torch.float64).index_add(
            0, seg, w_ad if mode == "mean" else w_ad * w_ad)
        den = torch.where(torch.tensor(lens) > 0, den, torch.ones_like(den))
        pooled = pooled / (den if mode == "mean" else den.sqrt()).unsqueeze(1)
    pooled.backward(g)

    out, bag_of, scale = ops.pool_fwd_weighted(rows, inverse, None, offsets,
                                               w, mode)
    torch.testing.assert_close(out, pooled.detach())
    ug, cnt = ops.reduce_bags_weighted_by_inverse(inverse, g, bag_of, w,
                                                  scale, u)
    dw = ops.pool_wgrad(rows, inverse, None, w, bag_of, scale, out, g, mode)
    torch.testing.assert_close(ug, rows_ad.grad)
    torch.testing.assert_close(dw[:nnz], w_ad.grad)
    assert torch.all(dw[nnz:] == 0)
    assert float(dw.abs().max()) > 1e-3

    # pool_rows(weights=) is the differentiable form of the same pool
    rows_ad.grad = None
    w2 = w.clone().requires_grad_()             # NaN tail included
    out2, _ = ops.pool_rows(rows_ad[inverse], offsets, mode, weights=w2)
    torch.testing.assert_close(out2, out)
    out2.backward(g)
    torch.testing.assert_close(rows_ad.grad, ug)
    torch.testing.assert_close(w2.grad, dw)


@pytest.mark.parametrize("mode", MODES)
def test_unit_weights_reproduce_unweighted_exactly(mode):
    offsets = _offsets(LENS)
    vals = _values(LENS, 41, tail=TAIL)
    gen = torch.Generator().manual_seed(42)
    uniq, inverse = torch.unique(vals, return_inverse=True)
    u = uniq.numel()
    rows = torch.randn(u, DIM, generator=gen)
    g = torch.randn(len(LENS), DIM, generator=gen)
    ones = torch.ones(vals.numel())
    ref, ref_bag = ops.pool_fwd(rows, inverse, None, offsets, mode)
    out, bag_of, scale = ops.pool_fwd_weighted(rows, inverse, None, offsets,
                                               ones, mode)
    assert torch.equal(out, ref) and torch.equal(bag_of, ref_bag)
    ref_g, ref_c = ops.reduce_bags_by_inverse(inverse, g, ref_bag, offsets,
                                              mode, u)
    ug, cnt = ops.reduce_bags_weighted_by_inverse(inverse, g, bag_of, ones,
                                                  scale, u)
    assert torch.equal(ug, ref_g) and torch.equal(cnt, ref_c)
    # weights=None leaves pool_rows as it was
    a, _ = ops.pool_rows(rows[inverse], offsets, mode)
    b, _ = ops.pool_rows(rows[inverse], offsets, mode, weights=ones)
    assert torch.equal(a, b)


# ----------------------------------------------------------------- end to end

class _Gate(torch.nn.Module):
    """Learned per-element weights: sigmoid(linear(feature))."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.lin = torch.nn.Linear(2, 1)

    def forward(self, feat):
        return torch.sigmoid(self.lin(feat)).squeeze(-1) * 2 - 0.5


def _feat(n, seed):
    return torch.randn(n, 2, generator=torch.Generator().manual_seed(seed))


def _train_w(make, fwd, batches, probe, prefetch=False):
    """3 Adagrad steps of (embedding, gate); returns (first output, table
    rows of ``probe``, gate parameters, first w.grad, row count)."""
    import openembedding_amd.torch as embed
    _reset()
    emb = make(embed)
    gate = _Gate()
    opt = embed.Adagrad(list(emb.parameters()) + list(gate.parameters()),
                        lr=0.1)
    t = torch.randn(len(LENS), DIM, generator=torch.Generator().manual_seed(9))
    first = wgrad = None
    for i, (vals, offsets) in enumerate(batches):
        opt.zero_grad()
        w = gate(_feat(vals.numel(), 70 + i))
        w.retain_grad()
        if prefetch:
            emb.prefetch(vals)
        out = fwd(emb, vals, offsets, w)
        if prefetch:
            assert not emb.variable._prefetched
        (out * t).sum().backward()
        if first is None:
            first, wgrad = out.detach().clone(), w.grad.clone()
        opt.step()
    rows = emb.variable.sparse_read(probe)
    n = emb.variable.sharded.shard.num_rows
    params = torch.cat([p.detach().reshape(-1) for p in gate.parameters()])
    _reset()
    return first, rows, params, wgrad, n


def _fwd_flat(mode):
    def fwd(emb, vals, offsets, w):
        nnz = int(offsets[-1])
        return ops.pool_rows(emb(vals[:nnz]), offsets, mode,
                             weights=w[:nnz])[0]
    return fwd


def _fwd_bag(emb, vals, offsets, w):
    return emb(vals, offsets, per_sample_weights=w)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_embeddings", [VOCAB, -1])
def test_weighted_bag_matches_flat_embedding(num_embeddings, mode):
    batches = _batches(3, tail=5)
    probe = torch.arange(VOCAB)
    o1, t1, p1, g1, n1 = _train_w(
        lambda e: e.EmbeddingBag(num_embeddings, DIM, mode=mode),
        _fwd_bag, batches, probe)
    o2, t2, p2, g2, n2 = _train_w(lambda e: e.Embedding(num_embeddings, DIM),
                                  _fwd_flat(mode), batches, probe)
    torch.testing.assert_close(o1, o2)
    torch.testing.assert_close(t1, t2)
    torch.testing.assert_close(p1, p2)
    nnz = int(batches[0][1][-1])
    torch.testing.assert_close(g1[:nnz], g2[:nnz])
    assert torch.all(g1[nnz:] == 0)             # dw of the tail
    assert float(g1.abs().max()) > 1e-3
    assert n1 == n2                             # the -1 tail created no row


def test_weighted_prefetched_pull():
    batches = _batches(3)
    probe = torch.arange(VOCAB)
    make = lambda e: e.EmbeddingBag(VOCAB, DIM, mode="sqrtn")
    a = _train_w(make, _fwd_bag, batches, probe, prefetch=True)
    b = _train_w(make, _fwd_bag, batches, probe)
    for x, y in zip(a[:4], b[:4]):
        torch.testing.assert_close(x, y)


def test_weighted_sparse_as_dense():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    nnz = int(offsets[-1])
    w = _weights(vals.numel(), 51, nnz).abs().requires_grad_()
    emb = embed.EmbeddingBag(VOCAB, DIM, mode="mean", sparse_as_dense=True)
    out = emb(vals, offsets, per_sample_weights=w)
    ref, _ = _wpool_loop(emb.dense.weight[vals[:nnz]], w, offsets, "mean")
    torch.testing.assert_close(out, ref)
    g_out = torch.autograd.grad(out.sum(), [emb.dense.weight, w])
    g_ref = torch.autograd.grad(ref.sum(), [emb.dense.weight, w])
    torch.testing.assert_close(g_out[0], g_ref[0])
    torch.testing.assert_close(g_out[1][:nnz], g_ref[1][:nnz])
    assert torch.all(g_out[1][nnz:] == 0)


def test_weighted_no_grad_is_readonly():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    w = _weights(vals.numel(), 52, int(offsets[-1]))
    emb = embed.EmbeddingBag(-1, DIM, mode="sqrtn")
    with torch.no_grad():
        out = emb(vals, offsets, per_sample_weights=w)
    assert float(out.abs().sum()) == 0.0            # missing rows are zeros
    assert emb.variable.sharded.shard.num_rows == 0  # and stay missing
    trained = emb(vals, offsets, per_sample_weights=w).detach()
    assert float(trained.abs().sum()) > 0
    with torch.no_grad():
        torch.testing.assert_close(emb(vals, offsets, per_sample_weights=w),
                                   trained)


def test_frozen_table_still_trains_the_weights():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    nnz = int(offsets[-1])
    emb = embed.EmbeddingBag(VOCAB, DIM, mode="mean")
    emb(vals, offsets)                      # a training pull makes the rows
    emb.grad_hook.requires_grad_(False)
    w = _weights(vals.numel(), 54, nnz).abs().requires_grad_()
    out = emb(vals, offsets, per_sample_weights=w)
    rows = emb.variable.sparse_read(vals[:nnz])
    ref, _ = _wpool_loop(rows, w, offsets, "mean")
    torch.testing.assert_close(out, ref)
    g_out, = torch.autograd.grad(out[:, 0].sum(), w)
    g_ref, = torch.autograd.grad(ref[:, 0].sum(), w)
    torch.testing.assert_close(g_out, g_ref)
    assert float(g_out.abs().max()) > 1e-3


def test_weighted_input_checks():
    import openembedding_amd.torch as embed
    vals, offsets = _batches(1, tail=3)[0]
    nnz = int(offsets[-1])
    w = _weights(vals.numel(), 53, nnz)
    emb = embed.EmbeddingBag(VOCAB, DIM, validate=True)
    with pytest.raises(ValueError):
        emb(vals, offsets, per_sample_weights=w[:-1])       # wrong length
    with pytest.raises(TypeError):
        emb(vals, offsets, per_sample_weights=torch.ones_like(vals))
    with pytest.raises(TypeError):
        emb(vals, offsets, per_sample_weights=w.view(1, -1))
    with pytest.raises(ValueError):
        emb(vals, offsets, per_sample_weights=w.to("meta"))  # wrong device
    bad = w.clone()
    bad[nnz - 1] = float("inf")
    with pytest.raises(ValueError):
        emb(vals, offsets, per_sample_weights=bad)          # validate=True
    # the NaN tail is fine, validated or not
    assert emb(vals, offsets, per_sample_weights=w).shape == (len(LENS), DIM)


def test_weighted_example_runs():
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OEAMD_DEVICE="cpu")
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(repo, "examples",
                                      "weighted_multihot.py")],
        cwd=repo, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "gate weight grad norm" in r.stdout


# ------------------------------------------------------------- gloo world 2

def _rank_weights(rank, n):
    return _weights(n, 80 + rank).abs()


def _worker_weighted(rank, world, port, tmp):
    from openembedding_amd.context import Context
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method=f"tcp://127.0.0.1:{port}")
    st, variables = _make_vars(Context(device="cpu"))
    vals, offsets, grad = _rank_bags(rank)
    w = _rank_weights(rank, vals.numel())
    res = {}
    for name, var in zip(("exact", "padded"), variables):
        out, h = var.pull_pooled(vals, offsets, "mean", weights=w,
                                 wgrad=True)
        assert h.padded == (name == "padded")
        res[name + "_dw"] = var.push_pooled(h, grad, offsets, "mean",
                                            weights=w, out=out, wgrad=True)
        res[name + "_out"] = out
    st.update_weights()
    for name, var in zip(("exact", "padded"), variables):
        res[name + "_table"], _ = var.pull(torch.arange(VOCAB), readonly=True)
    torch.save(res, os.path.join(tmp, f"weighted_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_weighted_matches_world1(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker_weighted, args=(2, port, str(tmp_path)), nprocs=2,
             join=True)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
              "MASTER_PORT"):
        os.environ.pop(v, None)

    from openembedding_amd.context import Context
    st, variables = _make_vars(Context(device="cpu"))
    outs, dws = {}, {}
    for name, var in zip(("exact", "padded"), variables):
        for rank in range(2):
            vals, offsets, grad = _rank_bags(rank)
            w = _rank_weights(rank, vals.numel())
            out, h = var.pull_pooled(vals, offsets, "mean", weights=w,
                                     wgrad=True)
            dws[name, rank] = var.push_pooled(h, grad, offsets, "mean",
                                              weights=w, out=out, wgrad=True)
            outs[name, rank] = out
    st.update_weights()
    for name, var in zip(("exact", "padded"), variables):
        table, _ = var.pull(torch.arange(VOCAB), readonly=True)
        for rank in range(2):
            r = torch.load(tmp_path / f"weighted_{rank}.pt",
                           weights_only=True)
            torch.testing.assert_close(r[name + "_out"], outs[name, rank])
            torch.testing.assert_close(r[name + "_dw"], dws[name, rank])
            assert float(r[name + "_dw"].abs().max()) > 1e-3
            torch.testing.assert_close(r[name + "_table"], table,
                                       rtol=1e-5, atol=1e-5)
