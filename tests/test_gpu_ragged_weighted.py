"""GPU tests of per-sample weights on the multi-hot pooled pull/push (all
@gpu): the weighted k_pool_fwd, the weighted bag-indirected reduce and
k_pool_wgrad against the CPU oracle (exact on integer data, derived fp32
bounds on random data), tail/guard behaviour, weighted EmbeddingBag training
GPU-vs-CPU on every route including the weights' own gradient, and hipGraph
capture/replay of the weighted step.

The geometry is that of tests/test_gpu_ragged.py (imported, not copied): 67
bags, one dim per rung of both ladders, bag lengths on every lane-group
edge, one bag above 256 elements, nnz no multiple of 256, a 37-element -1
tail, a key shared by many bags and one repeated inside a bag, a second-level
map with misses in int64 and int32. Weights of the tail are NaN throughout:
they must never reach a result."""

import functools

import pytest
import torch

from test_gpu_ragged import (B, DEV, DIMS, ENGINE_CASES, MODES, ROUTES, TAIL,
                             VOCAB, _engine_batches, _make, _maps, _ops,
                             _problem, _reset, _table)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
N_ROWS = VOCAB + 50


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _d(t):
    return t.to(DEV)


def _bag_pos(offsets, nnz_cap):
    """(bag [nnz_cap], position inside the bag, bag length) per element;
    bag = -1 in the tail."""
    lens = offsets[1:] - offsets[:-1]
    nnz = int(offsets[-1])
    bag = torch.full((nnz_cap,), -1, dtype=torch.int64)
    bag[:nnz] = torch.repeat_interleave(torch.arange(B), lens)
    pos = torch.arange(nnz_cap) - offsets[bag.clamp(min=0)]
    return bag, pos, lens


def _nan_tail(w, offsets):
    w = w.clone()
    w[int(offsets[-1]):] = float("nan")
    return w


def _run_gpu(ops, rows, inverse, row_map, offsets, w, grad_out, mode, u):
    """Forward, row-gradient reduce and weight gradient on the GPU."""
    out, bag_of, scale = ops.pool_fwd_weighted(
        _d(rows), _d(inverse), _d(row_map), _d(offsets), _d(w), mode)
    ug, cnt = ops.reduce_bags_weighted_by_inverse(
        _d(inverse), _d(grad_out), bag_of, _d(w), scale, u)
    dw = ops.pool_wgrad(_d(rows), _d(inverse), _d(row_map), _d(w), bag_of,
                        scale, out, _d(grad_out), mode)
    return out, bag_of, scale, ug, cnt, dw


def _run_cpu(ops, rows, inverse, row_map, offsets, w, grad_out, mode, u):
    out, bag_of, scale = ops.pool_fwd_weighted(rows, inverse, row_map,
                                               offsets, w, mode)
    ug, cnt = ops.reduce_bags_weighted_by_inverse(inverse, grad_out, bag_of,
                                                  w, scale, u)
    dw = ops.pool_wgrad(rows, inverse, row_map, w, bag_of, scale, out,
                        grad_out, mode)
    return out, bag_of, scale, ug, cnt, dw


# -------------------------------------------------------------- kernel, exact

@pytest.mark.parametrize("dim", DIMS)
def test_sum_exact_on_integer_data(dim):
    """Rows in [-8, 8], gradients in [-4, 4], weights from {-2 .. 4} in
    halves: every product and sum is exact in fp32 in any order, so out,
    bag_of, ugrads, counts AND dw equal the CPU oracle bit for bit."""
    ops = _ops()
    vals, offsets = _problem(pow2=False, seed=dim)
    g = torch.Generator().manual_seed(dim)
    rows = torch.randint(-8, 9, (N_ROWS, dim), generator=g).float()
    grad_out = torch.randint(-4, 5, (B, dim), generator=g).float()
    choices = torch.tensor([-2, -1, -0.5, 0, 0.5, 1, 2, 4])
    w = choices[torch.randint(0, 8, (vals.numel(),), generator=g)]
    w = _nan_tail(w, offsets)
    uniq, inverse, row_map = _maps(vals, N_ROWS, dim)
    u = uniq.numel()

    ref = _run_cpu(ops, rows, inverse, row_map, offsets, w, grad_out, "sum",
                   u)
    for mdt in (torch.int64, torch.int32):
        got = _run_gpu(ops, rows, inverse, row_map.to(mdt), offsets, w,
                       grad_out, "sum", u)
        for name, a, b in zip(("out", "bag_of", "bag_scale", "ugrads",
                               "counts", "dw"), got, ref):
            assert torch.equal(a.cpu(), b), (name, mdt)
    again = _run_gpu(ops, rows, inverse, row_map.to(mdt), offsets, w,
                     grad_out, "sum", u)
    assert torch.equal(again[0], got[0])    # run-to-run bitwise reproducible
    assert torch.equal(again[5], got[5])
    assert torch.all(ref[1][-TAIL:] == -1)
    assert int(ref[4][uniq < 0].sum()) == 0     # the tail adds no count
    assert int(ref[4].sum()) == int(offsets[-1])  # weight 0 still counts
    assert float(ref[5].abs().max()) >= 1

    # identity form (already-gathered rows): the non-fused routes' call
    elems = rows[row_map[inverse].clamp(min=0)]
    elems[row_map[inverse] < 0] = 0
    out3, bag3, sc3 = ops.pool_fwd_weighted(_d(elems), None, None,
                                            _d(offsets), _d(w), "sum")
    dw3 = ops.pool_wgrad(_d(elems), None, None, _d(w), bag3, sc3, out3,
                         _d(grad_out), "sum")
    assert torch.equal(out3.cpu(), ref[0])
    assert torch.equal(dw3.cpu(), ref[5])


@pytest.mark.parametrize("dim", DIMS)
def test_mean_exact_on_integer_data(dim):
    """Power-of-two bag lengths, weights alternating 0.5 / 1.5 inside a bag
    (1 for a length-1 bag): the sum of w is exactly the length and every
    product a multiple of 0.5, so out, bag_scale, ugrads and counts are
    bit-exact (dw is not asserted exact here)."""
    ops = _ops()
    vals, offsets = _problem(pow2=True, seed=dim)
    g = torch.Generator().manual_seed(dim)
    rows = torch.randint(-8, 9, (N_ROWS, dim), generator=g).float()
    grad_out = torch.randint(-4, 5, (B, dim), generator=g).float()
    bag, pos, lens = _bag_pos(offsets, vals.numel())
    w = torch.where(pos % 2 == 0, 0.5, 1.5)
    w[lens[bag.clamp(min=0)] == 1] = 1.0
    w = _nan_tail(w, offsets)
    uniq, inverse, row_map = _maps(vals, N_ROWS, dim)
    u = uniq.numel()

    ref = _run_cpu(ops, rows, inverse, row_map, offsets, w, grad_out, "mean",
                   u)
    want_scale = torch.where(lens > 0, 1.0 / lens.float(), 0.0)
    assert torch.equal(ref[2], want_scale)
    for mdt in (torch.int64, torch.int32):
        got = _run_gpu(ops, rows, inverse, row_map.to(mdt), offsets, w,
                       grad_out, "mean", u)
        for name, a, b in zip(("out", "bag_of", "bag_scale", "ugrads",
                               "counts"), got[:5], ref[:5]):
            assert torch.equal(a.cpu(), b), (name, mdt)


# ----------------------------------------------- kernel, random, fp32 bound

@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", MODES)
def test_random_within_fp32_bound(dim, mode):
    """Against the float64 evaluation of the oracle, eps = 2^-23, L the bag
    length, ``mag`` the oracle on |rows|, |w|.

    Forward: |err| <= (2L + 4) eps mag — L products and L adds at 2^-24
    each, the denominator with L roundings plus the divide / sqrt, a factor
    2 to spare. Row gradients: |err| <= (c + Lmax + 4) eps mag_g, c the
    key's count, Lmax the longest bag holding it, mag_g the oracle on
    |grad_out|, |w|, |scale|. Weight gradients: |err| <= (dim + 2L + 8) eps
    |scale_b| (sum_c |g||r_j| + |c_j| sum_c |g_c| mag_bc). Weights are
    uniform in [0.25, 2], 30 % negated for sum and sqrtn; mean keeps them
    positive (with a cancelling denominator no bound exists)."""
    ops = _ops()
    vals, offsets = _problem(pow2=False, seed=100 + dim)
    g = torch.Generator().manual_seed(200 + dim)
    rows = torch.randn(N_ROWS, dim, generator=g)
    grad_out = torch.randn(B, dim, generator=g)
    w = torch.rand(vals.numel(), generator=g) * 1.75 + 0.25
    if mode != "mean":
        w[torch.rand(vals.numel(), generator=g) < 0.3] *= -1
    w = _nan_tail(w, offsets)
    uniq, inverse, row_map = _maps(vals, N_ROWS, dim)
    u = uniq.numel()
    nnz = int(offsets[-1])
    bag, _, lens = _bag_pos(offsets, vals.numel())
    live = bag >= 0
    bc = bag.clamp(min=0)
    L = lens.double()

    out, bag_of, scale, ug, cnt, dw = _run_gpu(
        ops, rows, inverse, row_map, offsets, w, grad_out, mode, u)
    r_out, r_bag, r_scale, r_ug, r_cnt, r_dw = _run_cpu(
        ops, rows.double(), inverse, row_map, offsets, w.double(),
        grad_out.double(), mode, u)
    assert torch.equal(bag_of.cpu(), r_bag)
    assert torch.equal(cnt.cpu(), r_cnt)
    assert float(r_out.abs().max()) >= 1e-3     # vacuity guards
    assert float(r_dw.abs().max()) >= 1e-3

    # forward
    mag, _, _ = ops.pool_fwd_weighted(rows.double().abs(), inverse, row_map,
                                      offsets, w.double().abs(), mode)
    bound = (2 * L + 4).unsqueeze(1) * EPS * mag
    err = (out.cpu().double() - r_out).abs()
    print(f"fwd dim={dim} {mode}: max err {err.max():.3e}, "
          f"max err/bound {(err / (bound + 1e-300)).max():.3f}")
    assert torch.all(err <= bound)
    # bag_scale alone: the denominator's L roundings plus the divide / sqrt
    serr = (scale.cpu().double() - r_scale).abs()
    assert torch.all(serr <= (L + 2) * EPS * r_scale.abs())

    # row gradients
    mag_g, _ = ops.reduce_bags_weighted_by_inverse(
        inverse, grad_out.double().abs(), r_bag, w.double().abs(),
        r_scale.abs(), u)
    le = torch.where(live, L[bc], torch.zeros(()).double())
    lmax = torch.zeros(u, dtype=torch.float64).scatter_reduce(
        0, inverse, le, "amax")
    bound = (r_cnt.double() + lmax + 4).unsqueeze(1) * EPS * mag_g
    err = (ug.cpu().double() - r_ug).abs()
    print(f"bwd dim={dim} {mode}: max err {err.max():.3e}, "
          f"max err/bound {(err / (bound + 1e-300)).max():.3f}")
    assert torch.all(err <= bound)

    # weight gradients
    idx = row_map[inverse]
    r = rows.double()[idx.clamp(min=0)]
    r[idx < 0] = 0
    ga = grad_out.double().abs()[bc]
    if mode == "sum":
        cj = torch.zeros(vals.numel(), dtype=torch.float64)
    elif mode == "mean":
        cj = torch.ones(vals.numel(), dtype=torch.float64)
    else:
        cj = w.double() * r_scale[bc]
    inner = (ga * r.abs()).sum(1) + cj.abs() * (ga * mag[bc]).sum(1)
    bound = (dim + 2 * L[bc] + 8) * EPS * r_scale[bc].abs() * inner
    bound = torch.where(live, bound, torch.zeros_like(bound))
    err = (dw.cpu().double() - r_dw).abs()
    print(f"dw dim={dim} {mode}: max err {err.max():.3e}, "
          f"max err/bound {(err[:nnz] / (bound[:nnz] + 1e-300)).max():.3f}")
    assert torch.all(err <= bound)


# ------------------------------------------------------------ tail and guards

@pytest.mark.parametrize("dim", [9, 100, 260])
@pytest.mark.parametrize("mode", MODES)
def test_tail_and_guards(dim, mode):
    """NaN weights in the tail and NaN rows behind missed map entries change
    nothing, dw is exactly 0 in the tail, and canaries after dw[nnz],
    bag_scale[B] and out[B] are untouched."""
    ops, ext = _ops(), _ext()
    vals, offsets = _problem(pow2=False, seed=400 + dim)
    g = torch.Generator().manual_seed(500 + dim)
    uniq, inverse, row_map = _maps(vals, N_ROWS, dim)
    u = uniq.numel()
    rows = torch.randn(N_ROWS, dim, generator=g)
    grad_out = torch.randn(B, dim, generator=g)
    clean = torch.rand(vals.numel(), generator=g) + 0.5
    nnz = int(offsets[-1])
    clean[nnz:] = 0
    w = _nan_tail(clean, offsets)
    rows_nan = rows.clone()
    used = torch.zeros(N_ROWS, dtype=torch.bool)
    used[row_map[row_map >= 0]] = True
    rows_nan[~used] = float("nan")      # rows no live map entry names
    assert not used.all()

    a = _run_gpu(ops, rows, inverse, row_map, offsets, clean, grad_out, mode,
                 u)
    b = _run_gpu(ops, rows_nan, inverse, row_map, offsets, w, grad_out, mode,
                 u)
    names = ("out", "bag_of", "bag_scale", "ugrads", "counts", "dw")
    for name, x, y in zip(names, a, b):
        assert y.dtype != torch.float32 or bool(torch.isfinite(y).all()), name
        if name != "ugrads":
            assert torch.equal(x, y), name
    assert torch.all(b[5][nnz:] == 0)
    # ugrads are fp32 atomic sums, whose order differs run to run: each run
    # is within the row-gradient bound of test_random_within_fp32_bound of
    # the exact sum, so two runs are within twice that bound of each other
    bag, _, lens = _bag_pos(offsets, vals.numel())
    r_bag = b[1].cpu()
    r_scale = b[2].cpu().double()
    mag_g, cnt = ops.reduce_bags_weighted_by_inverse(
        inverse, grad_out.double().abs(), r_bag, clean.double(), r_scale, u)
    le = torch.where(bag >= 0, lens.double()[bag.clamp(min=0)],
                     torch.zeros(()).double())
    lmax = torch.zeros(u, dtype=torch.float64).scatter_reduce(
        0, inverse, le, "amax")
    bound = (cnt.double() + lmax + 4).unsqueeze(1) * EPS * mag_g
    assert torch.all((a[3] - b[3]).abs().cpu().double() <= 2 * bound)

    # canaries behind caller-provided outputs
    PAD, CANARY = 64, 12345.0
    cap = vals.numel()
    out_buf = torch.full((B * dim + PAD,), CANARY, device=DEV)
    sc_buf = torch.full((B + PAD,), CANARY, device=DEV)
    dw_buf = torch.full((cap + PAD,), CANARY, device=DEV)
    mode_i = ops.POOL_MODES[mode]
    out, bag_of, scale = ext.pool_fwd_weighted(
        _d(rows_nan), _d(inverse), _d(row_map), _d(offsets), _d(w), mode_i,
        out=out_buf[:B * dim].view(B, dim), bag_scale=sc_buf[:B])
    dw = ext.pool_wgrad(_d(rows_nan), _d(inverse), _d(row_map), _d(w), bag_of,
                        scale, out, _d(grad_out), mode_i, dw=dw_buf[:cap])
    assert out.data_ptr() == out_buf.data_ptr()
    assert torch.equal(out, b[0]) and torch.equal(scale, b[2])
    assert torch.equal(dw, b[5])
    for buf, n in ((out_buf, B * dim), (sc_buf, B), (dw_buf, cap)):
        assert torch.all(buf[n:] == CANARY)


# --------------------------------------------------------------------- engine

def _engine_weights(n=3):
    """Positive per-element weights, one tensor per engine batch."""
    out = []
    for i, (vals, offsets) in enumerate(_engine_batches(False, n)):
        g = torch.Generator().manual_seed(600 + i)
        out.append(_nan_tail(torch.rand(vals.numel(), generator=g) * 1.75
                             + 0.25, offsets))
    return out


def _step(ctx, emb, t, vals, offsets, w):
    """One train step; ``w`` is a leaf that requires grad."""
    w.grad = None
    out = emb(vals, offsets, per_sample_weights=w)
    (out * t).sum().backward()
    ctx.update_all_weights()
    return out


@functools.lru_cache(maxsize=None)
def _cpu_reference(hash_mode, dim, mode):
    """CPU-engine table and per-step w.grad (computed once, shared by the
    three routes)."""
    batches = _engine_batches(hash_mode)
    ctx, emb, t = _make("cpu", hash_mode, dim, mode)
    wgrads = []
    for (vals, offsets), w in zip(batches, _engine_weights()):
        w = w.clone().requires_grad_()
        _step(ctx, emb, t, vals, offsets, w)
        wgrads.append(w.grad.clone())
    table, _ = _table(emb, batches, "cpu")
    _reset()
    return table, wgrads


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("hash_mode,dim,mode", ENGINE_CASES)
def test_weighted_engine_matches_cpu(hash_mode, dim, mode, route):
    """3 Adagrad steps of the weighted EmbeddingBag on the GPU == the CPU
    engine on the same batches, table and the weights' own gradient."""
    force_remote, padded = ROUTES[route]
    batches = _engine_batches(hash_mode)
    ctx, emb, t = _make(DEV, hash_mode, dim, mode, force_remote, padded)
    wgrads = []
    for (vals, offsets), w in zip(batches, _engine_weights()):
        w = w.to(DEV).requires_grad_()
        _step(ctx, emb, t, vals.to(DEV), offsets.to(DEV), w)
        wgrads.append(w.grad.cpu())
    got, n_keys = _table(emb, batches, DEV)
    sharded = emb.variable.sharded
    assert sharded.shard.num_rows == n_keys     # the -1 tail made no row
    if padded:
        sharded.check_padded_overflow()
    _reset()
    ref, ref_wgrads = _cpu_reference(hash_mode, dim, mode)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    for (vals, offsets), a, b in zip(batches, wgrads, ref_wgrads):
        nnz = int(offsets[-1])
        assert float(b.abs().max()) > 1e-3
        assert torch.all(a[nnz:] == 0)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


# -------------------------------------------------------------- graph capture

@pytest.mark.parametrize("hash_mode,dim,mode", ENGINE_CASES)
def test_graph_replay_of_weighted_step(hash_mode, dim, mode):
    """One captured weighted train step (forward, backward with the weight
    gradient, commit) replayed over fresh batches trains the same table and
    gives the same w.grad as eager execution."""
    batches = _engine_batches(hash_mode)
    weights = _engine_weights()
    reserve = 16384 if hash_mode else 0

    # eager reference: the graph run below warms up with 6 steps on batch 0
    ctx, emb, t = _make(DEV, hash_mode, dim, mode, reserve=reserve)
    ref_wgrads = []
    seq = [(batches[0], weights[0])] * 6 + list(zip(batches, weights))
    for (vals, offsets), w in seq:
        w = w.to(DEV).requires_grad_()
        _step(ctx, emb, t, vals.to(DEV), offsets.to(DEV), w)
        ref_wgrads.append(w.grad.clone())
    ref_wgrads = ref_wgrads[6:]
    ref, _ = _table(emb, batches, DEV)

    ctx, emb, t = _make(DEV, hash_mode, dim, mode, reserve=reserve)
    cap = max(v.numel() for v, _ in batches)
    s_vals = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    s_off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    s_w = torch.zeros(cap, device=DEV, requires_grad=True)

    def load(batch, w):
        vals, offsets = batch
        s_vals.fill_(-1)
        s_vals[:vals.numel()].copy_(vals)
        s_off.copy_(offsets)
        with torch.no_grad():
            s_w.fill_(float("nan"))
            s_w[:w.numel()].copy_(w)

    # warm-up as in tests/test_gpu_graph.py: 3 eager + 3 side-stream steps
    load(batches[0], weights[0])
    for _ in range(3):
        _step(ctx, emb, t, s_vals, s_off, s_w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(ctx, emb, t, s_vals, s_off, s_w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(ctx, emb, t, s_vals, s_off, s_w)
    outs, wgrads = [], []
    for batch, w in zip(batches, weights):  # capture records, not executes
        load(batch, w)
        graph.replay()
        outs.append(out.clone())
        wgrads.append(s_w.grad.clone())
    torch.cuda.synchronize()
    assert not torch.equal(outs[0], outs[1])
    got, n_keys = _table(emb, batches, DEV)
    assert emb.variable.sharded.shard.num_rows == n_keys
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    for (vals, _), a, b in zip(batches, wgrads, ref_wgrads):
        assert float(b.abs().max()) > 1e-3
        torch.testing.assert_close(a[:vals.numel()], b, rtol=1e-4,
                                   atol=1e-5)
        assert torch.all(a[vals.numel():] == 0)
