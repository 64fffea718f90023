"""GPU tests of the multi-hot pooled pull/push (all @gpu): k_pool_fwd and the
bag-indirected reduce against the CPU oracle (exact on integer data, derived
fp32 bound on random data), EmbeddingBag training GPU-vs-CPU on every route,
and hipGraph capture/replay of the pooled step.

Shapes sit on the kernels' edges: 67 bags (no multiple of a block's group
count), one dim per rung of the reduce ladder (9, 64, 100, and 130 for the
atomic fallback) plus 24 and 260 for the gather's own rungs (two column
fragments on 16 lanes; more than one column pass), bag lengths
0 / 1 / G-1 / G / G+1 for every lane-group
width in use (8, 16, 64) and the gather's 4-element preload step, one bag
longer than a block's 256 elements, nnz no multiple of 256, and a -1 tail
behind offsets[-1]."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 67
DIMS = [9, 24, 64, 100, 130, 260]
MODES = ["sum", "mean", "sqrtn"]
TAIL = 37
VOCAB = 700

_EDGE = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300, 0]
_POW2 = [0, 1, 2, 4, 8, 16, 64, 512, 0, 32, 128]


def _lens(pow2: bool):
    g = torch.Generator().manual_seed(11)
    head = _POW2 if pow2 else _EDGE
    n_fill = B - len(head) - 1
    if pow2:
        fill = (2 ** torch.randint(0, 7, (n_fill,), generator=g)).tolist()
    else:
        fill = torch.randint(0, 90, (n_fill,), generator=g).tolist()
        fill[-1] += (256 - (sum(head) + sum(fill)) % 256) % 256 + 3
    lens = head + fill + [0]            # empty first, in the middle, last
    assert len(lens) == B
    assert pow2 or sum(lens) % 256 != 0
    return lens


def _problem(pow2: bool, seed: int = 0, vocab: int = VOCAB):
    """(values [nnz + TAIL] with a -1 tail, offsets [B+1]) on the CPU."""
    lens = _lens(pow2)
    g = torch.Generator().manual_seed(seed)
    nnz = sum(lens)
    vals = torch.randint(0, vocab, (nnz,), dtype=torch.int64, generator=g)
    vals[::5] = 7                       # a key shared by many bags
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64),
                         torch.tensor(lens).cumsum(0)])
    s = int(offsets[lens.index(max(lens))])
    vals[s + 1:s + 4] = vals[s]         # a key repeated inside one bag
    vals = torch.cat([vals, torch.full((TAIL,), -1, dtype=torch.int64)])
    return vals, offsets


def _ops():
    from openembedding_amd.ops import dispatch, require_hip
    require_hip()
    return dispatch


def _maps(vals, n_rows, seed):
    """unique/inverse plus a second-level map onto ``n_rows`` rows with
    misses: the tail key -1 and every 9th unique resolve to row -1."""
    uniq, inverse = torch.unique(vals, return_inverse=True)
    g = torch.Generator().manual_seed(seed)
    row_map = torch.randperm(n_rows, generator=g)[:uniq.numel()]
    row_map[uniq < 0] = -1
    row_map[4::9] = -1
    return uniq, inverse, row_map


# -------------------------------------------------------------- kernel, exact

@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_kernels_exact_on_integer_data(dim, mode):
    """Small-integer rows and gradients: fp32 sums are exact in any order
    (mean only with power-of-two lengths), so the HIP kernels must equal the
    CPU oracle bit for bit, counts included."""
    ops = _ops()
    vals, offsets = _problem(pow2=(mode == "mean"), seed=dim)
    g = torch.Generator().manual_seed(dim)
    n_rows = VOCAB + 50
    rows = torch.randint(-8, 9, (n_rows, dim), generator=g).float()
    grad_out = torch.randint(-4, 5, (B, dim), generator=g).float()
    uniq, inverse, row_map = _maps(vals, n_rows, dim)
    u = uniq.numel()
    d = lambda t: t.to(DEV)

    # second-level map, int64 (table slots) and int32 (padded pos_of)
    ref, ref_bag = ops.pool_fwd(rows, inverse, row_map, offsets, mode)
    for mdt in (torch.int64, torch.int32):
        out, bag_of = ops.pool_fwd(d(rows), d(inverse), d(row_map.to(mdt)),
                                   d(offsets), mode)
        assert torch.equal(out.cpu(), ref)
        assert torch.equal(bag_of.cpu(), ref_bag)
    assert torch.all(ref_bag[-TAIL:] == -1)
    again, _ = ops.pool_fwd(d(rows), d(inverse), d(row_map.to(mdt)),
                            d(offsets), mode)
    assert torch.equal(again, out)      # run-to-run bitwise reproducible

    # no-map form (inverse indexes rows) and identity form (gathered rows)
    ref2, _ = ops.pool_fwd(rows[:u], inverse, None, offsets, mode)
    out2, _ = ops.pool_fwd(d(rows[:u]), d(inverse), None, d(offsets), mode)
    assert torch.equal(out2.cpu(), ref2)
    elems = rows[vals.clamp(min=0)].contiguous()
    ref3, _ = ops.pool_fwd(elems, None, None, offsets, mode)
    out3, bag3 = ops.pool_fwd(d(elems), None, None, d(offsets), mode)
    assert torch.equal(out3.cpu(), ref3)
    assert torch.equal(bag3.cpu(), ref_bag)

    # backward: same (ugrads, counts) as the oracle, bit for bit
    ref_g, ref_c = ops.reduce_bags_by_inverse(inverse, grad_out, ref_bag,
                                              offsets, mode, u)
    got_g, got_c = ops.reduce_bags_by_inverse(d(inverse), d(grad_out),
                                              bag_of, d(offsets), mode, u)
    assert torch.equal(got_g.cpu(), ref_g)
    assert torch.equal(got_c.cpu(), ref_c)
    assert int(ref_c[uniq < 0].sum()) == 0      # the tail adds no count
    assert int(ref_c.sum()) == int(offsets[-1])


# ----------------------------------------------- kernel, random, fp32 bound

@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", MODES)
def test_kernels_random_within_fp32_bound(dim, mode):
    """Against a float64 oracle. Every output is a sum of ``terms`` fp32
    values (L per bag forward, c per key backward) rounded at most once per
    add (2^-24 relative each), scaled by a combiner scale that carries at
    most two more roundings, so |err| <= (terms + 2) * 2^-23 * sum|term|
    holds with a factor ~2 to spare; sum|term| comes from the oracle."""
    ops = _ops()
    vals, offsets = _problem(pow2=False, seed=100 + dim)
    g = torch.Generator().manual_seed(200 + dim)
    n_rows = VOCAB + 50
    rows = torch.randn(n_rows, dim, generator=g)
    grad_out = torch.randn(B, dim, generator=g)
    uniq, inverse, row_map = _maps(vals, n_rows, dim)
    u = uniq.numel()
    d = lambda t: t.to(DEV)
    eps = 2.0 ** -23

    out, bag_of = ops.pool_fwd(d(rows), d(inverse), d(row_map), d(offsets),
                               mode)
    ref, _ = ops.pool_fwd(rows.double(), inverse, row_map, offsets, mode)
    mag, _ = ops.pool_fwd(rows.double().abs(), inverse, row_map, offsets,
                          mode)
    terms = (offsets[1:] - offsets[:-1]).double().unsqueeze(1)
    err = (out.cpu().double() - ref).abs()
    print(f"fwd dim={dim} {mode}: max err {err.max():.3e}, "
          f"max err/bound {(err / ((terms + 2) * eps * mag + 1e-300)).max():.3f}")
    assert torch.all(err <= (terms + 2) * eps * mag)

    got_g, got_c = ops.reduce_bags_by_inverse(d(inverse), d(grad_out),
                                              bag_of, d(offsets), mode, u)
    bag_cpu = bag_of.cpu()
    ref_g, ref_c = ops.reduce_bags_by_inverse(inverse, grad_out.double(),
                                              bag_cpu, offsets, mode, u)
    mag_g, _ = ops.reduce_bags_by_inverse(inverse, grad_out.double().abs(),
                                          bag_cpu, offsets, mode, u)
    assert torch.equal(got_c.cpu(), ref_c)
    terms = ref_c.double().unsqueeze(1)
    err = (got_g.cpu().double() - ref_g).abs()
    print(f"bwd dim={dim} {mode}: max err {err.max():.3e}, "
          f"max err/bound {(err / ((terms + 2) * eps * mag_g + 1e-300)).max():.3f}")
    assert torch.all(err <= (terms + 2) * eps * mag_g)


# --------------------------------------------------------------------- engine

def _reset():
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()


def _engine_batches(hash_mode, n=3):
    vocab = (1 << 40) if hash_mode else VOCAB
    return [_problem(pow2=False, seed=300 + i, vocab=vocab) for i in range(n)]


def _make(device, hash_mode, dim, mode, force_remote=False, padded=None,
          reserve=0):
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    _reset()
    ctx = get_context(device)
    emb = embed.EmbeddingBag(-1 if hash_mode else VOCAB, dim, mode=mode)
    emb.variable.set_optimizer("adagrad", learning_rate=0.1,
                               initial_accumulator_value=0.1, epsilon=1e-10)
    emb.variable.sharded._force_remote = force_remote
    emb.variable.sharded._padded = padded
    if reserve:
        emb.variable.sharded.reserve_rows(reserve)
    w = torch.randn(B, dim, generator=torch.Generator().manual_seed(5))
    return ctx, emb, w.to(device)


def _step(ctx, emb, w, vals, offsets):
    out = emb(vals, offsets)
    (out * w).sum().backward()
    ctx.update_all_weights()
    return out


def _table(emb, batches, device):
    keys = torch.unique(torch.cat([v for v, _ in batches]))
    keys = keys[keys >= 0]
    return emb.variable.sparse_read(keys.to(device)).cpu(), keys.numel()


@functools.lru_cache(maxsize=None)
def _cpu_reference(hash_mode, dim, mode):
    """CPU-engine table after one step per batch (computed once, shared by
    the three routes)."""
    batches = _engine_batches(hash_mode)
    ctx, emb, w = _make("cpu", hash_mode, dim, mode)
    for vals, offsets in batches:
        _step(ctx, emb, w, vals, offsets)
    table, _ = _table(emb, batches, "cpu")
    _reset()
    return table


ENGINE_CASES = [(False, 9, "mean"), (True, 64, "sqrtn")]
ROUTES = {"fused": (False, None), "remote_exact": (True, False),
          "remote_padded": (True, True)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("hash_mode,dim,mode", ENGINE_CASES)
def test_engine_matches_cpu(hash_mode, dim, mode, route):
    """3 Adagrad steps of EmbeddingBag on the GPU == the CPU engine on the
    same batches (tolerance of tests/test_gpu_padded.py's GPU-vs-CPU
    check); _force_remote runs the multi-rank routes on one GPU."""
    force_remote, padded = ROUTES[route]
    batches = _engine_batches(hash_mode)
    ctx, emb, w = _make(DEV, hash_mode, dim, mode, force_remote, padded)
    for vals, offsets in batches:
        _step(ctx, emb, w, vals.to(DEV), offsets.to(DEV))
    got, n_keys = _table(emb, batches, DEV)
    sharded = emb.variable.sharded
    assert sharded.shard.num_rows == n_keys     # the -1 tail made no row
    if padded:
        sharded.check_padded_overflow()
    _reset()
    torch.testing.assert_close(got, _cpu_reference(hash_mode, dim, mode),
                               rtol=1e-4, atol=1e-5)


# -------------------------------------------------------------- graph capture

@pytest.mark.parametrize("hash_mode,dim,mode", ENGINE_CASES)
def test_graph_replay_of_pooled_step(hash_mode, dim, mode):
    """One captured pooled train step (fixed-capacity values buffer, device
    offsets) replayed over batches whose values AND offsets differ must
    train the same table as eager execution."""
    batches = _engine_batches(hash_mode)
    reserve = 16384 if hash_mode else 0

    # eager reference: the graph run below warms up with 6 steps on batch 0
    ctx, emb, w = _make(DEV, hash_mode, dim, mode, reserve=reserve)
    for vals, offsets in [batches[0]] * 6 + batches:
        _step(ctx, emb, w, vals.to(DEV), offsets.to(DEV))
    ref, _ = _table(emb, batches, DEV)

    ctx, emb, w = _make(DEV, hash_mode, dim, mode, reserve=reserve)
    cap = max(v.numel() for v, _ in batches)
    s_vals = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    s_off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)

    def load(vals, offsets):
        s_vals.fill_(-1)
        s_vals[:vals.numel()].copy_(vals)
        s_off.copy_(offsets)

    # warm-up as in tests/test_gpu_graph.py: 3 eager + 3 side-stream steps
    load(*batches[0])
    for _ in range(3):
        _step(ctx, emb, w, s_vals, s_off)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(ctx, emb, w, s_vals, s_off)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(ctx, emb, w, s_vals, s_off)
    outs = []
    for vals, offsets in batches:       # capture records without executing
        load(vals, offsets)
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    assert not torch.equal(outs[0], outs[1])
    got, n_keys = _table(emb, batches, DEV)
    assert emb.variable.sharded.shard.num_rows == n_keys
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
