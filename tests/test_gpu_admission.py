"""Feature admission on the GPU: k_admit_note / k_admit_resolve / k_admit_age
and HipVariableShard against the CPU shard and the independent emulation in
admission_ref.py. The kernels do integer work only, so key sets, sketch,
statistics and zero rows compare with ``torch.equal``; only trained rows use
the optimizer tolerance of test_gpu_numerics.py.

Slots are handed out by an atomic counter, so WHICH slot a key gets is not
fixed on the GPU; the tests compare which keys have a slot and that a key
keeps its slot, not the slot numbers. W = 256 makes many keys of one call
share cells: an estimate taken before all adds of the call landed would show
as a key set that differs from the emulation's."""

import pytest
import torch

import admission_ref as ar
from openembedding_amd.core.variable import VariableMeta, VariableShard
from openembedding_amd.parallel import sharded as sharded_mod
from openembedding_amd.parallel.sharded import ShardedVariable

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIM = 8
TOL = 3e-5      # test_gpu_numerics.py test_optimizer_parity_engine


@pytest.fixture(scope="module")
def ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


class Table:
    """The raw tensors ``ht_lookup_admit`` works on."""

    def __init__(self, W, D, cap=1 << 12, rows=1 << 12):
        self.tk = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
        self.tv = torch.zeros(cap, dtype=torch.int32, device=DEV)
        self.nrows = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.slot_keys = torch.full((rows,), -7, dtype=torch.int64,
                                    device=DEV)
        self.sketch = torch.zeros(D * W, dtype=torch.int32, device=DEV)
        self.stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.D = D

    def call(self, ext, keys, seed, min_count, u_dev=None):
        slots, new = ext.ht_lookup_admit(
            self.tk, self.tv, keys.to(DEV), self.nrows, self.slot_keys,
            self.sketch, self.D, seed, min_count, self.stats, u_dev)
        return slots.cpu(), new.cpu()


def _calls(n, rounds=4, seed=0):
    """``rounds`` batches of n unique keys out of a pool of 2n + 3, so keys
    come back in later calls."""
    g = torch.Generator().manual_seed(1000 * n + seed)
    pool = (torch.arange(2 * n + 3, dtype=torch.int64) * 2654435761) \
        % (1 << 40) + 1
    return [pool[torch.randperm(pool.numel(), generator=g)[:n]]
            for _ in range(rounds)]


def _check_call(t, ref, keys, got, want):
    """One call's (slots, new_mask) against the emulation's, and the state
    behind it."""
    slots, new = got
    rslots, rnew = want
    assert torch.equal(slots >= 0, rslots >= 0)
    assert torch.equal(slots[slots < 0], rslots[rslots < 0])     # all -1
    assert torch.equal(new, rnew)
    has = slots >= 0
    assert torch.equal(t.slot_keys.cpu()[slots[has]], keys[has])
    assert torch.equal(t.sketch.cpu(), torch.from_numpy(ref.sketch))
    assert t.stats.tolist() == [ref.admitted, ref.turned_away]
    assert int(t.nrows.item()) == len(ref.index)


@pytest.mark.parametrize("min_count", (1, 2, 3))
@pytest.mark.parametrize("D", (1, 4))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_kernels_match_emulation(ext, n, D, min_count):
    W, seed = 256, 7
    t, ref = Table(W, D), ar.RefAdmission(W, D, seed, min_count)
    seen = {}
    for keys in _calls(n):
        got = t.call(ext, keys, seed, min_count)
        _check_call(t, ref, keys, got, ref.call(keys))
        for k, s in zip(keys.tolist(), got[0].tolist()):
            if s >= 0:
                assert seen.setdefault(k, s) == s    # a key keeps its slot
    live = int(t.nrows.item())
    assert sorted(seen.values()) == list(range(live))
    assert torch.equal(t.slot_keys[:live].cpu().sort().values, ref.keys())
    if min_count == 1:
        assert ref.turned_away == 0 and live == len(seen)


def test_min_count_1_equals_plain_insert(ext):
    """Same hits, same inserts, same table as ht_lookup(insert=True)."""
    a, b = Table(256, 4), Table(256, 4)
    for keys in _calls(257):
        sa, na = a.call(ext, keys, 7, 1)
        sb, nb = ext.ht_lookup(b.tk, b.tv, keys.to(DEV), b.nrows,
                               b.slot_keys, True, None)
        assert torch.equal(na, nb.cpu())
        assert torch.equal(a.slot_keys.cpu()[sa], b.slot_keys.cpu()[sb.cpu()])
    assert int(a.nrows.item()) == int(b.nrows.item())


@pytest.mark.parametrize("n,live", ((300, 257), (300, 0), (64, 1)))
def test_bounded_call_ignores_the_garbage_tail(ext, n, live):
    W, D, seed, mc = 256, 4, 7, 2
    t, ref = Table(W, D), ar.RefAdmission(W, D, seed, mc)
    u_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    for keys in _calls(n, rounds=3):
        # the tail repeats live keys and names fresh ones: none may count
        keys = keys.clone()
        keys[live:] = torch.cat([keys[:live], keys + 12345])[:n - live]
        got = t.call(ext, keys, seed, mc, u_dev)
        _check_call(t, ref, keys, got, ref.call(keys, live))
        assert bool((got[0][live:] == -1).all())
        assert not got[1][live:].any()


def test_reserved_key_inside_the_batch(ext):
    W, D, seed, mc = 256, 4, 7, 2
    t, ref = Table(W, D), ar.RefAdmission(W, D, seed, mc)
    for keys in _calls(257, rounds=3):
        keys = keys.clone()
        keys[[0, 100, 256]] = -1
        got = t.call(ext, keys, seed, mc)
        _check_call(t, ref, keys, got, ref.call(keys))
        assert got[0][[0, 100, 256]].tolist() == [-1, -1, -1]


def test_overflow_of_the_slab_is_a_miss_and_counts_as_turned_away(ext):
    """A slab (reservation) of 8 rows and 40 keys that all qualify: 8 get a
    row, 32 get -1 now and at every later lookup; which 8 is up to the
    atomic counter."""
    t = Table(256, 4, rows=8)
    keys = _calls(40, rounds=1)[0]
    slots, new = t.call(ext, keys, 7, 1)
    assert sorted(slots[slots >= 0].tolist()) == list(range(8))
    assert int((slots == -1).sum()) == 32 and int(new.sum()) == 8
    assert torch.equal(new.bool(), slots >= 0)
    assert t.stats.tolist() == [8, 32]
    assert torch.equal(t.slot_keys.cpu()[slots[slots >= 0]],
                       keys[slots >= 0])
    sketch = t.sketch.clone()
    again, new2 = t.call(ext, keys, 7, 1)
    assert torch.equal(again, slots) and not new2.any()
    assert t.stats.tolist() == [8, 32]            # dropped keys: defined miss
    assert torch.equal(t.sketch, sketch)


# ------------------------------------------------------------------- ageing

@pytest.mark.parametrize("shift", (0, 1, 3, 30, 31, 64))
@pytest.mark.parametrize("W,D", ((1, 1), (1, 3), (2, 3), (4, 1), (256, 3),
                                 (4096, 4)))
def test_age_is_a_right_shift(ext, W, D, shift):
    g = torch.Generator().manual_seed(W * 10 + D)
    base = torch.randint(0, 1 << 31, (D * W,), generator=g,
                         dtype=torch.int64).to(torch.int32)
    base[::3] = base[::3] & 7                     # small counters too
    sk = base.to(DEV)
    ext.admit_age(sk, shift)
    want = torch.zeros_like(base) if shift >= 31 else base >> shift
    assert torch.equal(sk.cpu(), want)


def test_shard_age_matches_cpu():
    gpu, cpu = _hip(3, W=256, D=3), _cpu(3, W=256, D=3)
    for ks in ar.reference_stream()[:5]:
        gpu.pull(ks.to(DEV))
        cpu.pull(ks)
    assert torch.equal(gpu.export_admission().cpu(), cpu.export_admission())
    gpu.age_admission(1)
    cpu.age_admission(1)
    assert cpu.export_admission().any()
    assert torch.equal(gpu.export_admission().cpu(), cpu.export_admission())
    gpu.age_admission(31)
    assert not gpu.export_admission().any()


# ------------------------------------------------------------------- shards

def _setup(sh, min_count, W, D):
    sh.set_initializer("uniform", minval=-1.0, maxval=1.0)
    sh.set_optimizer("adagrad", learning_rate=0.1)
    if min_count:
        sh.set_admission(min_count, width=W, depth=D, seed=ar.STREAM_SEED)
    return sh


def _hip(min_count=None, W=4096, D=4):
    from openembedding_amd.core.variable_gpu import HipVariableShard
    return _setup(HipVariableShard(VariableMeta(0, DIM), device=DEV),
                  min_count, W, D)


def _cpu(min_count=None, W=4096, D=4):
    return _setup(VariableShard(VariableMeta(0, DIM)), min_count, W, D)


def _batch(i, ks):
    """Pull i of the reference stream with a seventh of it twice, shuffled,
    and a seeded gradient per element."""
    g = torch.Generator().manual_seed(50 + i)
    flat = torch.cat([ks, ks[::7]])
    flat = flat[torch.randperm(flat.numel(), generator=g)]
    return flat, torch.randn(flat.numel(), DIM, generator=g)


def _bags(i, nnz):
    """Ragged offsets over nnz elements (an empty bag among them) and a
    seeded gradient per bag."""
    g = torch.Generator().manual_seed(90 + i)
    cuts = torch.randint(0, nnz + 1, (99,), generator=g).sort().values
    offsets = torch.cat([torch.tensor([0, 0]), cuts, torch.tensor([nnz])])
    return offsets, torch.randn(offsets.numel() - 1, DIM, generator=g)


@pytest.fixture(scope="module")
def cpu_stream():
    """The CPU shard's run of the reference stream per route kind: the
    outputs of every step and the final rows by key (computed once)."""
    out = {}
    for kind in ("flat", "sum", "mean"):
        var = ShardedVariable(_cpu(ar.STREAM_MIN_COUNT))
        outs = []
        for i, ks in enumerate(ar.reference_stream()):
            outs.append(_route_step(var, kind, i, ks, "cpu"))
        k, w, s = var.shard.export_rows()
        o = k.argsort()
        out[kind] = (outs, k[o], w[o], s[o], var.shard.admission_stats())
    return out


def _route_step(var, kind, i, ks, dev):
    flat, grads = _batch(i, ks)
    if kind == "flat":
        out, h = var.pull(flat.to(dev))
        var.push(h, grads.to(dev))
    else:
        offsets, bag_grads = _bags(i, flat.numel())
        out, h = var.pull_pooled(flat.to(dev), offsets.to(dev), kind)
        var.push_pooled(h, bag_grads.to(dev), offsets.to(dev), kind)
    var.update_weights()
    return out.cpu()


ROUTES = ("pull", "pull_bounded", "pull_bounded_fused", "pooled_sum",
          "pooled_mean")


@pytest.mark.parametrize("route", ROUTES)
def test_reference_stream_through_every_pull_route(cpu_stream, monkeypatch,
                                                   route):
    ref = ar.stream_result(4096)
    gpu = _hip(ar.STREAM_MIN_COUNT)
    var = ShardedVariable(gpu)
    called = []
    for name in ("pull", "pull_bounded", "pull_bounded_fused",
                 "pull_pooled_bounded"):
        def spy(*a, _f=getattr(gpu, name), _n=name, **kw):
            called.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(gpu, name, spy)
    if route == "pull_bounded":
        monkeypatch.setattr(sharded_mod, "_FUSED_PULL", False)
    kind = {"pooled_sum": "sum", "pooled_mean": "mean"}.get(route, "flat")
    outs, ck, cw, cs, cstats = cpu_stream[kind]
    for i, ks in enumerate(ar.reference_stream()):
        if route == "pull":
            # the unique keys straight into the shard, reduced by hand
            flat, grads = _batch(i, ks)
            uk, inv = torch.unique(flat, return_inverse=True)
            ug = torch.zeros(uk.numel(), DIM).index_add_(0, inv, grads)
            rows = gpu.pull(uk.to(DEV))
            gpu.push(uk.to(DEV), ug.to(DEV),
                     torch.bincount(inv).to(DEV))
            gpu.update_weights()
            out = rows.cpu()[inv]
        else:
            out = _route_step(var, kind, i, ks, DEV)
        want = outs[i]
        assert torch.equal(out == 0, want == 0), f"zero rows differ, pull {i}"
        torch.testing.assert_close(out, want, rtol=TOL, atol=TOL)
    assert set(called) == {"pull_pooled_bounded" if kind != "flat"
                           else route}
    k, w, s = gpu.export_rows()
    o = k.cpu().argsort()
    assert torch.equal(k.cpu()[o], ref.keys()) and torch.equal(ck, ref.keys())
    assert torch.equal(gpu.export_admission().cpu(),
                       torch.from_numpy(ref.sketch))
    st = gpu.admission_stats()
    assert st == cstats
    assert (st["admitted"], st["turned_away"]) == (1194, ref.turned_away)
    torch.testing.assert_close(w.cpu()[o], cw, rtol=TOL, atol=TOL)
    torch.testing.assert_close(s.cpu()[o], cs, rtol=TOL, atol=TOL)


def test_unadmitted_pull_is_a_zero_row_and_push_is_dropped():
    gpu = _hip(2, W=256)
    keys = torch.tensor([5, 9, 11], device=DEV)
    ones = torch.ones(3, dtype=torch.int64, device=DEV)
    assert not gpu.pull(keys).any() and gpu.num_rows == 0
    gpu.push(keys, torch.ones(3, DIM, device=DEV), ones)
    gpu.update_weights()                        # a push is no sighting
    assert gpu.num_rows == 0 and gpu.admission_stats()["turned_away"] == 3
    rows = gpu.pull(keys)
    assert gpu.num_rows == 3 and bool((rows.abs().sum(1) > 0).all())
    for _ in range(3):                          # read-only never counts
        assert not gpu.pull_readonly(torch.tensor([77], device=DEV)).any()
    assert not gpu.pull(torch.tensor([77], device=DEV)).any()
    # import bypasses the filter
    gpu.import_rows(torch.tensor([500, 501], device=DEV),
                    torch.ones(2, DIM, device=DEV))
    assert gpu.num_rows == 5


def test_merged_commit_is_read_only():
    """Two pulls committed together go through _merge_bounded, whose lookup
    must not insert or count."""
    gpu = _hip(2, W=256)
    var = ShardedVariable(gpu)
    a = torch.tensor([1, 2, 3, 2], device=DEV)
    b = torch.tensor([3, 4, 4, 5], device=DEV)
    for _ in range(2):
        (oa, ha), (ob, hb) = var.pull(a), var.pull(b)
        var.push(ha, torch.ones_like(oa))
        var.push(hb, torch.ones_like(ob))
        var.update_weights()
    # first round: every key seen once, except 3 (twice: admitted by pull b)
    st = gpu.admission_stats()
    assert sorted(gpu.export_rows()[0].tolist()) == [1, 2, 3, 4, 5]
    assert (st["admitted"], st["turned_away"]) == (5, 5)


# ------------------------------------------------------------ graph capture

def test_captured_step_equals_eager():
    batches = [_batch(i, ks) for i, ks in
               enumerate(ar.reference_stream()[:5])]

    def make():
        sh = _hip(2, W=4096)
        sh.reserve_rows(4096)
        return sh, ShardedVariable(sh)

    def step(var, k, g):
        out, h = var.pull(k)
        var.push(h, g)
        var.update_weights()
        return out

    eager_sh, eager = make()
    for k, g in batches:
        step(eager, k.to(DEV), g.to(DEV))
    sh, var = make()
    static_k, static_g = batches[0][0].to(DEV), batches[0][1].to(DEV)
    step(var, static_k, static_g)
    torch.cuda.synchronize()
    static_k.copy_(batches[1][0])
    static_g.copy_(batches[1][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(var, static_k, static_g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(var, static_k, static_g)
    for k, g in batches[2:]:
        static_k.copy_(k)
        static_g.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sh.export_admission(), eager_sh.export_admission())
    assert sh.admission_stats() == eager_sh.admission_stats()
    assert sh.admission_stats()["admitted"] > 100
    (ka, wa, sa), (kb, wb, sb) = sh.export_rows(), eager_sh.export_rows()
    oa, ob = ka.argsort(), kb.argsort()
    assert torch.equal(ka[oa], kb[ob])
    torch.testing.assert_close(wa[oa], wb[ob], rtol=TOL, atol=TOL)
    torch.testing.assert_close(sa[oa], sb[ob], rtol=TOL, atol=TOL)
    # the last replay's output: zero rows where the emulation has no row yet
    rows = eager_sh.pull_readonly(batches[-1][0].to(DEV))
    assert torch.equal((static_out == 0).all(1), (rows == 0).all(1))


# ----------------------------------------------------------------- off path

class CountingExt:
    """Passes every attribute of the extension through, counting calls."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if not callable(fn):
            return fn

        def counted(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **kw)
        return counted


@pytest.mark.parametrize("on", (False, True))
def test_admission_off_launches_what_it_did_before(on):
    gpu = _hip(2 if on else None, W=256)
    assert hasattr(gpu, "admit_sketch") == on
    gpu.ext = proxy = CountingExt(gpu.ext)
    var = ShardedVariable(gpu)
    flat, grads = _batch(0, ar.reference_stream()[0])
    for _ in range(2):
        out, h = var.pull(flat.to(DEV))
        var.push(h, grads.to(DEV))
        var.update_weights()
        offsets, bag_grads = _bags(0, flat.numel())
        out, h = var.pull_pooled(flat.to(DEV), offsets.to(DEV), "sum")
        var.push_pooled(h, bag_grads.to(DEV), offsets.to(DEV), "sum")
        var.update_weights()
        gpu.pull(flat.unique().to(DEV))
    if on:
        assert proxy.calls["ht_lookup_admit"] == 6
        assert "ht_lookup" not in proxy.calls     # one block a commit
    else:
        assert proxy.calls["ht_lookup"] == 6
        assert "ht_lookup_admit" not in proxy.calls
        assert "admit_age" not in proxy.calls
