"""Delta checkpoints on the GPU: the four kernels against their torch forms
(k_mark_rows, k_delta_count + k_delta_compact, k_delta_gather), the
base + deltas == full dump chain on HipVariableShard eager and under a
captured step, the export's peak memory, live serving updates of fp32 /
int8 / fp16 tables, and the untouched default-off path. Every comparison
is exact: the feature copies rows and does no arithmetic."""

import os

import pytest
import torch

import delta_ref as dr
from openembedding_amd import checkpoint

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _dev(t, dtype=None):
    return torch.as_tensor(t, dtype=dtype).to(DEV)


# ------------------------------------------------------------- 9. mark_rows

@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 1025))
def test_mark_rows_matches_torch_form(ext, n, masked):
    R, PAD, CANARY, EPOCH = 300, 64, -7, 5
    g = torch.Generator().manual_seed(n * 2 + masked)
    slots = torch.randint(0, R, (n,), generator=g, dtype=torch.int64)
    slots[::3] = slots[0]                        # duplicated slots
    for i, bad in enumerate((-1, R, R + 5)):     # next to valid ones
        if n > 2 * i + 1:
            slots[2 * i + 1] = bad
    mask = (torch.rand(n, generator=g) < 0.6).to(torch.uint8) \
        if masked else None
    old = torch.randint(0, 4, (R,), generator=g, dtype=torch.int32)
    epoch_dev = _dev([EPOCH], torch.int32)
    for u in (None, 0, n - 1, n):
        buf = torch.full((R + 2 * PAD,), CANARY, dtype=torch.int32)
        buf[PAD:PAD + R] = old
        buf = buf.to(DEV)
        row_epoch = buf[PAD:PAD + R]
        ext.mark_rows(slots.to(DEV),
                      mask.to(DEV) if masked else None,
                      None if u is None else _dev([u], torch.int32),
                      epoch_dev, row_epoch)
        want = old.clone()
        live = torch.arange(n) < (n if u is None else u)
        if masked:
            live &= mask != 0
        live &= (slots >= 0) & (slots < R)
        want[slots[live]] = EPOCH
        got = buf.cpu()
        assert torch.equal(got[PAD:PAD + R], want), (n, masked, u)
        assert bool((got[:PAD] == CANARY).all())
        assert bool((got[PAD + R:] == CANARY).all())
    # a bool mask is a byte mask too
    if masked:
        re2 = old.clone().to(DEV)
        ext.mark_rows(slots.to(DEV), (mask != 0).to(DEV), None, epoch_dev,
                      re2)
        assert torch.equal(re2.cpu(), want)


# -------------------------------------------------------- 10. select_changed

def _patterns(R, g):
    idx = torch.arange(R)
    return {
        "none": torch.zeros(R, dtype=torch.bool),
        "all": torch.ones(R, dtype=torch.bool),
        "first": idx == 0,
        "last": idx == R - 1,
        "alternating": idx % 2 == 1,
        "random10": torch.rand(R, generator=g) < 0.1,
    }


@pytest.mark.parametrize("mode", ("hash", "array"))
@pytest.mark.parametrize("which", range(8))
def test_select_changed_matches_nonzero(ext, which, mode):
    tile = int(ext.DELTA_TILE_ROWS)
    R = (1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5)[which]
    g = torch.Generator().manual_seed(which)
    idx = torch.arange(R)
    if mode == "hash":
        nrows = max(1, (R * 2) // 3) if R > 1 else 1
        live = idx < nrows
    else:
        live = torch.rand(R, generator=g) < 0.7      # a sparse valid bitmap
        live[0] = live[R - 1] = True
    for name, changed in _patterns(R, g).items():
        # unchanged rows carry an older stamp (0 or 2), changed ones 5;
        # beyond the live rows the stamps are stale and must be ignored
        stamps = torch.where(torch.rand(R, generator=g) < 0.5, 0, 2)
        stamps = torch.where(changed, 5, stamps).to(torch.int32)
        stamps[~live & (idx % 3 == 0)] = 9
        row_epoch = stamps.to(DEV)
        for since in (1, 5, 6, 10):              # below, at, above, none
            if mode == "hash":
                slots, n_dev = ext.select_changed(
                    row_epoch, since, nrows_dev=_dev([nrows], torch.int32))
            else:
                slots, n_dev = ext.select_changed(
                    row_epoch, since, valid=live.to(torch.uint8).to(DEV))
            want = ((stamps >= since) & live).nonzero(as_tuple=True)[0]
            n = int(n_dev.item())
            slots = slots.cpu()
            tag = (R, mode, name, since)
            assert n_dev.dtype == torch.int32 and n_dev.numel() == 1
            assert slots.dtype == torch.int64 and slots.numel() == R
            assert n == want.numel(), tag
            assert torch.equal(slots[:n], want), tag
            assert bool((slots[n:] == -1).all()), tag
    # a live count beyond the buffer is clamped, never followed
    if mode == "hash":
        slots, n_dev = ext.select_changed(
            torch.full((R,), 3, dtype=torch.int32, device=DEV), 3,
            nrows_dev=_dev([R + 1000], torch.int32))
        assert int(n_dev.item()) == R
        assert torch.equal(slots.cpu(), idx)


def test_select_changed_empty_table(ext):
    slots, n_dev = ext.select_changed(
        torch.zeros(0, dtype=torch.int32, device=DEV), 1,
        nrows_dev=_dev([0], torch.int32))
    assert slots.numel() == 0 and int(n_dev.item()) == 0


# --------------------------------------------------- 11. gather_rows_by_slot

@pytest.mark.parametrize("mode", ("hash", "array"))
@pytest.mark.parametrize("sw", ("none", "dim", "2dim+1"))
@pytest.mark.parametrize("dim", (1, 9, 16, 17, 64, 65, 129))
def test_gather_rows_by_slot_matches_indexing(ext, dim, sw, mode):
    R, L, N = 200, 50, 37
    sd = {"none": 0, "dim": dim, "2dim+1": 2 * dim + 1}[sw]
    g = torch.Generator().manual_seed(dim * 7 + sd)
    weights = torch.randn(R, dim, generator=g)
    state = torch.randn(R, sd, generator=g)
    slots = torch.randperm(R, generator=g)[:L].sort().values
    slots[11] = R + 3                    # outside the slab
    slots[29] = -1
    slots[33] = R
    if mode == "hash":                   # keys across the signed range
        slot_keys = (torch.randint(0, 2**62, (R,), generator=g) - 2**61) * 4 \
            + torch.randint(0, 4, (R,), generator=g)
        slot_keys[int(slots[0])] = -2**63
        slot_keys[int(slots[1])] = 2**63 - 1
        want_keys = lambda s: slot_keys[s]          # noqa: E731
        kw = {"slot_keys": slot_keys.to(DEV)}
    else:
        want_keys = lambda s: s * 3 + 2             # noqa: E731
        kw = {"shard_num": 3, "shard_id": 2}
    w_dev, s_dev = weights.to(DEV), state.to(DEV)
    n_dev = _dev([N], torch.int32)
    CAP = 24
    # windows ending inside, at and beyond n_dev, and one wholly beyond
    for start, count in ((0, 10), (5, 24), (30, 7), (30, 20), (40, 5),
                         (36, 1), (0, 0)):
        k_out = torch.full((CAP,), -99, dtype=torch.int64, device=DEV)
        w_out = torch.full((CAP, dim), -7.0, device=DEV)
        s_out = torch.full((CAP, sd), -7.0, device=DEV)
        ext.gather_rows_by_slot(w_dev, s_dev, slots=slots.to(DEV),
                                start=start, count=count, n_dev=n_dev,
                                keys_out=k_out, w_out=w_out, s_out=s_out,
                                **kw)
        wk = torch.full((CAP,), -99, dtype=torch.int64)
        ww = torch.full((CAP, dim), -7.0)
        ws = torch.full((CAP, sd), -7.0)
        for i in range(count):
            pos = start + i
            s = int(slots[pos]) if pos < L else -1
            if pos < N and 0 <= s < R:
                wk[i], ww[i], ws[i] = want_keys(s), weights[s], state[s]
        tag = (dim, sd, mode, start, count)
        assert torch.equal(k_out.cpu(), wk), tag
        assert torch.equal(w_out.cpu(), ww), tag
        assert torch.equal(s_out.cpu(), ws), tag
    # a window past the slot list itself writes nothing either
    k_out = torch.full((CAP,), -99, dtype=torch.int64, device=DEV)
    w_out = torch.full((CAP, dim), -7.0, device=DEV)
    s_out = torch.full((CAP, sd), -7.0, device=DEV)
    ext.gather_rows_by_slot(w_dev, s_dev, slots=slots.to(DEV), start=L - 2,
                            count=10, n_dev=_dev([L + 100], torch.int32),
                            keys_out=k_out, w_out=w_out, s_out=s_out, **kw)
    assert bool((k_out[2:] == -99).all()) and bool((w_out[2:] == -7).all())
    assert torch.equal(w_out[:2].cpu(), weights[slots[L - 2:]])


# ------------------------------------- the stamp rules on HipVariableShard

@pytest.mark.parametrize("table", ("hash", "array"))
def test_stamp_rules_on_the_gpu_shard(table):
    """The device overrides under tracking: stamps of created, updated and
    imported rows, ``set_optimizer`` (which goes through the temporary
    ``_nrows`` / ``valid`` views), ``row_epoch`` growing with the slab past
    its initial capacity, and ``clear``. Same sets as computed by hand and
    as the CPU oracle gives."""
    from openembedding_amd.core.variable import (HASH_VOCAB_THRESHOLD,
                                                 VariableMeta, VariableShard)
    from openembedding_amd.core.variable_gpu import HipVariableShard
    grow = HipVariableShard.INITIAL_ROW_CAP + 3000
    vocab = HASH_VOCAB_THRESHOLD if table == "hash" else grow + 2000
    results = []
    for cls, dev in ((HipVariableShard, DEV), (VariableShard, "cpu")):
        sh = cls(VariableMeta(0, 4, vocabulary_size=vocab), device=dev)
        sh.set_optimizer("adagrad", learning_rate=0.1)
        sh.track_changes()
        if cls is HipVariableShard:
            cap0 = sh.row_epoch.numel()
            assert sh.row_epoch.is_cuda and sh.row_epoch.dtype == torch.int32
        results.append(dr.stamp_scenario(sh, grow))
        if cls is HipVariableShard:
            assert int(sh.epoch_dev.item()) == sh.epoch == 5
            if table == "hash":
                assert sh.row_epoch.numel() > cap0      # it did grow
    assert results[0] == dr.stamp_scenario_by_hand(grow)
    assert results[0] == results[1]


# -------------------------------------------- 12. the chain on the GPU shard

def _check_chain(tmp_path, var, info, table, opt):
    uri = info["uri"]
    _, k1 = dr.dump_rows(uri["D1"])
    _, k2 = dr.dump_rows(uri["D2"])
    assert sorted(k1) == sorted(dr.KEYS_B) and len(k1) == 150
    assert sorted(k2) == sorted(set(dr.KEYS_C))
    assert info["d1"] == {"since": 2, "epoch": 2, "rows": 150}
    assert info["d2"] == {"since": 3, "epoch": 3,
                          "rows": len(set(dr.KEYS_C))}
    c1, _, v1 = dr.make_consumer(DEV, table, opt)
    checkpoint.load_model(c1, uri["A"])
    checkpoint.apply_delta(c1, uri["D1"])
    checkpoint.apply_delta(c1, uri["D2"])
    c2, _, v2 = dr.make_consumer(DEV, table, opt)
    checkpoint.load_model(c2, uri["B"])
    got, want = dr.rows_by_key(v1.shard), dr.rows_by_key(v2.shard)
    assert want[2] is not None and want[0].numel() == 1060
    assert want[2].shape[1] == var.shard.state_dim > 0
    dr.assert_same_rows(got, want)
    dr.assert_same_rows(got, dr.rows_by_key(var.shard))


@pytest.mark.parametrize("opt", ("adagrad", "adam"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_chain_equals_full_dump_eager(tmp_path, table, opt):
    from openembedding_amd.core.variable_gpu import HipVariableShard
    ctx, st, var, info = dr.run_chain(tmp_path, DEV, table, opt)
    assert type(var.shard) is HipVariableShard
    assert var.shard.row_epoch.is_cuda and var.shard.epoch_dev.is_cuda
    assert int(var.shard.epoch_dev.item()) == var.shard.epoch == 5
    _check_chain(tmp_path, var, info, table, opt)


def _fixed_batch(keys, seed, n=1200):
    """Every key at least once, resampled up to the captured batch size."""
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor(keys, dtype=torch.int64)
    k = torch.cat([k, k[torch.randint(0, k.numel(), (n - k.numel(),),
                                      generator=g)]])
    k = k[torch.randperm(n, generator=g)]
    return k.to(DEV), torch.randn(n, dr.DIM, generator=g).to(DEV)


@pytest.mark.parametrize("opt", ("adagrad", "adam"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_chain_equals_full_dump_captured(tmp_path, table, opt):
    """One captured pull -> push -> update_weights, replayed on fresh
    batches with a delta cut between the replays. The second delta holding
    exactly the second batch's keys shows that the stamp kernel reads the
    epoch through ``epoch_dev`` (a by-value epoch would be frozen at 1)."""
    ctx, st, var = dr.make_trainer(DEV, table, opt, reserve=4096)
    uri = {n: os.path.join(str(tmp_path), n) for n in ("A", "D1", "D2", "B")}
    static_k, static_g = _fixed_batch(dr.KEYS_A, 1)

    def step():
        _, h = var.pull(static_k)
        var.push(h, static_g)
        st.update_weights()

    step()                                   # phase A, eagerly
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    checkpoint.dump_model(ctx, uri["A"])
    info = {"uri": uri}
    for name, keys, seed in (("d1", dr.KEYS_B, 2), ("d2", dr.KEYS_C, 3)):
        k, gr = _fixed_batch(keys, seed)
        static_k.copy_(k)
        static_g.copy_(gr)
        graph.replay()
        torch.cuda.synchronize()
        info[name] = checkpoint.dump_delta(ctx, uri[name.upper()])
    checkpoint.dump_model(ctx, uri["B"])
    _check_chain(tmp_path, var, info, table, opt)


def test_export_changed_reuses_one_staging_block(monkeypatch):
    monkeypatch.setattr(checkpoint, "BLOCK_ROWS", 64)
    ctx, st, var = dr.make_trainer(DEV, "hash", "adam")
    dr.train(st, var, dr.KEYS_A[:200], 1)
    sh = var.shard
    blocks, ptrs = [], set()
    for k, w, s in sh.export_changed(1):
        ptrs.add((k.data_ptr(), w.data_ptr(), s.data_ptr()))
        blocks.append((k.cpu(), w.cpu(), s.cpu()))
    assert [b[0].numel() for b in blocks] == [64, 64, 64, 8]
    assert len(ptrs) == 1
    n = int(sh.nrows_dev.item())
    assert torch.equal(torch.cat([b[0] for b in blocks]),
                       sh.slot_keys[:n].cpu())         # ascending slots
    assert torch.equal(torch.cat([b[1] for b in blocks]),
                       sh.weights[:n].cpu())
    assert torch.equal(torch.cat([b[2] for b in blocks]), sh.state[:n].cpu())
    assert list(sh.export_changed(2)) == []


# ----------------------------------------------------------- 13. peak memory

def test_export_changed_never_copies_the_slab():
    from openembedding_amd.core.variable import VariableMeta
    from openembedding_amd.core.variable_gpu import HipVariableShard
    ROWS, DIM = 1_000_000, 64
    sh = HipVariableShard(VariableMeta(0, DIM), device=DEV)
    sh.set_optimizer("adagrad", learning_rate=0.1)
    sh.reserve_rows(ROWS + ROWS // 50)
    step = 1 << 18
    for start in range(0, ROWS, step):
        keys = torch.arange(start, min(start + step, ROWS), device=DEV)
        sh.import_rows(keys, torch.randn(keys.numel(), DIM, device=DEV))
    sh.track_changes()
    changed = torch.arange(0, ROWS, 100, device=DEV)            # 1 %
    sh.import_rows(changed, torch.randn(changed.numel(), DIM, device=DEV))
    R, sd = sh.row_epoch.numel(), sh.state_dim
    assert R == sh.weights.shape[0] and sd == DIM
    slab = sh.weights.numel() * 4 + sh.state.numel() * 4

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = [k.cpu() for k, w, s in sh.export_changed(1)]
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert torch.equal(torch.cat(got).sort().values, changed.cpu())
    # the slot list; its scratch, all sized by the tile count: the int32
    # counts, their int32 scan, and the scan's own temporary storage, for
    # which one 8-byte descriptor per scanned element is an upper bound
    # (it keeps one per group of elements); the allocator's rounding of
    # each of the (fewer than 16) tensors to 512 bytes; two staging blocks
    tiles = -(-R // int(sh.ext.DELTA_TILE_ROWS))
    scratch = tiles * (4 + 4 + 8) + 16 * 512
    bound = (R * 8 + scratch
             + 2 * checkpoint.BLOCK_ROWS * (8 + 4 * DIM + 4 * sd))
    print(f"export_changed peak rise {rise} B, bound {bound} B, "
          f"slab {slab} B")
    assert rise < bound
    assert bound < slab // 4


# ------------------------------------------------------- 14. serving updates

@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    out = {}
    for table in ("hash", "array"):
        tmp = tmp_path_factory.mktemp(f"chain_{table}")
        ctx, _st, _var, info = dr.run_chain(tmp, "cpu", table, "adagrad")
        ctx.finalize()
        out[table] = info["uri"]
    return out


def _packed_by_key(sh):
    if sh.meta.use_hash_table:
        n = sh.num_rows
        keys, packed = sh.slot_keys[:n].cpu(), sh.slab[:n].cpu()
    else:
        slots = (sh.valid_u8 != 0).nonzero(as_tuple=True)[0]
        keys, packed = slots.cpu(), sh.slab[slots].cpu()
    order = torch.argsort(keys)
    return keys[order], packed[order]


@pytest.mark.parametrize("fmt", (None, "int8", "fp16"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_served_model_update_equals_fresh_load(chains, table, fmt):
    m, fresh = dr.check_served_chain(chains[table], DEV, fmt)
    a, b = m.variables[0].shard, fresh.variables[0].shard
    assert a.device.type == "cuda"
    if fmt is None:
        from openembedding_amd.core.variable_gpu import HipVariableShard
        assert type(a) is HipVariableShard
        dr.assert_same_rows(dr.rows_by_key(a, False),
                            dr.rows_by_key(b, False))
    else:
        ka, pa = _packed_by_key(a)
        kb, pb = _packed_by_key(b)
        assert torch.equal(ka, kb) and ka.numel() == 1060
        assert torch.equal(pa, pb)


# ------------------------------------------------ 15. default path untouched

class _Recorder:
    """Stands in for the extension module and lists the bindings called."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call


@pytest.mark.parametrize("table", ("hash", "array"))
def test_tracking_off_adds_no_launch_and_no_tensor(tmp_path, table):
    """With tracking off the shard makes the calls it made before tracking
    existed: no mark_rows among the bindings of a step, no tracking tensor,
    and a captured step replays to what eager computes. Tracking on adds
    exactly one mark_rows per lookup-or-insert and one per optimizer
    application, and changes no number."""
    def run(track, captured):
        ctx, st, var = dr.make_trainer(DEV, table, "adagrad", track=track,
                                       reserve=4096)
        sh = var.shard
        rec = _Recorder(sh.ext)
        sh.ext = rec
        k0, g0 = dr.batch(dr.KEYS_A[:500], 1, device=DEV)
        static_k, static_g = k0.clone(), g0.clone()

        def step():
            _, h = var.pull(static_k)
            var.push(h, static_g)
            st.update_weights()

        step()
        calls = list(rec.calls)
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
        for seed, lo in ((2, 100), (3, 400)):
            k, gr = dr.batch(list(range(lo, lo + 500)), seed, device=DEV)
            static_k.copy_(k)
            static_g.copy_(gr)
            graph.replay() if captured else step()
        torch.cuda.synchronize()
        return sh, calls, dr.rows_by_key(sh)

    sh_off, calls_off, rows_off = run(False, False)
    assert "mark_rows" not in calls_off
    for name in ("row_epoch", "epoch_dev", "_epoch"):
        assert not hasattr(sh_off, name)
    sh_on, calls_on, rows_on = run(True, False)
    assert calls_on.count("mark_rows") == 2
    assert [c for c in calls_on if c != "mark_rows"] == calls_off
    # a batch repeats a key at most twice, so the sums are order-free and
    # the runs comparable bit for bit
    dr.assert_same_rows(rows_on, rows_off)
    _, calls_cap, rows_cap = run(False, True)
    assert calls_cap == calls_off
    dr.assert_same_rows(rows_cap, rows_off)
