"""The segmented reduce that applies the optimizer (k_seg_reduce_apply of
ops/csrc/embops.hip) through ``reduce_apply_by_index``, and its routing in
push / update_weights (all @gpu). The reference is the two launches it
replaces, ``reduce_by_index`` then ``apply_optimizer``, on a clone of the
table: both walk the same index in the same order and share the optimizer's
device functions, so the tables must be torch.equal wherever the sums do not
depend on the arrival order inside a list. That holds for integer-valued
gradients (every partial sum is exact) with lists of any shape, and for
random gradients with lists of at most two elements (a + b == b + a).

``apply_optimizer`` itself is pinned to the fp64 oracle by
tests/test_gpu_sparse_core.py and ``reduce_by_index`` by
tests/test_gpu_segreduce.py. The checker and the key sets are
tests/fused_apply_ref.py, tested without a GPU in
tests/test_fused_apply_checkers.py.
"""

import os
import subprocess
import sys

import pytest
import torch

import fused_apply_ref as fref
import segreduce_ref as sref
import sparse_core_ref as ref
from openembedding_amd.core.variable_gpu import _OPT_IDS, _opt_cfg_vector
from openembedding_amd.ops import dispatch as ops
from openembedding_amd.parallel import sharded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = [1, 9, 10, 16, 17, 65, 128]
CATEGORIES = list(ref.CATEGORY_VARIANT)


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _T():
    return _ext().seg_reduce_threshold()


def _shapes_keys(g):
    """Lists of one, of a few, of exactly T and of T + 1 elements, and the
    reserved key: both roles and the boundary between them in one batch."""
    T = _T()
    parts = [torch.full((T,), 1002), torch.full((T + 1,), 1003),
             torch.arange(150), torch.randint(0, 40, (200,), generator=g),
             torch.full((5,), -1)]
    keys = torch.cat(parts).to(torch.int64)
    return keys[torch.randperm(keys.numel(), generator=g)]


def _key_set(kind, g):
    if kind == "shapes":
        return _shapes_keys(g)
    if kind == "one_list_20001":       # several rounds of the long role
        return torch.full((20001,), 42, dtype=torch.int64)
    if kind == "three_keys":           # three long lists
        pick = torch.randint(0, 3, (2049,), generator=g)
        return torch.tensor([3, -7, 1 << 40], dtype=torch.int64)[pick]
    if kind == "all_distinct":
        return torch.randperm(257, generator=g) * 2654435761 - 10 ** 12
    assert kind == "pairs"
    return fref.pair_keys(301, g)


def _index(flat):
    r = _ext().unique_bounded_indexed(flat.to(DEV), None)
    inv, u_dev, index = r[1], r[2], tuple(r[3:])
    u = int(u_dev.item())
    bad = sref.index_violations(inv.cpu(), u, *[t.cpu() for t in index],
                                _T())
    assert bad == [], bad
    return u, index, u_dev


def _run(variant, dim, flat, grads, call):
    """Both routes from the same table; returns what table_violations
    names. ``call(opt_id, w, s, slots, index, grads, cfg, u_dev)`` is the
    fused entry under test."""
    n = flat.numel()
    u, index, u_dev = _index(flat)
    case = ref.OptCase(variant, dim, n)
    slots = case.step(0)[0]            # distinct rows, -1 at every 7th
    opt_id = _OPT_IDS[case.category]
    cfg = _opt_cfg_vector(case.opt)
    gd, sl = grads.to(DEV), slots.to(DEV)
    want_w, want_s = case.weights.to(DEV), case.state.to(DEV)
    ugrads, counts = _ext().reduce_by_index(*index, gd, u_dev)
    _ext().apply_optimizer(opt_id, want_w, want_s, sl, ugrads, counts, cfg,
                           u_dev)
    got_w, got_s = case.weights.to(DEV), case.state.to(DEV)
    call(opt_id, got_w, got_s, sl, index, gd, cfg, u_dev)
    assert torch.equal(got_w, want_w) and torch.equal(got_s, want_s), \
        fref.table_violations(case.weights, case.state, got_w.cpu(),
                              got_s.cpu(), want_w.cpu(), want_s.cpu(),
                              slots, u)
    bad = fref.table_violations(case.weights, case.state, got_w.cpu(),
                                got_s.cpu(), want_w.cpu(), want_s.cpu(),
                                slots, u)
    assert bad == [], bad
    # the step is visible: some live row moved
    live = slots[:u][slots[:u] >= 0]
    if live.numel() and variant != "default_lr0":
        assert not ref.bits_equal(want_w.cpu()[live], case.weights[live])
    return u


def _ext_call(opt_id, w, s, slots, index, grads, cfg, u_dev):
    _ext().reduce_apply_by_index(opt_id, w, s, slots, *index, grads, cfg,
                                 u_dev)


def _int_grads(n, dim, g):
    # |sum| <= 8 * 20001 < 2^24: every partial sum is exact in float32
    return torch.randint(-8, 9, (n, dim), generator=g).float()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("category", CATEGORIES)
def test_every_optimizer_on_every_rung(category, dim):
    """All nine categories on the four (G, CF) rungs and their edges, both
    roles in one batch, slot -1 rows and rows named only beyond u_dev."""
    variant = ref.CATEGORY_VARIANT[category]
    g = torch.Generator().manual_seed(17 * CATEGORIES.index(category) + dim)
    flat = _key_set("shapes", g)
    u = _run(variant, dim, flat, _int_grads(flat.numel(), dim, g), _ext_call)
    # T, T + 1, arange (covers randint); every reserved -1 is its own uid
    assert u == 1 + 1 + 150 + 5


@pytest.mark.parametrize("variant", ["default_lr0", "ftrl_sqrt",
                                     "rmsprop_mom0", "sgd_mom09"])
def test_other_variants(variant):
    g = torch.Generator().manual_seed(3)
    flat = _key_set("shapes", g)
    _run(variant, 10, flat, _int_grads(flat.numel(), 10, g), _ext_call)


@pytest.mark.parametrize("dim", [10, 65])
@pytest.mark.parametrize("category", ["adagrad", "adam", "test"])
@pytest.mark.parametrize("kind", ["one_list_20001", "three_keys",
                                  "all_distinct"])
def test_list_shapes(kind, category, dim):
    g = torch.Generator().manual_seed(len(kind) + dim)
    flat = _key_set(kind, g)
    _run(ref.CATEGORY_VARIANT[category], dim, flat,
         _int_grads(flat.numel(), dim, g), _ext_call)


@pytest.mark.parametrize("dim", [9, 65])
@pytest.mark.parametrize("category", CATEGORIES)
def test_random_gradients_on_lists_of_at_most_two(category, dim):
    g = torch.Generator().manual_seed(23 * CATEGORIES.index(category) + dim)
    flat = _key_set("pairs", g)
    grads = torch.randn(flat.numel(), dim, generator=g)
    _run(ref.CATEGORY_VARIANT[category], dim, flat, grads, _ext_call)


def test_single_element_and_empty_long_list():
    """A batch with no long uid (n_long = 0) and a single element."""
    g = torch.Generator().manual_seed(9)
    flat = torch.tensor([77], dtype=torch.int64)
    _run("adagrad", 9, flat, _int_grads(1, 9, g), _ext_call)


# ------------------------------------------------------------------ dispatch

def test_dim_above_ladder_takes_the_two_launches():
    dim = _ext().seg_reduce_max_dim() + 1
    g = torch.Generator().manual_seed(5)
    flat = _key_set("all_distinct", g)
    grads = _int_grads(flat.numel(), dim, g)
    assert not ops.seg_reduce_covers(grads.to(DEV))
    u, index, u_dev = _index(flat)
    case = ref.OptCase("adagrad", dim, flat.numel())
    slots = case.step(0)[0]
    opt_id, cfg = _OPT_IDS["adagrad"], _opt_cfg_vector(case.opt)
    w, s = case.weights.to(DEV), case.state.to(DEV)
    with pytest.raises(RuntimeError):     # the extension has no such rung
        _ext_call(opt_id, w, s, slots.to(DEV), index, grads.to(DEV), cfg,
                  u_dev)
    assert ref.bits_equal(w.cpu(), case.weights)
    # the dispatch serves it with the two launches
    want_w, want_s = case.weights.to(DEV), case.state.to(DEV)
    ugrads, counts = ops.reduce_by_index(index, grads.to(DEV), u_dev)
    _ext().apply_optimizer(opt_id, want_w, want_s, slots.to(DEV), ugrads,
                           counts, cfg, u_dev)
    ops.reduce_apply_by_index(opt_id, w, s, slots.to(DEV), index,
                              grads.to(DEV), cfg, u_dev)
    assert torch.equal(w, want_w) and torch.equal(s, want_s)
    assert not ref.bits_equal(w.cpu(), case.weights)
    with pytest.raises(NotImplementedError):      # CPU tensors
        ops.reduce_apply_by_index(opt_id, case.weights, case.state, slots,
                                  tuple(t.cpu() for t in index), grads, cfg,
                                  u)


# ------------------------------------------------------------------- routing

def _make(dim, dtype=torch.float32, category="default", vocab=sref.SEQ_VOCAB,
          **hyper):
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    sref.seq_reset()
    get_context(DEV)
    emb = embed.Embedding(vocab, dim, dtype=dtype)
    emb.variable.set_optimizer(category, **(hyper or
                                            dict(learning_rate=0.5)))
    return emb


def _pending(emb):
    return list(getattr(emb.variable.sharded.shard, "_pending_bounded", []))


def test_push_queues_the_unreduced_block():
    emb = _make(9)
    var = emb.variable.sharded
    keys = torch.randint(0, sref.SEQ_VOCAB, (64, 3), device=DEV)
    _, h = var.pull(keys)
    assert h.bounded and h.index is not None and h.inverse is not None
    grad = torch.ones(64, 3, 9, device=DEV)
    var.push(h, grad)
    (block,) = _pending(emb)
    assert len(block) == 6 and block[4] is None
    assert block[3].data_ptr() == grad.data_ptr()     # held by reference
    var.update_weights()
    assert _pending(emb) == []
    # a gradient that is not contiguous is never queued by reference: it
    # takes the reduce at push time, which refuses it as it always did
    _, h = var.pull(keys)
    with pytest.raises(RuntimeError, match="contiguous"):
        var.push(h, torch.ones(64, 3, 18, device=DEV)[:, :, ::2])
    assert _pending(emb) == []
    sref.seq_reset()


def test_dim_129_and_float64_keep_the_old_route():
    emb = _make(129)
    var = emb.variable.sharded
    keys = torch.randint(0, sref.SEQ_VOCAB, (64, 3), device=DEV)
    _, h = var.pull(keys)
    var.push(h, torch.ones(64, 3, 129, device=DEV))
    (block,) = _pending(emb)
    assert len(block) == 5                   # reduced at push time
    var.update_weights()
    rows = emb.variable.sparse_read(keys[:1, 0].contiguous())
    assert bool(torch.isfinite(rows).all())

    emb = _make(9, dtype=torch.float64)
    var = emb.variable.sharded
    col = keys[:, 0].contiguous()
    before = emb.variable.sparse_read(col).clone()
    _, h = var.pull(keys)
    var.push(h, torch.ones(64, 3, 9, device=DEV, dtype=torch.float64))
    assert all(len(b) == 5 for b in _pending(emb))
    var.update_weights()
    after = emb.variable.sparse_read(col)
    assert after.dtype == torch.float64 and not torch.equal(before, after)
    sref.seq_reset()


def _two_block_table(monkeypatch, fused):
    monkeypatch.setattr(sharded, "_FUSED_APPLY", fused)
    g = torch.Generator().manual_seed(77)
    emb = _make(9, category="adagrad", learning_rate=0.1,
                initial_accumulator_value=0.3, epsilon=1e-2)
    var = emb.variable.sharded
    ka = torch.randint(0, 100, (64, 3), generator=g).to(DEV)
    kb = torch.randint(50, 150, (64, 3), generator=g).to(DEV)
    kb[:40] = 60                              # a long list in block two
    ga = torch.randint(-8, 9, (64, 3, 9), generator=g).float().to(DEV)
    gb = torch.randint(-8, 9, (64, 3, 9), generator=g).float().to(DEV)
    for _ in range(2):
        _, ha = var.pull(ka)
        _, hb = var.pull(kb)
        var.push(ha, ga)
        var.push(hb, gb)
        blocks = _pending(emb)
        assert [len(b) for b in blocks] == ([6, 6] if fused else [5, 5])
        var.update_weights()
    table = emb.variable.sparse_read(torch.arange(150, device=DEV)).cpu()
    sref.seq_reset()
    return table


def test_two_pending_blocks_give_what_they_give_today(monkeypatch):
    """Two pulls committed together: each indexed block is reduced first,
    then merged into ONE optimizer step per key, exactly as when the blocks
    were reduced at push time (integer gradients: the sums are exact)."""
    new = _two_block_table(monkeypatch, True)
    old = _two_block_table(monkeypatch, False)
    assert torch.equal(new, old)
    assert float((new - 0.0).abs().max()) > 0


def test_delta_tracking_marks_the_applied_rows():
    emb = _make(9)
    var = emb.variable.sharded
    shard = var.shard
    shard.track_changes(True)
    shard.set_epoch(1, reset=True)
    keys = torch.tensor([[3, 5, 3], [7, 5, 499]], device=DEV)
    _, h = var.pull(keys)
    var.update_weights()
    shard.set_epoch(2)
    _, h = var.pull(keys)
    var.push(h, torch.ones(2, 3, 9, device=DEV))
    assert len(_pending(emb)[0]) == 6
    var.update_weights()
    stamped = (shard.row_epoch == 2).nonzero().reshape(-1).cpu().tolist()
    assert stamped == [3, 5, 7, 499]
    sref.seq_reset()


# ------------------------------------------------------------------ capture

def _captured_table(hash_mode):
    """The sequence of segreduce_ref with the step captured once (after the
    warm-up steps on batch 0) and replayed on the two fresh batches."""
    bs, grad = sref.seq_batches(hash_mode)
    emb = sref.seq_make(DEV, hash_mode)
    grad = grad.to(DEV)
    static = bs[0].to(DEV).clone()
    for _ in range(sref.SEQ_WARM // 2):
        sref.seq_step(emb, static, grad)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(sref.SEQ_WARM - sref.SEQ_WARM // 2):
            sref.seq_step(emb, static, grad)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h = sref.seq_step(emb, static, grad)
    assert h.index is not None
    for b in bs[1:]:                   # capture records without executing
        static.copy_(b)
        graph.replay()
    torch.cuda.synchronize()
    keys = sref.seq_keys(hash_mode).to(DEV)
    return emb.variable.sparse_read(keys).cpu()


@pytest.mark.parametrize("hash_mode", [False, True])
def test_capture_replay_matches_eager(hash_mode, monkeypatch):
    """One captured pull -> push -> update_weights (64 x 3 keys, dim 9) on
    the fused routes, replayed on two fresh batches (the second with a key
    hot enough for the long role), against eager on the unfused launches,
    under the bound tests/test_gpu_segreduce.py uses for trained rows."""
    assert sharded._FUSED_APPLY is True and sharded._FUSED_PULL is True
    bs, _ = sref.seq_batches(hash_mode)
    assert int(torch.bincount(
        torch.unique(bs[2], return_inverse=True)[1].reshape(-1)).max()) > _T()
    got = _captured_table(hash_mode)
    monkeypatch.setattr(sharded, "_FUSED_APPLY", False)
    monkeypatch.setattr(sharded, "_FUSED_PULL", False)
    want, h = sref.seq_eager_table(DEV, hash_mode)
    sref.seq_reset()
    tol = sref.seq_tolerance(hash_mode)
    err = (got.double() - want.double()).abs()
    assert float(want.abs().max()) > 0.5     # the steps are visible
    assert bool((err <= tol).all()), float((err - tol).max())


def test_switch_off_in_child_process(tmp_path):
    """OEAMD_FUSED_PULL=0 and OEAMD_FUSED_APPLY=0 (read once at import,
    hence a fresh process) keep the eight launches; the trained tables agree
    within the bound."""
    out = tmp_path / "tables.pt"
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [%r, %r]; import fused_apply_ref as "
            "f; f.seq_child_main(%r)" % (root, tests_dir, str(out)))
    env = dict(os.environ, OEAMD_FUSED_APPLY="0", OEAMD_FUSED_PULL="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True,
                   timeout=300)
    old = torch.load(out)
    for hash_mode in (False, True):
        want, h = sref.seq_eager_table(DEV, hash_mode)
        assert h.index is not None
        sref.seq_reset()
        err = (old[hash_mode].double() - want.double()).abs()
        assert bool((err <= sref.seq_tolerance(hash_mode)).all())
