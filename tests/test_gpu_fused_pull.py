"""The fused flat bounded pull of ops/csrc/embops.hip (all @gpu): the array
touch inside k_unique_assign and k_pull_merged (inverse + index filing +
gather / lazy init), through ``HipVariableShard.pull_bounded_fused``.

The reference is the unfused path, ``unique_bounded_indexed`` then
``pull_bounded`` (k_unique_inverse, k_array_touch, k_gather_init), run from
the same snapshot of the table. uids are not reproducible from run to run,
so everything is compared through keys: ``out`` must be torch.equal (rows
are copies or the deterministic init), uk[inverse] == keys, the index has
the properties of tests/segreduce_ref.py, slots[inverse] == key // shard_num
with the guards, and the table, the state and the valid bitmap after the
call are those of the unfused pull, with every row outside the batch and
every row that was live bit for bit what it was. The checkers are
tests/fused_pull_ref.py, tested without a GPU in
tests/test_fused_pull_checkers.py.
"""

import pytest
import torch

import fused_pull_ref as pref
import segreduce_ref as sref
import sparse_core_ref as ref
from openembedding_amd.core import rng
from openembedding_amd.core.variable import VariableMeta
from openembedding_amd.core.variable_gpu import HipVariableShard

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VOCAB = 30011
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 20001]
DIMS = [1, 9, 10, 16, 17, 33, 65, 129]
KEY_SETS = ["one_hot", "all_distinct", "three_keys", "reserved_mix"]
# state widths that are no multiple of G: adam 2 * dim + 2, test 2
OPTS = [ref.VARIANTS[v] for v in ("adagrad", "adam", "test", "default")]


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _T():
    return _ext().seg_reduce_threshold()


LDS_VOCAB = 400_000     # 220 keys of one LDS bucket need about 225k


def _shard(dim, opt=0, shard_num=1, hash_mode=False, vocab=VOCAB):
    meta = VariableMeta(variable_id=1, embedding_dim=dim,
                        **({} if hash_mode else
                           dict(vocabulary_size=vocab * shard_num)))
    s = HipVariableShard(meta, 0, shard_num, device=DEV, seed=3)
    s.set_initializer("uniform", minval=-0.5, maxval=0.5)
    s.set_optimizer(OPTS[opt][0], **OPTS[opt][1])
    return s


def _key_set(kind, n, g, hi=VOCAB):
    if kind == "one_hot":
        return torch.full((n,), 42, dtype=torch.int64)
    if kind == "all_distinct":
        return torch.randperm(hi, generator=g)[:n].to(torch.int64)
    if kind == "three_keys":
        pick = torch.randint(0, 3, (n,), generator=g)
        return torch.tensor([3, 7, hi - 1], dtype=torch.int64)[pick]
    if kind == "reserved_mix":
        keys = torch.randint(0, max(2, n // 3), (n,), generator=g,
                             dtype=torch.int64)
        keys[torch.rand(n, generator=g) < 0.2] = -1
        keys[n // 2] = -1
        return keys
    if kind == "neg_and_out_of_range":
        keys = torch.randint(0, 200, (n,), generator=g, dtype=torch.int64)
        odd = torch.tensor([-5, -(1 << 40), hi, hi + 7, 1 << 40, -1, hi - 1,
                            0], dtype=torch.int64)
        where = torch.rand(n, generator=g) < 0.3
        keys[where] = odd[torch.randint(0, 8, (int(where.sum()),),
                                        generator=g)]
        return keys
    if kind == "threshold_lengths":
        T = _T()
        parts = [torch.full((T - 1,), 1001), torch.full((T,), 1002),
                 torch.full((T + 1,), 1003), torch.arange(300)]
        keys = torch.cat(parts).to(torch.int64)
        return keys[torch.randperm(keys.numel(), generator=g)]
    assert kind == "lds_overflow"
    # the construction of tests/test_gpu_segreduce.py with keys that are
    # valid table rows: > 64 distinct keys of one block in one LDS bucket
    coll = ref.colliding_keys(1023, [5], 220, limit=LDS_VOCAB)
    assert bool(((rng.splitmix64(coll) & 1023) == 5).all())
    hot = torch.cat([coll, coll[torch.randint(0, 220, (36,), generator=g)]])
    hot = hot[torch.randperm(256, generator=g)]

    def ordinary(m):
        blk = torch.randint(0, 1000, (m,), generator=g, dtype=torch.int64)
        blk[::5] = coll[torch.randint(0, 220, (len(blk[::5]),),
                                      generator=g)]
        return blk
    return torch.cat([ordinary(256), hot, ordinary(256), ordinary(17)])


class _Snap:
    """The shard's table tensors, to run two pulls from one state."""

    NAMES_ARRAY = ["weights", "state", "valid_u8"]
    NAMES_HASH = ["weights", "state", "tk", "tv", "nrows_dev", "slot_keys"]

    def __init__(self, shard):
        self.names = (self.NAMES_HASH if shard.meta.use_hash_table
                      else self.NAMES_ARRAY)
        self.t = {k: getattr(shard, k).clone() for k in self.names}
        self.upper = getattr(shard, "_nrows_upper", 0)

    def restore(self, shard):
        for k in self.names:
            assert getattr(shard, k).shape == self.t[k].shape, k
            getattr(shard, k).copy_(self.t[k])
        if shard.meta.use_hash_table:
            shard._nrows_upper = self.upper


def _prepare(shard, flat_eff, g):
    """Mixed new and existing rows: every third distinct key is pulled
    beforehand, then every row and state entry of the slab is moved off its
    init value, so a row that is wrongly re-initialised or a canary that is
    written shows."""
    uniq = torch.unique(flat_eff)
    pre = uniq[::3]
    if shard.meta.use_hash_table:
        pre = pre[pre != -1]
        shard.reserve_rows(4 * flat_eff.numel() + 4096)
    if pre.numel():
        uk, inv, u_dev = _ext().unique_bounded(pre.to(DEV))
        shard.pull_bounded(uk, u_dev, inv)
    shard.weights.add_(torch.rand(shard.weights.shape, generator=g).to(DEV)
                       + 1.0)
    shard.state.add_(0.25)


def _unfused(shard, flat, foff):
    r = _ext().unique_bounded_indexed(flat, foff)
    uk, inv, u_dev, index = r[0], r[1], r[2], tuple(r[3:])
    out, slots = shard.pull_bounded(uk, u_dev, inv)
    return out, uk, inv, u_dev, index, slots


def _table(shard):
    if shard.meta.use_hash_table:
        return shard.weights.cpu(), shard.state.cpu(), None
    return shard.weights.cpu(), shard.state.cpu(), shard.valid_u8.cpu()


def _check(shard, raw, foff=None, seed=0):
    """Both pulls of ``raw`` (+ field offsets) from one snapshot."""
    g = torch.Generator().manual_seed(seed)
    n = raw.numel()
    flat_eff = raw if foff is None else \
        (raw.reshape(-1, foff.numel()) + foff).reshape(-1)
    hash_mode = shard.meta.use_hash_table
    _prepare(shard, flat_eff, g)
    snap = _Snap(shard)
    before = _table(shard)
    rd, fd = raw.to(DEV), None if foff is None else foff.to(DEV)

    want_out, *_ = _unfused(shard, rd, fd)
    want = _table(shard)
    want_nrows = int(shard.nrows_dev.item()) if hash_mode else 0
    snap.restore(shard)
    out, uk, inv, u_dev, index, slots = shard.pull_bounded_fused(rd, fd)
    after = _table(shard)
    u = int(u_dev.item())
    out_c, inv_c, slots_c = out.cpu(), inv.cpu(), slots.cpu()

    assert out.shape == (n, shard.dim)
    assert torch.equal(out_c, want_out.cpu())
    assert pref.duplicate_violations(flat_eff, out_c) == []
    bad = ref.dedup_violations(flat_eff, uk.cpu(), inv_c, u)
    assert bad == [], bad
    bad = sref.index_violations(inv_c, u, *[t.cpu() for t in index], _T())
    assert bad == [], bad
    es = slots_c[inv_c]                      # slot of every element
    live = es >= 0
    w1, s1, v1 = after
    if hash_mode:
        # slots are handed out by a bump counter: compare through keys
        assert int(shard.nrows_dev.item()) == want_nrows
        assert bool((es[flat_eff == -1] == -1).all())
        assert bool(live[flat_eff != -1].all())
        assert torch.equal(w1[es[live]], out_c[live])
        old = before[0].shape[0]
        n0 = int(snap.t["nrows_dev"].item())
        assert ref.bits_equal(w1[:n0], before[0][:n0])
        assert ref.bits_equal(s1[:n0], before[1][:n0])
        assert ref.bits_equal(w1[want_nrows:old], before[0][want_nrows:old])
        assert ref.bits_equal(s1[want_nrows:old], before[1][want_nrows:old])
        new_rows = es[live & (es >= n0)]
        if new_rows.numel() and shard.state_dim:
            sir = shard._state_init_row.cpu().reshape(-1)
            assert torch.equal(s1[new_rows],
                               sir.expand(new_rows.numel(), -1))
    else:
        cap = shard.valid_u8.numel()
        assert torch.equal(es, pref.expected_slots(flat_eff, shard.shard_num,
                                                   cap))
        assert bool((slots_c[u:] == -1).all())
        bad = pref.table_violations(before, after, want, es[live])
        assert bad == [], bad
        assert torch.equal(w1, want[0]) and torch.equal(s1, want[1])
        assert torch.equal(v1, want[2])
    assert bool((out_c[~live] == 0).all())
    if bool(live.any()):
        assert torch.equal(w1[es[live]], out_c[live])

    # a second call on the same keys: nothing is new, nothing is written
    out2, *_ = shard.pull_bounded_fused(rd, fd)
    again = _table(shard)
    assert torch.equal(out2.cpu(), out_c)
    assert ref.bits_equal(again[0], w1) and ref.bits_equal(again[1], s1)
    if not hash_mode:
        assert torch.equal(again[2], v1)

    # want_out=False from the snapshot: same table, no output
    snap.restore(shard)
    out3, *_ = shard.pull_bounded_fused(rd, fd, want_out=False)
    assert out3.numel() == 0
    quiet = _table(shard)
    if hash_mode:
        assert int(shard.nrows_dev.item()) == want_nrows
    else:
        assert ref.bits_equal(quiet[0], w1) and ref.bits_equal(quiet[1], s1)
        assert torch.equal(quiet[2], v1)
    return u


# --------------------------------------------------------------- array table

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KEY_SETS)
def test_sizes_and_key_sets(kind, n):
    """Sizes around the per-thread factors, the wave and the block of the
    assign and merged kernels, at the flagship's dim 9."""
    g = torch.Generator().manual_seed(100 * KEY_SETS.index(kind) + n)
    shard = _shard(9, opt=SIZES.index(n) % len(OPTS))
    u = _check(shard, _key_set(kind, n, g), seed=n)
    if kind == "one_hot":
        assert u == 1
    if kind == "all_distinct":
        assert u == n


@pytest.mark.parametrize("dim", DIMS)
def test_dims_and_state_widths(dim):
    """G = 16 up to dim 32, a wave above, beyond one pass of the wave at
    129; the optimizer rotates so that the state width is dim, 2 dim + 2, 2
    and 0."""
    g = torch.Generator().manual_seed(dim)
    shard = _shard(dim, opt=DIMS.index(dim) % len(OPTS))
    _check(shard, _key_set("reserved_mix", 1025, g), seed=dim)


@pytest.mark.parametrize("kind,dim", [("neg_and_out_of_range", 10),
                                      ("neg_and_out_of_range", 65),
                                      ("threshold_lengths", 10),
                                      ("threshold_lengths", 65),
                                      ("lds_overflow", 10)])
def test_special_constructions(kind, dim):
    g = torch.Generator().manual_seed(7 + dim)
    n = 785 if kind == "neg_and_out_of_range" else 0
    shard = _shard(dim, opt=1, vocab=LDS_VOCAB if kind == "lds_overflow"
                   else VOCAB)
    _check(shard, _key_set(kind, n, g), seed=dim)


@pytest.mark.parametrize("dim", [9, 33])
def test_fused_field_offsets_26_fields(dim):
    g = torch.Generator().manual_seed(26 + dim)
    F, B = 26, 37
    raw = torch.randint(0, 50, (B, F), generator=g, dtype=torch.int64)
    foff = torch.arange(F, dtype=torch.int64) * 40 - 17   # fields overlap
    raw[2, F - 1] = -1 - foff[F - 1]                      # the reserved key
    shard = _shard(dim, opt=0)
    _check(shard, raw.reshape(-1), foff, seed=dim)


@pytest.mark.parametrize("kind", ["reserved_mix", "neg_and_out_of_range",
                                  "all_distinct"])
def test_shard_num_3(kind):
    """Keys of shard 0 of 3 (multiples of 3; -1 and the out-of-range ones
    stay what they are): slot = key / 3."""
    g = torch.Generator().manual_seed(33)
    keys = _key_set(kind, 1025, g)
    ok = (keys >= 0) & (keys < VOCAB)
    keys = torch.where(ok, keys * 3, keys)
    shard = _shard(9, opt=1, shard_num=3)
    assert shard.valid_u8.numel() == VOCAB
    _check(shard, keys, seed=3)


# ---------------------------------------------------------------- hash table

def _hash_keys(kind, n, g):
    keys = _key_set(kind, n, g, hi=1 << 20)
    big = keys >= 0
    return torch.where(big, keys * 1048573 + 11, keys)    # spread, -1 kept


@pytest.mark.parametrize("n", [1, 65, 257, 1025, 20001])
@pytest.mark.parametrize("kind", KEY_SETS)
def test_hash_table_through_the_slots_policy(kind, n):
    g = torch.Generator().manual_seed(500 + 10 * KEY_SETS.index(kind) + n)
    shard = _shard(9, opt=n % len(OPTS), hash_mode=True)
    _check(shard, _hash_keys(kind, n, g), seed=n)


@pytest.mark.parametrize("dim", [1, 17, 65, 129])
def test_hash_table_dims(dim):
    g = torch.Generator().manual_seed(600 + dim)
    shard = _shard(dim, opt=1, hash_mode=True)
    _check(shard, _hash_keys("reserved_mix", 1025, g), seed=dim)


# ------------------------------------------------------------------- routing

def test_flat_bounded_pull_takes_the_fused_route(monkeypatch):
    """ShardedVariable.pull fills the handle as before (inverse, index,
    slots, unique) whichever route ran, and OEAMD_FUSED_PULL's flag picks
    the route."""
    from openembedding_amd.parallel import sharded
    calls = []
    real = HipVariableShard.pull_bounded_fused

    def spy(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(HipVariableShard, "pull_bounded_fused", spy)
    keys = torch.randint(0, sref.SEQ_VOCAB, (64, 3))
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(sharded, "_FUSED_PULL", flag)
        emb = sref.seq_make(DEV, False)
        var = emb.variable.sharded
        var.shard.set_initializer("uniform", minval=-0.5, maxval=0.5)
        out, h = var.pull(keys.to(DEV))
        assert len(calls) == 1
        assert h.bounded and h.index is not None and h.slots is not None
        u = int(h.u_dev.item())
        assert ref.dedup_violations(keys.reshape(-1), h.unique.cpu(),
                                    h.inverse.cpu(), u) == []
        assert torch.equal(h.slots.cpu()[h.inverse.cpu()], keys.reshape(-1))
        outs.append(out.cpu())
        sref.seq_reset()
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
