"""The sparse-engine kernels of ops/csrc/embops.hip, called directly through
the extension's entry points on small hand-built tables (all @gpu).

Covered: the nine fused sparse optimizers (k_apply_opt<G,OPT>), the batch
dedup (k_unique_insert/_assign/_inverse), the persistent hash table
(k_ht_lookup/k_ht_rehash), the array table (k_array_touch) and gather +
lazy init (k_gather_init<16|64>). The reference side (float64 stepper,
tolerance rule, dedup property checker, colliding-key search) is
tests/sparse_core_ref.py and is itself tested without a GPU in
tests/test_sparse_core_checkers.py.

Guards are tested so that a broken guard fails an assertion instead of
reaching memory it must not: tables are views into larger canary-filled
buffers (a slot of -1 taken at face value lands in the front canary),
length-limited tensors are narrow() views, and every index handed to a
kernel is in range.

Tolerance. No number is fixed in advance: for every output tensor
e32 = max|fp32 oracle - fp64 oracle| measures the reference's own rounding,
ek = max|kernel - fp64 oracle|, and the test asserts
ek <= margin * e32 + one fp32 ulp at the tensor's largest magnitude. The
margin covers the device's sqrtf / division / powf / logf / cosf rounding
differently from the CPU's; it is the next power of two above the worst
ratio (ek - ulp) / e32 measured on an MI355X, and never above 8.

Measured worst ratios (MI355X, all dims/row counts/steps of this module;
"0" = the kernel is within one ulp of the float64 oracle everywhere):

    kernel / tensors                      worst ratio   margin
    default (incl. lr = 0)                0             1
    adadelta                              1.000         2
    adagrad                               0             1
    adam                                  3.764         4
    adamax                                0.615         1
    ftrl (power -0.4: 1.006, -0.5: 0.645) 1.006         2
    rmsprop (momentum 0: 0.985, 0.3: 1.24) 1.240        2
    sgd (plain 0, momentum 0.091,
         Nesterov 0.100)                  0.100         1
    test                                  0             1
    engine loop, 3 steps (worst: adam v)  5.372         8
    truncated-normal init                 0.740         1

A margin is never set below 1 (= as close to float64 as the float32 oracle,
plus one ulp). adam's figure is its v block: the kernel evaluates
1.0f - beta_2 in float32 (0.100000024 for 0.9) where the oracle rounds the
double 1 - 0.9 (0.1000000015); replaying that one difference on the CPU
reproduces the measured ek to all printed digits. Everything else is
division / sqrtf / powf rounding.

Out of scope: the dedup's GLOBAL-table overflow path (an element that finds
the scratch table full becomes its own unique) cannot be reached through
the bindings, which size the table as next_pow2(2n) for n elements.
"""

import pytest
import torch

import sparse_core_ref as ref
from openembedding_amd.core import rng
from openembedding_amd.core.initializers import make_initializer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# margin per optimizer category / initializer: next power of two above the
# measured worst ratio (module docstring), never above ref.MAX_MARGIN
MARGIN = {"default": 1.0, "adadelta": 2.0, "adagrad": 1.0, "adam": 4.0,
          "adamax": 1.0, "ftrl": 2.0, "rmsprop": 2.0, "sgd": 1.0,
          "test": 1.0, "engine": 8.0, "normal_init": 1.0}
assert max(MARGIN.values()) <= ref.MAX_MARGIN

CANARY = 777.25


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _ids():
    from openembedding_amd.core import variable_gpu as vg
    return vg._OPT_IDS, vg._opt_cfg_vector, vg._init_params


class Guarded:
    """A device tensor that is a narrow() view into a larger buffer whose
    front and back rows hold a canary value."""

    def __init__(self, t, front=2, back=2, fill=CANARY):
        n = t.shape[0]
        big = torch.full((front + n + back,) + tuple(t.shape[1:]), fill,
                         dtype=t.dtype)
        big[front:front + n] = t
        self.fill, self.front, self.n = fill, front, n
        self.big = big.to(DEV)
        self.view = self.big.narrow(0, front, n)
        assert self.view.is_contiguous()

    def cpu(self):
        return self.view.cpu()

    def guards_intact(self):
        b = self.big.cpu()
        return bool((b[:self.front] == self.fill).all()
                    and (b[self.front + self.n:] == self.fill).all())


def _dev_count(k):
    return torch.tensor([k], dtype=torch.int32, device=DEV)


# =================================================== A. fused optimizers

def _run_opt_case(case, margin, steps, live=None):
    ext = _ext()
    opt_ids, cfg_vector, _ = _ids()
    W, S = Guarded(case.weights), Guarded(case.state)
    u_dev = None if live is None else _dev_count(live)
    fails = []
    for t in range(steps):
        slots, grads, counts = case.step(t)
        # the kernel's own current fp32 table: errors do not compound
        w0, s0 = W.cpu(), S.cpu()
        ext.apply_optimizer(opt_ids[case.category], W.view, S.view,
                            slots.to(DEV), grads.to(DEV), counts.to(DEV),
                            cfg_vector(case.opt), u_dev)
        w1, s1 = W.cpu(), S.cpu()
        report = []
        found = ref.check_step(case, w0, s0, w1, s1, slots, grads, counts,
                               margin, live=live, report=report)
        for name, ek, e32, ulp, ratio in report:
            print(f"RATIO kind={case.category} variant={case.variant} "
                  f"dim={case.dim} n={case.n} step={t} tensor={name} "
                  f"ek={ek:.4g} e32={e32:.4g} ulp={ulp:.4g} "
                  f"ratio={ratio:.4g}")
        fails += [f"step {t}: {f}" for f in found]
    assert W.guards_intact(), "weights written outside the table"
    assert S.guards_intact(), "state written outside the table"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dim", ref.DIMS)
@pytest.mark.parametrize("variant", list(ref.VARIANTS))
def test_apply_optimizer_single_steps(variant, dim):
    """Three steps over different overlapping row subsets, each judged
    against a float64 step from the kernel's own snapshot: weights AND
    every state column within the reference-derived tolerance; rows that
    no slot names (canaries, rows behind a -1 slot) bit-unchanged."""
    case = ref.OptCase(variant, dim, ref.case_n(variant, dim))
    _run_opt_case(case, MARGIN[case.category], case.STEPS)


@pytest.mark.parametrize("dim", [16, 33])
@pytest.mark.parametrize("category", list(ref.CATEGORY_VARIANT))
def test_apply_optimizer_device_count_guard(category, dim):
    """u_dev = k < n, both lane-group widths: positions >= k are not
    applied (rows named only there stay bit-identical), positions < k
    are."""
    case = ref.OptCase(ref.CATEGORY_VARIANT[category], dim, 17, seed=1)
    _run_opt_case(case, MARGIN[category], 2, live=9)


def _shards(category, hyper, mode, dim):
    from openembedding_amd.core import VariableMeta, VariableShard
    from openembedding_amd.core.variable_gpu import HipVariableShard
    vocab = 400 if mode == "array" else (1 << 63)
    out = []
    for dtype, cls, dev in ((torch.float64, VariableShard, "cpu"),
                            (torch.float32, VariableShard, "cpu"),
                            (torch.float32, HipVariableShard, DEV)):
        meta = VariableMeta(variable_id=1, embedding_dim=dim, dtype=dtype,
                            vocabulary_size=vocab)
        s = cls(meta, 0, 1, device=dev, seed=3)
        s.set_initializer("uniform", minval=-0.5, maxval=0.5)
        s.set_optimizer(category, **hyper)
        out.append(s)
    return out


def _export_sorted(shard):
    keys, w, s = shard.export_rows()
    order = torch.argsort(keys.cpu())
    s = s.cpu()[order] if s is not None else torch.zeros(keys.numel(), 0)
    return keys.cpu()[order], w.cpu()[order], s


@pytest.mark.parametrize("dim", [9, 33])
@pytest.mark.parametrize("mode", ["array", "hash"])
@pytest.mark.parametrize("category", list(ref.CATEGORY_VARIANT))
def test_engine_weights_and_state(category, mode, dim):
    """The full pull/push/update loop like test_gpu_numerics'
    test_optimizer_parity_engine, but with hyper-parameters that all show,
    and comparing weights AND state of the exported rows, matched by key,
    with the reference-derived tolerance (float64 CPU shard = oracle,
    float32 CPU shard = its rounding)."""
    _, hyper = ref.VARIANTS[ref.CATEGORY_VARIANT[category]]
    s64, s32, gpu = _shards(category, hyper, mode, dim)
    g = torch.Generator().manual_seed(17)
    for step in range(3):
        keys = torch.randint(0, 400, (96,), generator=g, dtype=torch.int64)
        uk, inv = torch.unique(keys, return_inverse=True)
        grads = torch.randn(96, dim, generator=g)
        ug = torch.zeros(uk.numel(), dim).index_add_(0, inv, grads)
        counts = torch.bincount(inv, minlength=uk.numel())
        for s in (s64, s32):
            s.pull(uk)
            s.push(uk, ug.to(s.dtype), counts)
            s.update_weights()
        gpu.pull(uk.to(DEV))
        gpu.push(uk.to(DEV), ug.to(DEV), counts.to(DEV))
        gpu.update_weights()
    k64, w64, st64 = _export_sorted(s64)
    k32, w32, st32 = _export_sorted(s32)
    kg, wg, stg = _export_sorted(gpu)
    assert torch.equal(k64, k32) and torch.equal(k64, kg)
    init = rng.init_rows("uniform", {"minval": -0.5, "maxval": 0.5},
                         s64.seed, k64, dim, torch.float64)
    assert float((w64 - init).abs().median()) >= 1e-3, "vacuous case"
    fails = []
    tensors = [("w", wg, w32, w64)]
    tensors += [(name, stg[:, a:b], st32[:, a:b], st64[:, a:b])
                for name, a, b, _ in ref.state_blocks(category, dim)]
    for name, got, r32, r64 in tensors:
        ok, (ek, e32, ulp, ratio) = ref.within_reference_error(
            got, r32, r64, MARGIN["engine"])
        print(f"RATIO kind=engine variant={category} mode={mode} dim={dim} "
              f"tensor={name} ek={ek:.4g} e32={e32:.4g} ulp={ulp:.4g} "
              f"ratio={ratio:.4g}")
        if not ok:
            fails.append(f"{name}: ek {ek:.3g} e32 {e32:.3g} ulp {ulp:.3g}")
    assert not fails, "\n".join(fails)


# ======================================================== B. batch dedup

UNIQUE_SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049,
                20001]
KEY_SETS = ["all_equal", "all_distinct", "three_keys", "full_range",
            "reserved_mix"]


def _key_set(kind, n, g):
    if kind == "all_equal":
        return torch.full((n,), 42, dtype=torch.int64)
    if kind == "all_distinct":
        return torch.randperm(n, generator=g) * 2654435761 - 10 ** 12
    if kind == "three_keys":
        pick = torch.randint(0, 3, (n,), generator=g)
        return torch.tensor([3, -7, 1 << 40], dtype=torch.int64)[pick]
    if kind == "full_range":
        base = ref.full_range_keys(max(1, (n + 1) // 2), g)
        keys = base[torch.randint(0, base.numel(), (n,), generator=g)]
        keys[:base.numel()] = base   # the planted extremes occur
        return keys
    assert kind == "reserved_mix"
    keys = torch.randint(0, max(2, n // 3), (n,), generator=g,
                         dtype=torch.int64)
    keys[torch.rand(n, generator=g) < 0.2] = -1
    keys[n // 2] = -1
    return keys


def _check_unique(flat, raw=None, foff=None):
    """Run unique_bounded (and unique_inverse when there are no fused
    offsets) and hold the result against the property checker."""
    ext = _ext()
    src = (flat if raw is None else raw.reshape(-1)).to(DEV)
    uk, inv, cnt = ext.unique_bounded(
        src, None if foff is None else foff.to(DEV))
    assert cnt.dtype == torch.int32 and cnt.numel() == 1
    u = int(cnt.item())
    bad = ref.dedup_violations(flat, uk.cpu(), inv.cpu(), u)
    assert bad == [], bad
    if foff is None:
        uk2, inv2 = ext.unique_inverse(src)
        assert uk2.numel() == u
        bad = ref.dedup_violations(flat, uk2.cpu(), inv2.cpu(), u)
        assert bad == [], bad


@pytest.mark.parametrize("n", UNIQUE_SIZES)
@pytest.mark.parametrize("kind", KEY_SETS)
def test_unique_properties(kind, n):
    """Sizes around every per-thread factor (8 in the assign kernel, 4 in
    the inverse kernel), the wave and the block; key sets from one hot key
    to the full signed range with the reserved key -1."""
    g = torch.Generator().manual_seed(
        100 * KEY_SETS.index(kind) + UNIQUE_SIZES.index(n))
    _check_unique(_key_set(kind, n, g))


def test_unique_lds_overflow_path():
    """More than 64 distinct keys of ONE block hash to the same LDS bucket:
    elements past the 64th colliding key skip the LDS pre-filter and insert
    into the global table without publishing; their in-block duplicates
    and the copies in neighbouring blocks must still share one uid."""
    g = torch.Generator().manual_seed(3)
    coll = ref.colliding_keys(1023, [5], 220)
    assert bool(((rng.splitmix64(coll) & 1023) == 5).all())
    hot = torch.cat([coll, coll[torch.randint(0, 220, (36,), generator=g)]])
    hot = hot[torch.randperm(256, generator=g)]
    assert torch.unique(hot).numel() >= 200

    def ordinary(m):
        blk = torch.randint(0, 1000, (m,), generator=g, dtype=torch.int64)
        blk[::5] = coll[torch.randint(0, 220, (len(blk[::5]),),
                                      generator=g)]
        return blk

    keys = torch.cat([ordinary(256), hot, ordinary(256), ordinary(17)])
    assert keys.numel() == 785 and torch.equal(keys[256:512], hot)
    _check_unique(keys)


@pytest.mark.parametrize("F", [1, 3, 26])
def test_unique_fused_field_offsets(F):
    """unique_bounded(raw.view(-1), field_offsets) dedups raw +
    field_offsets, including an element whose sum is the reserved -1."""
    g = torch.Generator().manual_seed(F)
    B = 37
    raw = torch.randint(0, 50, (B, F), generator=g, dtype=torch.int64)
    foff = torch.arange(F, dtype=torch.int64) * 40 - 17   # fields overlap
    raw[2, F - 1] = -1 - foff[F - 1]
    flat = (raw + foff).reshape(-1)
    assert int((flat == -1).sum()) >= 1
    _check_unique(flat, raw=raw, foff=foff)


# ========================================== C. hash table and array table

TV_FILL = -77
SK_FILL = -(1 << 40)


class HashTable:
    def __init__(self, cap, row_cap, sk_extra=8):
        self.tk = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
        self.tv = torch.full((cap,), TV_FILL, dtype=torch.int32,
                             device=DEV)
        self.nrows = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.sk_buf = torch.full((row_cap + sk_extra,), SK_FILL,
                                 dtype=torch.int64, device=DEV)
        self.slot_keys = self.sk_buf.narrow(0, 0, row_cap)
        self.row_cap = row_cap

    def lookup(self, keys, insert, u_dev=None):
        slots, mask = _ext().ht_lookup(self.tk, self.tv, keys.to(DEV),
                                       self.nrows, self.slot_keys, insert,
                                       u_dev)
        return slots.cpu(), mask.cpu()

    def snapshot(self):
        return (self.tk.cpu(), self.tv.cpu(), self.nrows.cpu(),
                self.sk_buf.cpu())

    def unchanged_since(self, snap):
        return all(torch.equal(a, b) for a, b in zip(snap, self.snapshot()))

    def count(self):
        return int(self.nrows.item())

    def sk_tail_intact(self):
        return bool((self.sk_buf.cpu()[self.row_cap:] == SK_FILL).all())


def _table_keys(cap, n, g):
    """n distinct keys for a cap-entry table: eight whose home slot is one
    of the last three (their probe chain wraps past the table end), four
    more of those kept back as absent keys, the rest over the full signed
    range."""
    coll = ref.colliding_keys(cap - 1, [cap - 3, cap - 2, cap - 1], 12)
    rest = ref.full_range_keys(n - 8, g)
    keys = torch.cat([coll[:4], rest[:(n - 8) // 2], coll[4:8],
                      rest[(n - 8) // 2:]])
    assert torch.unique(keys).numel() == n
    return keys, coll[8:]


@pytest.mark.parametrize("cap", [16, 64, 256])
def test_ht_insert_lookup_rehash(cap):
    g = torch.Generator().manual_seed(cap)
    n = cap * 3 // 4 - 1          # one more row joins below: never > 3/4
    keys, absent = _table_keys(cap, n, g)
    ht = HashTable(cap, row_cap=cap)
    half = n // 2
    # two calls: the second call's colliding keys probe over the first's
    s1, m1 = ht.lookup(keys[:half], True)
    assert ht.count() == half
    s2, m2 = ht.lookup(keys[half:], True)
    slots = torch.cat([s1, s2])
    assert torch.equal(torch.sort(slots)[0], torch.arange(n))
    assert torch.equal(ht.slot_keys.cpu()[slots], keys)
    assert bool((torch.cat([m1, m2]) == 1).all())
    assert ht.count() == n
    assert int((ht.tk.cpu() != -1).sum()) == n
    assert ht.sk_tail_intact()
    # the wrap really happened: a colliding key sits at the table's start
    tk = ht.tk.cpu()
    homes = rng.splitmix64(tk[:8]) & (cap - 1)
    assert bool(((tk[:8] != -1) & (homes >= cap - 3)).any())

    snap = ht.snapshot()
    s_again, m_again = ht.lookup(keys, True)         # second insert call
    assert torch.equal(s_again, slots) and bool((m_again == 0).all())
    s_ro, m_ro = ht.lookup(keys, False)              # read-only, present
    assert torch.equal(s_ro, slots) and bool((m_ro == 0).all())
    miss = torch.cat([absent, torch.tensor([-1, 123456789012345])])
    s_miss, m_miss = ht.lookup(miss, False)          # read-only, absent
    assert bool((s_miss == -1).all()) and bool((m_miss == 0).all())
    assert ht.unchanged_since(snap), "a lookup of known/absent keys wrote"

    # the reserved key -1 is a miss even when inserting, and takes no row
    s3, m3 = ht.lookup(torch.tensor([-1, int(absent[0])]), True)
    assert s3.tolist() == [-1, n] and m3.tolist() == [0, 1]
    assert ht.count() == n + 1
    keys = torch.cat([keys, absent[:1]])
    slots = torch.cat([slots, s3[1:]])

    for factor in (2, 4):
        big = HashTable(cap * factor, row_cap=cap)
        big.sk_buf.copy_(ht.sk_buf)
        big.nrows.copy_(ht.nrows)
        _ext().ht_rehash(ht.tk, ht.tv, big.tk, big.tv)
        assert int((big.tk.cpu() != -1).sum()) == n + 1
        s_big, _ = big.lookup(keys, False)
        assert torch.equal(s_big, slots)
        s_big, _ = big.lookup(torch.cat([absent[1:], torch.tensor([-1])]),
                              False)
        assert bool((s_big == -1).all())


def test_ht_device_count_guard():
    g = torch.Generator().manual_seed(1)
    keys = ref.full_range_keys(20, g)
    ht = HashTable(64, row_cap=32)
    k = 7
    slots, mask = ht.lookup(keys, True, _dev_count(k))
    assert torch.equal(torch.sort(slots[:k])[0], torch.arange(k))
    assert bool((mask[:k] == 1).all())
    assert bool((slots[k:] == -1).all()) and bool((mask[k:] == 0).all())
    assert ht.count() == k
    assert torch.equal(ht.slot_keys.cpu()[slots[:k]], keys[:k])
    assert int((ht.tk.cpu() != -1).sum()) == k
    s_ro, _ = ht.lookup(keys, False)
    assert torch.equal(s_ro, slots)


def test_ht_row_capacity_guard():
    """More new keys than rows: exactly row_cap keys get a row, the rest
    are dropped as misses — now and on every later lookup — and nothing is
    written behind the end of slot_keys."""
    g = torch.Generator().manual_seed(2)
    keys = ref.full_range_keys(20, g)
    cap_rows = 12
    ht = HashTable(64, row_cap=cap_rows, sk_extra=16)
    slots, mask = ht.lookup(keys, True)
    got = slots >= 0
    assert int(got.sum()) == cap_rows
    assert torch.equal(torch.sort(slots[got])[0], torch.arange(cap_rows))
    assert torch.equal(mask != 0, got)
    assert bool((slots[~got] == -1).all())
    assert torch.equal(ht.slot_keys.cpu()[slots[got]], keys[got])
    assert ht.sk_tail_intact()
    assert ht.count() >= cap_rows
    for insert in (False, True):
        s_later, m_later = ht.lookup(keys, insert)
        assert torch.equal(s_later, slots) and bool((m_later == 0).all())
    assert ht.sk_tail_intact()


@pytest.mark.parametrize("shard_num", [1, 3])
def test_array_touch(shard_num):
    cap, shard_id = 40, shard_num - 1
    g = torch.Generator().manual_seed(shard_num)
    pre = torch.zeros(cap, dtype=torch.uint8)
    pre[torch.randperm(cap, generator=g)[:10]] = 1
    # the bitmap sits 8 entries into a zero-filled buffer: a slot the
    # guards should have refused shows up as a 1 outside the view
    V = Guarded(pre, front=8, back=8, fill=0)
    want = torch.randperm(cap, generator=g)[:23]
    good = want * shard_num + shard_id
    bad = torch.tensor([-1, -2, -7, cap * shard_num, cap * shard_num + 1,
                        cap * shard_num + 5])
    keys = torch.cat([good[:12], bad[:3], good[12:], bad[3:]])
    expect = torch.cat([want[:12], torch.full((3,), -1), want[12:],
                        torch.full((3,), -1)])
    ext = _ext()
    slots, mask = (t.cpu() for t in ext.array_touch(
        V.view, keys.to(DEV), shard_num, None))
    assert torch.equal(slots, expect)
    hit = expect >= 0
    assert torch.equal(mask[hit], 1 - pre[expect[hit]])   # first touch
    assert bool((mask[~hit] == 0).all())
    after = pre.clone()
    after[want] = 1
    assert torch.equal(V.cpu(), after) and V.guards_intact()
    slots, mask = (t.cpu() for t in ext.array_touch(
        V.view, keys.to(DEV), shard_num, None))
    assert torch.equal(slots, expect) and bool((mask == 0).all())
    assert torch.equal(V.cpu(), after) and V.guards_intact()

    # device count: positions >= k are misses and leave the bitmap alone
    V = Guarded(pre, front=8, back=8, fill=0)
    k = 9
    slots, mask = (t.cpu() for t in ext.array_touch(
        V.view, keys.to(DEV), shard_num, _dev_count(k)))
    assert torch.equal(slots[:k], expect[:k])
    assert bool((slots[k:] == -1).all()) and bool((mask[k:] == 0).all())
    assert torch.equal(mask[:k], 1 - pre[expect[:k]])
    after = pre.clone()
    after[expect[:k]] = 1
    assert torch.equal(V.cpu(), after) and V.guards_intact()


# ================================================ D. gather + lazy init

SEED = 0x1234ABCD5678
GATHER_DIMS = [1, 9, 16, 17, 32, 33, 64, 65, 130]
GATHER_NS = [1, 3, 4, 5, 67]   # 4 elements per lane group
# ranges where u * (max - min) rounds, and where max - min itself rounds
INITS = [("uniform", {"minval": -0.05, "maxval": 0.05}),
         ("uniform", {"minval": 0.1, "maxval": 0.7}),
         ("constant", {"value": 0.3})]
WIDE_KEYS = [7, -3, (1 << 44) + 5, -(1 << 62), ref.I64_MAX, ref.I64_MIN,
             123456789, (1 << 52) + 1, -(1 << 44) - 9]


class GatherCase:
    """u unique entries with mixed fates (new / existing / slot -1) over a
    canary-guarded table, optionally read through an ``inverse`` with
    duplicates and a hot uid."""

    def __init__(self, dim, n, with_inverse, sd, g):
        self.dim, self.n, self.sd = dim, n, sd
        u = n // 2 + 1 if with_inverse else n
        self.u = u
        self.inverse = None
        if with_inverse:
            inv = torch.randint(0, u, (n,), generator=g, dtype=torch.int64)
            inv[::3] = 0                                   # hot uid
            self.inverse = inv
        R = 2 * u + 4
        self.R = R
        keys = ref.full_range_keys(u, g)
        m = min(u, len(WIDE_KEYS))
        keys[:m] = torch.tensor(WIDE_KEYS[:m], dtype=torch.int64)
        self.keys = keys
        fate = torch.arange(u) % 4          # 0, 2: new; 1: existing; 3: miss
        self.slots = torch.randperm(R, generator=g)[:u].clone()
        self.slots[fate == 3] = -1
        self.new_mask = ((fate == 0) | (fate == 2)).to(torch.uint8)
        self.weights = torch.randn(R, dim, generator=g)
        self.state = torch.randn(R, sd, generator=g)
        self.sir = torch.randn(sd, generator=g)

    def expect(self, init, live=None):
        """(table weights, table state, out, rows of out that are defined)
        after the gather."""
        cat, cfg = init
        u = self.u
        uid = self.inverse if self.inverse is not None else torch.arange(u)
        seen = torch.zeros(u, dtype=torch.bool)
        seen[uid] = True
        defined = torch.ones(uid.numel(), dtype=torch.bool)
        if live is not None and self.inverse is None:
            seen &= torch.arange(u) < live
            defined = torch.arange(u) < live
        new = seen & (self.new_mask != 0) & (self.slots >= 0)
        w, s = self.weights.clone(), self.state.clone()
        if bool(new.any()):
            w[self.slots[new]] = rng.init_rows(cat, cfg, SEED,
                                               self.keys[new], self.dim)
            if self.sd:
                s[self.slots[new]] = self.sir
        sl = self.slots[uid]
        out = torch.where((sl >= 0).unsqueeze(1), w[sl.clamp(min=0)],
                          torch.zeros(1, self.dim))
        return w, s, out, defined

    def run(self, init, want_out=True, live=None):
        _, _, init_params = _ids()
        cat, p0, p1, p2 = init_params(make_initializer(init[0], **init[1]))
        W, S = Guarded(self.weights), Guarded(self.state)
        out = _ext().gather_init(
            W.view, S.view, self.slots.to(DEV), self.new_mask.to(DEV),
            self.keys.to(DEV),
            None if self.inverse is None else self.inverse.to(DEV),
            cat, p0, p1, p2, SEED, self.sir.to(DEV), want_out,
            None if live is None else _dev_count(live))
        assert W.guards_intact() and S.guards_intact()
        return W.cpu(), S.cpu(), out.cpu()

    def check(self, init, want_out=True, live=None):
        w, s, out = self.run(init, want_out, live)
        ew, es, eout, defined = self.expect(init, live)
        tag = f"{init} dim={self.dim} n={self.n} inv={self.inverse is not None}"
        assert ref.bits_equal(w, ew), f"table weights {tag}"
        assert ref.bits_equal(s, es), f"table state {tag}"
        if want_out:
            assert out.shape == eout.shape
            assert ref.bits_equal(out[defined], eout[defined]), f"out {tag}"
        else:
            assert out.numel() == 0


@pytest.mark.parametrize("n", GATHER_NS)
@pytest.mark.parametrize("dim", GATHER_DIMS)
def test_gather_init_bit_exact(dim, n):
    """Uniform and constant init bit-identical to core/rng.init_rows for
    keys across the signed 64-bit range (key * 2^20 wraps) and columns up
    to 129; new rows are initialised, written and returned; existing rows
    are returned and — with every state row — left bit-unchanged; slot -1
    returns zeros; want_out=False writes the table only."""
    g = torch.Generator().manual_seed(1000 * dim + n)
    for with_inverse in (False, True):
        case = GatherCase(dim, n, with_inverse, 2 * dim + 2, g)
        for init in INITS:
            case.check(init)
        case.check(INITS[1], want_out=False)


@pytest.mark.parametrize("sd", [0, 3])
@pytest.mark.parametrize("dim", [9, 65])
def test_gather_init_state_widths(dim, sd):
    g = torch.Generator().manual_seed(10 * dim + sd)
    for with_inverse in (False, True):
        GatherCase(dim, 67, with_inverse, sd, g).check(INITS[1])


@pytest.mark.parametrize("dim", [16, 33])
def test_gather_init_device_count_guard(dim):
    """Without ``inverse`` positions >= u_dev are not initialised and the
    rows they name stay as they were; with ``inverse`` the count is
    documented as not applied (the element list is always fully live)."""
    g = torch.Generator().manual_seed(dim)
    GatherCase(dim, 67, False, 2 * dim + 2, g).check(INITS[1], live=30)
    GatherCase(dim, 67, True, 2 * dim + 2, g).check(INITS[1], live=5)


NORMAL = dict(mean=0.5, stddev=0.2, truncated=0.5)
NORMAL_SEED = 11   # < 1% of elements within 1e-4 of the cut (checked on
                   # the CPU in test_sparse_core_checkers.py)


@pytest.mark.parametrize("dim", [9, 130])
def test_gather_init_truncated_normal(dim):
    """Normal init with a cut low enough that resampling happens (31% of
    first samples), against a float64 evaluation of the same Box-Muller
    chain. Elements whose float64 sample lies within 1e-4 of the cut may
    legitimately resample differently and are excluded (< 1%)."""
    g = torch.Generator().manual_seed(5)
    n = 67
    keys = ref.full_range_keys(n, g)
    r64, unsure = ref.normal_init_fp64(NORMAL_SEED, keys, dim, **NORMAL)
    r32 = rng.init_rows("normal", NORMAL, NORMAL_SEED, keys, dim)
    assert float(unsure.float().mean()) < 0.01
    sure = ~unsure
    _, _, init_params = _ids()
    cat, p0, p1, p2 = init_params(make_initializer("normal", **NORMAL))
    slots = torch.randperm(n, generator=g)
    W = Guarded(torch.zeros(n, dim))
    S = Guarded(torch.zeros(n, 0))
    out = _ext().gather_init(
        W.view, S.view, slots.to(DEV),
        torch.ones(n, dtype=torch.uint8, device=DEV), keys.to(DEV), None,
        cat, p0, p1, p2, NORMAL_SEED, torch.zeros(0, device=DEV), True,
        None).cpu()
    assert W.guards_intact()
    assert ref.bits_equal(W.cpu()[slots], out)
    ok, (ek, e32, ulp, ratio) = ref.within_reference_error(
        out[sure], r32[sure], r64[sure], MARGIN["normal_init"])
    print(f"RATIO kind=normal_init dim={dim} tensor=out ek={ek:.4g} "
          f"e32={e32:.4g} ulp={ulp:.4g} ratio={ratio:.4g}")
    assert ok, (ek, e32, ulp, ratio)
