"""Shared scenario of the delta-checkpoint tests (CPU and GPU).

One trainer goes through three phases with hand-chosen key sets, so that
every test can state the exact content of each delta:

  phase A  touches keys 0..999                       -> full dump A
  phase B  updates 200..299, creates 1000..1049      -> delta D1 (150 keys)
  phase C  updates 250..349 and 1040..1049, creates
           1050..1059, updates 5 and 7               -> delta D2 (122 keys)
                                                     -> full dump B
"""

import os

import torch

from openembedding_amd import checkpoint
from openembedding_amd.context import Context

DIM = 6
VOCAB = 1200          # array tables: covers every key used below

KEYS_A = list(range(1000))
KEYS_B = list(range(200, 300)) + list(range(1000, 1050))
KEYS_C = list(range(250, 350)) + list(range(1040, 1060)) + [5, 7]


def make_trainer(device="cpu", table="hash", opt="adagrad", track=True,
                 dim=DIM, reserve=0):
    """(ctx, storage, variable) with one variable, tracking on by default."""
    ctx = Context(device=device)
    st = ctx.create_storage()
    var = st.create_variable(VOCAB if table == "array" else -1, dim)
    var.set_initializer("normal", mean=0.0, stddev=0.1)
    var.set_optimizer(opt, learning_rate=0.05)
    if reserve and table == "hash":   # an array table is sized already
        var.reserve_rows(reserve)
    if track:
        var.shard.track_changes()
    return ctx, st, var


def make_consumer(device="cpu", table="hash", opt="adagrad", dim=DIM):
    return make_trainer(device, table, opt, track=False, dim=dim)


def batch(keys, seed, dim=DIM, device="cpu"):
    """The keys once each in a seeded order, a tenth of them twice, and one
    seeded gradient row per element."""
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor(keys, dtype=torch.int64)
    k = torch.cat([k, k[::10]])
    k = k[torch.randperm(k.numel(), generator=g)]
    grads = torch.randn(k.numel(), dim, generator=g)
    return k.to(device), grads.to(device)


def train(st, var, keys, seed, dim=DIM):
    k, grads = batch(keys, seed, dim, str(var.shard.device))
    _, h = var.pull(k)
    var.push(h, grads)
    st.update_weights()


def rows_by_key(shard, include_state=True):
    """(keys, weights, state) of every row, on the CPU, sorted by key."""
    keys, w, s = shard.export_rows(include_state=include_state)
    keys = keys.cpu()
    order = torch.argsort(keys)
    return (keys[order], w.cpu()[order],
            s.cpu()[order] if s is not None else None)


def assert_same_rows(a, b):
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert (a[2] is None) == (b[2] is None)
    if a[2] is not None:
        assert torch.equal(a[2], b[2])


def dump_rows(uri):
    """{key: (weights, state)} of a dump or delta, later blocks winning,
    and the list of all keys in file order."""
    rows, order = {}, []
    for _hdr, keys, w, s in checkpoint.iter_blocks(uri):
        for i, k in enumerate(keys.tolist()):
            rows[k] = (w[i].tobytes(), s[i].tobytes() if s is not None
                       else None)
            order.append(k)
    return rows, order


def run_chain(tmp, device="cpu", table="hash", opt="adagrad", step=train):
    """Phases A, B, C on a fresh tracked trainer; writes A, D1, D2, B under
    ``tmp`` and returns (ctx, st, var, info) with the dump_delta results."""
    ctx, st, var = make_trainer(device, table, opt)
    uri = {n: os.path.join(str(tmp), n) for n in ("A", "D1", "D2", "B")}
    step(st, var, KEYS_A, 1)
    checkpoint.dump_model(ctx, uri["A"])
    step(st, var, KEYS_B, 2)
    d1 = checkpoint.dump_delta(ctx, uri["D1"])
    step(st, var, KEYS_C, 3)
    d2 = checkpoint.dump_delta(ctx, uri["D2"])
    checkpoint.dump_model(ctx, uri["B"])
    return ctx, st, var, {"uri": uri, "d1": d1, "d2": d2}


PROBE = sorted(set(KEYS_A + KEYS_B + KEYS_C)) + [1100, 1150, 1199]  # absent


def _bags():
    """Ragged bags over EVERY key of B plus the absent ones: the keys in a
    seeded order, a tenth of them twice, split into bags of 0..7 keys."""
    g = torch.Generator().manual_seed(11)
    v = torch.tensor(PROBE)
    v = torch.cat([v, v[::10]])
    v = v[torch.randperm(v.numel(), generator=g)]
    off = [0]
    while off[-1] < v.numel():
        off.append(min(v.numel(), off[-1] + len(off) % 8))
    return v.tolist(), off


BAG_VALUES, BAG_OFFSETS = _bags()


def check_served_chain(uri, device, fmt):
    """A ServedModel loaded from A that applies D1 and D2 must answer like
    one freshly loaded from B in the same row format, bit for bit. Returns
    (updated, fresh)."""
    from openembedding_amd.serving import ServedModel
    m = ServedModel("live", uri["A"])
    m.load(device=device, quantize=fmt)
    assert m.loaded_epoch == 1 and m.describe()["epoch"] == 1
    stale = m.variables[0].pull_weights(torch.tensor(PROBE)).cpu()
    r1 = m.apply_delta(uri["D1"])
    assert r1 == {"since": 2, "epoch": 2, "rows": 150}
    r2 = m.apply_delta(uri["D2"])
    assert r2["epoch"] == 3 and m.describe()["epoch"] == 3
    fresh = ServedModel("fresh", uri["B"])
    fresh.load(device=device, quantize=fmt)
    got = m.variables[0].pull_weights(torch.tensor(PROBE)).cpu()
    want = fresh.variables[0].pull_weights(torch.tensor(PROBE)).cpu()
    assert torch.equal(got, want) and not torch.equal(got, stale)
    assert bool((want[-3:] == 0).all()) and bool((want[:-3] != 0).any())
    assert set(BAG_VALUES) == set(PROBE) and BAG_OFFSETS[-1] == len(BAG_VALUES)
    for mode in ("sum", "mean", "sqrtn"):
        a = m.variables[0].pull_pooled(BAG_VALUES, BAG_OFFSETS, mode)
        b = fresh.variables[0].pull_pooled(BAG_VALUES, BAG_OFFSETS, mode)
        assert torch.equal(a.cpu(), b.cpu())
    assert m.variables[0].storage == (fmt or "fp32")
    assert m.variables[0].shard.num_rows == fresh.variables[0].shard.num_rows
    return m, fresh


def changed_keys(sh, since):
    keys = [k for blk in sh.export_changed(since)
            for k in blk[0].cpu().tolist()]
    assert len(keys) == len(set(keys))
    return set(keys)


def stamp_scenario(sh, grow_to):
    """Every stamp rule in turn on a tracked shard of dim 4 (adagrad set);
    returns [(label, changed key set)] for comparison with the set computed
    by hand or with another backend. ``grow_to`` new keys are pulled at the
    end to make the row slab (and row_epoch with it) grow."""
    dev = sh.device
    t = lambda *a: torch.tensor(a, dtype=torch.int64, device=dev)  # noqa
    out = []
    sh.pull(t(3, 9, 27, 81))
    out.append(("pull new", changed_keys(sh, 1)))
    sh.set_epoch(2)
    sh.pull(t(3, 9))
    sh.pull_readonly(t(3, 9, 100))
    sh.pull_pooled_readonly(t(3, 9, 100), t(0, 2, 3), "sum")
    out.append(("pull existing", changed_keys(sh, 2)))
    sh.push(t(9, 27, 200), torch.ones(3, 4, device=dev), t(1, 1, 1))
    sh.update_weights()
    out.append(("push+update", changed_keys(sh, 2)))
    sh.set_epoch(3)
    sh.import_rows(t(81, 300), torch.zeros(2, 4, device=dev))
    out.append(("import", changed_keys(sh, 3)))
    out.append(("import, since 2", changed_keys(sh, 2)))
    sh.set_epoch(4)
    sh.set_optimizer("adagrad", learning_rate=0.5)
    out.append(("same optimizer", changed_keys(sh, 4)))
    sh.set_optimizer("adam", learning_rate=0.1)
    out.append(("new optimizer", changed_keys(sh, 4)))
    sh.set_epoch(5)
    sh.pull(torch.arange(1000, 1000 + grow_to, dtype=torch.int64, device=dev))
    assert sh.row_epoch.numel() == sh.weights.shape[0]
    out.append(("grown", changed_keys(sh, 5)))
    out.append(("grown, since 4", changed_keys(sh, 4)))
    sh.clear()
    out.append(("clear", changed_keys(sh, 0)))
    assert int(sh.row_epoch.abs().sum()) == 0
    sh.pull(t(3))
    out.append(("after clear", changed_keys(sh, 1)))
    return out


def stamp_scenario_by_hand(grow_to):
    live = {3, 9, 27, 81, 200, 300}
    grown = set(range(1000, 1000 + grow_to))
    return [("pull new", {3, 9, 27, 81}), ("pull existing", set()),
            ("push+update", {9, 27, 200}), ("import", {81, 300}),
            ("import, since 2", {9, 27, 200, 81, 300}),
            ("same optimizer", set()), ("new optimizer", live),
            ("grown", grown), ("grown, since 4", grown | live),
            ("clear", set()), ("after clear", {3})]


def all_files(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out
