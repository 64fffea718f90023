"""The multi-rank routes of ShardedVariable at world 2, 3 and 8 in one
process (padded_wire_ref.SimWorld: a thread per rank, the all-to-alls of
parallel.comm faked as index permutations), against the CPU engine at world
1 fed every rank's batch of a step in rank order.

Gradients are integers in [-3, 3] and the optimizer is SGD with lr = 2^-3
and no momentum, so every gradient sum and lr * sum are exact in fp32 in
any order and w - lr * sum rounds once, the same on both engines. The
initializer is uniform in [-1, 1): u * 2 is exact, so a fused multiply-add
on the device gives the CPU's bits (core/rng.py pins the uniforms
themselves as bit-identical). Every comparison is therefore torch.equal.

Steps are pipelined as the prefetching trainer does it: the pull of step
t + 1 is issued before the push of step t, so the two rotating wire plans
of a shape are both live and a push reads the pos_of / send_src of the plan
that was not written last.
"""

import pytest
import torch

import padded_wire_ref as wref
from openembedding_amd.core.variable import VariableMeta, VariableShard
from openembedding_amd.parallel.sharded import ShardedVariable

DEV = "cuda:0"
SEED = 11
LR = 2.0 ** -3
STEPS = 3
# keys per rank and step: 300 and 257 are no multiple of the 256-thread
# block; at world 8 each of 64 keys meets a [8, 64] wire that is mostly -1
N_OF = {2: 300, 3: 257, 8: 64}


def _configure(v):
    v.set_initializer("uniform", minval=-1.0, maxval=1.0)
    v.set_optimizer("sgd", learning_rate=LR)


def _reference(dim, hash_mode, vocab):
    from openembedding_amd.context import Context
    st = Context(device="cpu", seed=SEED).create_storage()
    var = st.create_variable((1 << 63) if hash_mode else vocab, dim)
    _configure(var)
    return var


def _world(W, device, dim, hash_mode, vocab, padded, variable_id):
    if device == "cpu":
        cls = VariableShard
    else:
        from openembedding_amd.core.variable_gpu import HipVariableShard
        cls = HipVariableShard
    meta = VariableMeta(variable_id=variable_id, embedding_dim=dim,
                        **({} if hash_mode else
                           dict(vocabulary_size=vocab)))
    out = []
    for r in range(W):
        v = ShardedVariable(cls(meta, r, W, device=device, seed=SEED))
        _configure(v)
        v._padded = padded
        out.append(v)
    return out


def _batches(W, n, dim, hash_mode, reserved, seed):
    """[step][rank] -> (keys [n], grads [n, dim]). The vocabulary holds 40
    keys per owner, so keys repeat within a rank and across ranks. Step 0:
    no key belongs to owner 0 and all of rank 0's belong to owner 1 (at
    world 2 that is every rank); step 2: all of the last rank's belong to
    owner 0. ``reserved`` puts the key -1 inside the batches of steps 0
    and 2."""
    g = torch.Generator().manual_seed(seed)
    per = 40
    base = W * (1 << 40) if hash_mode else 0
    steps = []
    for t in range(STEPS):
        ranks = []
        for r in range(W):
            row = torch.randint(0, per, (n,), generator=g)
            own = torch.randint(0, W, (n,), generator=g)
            if t == 0:
                own = torch.randint(1, W, (n,), generator=g)
                if r == 0:
                    own.fill_(1)
            if t == 2 and r == W - 1:
                own.zero_()
            keys = row * W + own + base
            if reserved and t != 1:
                keys[3] = -1
                keys[n - 1] = -1
            grads = torch.randint(-3, 4, (n, dim), generator=g).float()
            ranks.append((keys, grads))
        steps.append(ranks)
    return steps, per * W


def _pipeline(pull, push, commit):
    """pull(t) -> (out, handle); the pull of step t + 1 goes out before
    the push of step t."""
    outs, hs = [None] * STEPS, [None] * STEPS
    outs[0], hs[0] = pull(0)
    for t in range(STEPS):
        if t + 1 < STEPS:
            outs[t + 1], hs[t + 1] = pull(t + 1)
        push(t, hs[t])
        commit(t)
    return outs


def _run_reference(ref, steps, W, dim):
    """Per step and rank the rows that rank must have pulled: the world-1
    CPU engine on the concatenation of the ranks' batches. The CPU engine
    refuses the reserved key, so it is cut out; its rows are zero."""
    def live(t):
        return torch.cat([k for k, _ in steps[t]]) >= 0

    def pull(t):
        keys = torch.cat([k for k, _ in steps[t]])
        rows, h = ref.pull(keys[live(t)])
        full = torch.zeros(keys.numel(), dim)
        full[live(t)] = rows
        return list(full.chunk(W)), h

    def push(t, h):
        ref.push(h, torch.cat([g for _, g in steps[t]])[live(t)])

    return _pipeline(pull, push, lambda t: ref.update_weights())


def _run_world(sim, variables, steps, W, device):
    """Every rank's pulled rows [rank][step], through the production
    routes. Between push and commit each owner's queued block must be the
    exact per-key sums over all ranks."""
    def rank_fn(r):
        var = variables[r]

        def pull(t):
            out, h = var.pull(steps[t][r][0].to(device))
            return out.cpu(), h

        def push(t, h):
            var.push(h, steps[t][r][1].to(device))

        def commit(t):
            keys, gsum, csum = wref.expected_owner_payload(
                [k for k, _ in steps[t]], [g for _, g in steps[t]], W, r)
            got = wref.queued_payload(var.shard)
            assert torch.equal(got[0], keys), (t, r)
            assert torch.equal(got[1], gsum), (t, r)
            assert torch.equal(got[2], csum), (t, r)
            var.update_weights()

        return _pipeline(pull, push, commit)

    return sim.run(rank_fn)


def _probe(ref, variables, steps, W, device):
    """Every touched key, read from its owner's shard, against the
    reference."""
    keys = torch.unique(torch.cat([k for s in steps for k, _ in s]))
    keys = keys[keys >= 0]
    for o in range(W):
        k = keys[keys % W == o]
        assert k.numel()
        got = variables[o].shard.pull_readonly(k.to(device)).cpu()
        assert torch.equal(got, ref.pull(k, readonly=True)[0]), o


def _case(monkeypatch, device, W, dim, hash_mode, padded, reserved):
    n = N_OF[W]
    steps, vocab = _batches(W, n, dim, hash_mode, reserved,
                            seed=100 * W + dim + 2 * hash_mode + padded)
    assert len(torch.unique(steps[1][0][0])) < n       # keys repeat
    ref = _reference(dim, hash_mode, vocab)
    variables = _world(W, device, dim, hash_mode, vocab, padded,
                       ref.variable_id)
    sim = wref.SimWorld(W)
    sim.install(monkeypatch)
    exp = _run_reference(ref, steps, W, dim)
    got = _run_world(sim, variables, steps, W, device)
    for t in range(STEPS):
        for r in range(W):
            assert got[r][t].shape == (n, dim)
            assert torch.equal(got[r][t], exp[t][r]), (t, r)
    _probe(ref, variables, steps, W, device)
    for v in variables:
        v.check_padded_overflow()


@pytest.mark.parametrize("hash_mode", [False, True], ids=["array", "hash"])
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "exact"])
@pytest.mark.parametrize("W", [2, 3])
def test_harness_on_the_cpu_engine(monkeypatch, W, padded, hash_mode):
    """The harness itself, where no kernel runs: CPU shards through the
    padded torch route (and, without the reserved key, which the CPU owner
    refuses, through the exact route) equal the world-1 CPU engine bit for
    bit."""
    _case(monkeypatch, "cpu", W, 9, hash_mode, padded, reserved=padded)


def test_a_failing_rank_fails_the_run_at_once():
    sim = wref.SimWorld(3, timeout=30.0)

    def rank_fn(r):
        if r == 1:
            raise ValueError("rank 1 gave up")
        return sim.all_to_all_equal(torch.zeros(3), 3)

    with pytest.raises(ValueError, match="rank 1 gave up"):
        sim.run(rank_fn)


def test_fake_all_to_all_v_and_lengths():
    W = 3
    sim = wref.SimWorld(W)
    # rank r sends r + o + 1 elements [100 r + 10 o + j] to rank o
    def rank_fn(r):
        splits = [r + o + 1 for o in range(W)]
        inp = torch.cat([100 * r + 10 * o + torch.arange(splits[o])
                         for o in range(W)])
        recv = sim.all_to_all_lengths(torch.tensor(splits))
        assert recv.tolist() == [s + r + 1 for s in range(W)]
        return sim.all_to_all_v(inp, splits, recv.tolist())

    for r, out in enumerate(sim.run(rank_fn)):
        exp = torch.cat([100 * s + 10 * r + torch.arange(s + r + 1)
                         for s in range(W)])
        assert torch.equal(out, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 9])
@pytest.mark.parametrize("hash_mode", [False, True], ids=["array", "hash"])
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "bounded"])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_gpu_routes_match_the_cpu_engine(monkeypatch, W, padded, hash_mode,
                                         dim):
    """_pull_remote_padded / _apply_padded (padded) and _pull_remote_bounded
    / _apply_reduced (bounded) on HipVariableShards: block transposition,
    owner = key % world, slot = key // world on a real owner shard, the
    owner's dedup over a block that is mostly -1, the cross-rank reduce of
    grads ‖ count. Both routes define the reserved key as a zero row."""
    _case(monkeypatch, DEV, W, dim, hash_mode, padded, reserved=True)


@pytest.mark.gpu
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "bounded"])
def test_gpu_routes_are_the_ones_named(monkeypatch, padded):
    """_padded picks the route the cases above mean to run."""
    calls = []
    for name in ("_pull_remote_padded", "_pull_remote_bounded"):
        orig = getattr(ShardedVariable, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            calls.append(_name)
            return _orig(self, *a, **k)

        monkeypatch.setattr(ShardedVariable, name, spy)
    variables = _world(2, DEV, 1, False, 80, padded, 0)
    sim = wref.SimWorld(2)
    sim.install(monkeypatch)
    keys = torch.arange(64, dtype=torch.int64, device=DEV)
    sim.run(lambda r: variables[r].pull(keys))
    want = "_pull_remote_padded" if padded else "_pull_remote_bounded"
    assert calls == [want, want]


@pytest.mark.gpu
@pytest.mark.parametrize("hash_mode", [False, True], ids=["array", "hash"])
def test_gpu_overflow_end_to_end(monkeypatch, hash_mode):
    """Slack 0.5 at world 2 and n = 1024 gives cap 256; rank 0's 1024
    distinct even keys all belong to owner 0, so 768 of them overflow.
    Which 256 ship follows the atomics' order and is read from the plan.
    Shipped keys read their rows, unshipped ones exact zeros; the push
    leaves the unshipped keys' rows as they were on the owner, and the
    host-side check names the 768."""
    monkeypatch.setenv("OEAMD_A2A_SLACK", "0.5")
    W, n, dim = 2, 1024, 9
    g = torch.Generator().manual_seed(5)
    base = W * (1 << 40) if hash_mode else 0
    keys = [torch.randperm(2048, generator=g)[:n] * 2 + base,
            torch.randint(0, 100, (n,), generator=g) * 2 + 1 + base]
    grads = [torch.randint(-3, 4, (n, dim), generator=g).float()
             for _ in range(W)]
    ref = _reference(dim, hash_mode, 4096)
    variables = _world(W, DEV, dim, hash_mode, 4096, True, ref.variable_id)
    sim = wref.SimWorld(W)
    sim.install(monkeypatch)
    # every key has its row before the step, so an untouched row is a row
    # with content and not a missing one
    uniq = [torch.unique(k) for k in keys]
    ref.pull(torch.cat(uniq))
    before = [variables[o].shard.pull(uniq[o].to(DEV)).cpu()
              for o in range(W)]
    for o in range(W):
        assert torch.equal(before[o], ref.pull(uniq[o], readonly=True)[0])

    def rank_fn(r):
        var = variables[r]
        out, h = var.pull(keys[r].to(DEV))
        assert h.plan.cap == 256
        shipped = (h.plan.pos_of.long()[h.inverse] >= 0).cpu()
        var.push(h, grads[r].to(DEV))
        var.update_weights()
        return out.cpu(), shipped

    res = sim.run(rank_fn)
    shipped = [s for _, s in res]
    assert int(shipped[0].sum()) == 256 and bool(shipped[1].all())
    for r in range(W):
        exp = wref.expected_pull(keys[r], shipped[r],
                                 lambda k: ref.pull(k, readonly=True)[0])
        assert torch.equal(res[r][0], exp), r
    assert bool((res[0][0][~shipped[0]] == 0).all())
    # the reference trains on what reached the wire
    sent = torch.cat(shipped)
    _, h = ref.pull(torch.cat(keys)[sent])
    ref.push(h, torch.cat(grads)[sent])
    ref.update_weights()
    after = [variables[o].shard.pull_readonly(uniq[o].to(DEV)).cpu()
             for o in range(W)]
    for o in range(W):
        assert torch.equal(after[o], ref.pull(uniq[o], readonly=True)[0])
    lost = torch.isin(uniq[0], keys[0][~shipped[0]])
    assert int(lost.sum()) == 768
    assert torch.equal(after[0][lost], before[0][lost])
    assert not torch.equal(after[0][~lost], before[0][~lost])
    with pytest.raises(RuntimeError, match=r": 768 keys were dropped"):
        variables[0].check_padded_overflow()
    variables[1].check_padded_overflow()
