"""The wire model of padded_wire_ref against the torch form of the padded
bucketize (ShardedVariable._bucketize_pad_torch), and against one hand-made
mutant per way a bucketize can go wrong. No GPU."""

import pytest
import torch

import padded_wire_ref as wref
from openembedding_amd.parallel.sharded import ShardedVariable, _PaddedPlan

WORLDS = [1, 2, 3, 8]


def _plan(world, cap, n):
    """A _PaddedPlan with a capacity of the test's choosing (the class
    derives its own from n and OEAMD_A2A_SLACK)."""
    p = _PaddedPlan.__new__(_PaddedPlan)
    p.world, p.cap = world, cap
    p.send_keys = torch.full((world * cap,), 5, dtype=torch.int64)
    p.send_src = torch.full((world * cap,), 5, dtype=torch.int32)
    p.pos_of = torch.full((n,), 5, dtype=torch.int32)
    p.overflow_host = 0
    return p


def _keys(n, seed):
    """n distinct keys, some above 2^40, with reserved -1 keys inside."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randperm(4 * n, generator=g)[:n].to(torch.int64)
    k[1::3] += 1 << 41
    k[5::11] = -1
    return k


def _bucketize(world, cap, uk):
    plan = _plan(world, cap, uk.numel() + 3)
    ShardedVariable._bucketize_pad_torch(None, uk, plan)
    return plan


def _cmax(uk, world):
    live = uk[uk >= 0]
    return int(torch.bincount(live % world, minlength=world).max())


def _check(uk, plan, u=None, overflow=None):
    wref.check_bucketize(uk, u, plan.world, plan.cap, plan.send_keys,
                         plan.send_src, plan.pos_of, None, 0,
                         plan.overflow_host if overflow is None
                         else overflow)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n", [1, 40, 257])
def test_accepts_the_torch_bucketize(world, n):
    uk = _keys(n, 10 * world + n)
    cmax = _cmax(uk, world)
    for cap in {cmax + 3, max(cmax, 1), max(cmax - 1, 1), 1}:
        plan = _bucketize(world, cap, uk)
        _check(uk, plan)
        live = uk[uk >= 0]
        dropped = (torch.bincount(live % world, minlength=world)
                   - cap).clamp(min=0).sum()
        assert plan.overflow_host == int(dropped)
        # a second call on the same buffers with fewer keys
        few = uk[:max(1, n // 5)].clone()
        before = plan.overflow_host
        ShardedVariable._bucketize_pad_torch(None, few, plan)
        wref.check_bucketize(few, None, world, cap, plan.send_keys,
                             plan.send_src, plan.pos_of, None, before,
                             plan.overflow_host)


def _case(world=3, n=60, slack=2, seed=1):
    uk = _keys(n, seed)
    plan = _bucketize(world, _cmax(uk, world) + slack, uk)
    _check(uk, plan)
    return uk, plan


def _prefix(uk, plan, o):
    """Positions of bucket o's shipped prefix."""
    c = int(((uk >= 0) & (uk % plan.world == o)).sum())
    return list(range(o * plan.cap, o * plan.cap + min(c, plan.cap)))


def _rejects(uk, plan, match, **kw):
    with pytest.raises(AssertionError, match=match):
        _check(uk, plan, **kw)


def test_rejects_a_key_in_the_wrong_bucket():
    uk, plan = _case()
    a, b = _prefix(uk, plan, 0)[-1], _prefix(uk, plan, 1)[-1]
    for t in (plan.send_keys, plan.send_src):
        t[a], t[b] = t[b].clone(), t[a].clone()
    plan.pos_of[plan.send_src[a].long()] = a
    plan.pos_of[plan.send_src[b].long()] = b
    _rejects(uk, plan, "another owner")


def test_rejects_a_hole_inside_a_prefix():
    uk, plan = _case()
    s = _prefix(uk, plan, 1)[1]
    plan.pos_of[plan.send_src[s].long()] = -1
    plan.send_keys[s] = -1
    plan.send_src[s] = -1
    _rejects(uk, plan, "hole")


def test_rejects_a_key_shipped_twice():
    uk, plan = _case()
    p = _prefix(uk, plan, 2)
    plan.pos_of[plan.send_src[p[1]].long()] = -1
    plan.send_keys[p[1]] = plan.send_keys[p[0]]
    plan.send_src[p[1]] = plan.send_src[p[0]]
    _rejects(uk, plan, "twice")


def test_rejects_pos_of_not_inverse_of_send_src():
    uk, plan = _case()
    p = _prefix(uk, plan, 0)
    i, j = plan.send_src[p[0]].long(), plan.send_src[p[1]].long()
    plan.pos_of[i], plan.pos_of[j] = p[1], p[0]
    _rejects(uk, plan, "inverse")


def test_rejects_overflow_off_by_one():
    uk = _keys(60, 2)
    plan = _bucketize(3, _cmax(uk, 3) - 2, uk)
    _check(uk, plan)
    assert plan.overflow_host >= 2
    _rejects(uk, plan, "overflow", overflow=plan.overflow_host + 1)
    _rejects(uk, plan, "overflow", overflow=plan.overflow_host - 1)


def test_rejects_a_stale_entry_behind_the_prefix():
    uk, plan = _case(slack=4)
    p = _prefix(uk, plan, 1)
    # what a missing reset leaves: the previous call's last entry
    plan.send_keys[p[-1] + 2] = plan.send_keys[p[0]]
    plan.send_src[p[-1] + 2] = plan.send_src[p[0]]
    _rejects(uk, plan, "behind the prefix")


def test_rejects_a_shipped_tail_key():
    uk, plan = _case()
    u = 40
    head = uk.clone()
    head[u:] = -1
    good = _bucketize(3, plan.cap, head)
    wref.check_bucketize(uk, u, 3, plan.cap, good.send_keys, good.send_src,
                         good.pos_of, None, 0, 0)
    # the full buffer's plan ships keys behind u
    _rejects(uk, plan, "positions|reserved or tail", u=u)
    # exactly one tail key in place of a live one
    tail = next(i for i in range(u, 60) if uk[i] >= 0 and uk[i] % 3 == 0)
    s = _prefix(head, good, 0)[0]
    good.pos_of[good.send_src[s].long()] = -1
    good.send_keys[s], good.send_src[s] = uk[tail], tail
    good.pos_of[tail] = s
    with pytest.raises(AssertionError, match="reserved or tail"):
        wref.check_bucketize(uk, u, 3, plan.cap, good.send_keys,
                             good.send_src, good.pos_of, None, 0, 0)


def test_rejects_a_shipped_reserved_key():
    uk, plan = _case()
    i = int((uk < 0).nonzero()[0])
    s = _prefix(uk, plan, 2)[0]
    plan.pos_of[plan.send_src[s].long()] = -1
    plan.send_keys[s], plan.send_src[s] = -1, i
    plan.pos_of[i] = s
    _rejects(uk, plan, "reserved or tail")


def test_rejects_wrong_counts_and_a_written_pos_of_tail():
    uk, plan = _case()
    live = uk[uk >= 0]
    counts = torch.bincount(live % 3, minlength=3)
    args = (uk, None, 3, plan.cap, plan.send_keys, plan.send_src,
            plan.pos_of)
    before = plan.pos_of.clone()
    wref.check_bucketize(*args, counts, 0, 0, pos_of_before=before)
    counts[1] += 1
    with pytest.raises(AssertionError, match="counts"):
        wref.check_bucketize(*args, counts, 0, 0)
    before[-1] += 1
    with pytest.raises(AssertionError, match="behind the key buffer"):
        wref.check_bucketize(*args, None, 0, 0, pos_of_before=before)


@pytest.mark.parametrize("world", WORLDS)
def test_transpose_moves_chunks_and_is_an_involution(world):
    cap = 3
    blocks = [torch.arange(world * cap * 2).view(world * cap, 2)
              + 1000 * r for r in range(world)]
    out = wref.transpose(blocks, world)
    for r in range(world):
        for o in range(world):
            assert torch.equal(out[o][r * cap:(r + 1) * cap],
                               blocks[r][o * cap:(o + 1) * cap])
    back = wref.transpose(out, world)
    assert all(torch.equal(a, b) for a, b in zip(back, blocks))


def test_expected_pull_and_owner_payload():
    keys = torch.tensor([4, -1, 7, 4, 9])
    shipped = torch.tensor([True, True, False, True, True])
    out = wref.expected_pull(
        keys, shipped, lambda k: k.double().unsqueeze(1).expand(-1, 2))
    assert torch.equal(out, torch.tensor(
        [[4., 4.], [0., 0.], [0., 0.], [4., 4.], [9., 9.]],
        dtype=torch.float64))
    rk = [torch.tensor([4, 6, -1, 4]), torch.tensor([6, 3, 4, 8])]
    rg = [torch.tensor([[1.], [2.], [9.], [3.]]),
          torch.tensor([[-1.], [5.], [2.], [7.]])]
    k, g, c = wref.expected_owner_payload(rk, rg, 2, 0)
    assert k.tolist() == [4, 6, 8]
    assert g.tolist() == [[6.], [1.], [7.]] and c.tolist() == [3., 2., 1.]
    k, g, c = wref.expected_owner_payload(
        rk, rg, 2, 0, [torch.tensor([True, False, True, True]),
                       torch.tensor([True, True, True, False])])
    assert k.tolist() == [4, 6]
    assert g.tolist() == [[6.], [-1.]] and c.tolist() == [3., 1.]
