"""Exact model of the padded all-to-all wire (ops/csrc/embops.hip, "padded
all-to-all bucketize"; parallel/sharded.py, the padded and bounded remote
routes), in torch on the CPU with int64 / float64.

Slot order inside a bucket follows the order of the kernel's atomics, so the
wire is pinned by order-independent checkers (``check_bucketize``) plus exact
expected values (``expected_pull``, ``expected_owner_payload``).
``transpose`` is the equal-split all-to-all as an index permutation and
``SimWorld`` runs W ranks of the production routes in one process on top of
it: one thread per rank, the collectives of ``parallel.comm`` replaced by
fakes that meet at a barrier.
"""

import threading

import torch


def _cpu(t, dtype=torch.int64):
    return torch.as_tensor(t).detach().cpu().to(dtype).reshape(-1)


def check_bucketize(uk, u, world, cap, send_keys, send_src, pos_of, counts,
                    overflow_before, overflow_after, pos_of_before=None):
    """What one ``bucketize_pad`` call must leave behind, whatever order its
    atomics ran in. ``uk`` is the key buffer, ``u`` its live count (None: all
    of it); entry i is live when ``i < u and uk[i] >= 0``. ``counts`` may be
    None for a writer that keeps none (the torch form). Raises
    AssertionError."""
    uk = _cpu(uk)
    n = uk.numel()
    u = n if u is None else int(u)
    send_keys, send_src, pos_of = _cpu(send_keys), _cpu(send_src), _cpu(pos_of)
    counts = None if counts is None else _cpu(counts)
    assert send_keys.numel() == world * cap, "send_keys length"
    assert send_src.numel() == world * cap, "send_src length"
    assert pos_of.numel() >= n, "pos_of shorter than the key buffer"
    live = (torch.arange(n) < u) & (uk >= 0)
    owner = torch.remainder(uk, world)
    c = torch.bincount(owner[live], minlength=world)
    exp_pos = torch.full((n,), -1, dtype=torch.int64)
    for o in range(world):
        c_o = int(c[o])
        m = min(c_o, cap)
        keys_o = send_keys[o * cap:(o + 1) * cap]
        src_o = send_src[o * cap:(o + 1) * cap]
        pre = src_o[:m]
        assert bool(((pre >= 0) & (pre < n)).all()), \
            f"bucket {o}: hole or bad source inside the first {m} positions"
        assert bool(live[pre].all()), \
            f"bucket {o}: a reserved or tail key was shipped"
        assert bool((owner[pre] == o).all()), \
            f"bucket {o}: holds a key of another owner"
        assert torch.unique(pre).numel() == m, \
            f"bucket {o}: a key was shipped twice"
        assert torch.equal(keys_o[:m], uk[pre]), \
            f"bucket {o}: send_keys[s] != uk[send_src[s]]"
        assert bool((keys_o[m:] == -1).all()) \
            and bool((src_o[m:] == -1).all()), \
            f"bucket {o}: positions behind the prefix are not -1 / -1"
        if counts is not None:
            assert int(counts[o]) == c_o, \
                f"counts[{o}] = {int(counts[o])}, {c_o} live keys"
        exp_pos[pre] = o * cap + torch.arange(m)
    dropped = int((c - cap).clamp(min=0).sum())
    got = int(overflow_after) - int(overflow_before)
    assert got == dropped, f"overflow grew by {got}, {dropped} keys dropped"
    # shipped entries point at their position; reserved keys, the tail and
    # the unshipped keys of an overflowing owner read -1
    assert torch.equal(pos_of[:n], exp_pos), "pos_of is not send_src's inverse"
    if pos_of_before is not None:
        assert torch.equal(pos_of[n:], _cpu(pos_of_before)[n:]), \
            "pos_of was written behind the key buffer"


def transpose(blocks, world):
    """The equal-split all-to-all: ``blocks[r]`` is rank r's [world * cap,
    ...] send buffer; chunk o of rank r becomes chunk r of rank o."""
    assert len(blocks) == world
    cap = blocks[0].shape[0] // world
    for b in blocks:
        assert b.shape[0] == world * cap and b.shape == blocks[0].shape
    return [torch.cat([blocks[r][o * cap:(o + 1) * cap]
                       for r in range(world)]) for o in range(world)]


def expected_pull(keys, shipped_mask, row_of_key):
    """The exact pull output: ``row_of_key(keys)`` (a callable, 1-D int64
    keys -> [m, dim] rows) where ``shipped_mask`` holds and the key is not
    reserved, zero rows everywhere else."""
    keys = _cpu(keys)
    sel = _cpu(shipped_mask, torch.bool) & (keys >= 0)
    rows = row_of_key(keys[sel])
    out = torch.zeros(keys.numel(), rows.shape[1], dtype=rows.dtype)
    out[sel] = rows
    return out


def expected_owner_payload(rank_keys, rank_grads, world, owner,
                           rank_shipped=None):
    """What owner ``owner`` must hold after every rank pushed: (keys
    ascending, per-key sums of the gradients float64 [m, dim], per-key
    occurrence counts float64 [m]) over all ranks' elements. ``rank_keys[r]``
    is rank r's flat batch, ``rank_grads[r]`` its [n, dim] gradient and
    ``rank_shipped[r]`` (optional, bool [n]) the elements whose key reached
    the wire."""
    ks, gs = [], []
    for r in range(world):
        k = _cpu(rank_keys[r])
        sel = (k >= 0) & (torch.remainder(k, world) == owner)
        if rank_shipped is not None:
            sel &= _cpu(rank_shipped[r], torch.bool)
        ks.append(k[sel])
        gs.append(rank_grads[r].detach().cpu().double()[sel])
    k, g = torch.cat(ks), torch.cat(gs)
    uk, inv = torch.unique(k, return_inverse=True)
    gsum = torch.zeros(uk.numel(), g.shape[1], dtype=torch.float64)
    gsum.index_add_(0, inv, g)
    csum = torch.zeros(uk.numel(), dtype=torch.float64)
    csum.index_add_(0, inv, torch.ones(k.numel(), dtype=torch.float64))
    return uk, gsum, csum


def queued_payload(shard):
    """The one block a shard holds between push and commit as (keys
    ascending, grads float64, counts float64), reserved keys and the
    bounded tail dropped: the form ``expected_owner_payload`` returns."""
    bounded = getattr(shard, "_pending_bounded", None)
    if bounded:
        assert len(bounded) == 1 and not shard._pending
        keys, u_dev, _, grads, counts = bounded[0]
        u = keys.numel() if u_dev is None else int(u_dev.item())
        keys, grads, counts = keys[:u], grads[:u], counts[:u]
    elif shard._pending:
        assert len(shard._pending) == 1
        keys, grads, counts = shard._pending[0]
    else:
        return (torch.empty(0, dtype=torch.int64),
                torch.empty(0, shard.dim, dtype=torch.float64),
                torch.empty(0, dtype=torch.float64))
    keys = keys.cpu()
    sel = keys >= 0
    keys, grads, counts = keys[sel], grads.cpu()[sel], counts.cpu()[sel]
    order = torch.argsort(keys)
    return keys[order], grads.double()[order], counts.double()[order]


class SimWorld:
    """W ranks in one process. ``install(monkeypatch)`` replaces the three
    all-to-alls of ``openembedding_amd.parallel.comm``; ``run(fn)`` calls
    ``fn(rank)`` on one thread per rank and returns the results in rank
    order. A fake deposits the calling rank's input, meets the other ranks
    at a barrier and cuts its own output out of everybody's input. An
    exception on one rank aborts the barrier, so the others fail at once
    instead of waiting, and ``run`` raises it."""

    def __init__(self, world, timeout=120.0):
        self.world = world
        self.timeout = timeout
        self._barrier = threading.Barrier(world, timeout=timeout)
        self._box = [None] * world
        self._tls = threading.local()

    @property
    def rank(self):
        return self._tls.rank

    def _exchange(self, value):
        self._box[self.rank] = value
        self._barrier.wait()
        box = list(self._box)
        self._barrier.wait()    # everyone has read before the next deposit
        return box

    def all_to_all_equal(self, inp, world):
        assert world == self.world
        return transpose(self._exchange(inp), world)[self.rank].clone()

    def all_to_all_lengths(self, send_counts):
        return self.all_to_all_equal(send_counts, self.world)

    def all_to_all_v(self, inp, in_splits, out_splits):
        box = self._exchange((inp, [int(s) for s in in_splits]))
        r = self.rank
        chunks = []
        for src, (t, splits) in enumerate(box):
            off = sum(splits[:r])
            assert splits[r] == int(out_splits[src]), "split sizes disagree"
            chunks.append(t[off:off + splits[r]])
        return torch.cat(chunks)

    def install(self, monkeypatch):
        from openembedding_amd.parallel import comm
        for name in ("all_to_all_equal", "all_to_all_v",
                     "all_to_all_lengths"):
            monkeypatch.setattr(comm, name, getattr(self, name))

    def run(self, fn):
        results = [None] * self.world
        errors = [None] * self.world

        def body(r):
            self._tls.rank = r
            try:
                results[r] = fn(r)
            except BaseException as e:      # noqa: BLE001 - re-raised below
                errors[r] = e
                self._barrier.abort()

        threads = [threading.Thread(target=body, args=(r,), daemon=True)
                   for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(self.timeout)
        alive = [t for t in threads if t.is_alive()]
        self._barrier.reset()
        first = [e for e in errors
                 if e is not None
                 and not isinstance(e, threading.BrokenBarrierError)]
        if first:
            raise first[0]
        if alive or any(errors):
            raise RuntimeError("simulated ranks did not finish together")
        return results
