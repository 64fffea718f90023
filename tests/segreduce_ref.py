"""Reference side of tests/test_gpu_segreduce.py: plain torch, no GPU.

  - ``index_violations``: the property checker for a batch's inverted index
    (what ``unique_bounded_indexed`` returns beside the dedup result);
  - ``build_index``: a valid index built on the CPU from ``inverse``, with
    the lists laid out in a shuffled order like the GPU's bump allocator;
  - ``reduce_by_index``: the torch form of the segmented reduce
    (``ops.dispatch.reduce_by_index`` on CPU tensors);
  - ``sum_bound``: the derived error bound of a float32 sum of ``c`` rows.

The checker is itself tested in tests/test_segreduce_checkers.py.
"""

from __future__ import annotations

import torch

from openembedding_amd.ops import dispatch as ops


def _walk(seg_off, seg_cnt, u):
    """Flat walk over the lists of uids [0, u): (uid of every visited
    position, the position in perm)."""
    cnt = seg_cnt[:u].to(torch.int64)
    off = seg_off[:u].to(torch.int64)
    uid = torch.repeat_interleave(torch.arange(u), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    pos = (torch.arange(uid.numel())
           + torch.repeat_interleave(off - first, cnt))
    return uid, pos


def index_violations(inverse, u, seg_off, seg_cnt, perm, long_list, n_long,
                     T):
    """Properties of an inverted index of ``inverse`` [n] with ``u`` live
    uids; returns the violated ones (empty = valid):

      - the lists are disjoint and together cover [0, n);
      - inverse[perm[p]] == uid for every p in uid's list;
      - seg_cnt == bincount(inverse);
      - long_list[:n_long] is exactly {uid : seg_cnt > T}, each once.
    """
    n = inverse.numel()
    u, n_long = int(u), int(n_long)
    if perm.numel() != n:
        return ["perm length != n"]
    if not (0 <= u <= min(seg_off.numel(), seg_cnt.numel())):
        return [f"u = {u} outside the seg arrays"]
    if n and (bool((inverse < 0).any()) or bool((inverse >= u).any())):
        return ["inverse outside [0, u)"]
    if not (0 <= n_long <= long_list.numel()):
        return [f"n_long = {n_long} outside [0, {long_list.numel()}]"]
    cnt = seg_cnt[:u].to(torch.int64)
    off = seg_off[:u].to(torch.int64)
    if bool((cnt < 0).any()) or bool((off < 0).any()) \
            or bool((off + cnt > n).any()):
        return ["a list leaves [0, n)"]
    bad = []
    if not torch.equal(cnt, torch.bincount(inverse, minlength=u)[:u]):
        bad.append("seg_cnt != bincount(inverse)")
    uid, pos = _walk(seg_off, seg_cnt, u)
    elems = perm.to(torch.int64)[pos]
    if bool((elems < 0).any()) or bool((elems >= n).any()):
        return bad + ["a perm entry outside [0, n)"]
    seen = torch.bincount(elems, minlength=n)
    if bool((seen > 1).any()):
        bad.append("an element is in more than one list (lists overlap)")
    if bool((seen == 0).any()):
        bad.append("an element is in no list")
    if not torch.equal(inverse[elems], uid):
        bad.append("an element is filed under another uid")
    ll = long_list[:n_long].to(torch.int64)
    want = (cnt > T).nonzero(as_tuple=True)[0]
    if torch.unique(ll).numel() != ll.numel():
        bad.append("a uid is in long_list twice")
    if bool((~torch.isin(want, ll)).any()):
        bad.append("a long uid is missing from long_list")
    if bool((~torch.isin(ll, want)).any()):
        bad.append("long_list names a uid that is not long")
    return bad


def build_index(inverse, u, T, g=None):
    """A valid index of ``inverse`` as int32 tensors (seg_off, seg_cnt,
    perm, long_list, n_long): lists in a random order of the uids, elements
    inside a list in ascending order, seg arrays n long like the GPU's."""
    n = inverse.numel()
    cnt = torch.bincount(inverse, minlength=u)[:u]
    order = torch.randperm(u, generator=g)
    off = torch.empty(u, dtype=torch.int64)
    off[order] = torch.cumsum(cnt[order], 0) - cnt[order]
    by_uid = torch.argsort(inverse, stable=True)       # elements, uid-major
    start_sorted = torch.cumsum(cnt, 0) - cnt
    perm = torch.empty(n, dtype=torch.int64)
    uid_sorted = inverse[by_uid]
    within = torch.arange(n) - start_sorted[uid_sorted]
    perm[off[uid_sorted] + within] = by_uid
    seg_off = torch.zeros(n, dtype=torch.int32)
    seg_cnt = torch.zeros(n, dtype=torch.int32)
    seg_off[:u] = off.to(torch.int32)
    seg_cnt[:u] = cnt.to(torch.int32)
    longs = (cnt > T).nonzero(as_tuple=True)[0].to(torch.int32)
    long_list = torch.full((n // (T + 1) + 1,), -5, dtype=torch.int32)
    long_list[:longs.numel()] = longs
    n_long = torch.tensor([longs.numel()], dtype=torch.int32)
    return seg_off, seg_cnt, perm.to(torch.int32), long_list, n_long


def reduce_by_index(index, grads, u):
    """The torch form on the CPU: (ugrads [n, dim], counts int64 [n])."""
    index = tuple(t.cpu() for t in index)
    return ops.reduce_by_index(index, grads.cpu(), int(u))


# ------------------------------------------------ small engine sequence
# pull -> push -> update_weights of one small variable with a FIXED gradient
# tensor, so that every route (eager, captured, the atomic reduce) applies
# the same mathematical update and only the order of the float32 adds
# differs. The optimizer is the stateless "default" with lr = 0.5: the
# update w -= 0.5 * G multiplies exactly and rounds once.

SEQ_B, SEQ_F, SEQ_DIM, SEQ_LR, SEQ_VOCAB = 64, 3, 9, 0.5, 500
SEQ_WARM = 6     # steps on batch 0 before the two fresh batches


def seq_batches(hash_mode):
    """([warm batch, fresh batch, fresh batch with a hot key], grad)."""
    g = torch.Generator().manual_seed(11 + int(hash_mode))
    hi = (1 << 40) if hash_mode else SEQ_VOCAB
    bs = [torch.randint(0, hi, (SEQ_B, SEQ_F), generator=g,
                        dtype=torch.int64) for _ in range(3)]
    hot = torch.rand(SEQ_B, SEQ_F, generator=g) < 0.8
    bs[2][hot] = bs[1][0, 0]
    grad = torch.randn(SEQ_B, SEQ_F, SEQ_DIM, generator=g) * 0.1
    return bs, grad


def seq_reset():
    import openembedding_amd.context as cm
    import openembedding_amd.torch as api
    if cm._context is not None:
        cm._context.finalize()
        cm._context = None
    api._tracked.clear()


def seq_make(device, hash_mode):
    import openembedding_amd.torch as embed
    from openembedding_amd.context import get_context
    seq_reset()
    get_context(device)
    emb = embed.Embedding(-1 if hash_mode else SEQ_VOCAB, SEQ_DIM)
    emb.variable.set_optimizer("default", learning_rate=SEQ_LR)
    if hash_mode:
        emb.variable.sharded.reserve_rows(4096)
    return emb


def seq_step(emb, keys, grad):
    var = emb.variable.sharded
    _, h = var.pull(keys)
    var.push(h, grad)
    var.update_weights()
    return h


def seq_keys(hash_mode):
    return torch.unique(torch.cat([b.reshape(-1)
                                   for b in seq_batches(hash_mode)[0]]))


def seq_eager_table(device, hash_mode):
    """(table rows of seq_keys after the whole sequence, last handle)."""
    bs, grad = seq_batches(hash_mode)
    emb = seq_make(device, hash_mode)
    grad = grad.to(device)
    for b in [bs[0]] * SEQ_WARM + bs[1:]:
        h = seq_step(emb, b.to(device), grad)
    table = emb.variable.sparse_read(seq_keys(hash_mode).to(device)).cpu()
    return table, h


def seq_tolerance(hash_mode):
    """Per-entry tolerance [n_keys, dim] (float64) between two float32 runs
    of the sequence. Each step's summed gradient G is within ``sum_bound``
    of the exact sum in either run, the update multiplies by 0.5 exactly
    and rounds the subtraction once (<= 2^-24 relative to a weight that is
    at most 1 + 0.5 * sum of the |g| applied so far); the errors of the
    steps add, and two runs differ by at most twice that."""
    bs, grad = seq_batches(hash_mode)
    keys = seq_keys(hash_mode)
    g2 = grad.reshape(-1, SEQ_DIM)
    tol = torch.zeros(keys.numel(), SEQ_DIM, dtype=torch.float64)
    wcap = torch.ones(keys.numel(), SEQ_DIM, dtype=torch.float64)
    for b in [bs[0]] * SEQ_WARM + bs[1:]:
        inv = torch.searchsorted(keys, b.reshape(-1))
        mag = torch.zeros(keys.numel(), SEQ_DIM, dtype=torch.float64)
        mag.index_add_(0, inv, g2.double().abs())
        c = torch.bincount(inv, minlength=keys.numel()).double().unsqueeze(1)
        bound = c * 2.0 ** -23 * mag
        wcap += SEQ_LR * mag
        tol += SEQ_LR * bound + 2.0 ** -24 * wcap
    return 2.0 * tol


def seq_child_main(out_path):
    """Entry of the child process of the OEAMD_SEG_REDUCE=0 test: the eager
    sequence for both table kinds on the old route."""
    from openembedding_amd.parallel import sharded
    assert sharded._SEG_REDUCE is False
    out = {}
    for hash_mode in (False, True):
        table, h = seq_eager_table("cuda:0", hash_mode)
        assert h.index is None
        out[hash_mode] = table
    seq_reset()
    torch.save(out, out_path)


def sum_bound(inverse, grads, u):
    """Per-entry bound [n, dim] (float64) of a float32 sum of a uid's rows
    in ANY order: c - 1 adds, each with relative error <= 2^-24 of a partial
    sum that is itself <= (1 + small) * sum_e |g_e[j]|, so
    c * 2^-23 * sum_e |g_e[j]| covers it with room for the second-order
    terms (c = the uid's count)."""
    n = grads.shape[0]
    mag = torch.zeros((n, grads.shape[1]), dtype=torch.float64)
    mag.index_add_(0, inverse, grads.double().abs())
    c = torch.bincount(inverse, minlength=n).double().unsqueeze(1)
    return c * 2.0 ** -23 * mag
