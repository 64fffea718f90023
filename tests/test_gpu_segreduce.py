"""The indexed dedup (k_unique_*<true>) and the segmented reduce
(k_seg_reduce) of ops/csrc/embops.hip, called through the extension (all
@gpu). The reference side (index property checker, torch form of the
reduce, derived error bound, the small engine sequence) is
tests/segreduce_ref.py, tested without a GPU in
tests/test_segreduce_checkers.py.

Sums. With integer-valued gradients every order of adds gives the same
float32 result, so the kernel must be torch.equal to the torch form. With
random data the bound per entry is c * 2^-23 * sum_e |g_e[j]| (c = the
uid's count): c - 1 float32 adds in any order, each within 2^-24 relative.
It is derived, not fitted; the float32 index_add of torch on the same data
is held to it first, so that the inputs are known to be fair.

Measured on an MI355X (max err / bound over the cases of
test_sums_random_within_derived_bound, n = 20001): 0.29 at dim 10 and 0.31
at dim 65 for the mixed key set, below 5e-5 for the others.
"""

import os
import subprocess
import sys

import pytest
import torch

import segreduce_ref as sref
import sparse_core_ref as ref
from openembedding_amd.core import rng
from openembedding_amd.ops import dispatch as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 20001]
KEY_SETS = ["all_equal", "all_distinct", "three_keys", "reserved_mix"]


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _T():
    return _ext().seg_reduce_threshold()


def _key_set(kind, n, g):
    if kind == "all_equal":
        return torch.full((n,), 42, dtype=torch.int64)
    if kind == "all_distinct":
        return torch.randperm(n, generator=g) * 2654435761 - 10 ** 12
    if kind == "three_keys":
        pick = torch.randint(0, 3, (n,), generator=g)
        return torch.tensor([3, -7, 1 << 40], dtype=torch.int64)[pick]
    assert kind == "reserved_mix"
    keys = torch.randint(0, max(2, n // 3), (n,), generator=g,
                         dtype=torch.int64)
    keys[torch.rand(n, generator=g) < 0.2] = -1
    keys[n // 2] = -1
    return keys


def _threshold_lengths_keys(g):
    """Lists of exactly T-1, T and T+1 elements among singles."""
    T = _T()
    parts = [torch.full((T - 1,), 1001), torch.full((T,), 1002),
             torch.full((T + 1,), 1003), torch.arange(300)]
    keys = torch.cat(parts).to(torch.int64)
    return keys[torch.randperm(keys.numel(), generator=g)]


def _lds_overflow_keys(g):
    """More than 64 distinct keys of ONE block in one bucket of the 1024-
    entry LDS pre-filter: the elements past the 64th take the overflow
    route (their own tcount add); copies in the neighbouring blocks rank
    through the LDS route and must land in the same lists."""
    coll = ref.colliding_keys(1023, [5], 220)
    assert bool(((rng.splitmix64(coll) & 1023) == 5).all())
    hot = torch.cat([coll, coll[torch.randint(0, 220, (36,), generator=g)]])
    hot = hot[torch.randperm(256, generator=g)]

    def ordinary(m):
        blk = torch.randint(0, 1000, (m,), generator=g, dtype=torch.int64)
        blk[::5] = coll[torch.randint(0, 220, (len(blk[::5]),),
                                      generator=g)]
        return blk

    keys = torch.cat([ordinary(256), hot, ordinary(256), ordinary(17)])
    assert keys.numel() == 785 and torch.equal(keys[256:512], hot)
    return keys


def _fused_offsets_case(g, F=26, B=37):
    raw = torch.randint(0, 50, (B, F), generator=g, dtype=torch.int64)
    foff = torch.arange(F, dtype=torch.int64) * 40 - 17   # fields overlap
    raw[2, F - 1] = -1 - foff[F - 1]
    flat = (raw + foff).reshape(-1)
    assert int((flat == -1).sum()) >= 1
    return flat, raw, foff


def _indexed(flat, raw=None, foff=None):
    """unique_bounded_indexed on the GPU, held against both property
    checkers. Returns (inverse cpu, u, index on the device, u_dev)."""
    ext = _ext()
    src = (flat if raw is None else raw.reshape(-1)).to(DEV)
    r = ext.unique_bounded_indexed(
        src, None if foff is None else foff.to(DEV))
    uk, inv, u_dev, index = r[0], r[1], r[2], tuple(r[3:])
    assert all(t.dtype == torch.int32 for t in index)
    n = flat.numel()
    assert [t.numel() for t in index[:3]] == [n, n, n]
    assert index[3].numel() >= n // (_T() + 1) + 1 and index[4].numel() == 1
    u = int(u_dev.item())
    bad = ref.dedup_violations(flat, uk.cpu(), inv.cpu(), u)
    assert bad == [], bad
    bad = sref.index_violations(inv.cpu(), u, *[t.cpu() for t in index],
                                _T())
    assert bad == [], bad
    return inv.cpu(), u, index, u_dev


def _int_grads(n, dim, g):
    # |sum| <= 8 * 20001 < 2^24: every partial sum is exact in float32
    return torch.randint(-8, 9, (n, dim), generator=g).float()


def _check_exact(inv, u, index, u_dev, dim, g):
    n = inv.numel()
    grads = _int_grads(n, dim, g)
    ugrads, counts = ops.reduce_by_index(index, grads.to(DEV), u_dev)
    want_g, want_c = sref.reduce_by_index(index, grads, u)
    assert ugrads.shape == (n, dim) and counts.dtype == torch.int64
    assert torch.equal(ugrads.cpu(), want_g)
    assert torch.equal(counts.cpu(), want_c)
    # the torch form walked the same index; hold it to a plain index_add
    assert torch.equal(want_g, torch.zeros(n, dim).index_add_(0, inv, grads))
    assert torch.equal(want_c, torch.bincount(inv, minlength=n))
    assert not bool(ugrads[u:].any()) and not bool(counts[u:].any())


# ------------------------------------------------------- index properties

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KEY_SETS)
def test_index_properties_and_exact_sums(kind, n):
    """Sizes around the wave, the block and the per-thread factors of the
    three dedup kernels; the flagship's dim-10 sums on every one of them."""
    g = torch.Generator().manual_seed(
        100 * KEY_SETS.index(kind) + SIZES.index(n))
    flat = _key_set(kind, n, g)
    inv, u, index, u_dev = _indexed(flat)
    if kind == "all_equal":
        # one list of n: beyond T it goes through the long role, at 20001
        # over several block rounds
        cnt = index[1].cpu()
        assert u == 1 and int(cnt[0]) == n
        assert int(index[4].item()) == (1 if n > _T() else 0)
    _check_exact(inv, u, index, u_dev, 10, g)


SPECIAL = ["threshold_lengths", "lds_overflow", "fused_offsets"]


def _special(kind, g):
    """(flat, raw, foff) of a special construction."""
    if kind == "threshold_lengths":
        return _threshold_lengths_keys(g), None, None
    if kind == "lds_overflow":
        return _lds_overflow_keys(g), None, None
    return _fused_offsets_case(g)


@pytest.mark.parametrize("dim", [10, 65])
@pytest.mark.parametrize("kind", SPECIAL)
def test_special_constructions(kind, dim):
    g = torch.Generator().manual_seed(7 + SPECIAL.index(kind))
    flat, raw, foff = _special(kind, g)
    inv, u, index, u_dev = _indexed(flat, raw, foff)
    if kind == "threshold_lengths":
        T = _T()
        cnt = index[1].cpu()[:u]
        assert sorted(cnt[cnt > 1].tolist()) == [T - 1, T, T + 1]
        assert int(index[4].item()) == 1
    _check_exact(inv, u, index, u_dev, dim, g)


# ------------------------------------------------------------ sums, exact

def _ladder_top():
    return _ext().seg_reduce_max_dim()


@pytest.mark.parametrize("dim", [1, 9, 16, 17, 65, "top"])
@pytest.mark.parametrize("kind", KEY_SETS)
def test_sums_exact_over_dims(kind, dim):
    """Every rung of the launcher's ladder (dim 10 runs above), n = 2049:
    all_equal is one long list over several rounds of the long role,
    three_keys three of them, reserved_mix lists of one among short ones."""
    dim = _ladder_top() if dim == "top" else dim
    g = torch.Generator().manual_seed(31 * KEY_SETS.index(kind) + dim)
    inv, u, index, u_dev = _indexed(_key_set(kind, 2049, g))
    _check_exact(inv, u, index, u_dev, dim, g)


def test_dim_above_ladder_keeps_the_old_route():
    dim = _ladder_top() + 1
    g = torch.Generator().manual_seed(5)
    flat = _key_set("reserved_mix", 2049, g)
    inv, u, index, u_dev = _indexed(flat)
    grads = _int_grads(flat.numel(), dim, g)
    gd = grads.to(DEV)
    assert not ops.seg_reduce_covers(gd)
    assert ops.seg_reduce_covers(gd[:, :dim - 1].contiguous())
    assert not ops.seg_reduce_covers(gd.double())
    assert not ops.seg_reduce_covers(grads)
    with pytest.raises(RuntimeError):
        _ext().reduce_by_index(*index, gd, u_dev)
    # what push() then takes
    n = flat.numel()
    ugrads, counts = ops.reduce_by_inverse(inv.to(DEV), gd, n)
    assert torch.equal(ugrads.cpu(),
                       torch.zeros(n, dim).index_add_(0, inv, grads))
    assert torch.equal(counts.cpu(), torch.bincount(inv, minlength=n))


# ------------------------------------------------------ sums, random data

@pytest.mark.parametrize("dim", [10, 65])
@pytest.mark.parametrize("kind", KEY_SETS)
def test_sums_random_within_derived_bound(kind, dim):
    n = 20001
    g = torch.Generator().manual_seed(900 + 10 * KEY_SETS.index(kind) + dim)
    flat = _key_set(kind, n, g)
    inv, u, index, u_dev = _indexed(flat)
    grads = torch.randn(n, dim, generator=g)
    ref64 = torch.zeros(n, dim, dtype=torch.float64).index_add_(
        0, inv, grads.double())
    bound = sref.sum_bound(inv, grads, u)
    # the inputs are fair: torch's own float32 sum meets the bound
    cpu32 = torch.zeros(n, dim).index_add_(0, inv, grads)
    assert bool(((cpu32.double() - ref64).abs() <= bound).all())
    ugrads, counts = ops.reduce_by_index(index, grads.to(DEV), u_dev)
    err = (ugrads.cpu().double() - ref64).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.
    print(f"seg_reduce {kind} dim {dim}: max err/bound = {ratio:.3g}")
    assert bool((err <= bound).all()), ratio
    assert torch.equal(counts.cpu(), torch.bincount(inv, minlength=n))


# ------------------------------------------------------ old route unchanged

@pytest.mark.parametrize("kind,n", [("three_keys", 2049),
                                    ("reserved_mix", 20001),
                                    ("all_equal", 257)])
def test_old_route_unchanged(kind, n):
    """unique_bounded + reduce_by_inverse (the routes that keep them) give
    the same dedup properties and sums as before."""
    ext = _ext()
    g = torch.Generator().manual_seed(1234 + n)
    flat = _key_set(kind, n, g)
    uk, inv, u_dev = ext.unique_bounded(flat.to(DEV))
    u = int(u_dev.item())
    bad = ref.dedup_violations(flat, uk.cpu(), inv.cpu(), u)
    assert bad == [], bad
    grads = _int_grads(n, 10, g)
    ugrads, counts = ops.reduce_by_inverse(inv, grads.to(DEV), n)
    assert torch.equal(ugrads.cpu(),
                       torch.zeros(n, 10).index_add_(0, inv.cpu(), grads))
    assert torch.equal(counts.cpu(), torch.bincount(inv.cpu(), minlength=n))


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
def test_capture_replay_matches_eager(hash_mode):
    """One captured pull -> push -> update_weights (64 samples x 3 fields,
    dim 9) replayed on two fresh key batches, the second with a key hot
    enough for the long role, trains the table eager execution trains."""
    bs, _ = sref.seq_batches(hash_mode)
    assert int(torch.bincount(
        torch.unique(bs[2], return_inverse=True)[1].reshape(-1)).max()) > _T()
    want, h = sref.seq_eager_table(DEV, hash_mode)
    assert h.index is not None          # the segmented route ran
    got = _captured_table(hash_mode)
    sref.seq_reset()
    tol = sref.seq_tolerance(hash_mode)
    err = (got.double() - want.double()).abs()
    assert float(want.abs().max()) > 0.5     # the steps are visible
    assert bool((err <= tol).all()), float((err - tol).max())


def test_old_route_switch_in_child_process(tmp_path):
    """OEAMD_SEG_REDUCE=0 (read once at import, hence a fresh process)
    keeps the atomic reduce; the trained tables agree within the bound."""
    out = tmp_path / "tables.pt"
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [%r, %r]; import segreduce_ref as s; "
            "s.seq_child_main(%r)" % (root, tests_dir, str(out)))
    env = dict(os.environ, OEAMD_SEG_REDUCE="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True,
                   timeout=300)
    old = torch.load(out)
    for hash_mode in (False, True):
        want, h = sref.seq_eager_table(DEV, hash_mode)
        assert h.index is not None
        sref.seq_reset()
        err = (old[hash_mode].double() - want.double()).abs()
        assert bool((err <= sref.seq_tolerance(hash_mode)).all())
