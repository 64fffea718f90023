"""k_pad_reset / k_bucketize_pad / k_gather_pad / k_scatter_out /
k_split_payload / k_mask_tail (ops/csrc/embops.hip) through their bindings
against the wire model of padded_wire_ref. The bucketize is checked by the
order-independent ``check_bucketize``; the other five are copies and are
compared bit for bit. Inputs are views between canaries of larger buffers;
outputs the bindings allocate come from an allocator poisoned with NaN
patterns."""

import pytest
import torch

import padded_wire_ref as wref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 8                 # canary elements / rows on either side
DIMS = [1, 9, 64, 65]   # 64 / 65: either side of a wavefront of columns


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _poison_allocator(nbytes):
    """Free blocks of the size of the next output, full of NaN patterns:
    the caching allocator hands a freed block of the same size class
    back."""
    junk = [torch.full(((nbytes + 3) // 4,), 0x7FC07FC0, dtype=torch.int32,
                       device=DEV) for _ in range(4)]
    del junk


def _between(t, canary):
    """t on the device as a contiguous view between PAD canary rows of a
    larger buffer -> (buffer, view)."""
    buf = torch.full((t.shape[0] + 2 * PAD,) + tuple(t.shape[1:]), canary,
                     dtype=t.dtype, device=DEV)
    buf[PAD:PAD + t.shape[0]] = t
    return buf, buf[PAD:PAD + t.shape[0]]


def _intact(buf, canary):
    return bool((buf[:PAD] == canary).all()) \
        and bool((buf[-PAD:] == canary).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _u_dev(u):
    return None if u is None else torch.tensor([u], dtype=torch.int32,
                                               device=DEV)


# ------------------------------------------------------------ bucketize_pad

KEY_CANARY = 4242       # a valid-looking key: a read past the view ships it


def _keys(n, seed, world=None):
    """n distinct keys: some above 2^40, one 2^63 - 1, reserved -1 keys
    scattered inside. With ``world`` every key belongs to owner world - 1."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randperm(4 * n + 8, generator=g)[:n].to(torch.int64)
    k[1::3] += 1 << 41
    if world is not None:
        k = k * world + (world - 1)
    elif n > 2:
        k[n // 2] = (1 << 63) - 1
    if n > 4:
        k[4::9] = -1
    if n > 16:
        # the kernel's contract as it stands: every negative key is
        # reserved - never shipped, counted neither in counts nor in overflow
        k[7::31] = -5
        k[16] = -(1 << 63)
    return k


class _Wire:
    """Plan buffers of a test's own capacity, full of junk, each between
    canaries; pos_of is 3 longer than the key buffer."""

    def __init__(self, world, cap, n):
        self.world, self.cap = world, cap
        junk = lambda m, dt: torch.full((m,), 77, dtype=dt)
        self.bufs = {}
        for name, m, dt in (("send_keys", world * cap, torch.int64),
                            ("send_src", world * cap, torch.int32),
                            ("pos_of", n + 3, torch.int32),
                            ("counts", world, torch.int32),
                            ("overflow", 1, torch.int32)):
            self.bufs[name], view = _between(junk(m, dt), 99)
            setattr(self, name, view)
        self.overflow.fill_(5)      # the kernel adds, it never clears

    def call(self, uk, u):
        before = (int(self.overflow.item()), self.pos_of.cpu())
        _ext().bucketize_pad(uk, _u_dev(u), self.world, self.cap,
                             self.send_keys, self.send_src, self.pos_of,
                             self.counts, self.overflow)
        torch.cuda.synchronize()
        wref.check_bucketize(uk, u, self.world, self.cap, self.send_keys,
                             self.send_src, self.pos_of, self.counts,
                             before[0], int(self.overflow.item()),
                             pos_of_before=before[1])
        assert all(_intact(b, 99) for b in self.bufs.values())
        return int(self.overflow.item()) - before[0]


def _cmax(keys, u, world):
    live = keys[:u]
    live = live[live >= 0]
    if not live.numel():
        return 0
    return int(torch.bincount(torch.remainder(live, world),
                              minlength=world).max())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_bucketize_pad(world, n):
    """Roomy, exactly full and one-short buckets for every live count: the
    whole buffer (u_dev None and u_dev == n), a count in the middle whose
    tail holds valid-looking keys, and 0. counts[o] runs past cap and
    overflow grows by what was dropped (pinned as the kernel has it)."""
    keys = _keys(n, 1000 * world + n)
    buf, uk = _between(keys, KEY_CANARY)
    for u in (None, n, n // 2, 0):
        cmax = _cmax(keys, n if u is None else u, world)
        caps = {cmax + 3, max(cmax, 1)}
        if cmax >= 2:
            caps.add(cmax - 1)      # drops one key of every fullest owner
        for cap in sorted(caps):
            dropped = _Wire(world, cap, n).call(uk, u)
            if cap >= cmax:
                assert dropped == 0
            else:
                assert dropped >= 1
    assert _intact(buf, KEY_CANARY) and torch.equal(uk.cpu(), keys)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_bucketize_pad_one_owner_cap_1(world, n):
    keys = _keys(n, 7 * world + n, world=world)
    buf, uk = _between(keys, KEY_CANARY)
    live = int((keys >= 0).sum())
    wire = _Wire(world, 1, n)
    assert wire.call(uk, None) == live - 1
    assert int(wire.counts[world - 1].item()) == live
    assert _intact(buf, KEY_CANARY)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_bucketize_pad_twice_on_one_plan(world):
    """Many keys, then few, into the same buffers: the second result is
    checked from scratch, so nothing of the first call may be left, and
    overflow is the sum of both calls."""
    many = _keys(1025, 50 + world)
    few = _keys(9, 60 + world)
    cap = _cmax(many, 1025, world) - 2
    wire = _Wire(world, cap, 1025)
    first = wire.call(_between(many, KEY_CANARY)[1], None)
    assert first >= 2
    second = wire.call(_between(few, KEY_CANARY)[1], None)
    assert second == 0
    assert int(wire.overflow.item()) == 5 + first
    third = wire.call(_between(many, KEY_CANARY)[1], 700)
    assert int(wire.overflow.item()) == 5 + first + third


def test_bucketize_pad_refuses_wrong_buffers():
    ext = _ext()
    uk = _keys(16, 1).to(DEV)

    def call(send_keys_len=8, counts_dtype=torch.int32):
        z = lambda m, dt: torch.zeros(m, dtype=dt, device=DEV)
        ext.bucketize_pad(uk, None, 2, 4, z(send_keys_len, torch.int64),
                          z(8, torch.int32), z(16, torch.int32),
                          z(2, counts_dtype), z(1, torch.int32))

    call()
    with pytest.raises(RuntimeError, match="buffer sizes"):
        call(send_keys_len=7)
    with pytest.raises(RuntimeError, match="int32"):
        call(counts_dtype=torch.int64)
    torch.cuda.synchronize()


# --------------------------------------------------------------- gather_pad

def _special_floats(shape, g):
    """randn with -0.0, denormals and infinities in it."""
    t = torch.randn(shape, generator=g)
    flat = t.view(-1)
    special = torch.tensor([-0.0, 1e-40, -1e-45, float("inf"),
                            float("-inf")])
    m = min(flat.numel(), special.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:m]] = special[:m]
    return t


@pytest.mark.parametrize("total", [1, 257, 1000])
@pytest.mark.parametrize("dim", DIMS)
def test_gather_pad(dim, total):
    assert total * (dim + 1) % 256       # the last block is partial
    g = torch.Generator().manual_seed(dim * 1000 + total)
    nu = 37
    ugrads = _special_floats((nu, dim), g)
    counts = torch.randint(1, 9, (nu,), generator=g)
    counts[:3] = torch.tensor([1, (1 << 24) - 1, 1 << 24])
    src = torch.randint(-1, nu, (total,), generator=g, dtype=torch.int32)
    if total > 1:
        src[0], src[total // 2], src[-1] = 1, -1, 2
        src[1:4] = torch.tensor([0, 1, 2], dtype=torch.int32)[:total - 1]
    gb, gv = _between(ugrads, 7.0)
    cb, cv = _between(counts, 7)
    sb, sv = _between(src, 5)
    _poison_allocator(total * (dim + 1) * 4)
    out = _ext().gather_pad(gv, cv, sv)
    assert out.shape == (total, dim + 1) and out.dtype == torch.float32
    exp = torch.zeros(total, dim + 1)
    sel = src >= 0
    exp[sel, :dim] = ugrads[src[sel].long()]
    exp[sel, dim] = counts[src[sel].long()].float()
    assert (1 << 24) in exp[:, dim].long().tolist() or total == 1
    assert torch.equal(_bits(out.cpu()), _bits(exp))
    assert bool((_bits(out.cpu())[~sel] == 0).all())    # +0.0, not -0.0
    assert _intact(gb, 7.0) and _intact(cb, 7) and _intact(sb, 5)


# -------------------------------------------------------------- scatter_out

@pytest.mark.parametrize("n_elems", [1, 255, 257])
@pytest.mark.parametrize("dim", DIMS)
def test_scatter_out(dim, n_elems):
    g = torch.Generator().manual_seed(dim * 1000 + n_elems)
    u, R = 40, 200
    rows = _special_floats((R + 5, dim), g)
    # rows no position points at: NaN. A kernel that clamps or multiplies
    # instead of selecting reads one of them for pos -1
    rows[0] = float("nan")
    rows[R:] = float("nan")
    pos = (torch.randperm(R - 1, generator=g)[:u] + 1).to(torch.int32)
    pos[::5] = -1
    inverse = torch.randint(0, u, (n_elems,), generator=g)
    if n_elems > 1:
        inverse[:3] = torch.tensor([0, 1, 1])   # a miss and a duplicate
    rb, rv = _between(rows, 7.0)
    ib, iv = _between(inverse, 0)
    pb, pv = _between(pos, 3)
    _poison_allocator(n_elems * dim * 4)
    out = _ext().scatter_out(rv, iv, pv, n_elems)
    assert out.shape == (n_elems, dim)
    p = pos.long()[inverse]
    exp = torch.where((p >= 0).unsqueeze(1), rows[p.clamp(min=0)],
                      torch.zeros(1, dim))
    assert not bool(exp.isnan().any())
    assert torch.equal(_bits(out.cpu()), _bits(exp))
    assert bool((_bits(out.cpu())[p < 0] == 0).all())
    assert _intact(rb, 7.0) and _intact(ib, 0) and _intact(pb, 3)


# ------------------------------------------------------------ split_payload

@pytest.mark.parametrize("u", [1, 257])
@pytest.mark.parametrize("dim", DIMS)
def test_split_payload(dim, u):
    """The count column holds sums of exactly representable counts up to
    2^24. Behind u_dev the outputs are documented as uninitialised and are
    not looked at."""
    g = torch.Generator().manual_seed(dim * 1000 + u)
    g2c = _special_floats((u, dim + 1), g)
    cnt = torch.randint(0, 1 << 24, (u,), generator=g)
    cnt[-1] = 1 << 24
    if u > 4:
        cnt[:4] = torch.tensor([0, 1, 2, (1 << 24) - 1])
    g2c[:, dim] = cnt.float()
    assert torch.equal(g2c[:, dim].long(), cnt)
    buf, view = _between(g2c, 7.0)
    for live in (None, u, u // 2, 0):
        _poison_allocator(u * dim * 4)
        _poison_allocator(u * 8)
        grads, counts = _ext().split_payload(view, _u_dev(live))
        assert grads.shape == (u, dim) and counts.shape == (u,)
        assert counts.dtype == torch.int64
        m = u if live is None else live
        assert torch.equal(_bits(grads.cpu()[:m]), _bits(g2c[:m, :dim]))
        assert torch.equal(counts.cpu()[:m], cnt[:m])
    assert _intact(buf, 7.0)


# ---------------------------------------------------------------- mask_tail

@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("dim", [1, 9, 65])
def test_mask_tail(dim, n):
    g = torch.Generator().manual_seed(dim * 1000 + n)
    keys = torch.randint(0, 1 << 40, (n,), generator=g)
    keys[0] = (1 << 63) - 1
    grads = _special_floats((n, dim), g)
    counts = torch.randint(1, 1 << 30, (n,), generator=g)
    for live in (None, n, n // 2, 0):
        kb, kv = _between(keys, 7)
        gb, gv = _between(grads, 7.0)
        cb, cv = _between(counts, 7)
        _ext().mask_tail(kv, gv, cv, _u_dev(live))
        m = n if live is None else live
        assert torch.equal(kv.cpu()[:m], keys[:m])
        assert torch.equal(_bits(gv.cpu()[:m]), _bits(grads[:m]))
        assert torch.equal(cv.cpu()[:m], counts[:m])
        assert bool((kv[m:] == -1).all())
        assert bool((_bits(gv.cpu()[m:]) == 0).all())
        assert bool((cv[m:] == 0).all())
        assert _intact(kb, 7) and _intact(gb, 7.0) and _intact(cb, 7)
