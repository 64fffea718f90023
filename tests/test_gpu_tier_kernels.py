"""The capacity tier's kernels through their bindings — ``fault_in``,
``spill_rows`` and ``gather_host`` — against the exact two-tier model of
tests/tier_ref.py (tested on its own, without a GPU, in
tests/test_tier_ref_checkers.py).

The kernels probe a table and copy rows, so every comparison is bitwise:
the rows a kernel must write, the rows it must not touch (canary rows, rows
behind a -1 slot, rows past the device count, cached rows whose host copy is
stale) and the operands it only reads. The grid covers both lane-group
widths (G=16 up to dim 32, G=64 above), their boundary, more than one stride
trip for each, the four state layouts (none, 2, dim, 2*dim+2) and row counts
on both sides of a block.

The last section holds the refusals: every mis-shaped call of the three
bindings raises before anything is launched.
"""

import pytest
import torch

import tier_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _case(dim, sd, n):
    c = ref.make_case(dim, sd, n,
                      torch.Generator().manual_seed(1000 * dim + sd))
    ref.assert_layout(c)
    return c


def _pin(t):
    return None if t is None else t.clone().pin_memory()


def _count(k):
    return torch.tensor([k], dtype=torch.int32, device=DEV)


def _table(table):
    return table[0].to(DEV), table[1].to(DEV)


def _fault_in(keys, live, table, host_w, host_s, weights, state, slots,
              new_mask, faulted0=0):
    """One ``fault_in`` launch from CPU operands; returns the checker's
    violations and what came back."""
    tk, tv = _table(table)
    hw, hs = _pin(host_w), _pin(host_s)
    W, S, M = weights.to(DEV), state.to(DEV), new_mask.to(DEV)
    F = _count(faulted0)
    _ext().fault_in(keys.to(DEV), None if live is None else _count(live),
                    tk, tv, hw, hs, W, S, slots.to(DEV), M, F)
    torch.cuda.synchronize()
    got = (W.cpu(), S.cpu(), M.cpu(), int(F.item()) - faulted0)
    fails = ref.check_fault_in(keys, live, table, host_w, host_s, weights,
                               state, slots, new_mask, *got, hw, hs)
    return fails, got


GRID = ref.grid()


# ================================================================ fault_in

@pytest.mark.parametrize("dim,sd,n", GRID)
def test_fault_in(dim, sd, n):
    """All positions live (no device count), then a device count
    ``live < n``: rows of class a (and f, when nothing bounds them) are the
    host rows bit for bit, everything else is untouched, the mask is cleared
    exactly for the copied rows and the counter grows by their number."""
    c = _case(dim, sd, n)
    for live in (None, c.live):
        fails, got = _fault_in(c.keys, live, c.table, c.host_w, c.host_s,
                               c.weights, c.state, c.slots, c.new_mask)
        assert not fails, f"live={live}: " + "\n".join(fails)
        lim = n if live is None else live
        assert got[3] == sum(1 for i, k in enumerate(c.cls)
                             if i < lim and k in "af")


@pytest.mark.parametrize("dim,sd,n", [g for g in GRID if g[2] >= 5])
def test_fault_in_counter_accumulates(dim, sd, n):
    """Two calls in a row on disjoint key halves with ONE counter that
    starts at a non-zero value: it ends at exactly initial + count_1 +
    count_2 (accumulated, not reset, once per row and not once per lane),
    and the table holds what the model gives for the whole batch."""
    c = _case(dim, sd, n)
    ext = _ext()
    tk, tv = _table(c.table)
    hw, hs = _pin(c.host_w), _pin(c.host_s)
    W, S = c.weights.to(DEV), c.state.to(DEV)
    M = c.new_mask.to(DEV)
    keys, slots = c.keys.to(DEV), c.slots.to(DEV)
    initial = 1000003
    F = _count(initial)
    h = n // 2
    counts = []
    for lo, hi in ((0, h), (h, n)):
        ext.fault_in(keys[lo:hi], None, tk, tv, hw, hs, W, S, slots[lo:hi],
                     M[lo:hi], F)
        counts.append(ref.fault_in_reference(
            c.keys[lo:hi], None, c.table, c.host_w, c.host_s, c.weights,
            c.state, c.slots[lo:hi], c.new_mask[lo:hi])[3])
    torch.cuda.synchronize()
    assert sum(counts) > 0
    assert int(F.item()) == initial + counts[0] + counts[1]
    fails = ref.check_fault_in(c.keys, None, c.table, c.host_w, c.host_s,
                               c.weights, c.state, c.slots, c.new_mask,
                               W.cpu(), S.cpu(), M.cpu(),
                               int(F.item()) - initial, hw, hs)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dim,sd,n", [(17, 36, 67), (65, 2, 67)])
def test_fault_in_with_a_table_built_like_the_shard(dim, sd, n):
    """The host map built the way ``_spill`` and ``_host_maybe_rehash`` do
    it — ``ht_lookup(insert=True)``, then ``ht_rehash`` into a table twice
    as large — serves ``fault_in`` like the model's own table."""
    c = _case(dim, sd, n)
    ext = _ext()
    nt = c.table_keys.numel()
    tk = torch.full((c.cap,), -1, dtype=torch.int64, device=DEV)
    tv = torch.zeros(c.cap, dtype=torch.int32, device=DEV)
    nrows = torch.zeros(1, dtype=torch.int32, device=DEV)
    slot_keys = torch.zeros(c.host_rows, dtype=torch.int64, device=DEV)
    hslots, _ = ext.ht_lookup(tk, tv, c.table_keys.to(DEV), nrows, slot_keys,
                              True, None)
    hslots = hslots.cpu()
    assert torch.equal(torch.sort(hslots)[0], torch.arange(nt))
    tk2 = torch.empty(2 * c.cap, dtype=torch.int64, device=DEV)
    tv2 = torch.empty(2 * c.cap, dtype=torch.int32, device=DEV)
    ext.ht_rehash(tk, tv, tk2, tv2)
    # the slab laid out by the slots the device handed out
    host_w = ref.canary(c.host_rows, dim)
    host_w[hslots] = c.host_w[c.table_slots]
    host_s = ref.canary(c.host_rows, sd)
    host_s[hslots] = c.host_s[c.table_slots]
    model_table = ref.build_table(c.table_keys, hslots, 2 * c.cap)
    hw, hs = _pin(host_w), _pin(host_s)
    W, S, M = c.weights.to(DEV), c.state.to(DEV), c.new_mask.to(DEV)
    F = _count(0)
    ext.fault_in(c.keys.to(DEV), _count(c.live), tk2, tv2, hw, hs, W, S,
                 c.slots.to(DEV), M, F)
    torch.cuda.synchronize()
    fails = ref.check_fault_in(c.keys, c.live, model_table, host_w, host_s,
                               c.weights, c.state, c.slots, c.new_mask,
                               W.cpu(), S.cpu(), M.cpu(), int(F.item()),
                               hw, hs)
    assert not fails, "\n".join(fails)
    assert int(F.item()) > 0


# ============================================================== spill_rows

@pytest.mark.parametrize("dim,sd,n", GRID)
def test_spill_rows_and_round_trip(dim, sd, n):
    """Spill with -1 entries on either side (``host_s=None`` without
    state), then fault the same keys back into a fresh cache slab at other
    slots: the round trip reproduces every spilled row bit for bit."""
    c = _case(dim, sd, n)
    ext = _ext()
    hw, hs = _pin(c.host_w), _pin(c.host_s)
    W, S = c.weights.to(DEV), c.state.to(DEV)
    ext.spill_rows(c.spill_cache.to(DEV), c.spill_host.to(DEV), W, S, hw, hs)
    torch.cuda.synchronize()
    fails = ref.check_spill(c.spill_cache, c.spill_host, c.weights, c.state,
                            c.host_w, c.host_s, hw, hs, W.cpu(), S.cpu())
    assert not fails, "\n".join(fails)

    valid = (c.spill_cache >= 0) & (c.spill_host >= 0) & (c.keys != ref.EMPTY)
    table = ref.build_table(c.keys[valid], c.spill_host[valid], c.cap)
    g = torch.Generator().manual_seed(n)
    R2 = 3 * n + 4
    slots2 = (torch.randperm(R2 - 2, generator=g) + 1)[:n]
    host_w1 = hw.clone()
    host_s1 = None if hs is None else hs.clone()
    fails, got = _fault_in(c.keys, None, table, host_w1, host_s1,
                           ref.canary(R2, dim),
                           ref.canary(R2, sd) if sd else torch.zeros(R2, 0),
                           slots2, torch.ones(n, dtype=torch.uint8))
    assert not fails, "round trip: " + "\n".join(fails)
    w2, s2, m2, count = got
    assert count == int(valid.sum())
    assert ref.bits_equal(w2[slots2[valid]], c.weights[c.spill_cache[valid]])
    assert ref.bits_equal(s2[slots2[valid]], c.state[c.spill_cache[valid]])
    assert torch.equal(m2 == 0, valid)


# ============================================================= gather_host

@pytest.mark.parametrize("dim,sd,n", [g for g in GRID if g[1] in (0, 2)])
def test_gather_host(dim, sd, n):
    """``out`` arrives holding a sentinel pattern: cache hits, unknown keys
    and the key -1 keep it, host hits get the host row. (The kernel has no
    state operand; two cases per dim give it two row counts.)"""
    c = _case(dim, sd, n)
    tk, tv = _table(c.table)
    hw = _pin(c.host_w)
    out = c.out.to(DEV)
    _ext().gather_host(c.keys.to(DEV), c.gather_slots.to(DEV), tk, tv, hw,
                       out)
    torch.cuda.synchronize()
    fails = ref.check_gather_host(c.keys, c.gather_slots, c.table, c.host_w,
                                  c.out, out.cpu(), hw)
    assert not fails, "\n".join(fails)


# ================================================================ refusals

class _Args:
    """Valid operands of the three bindings for one case, on the device."""

    def __init__(self, dim=17, sd=36, n=5):
        c = self.c = _case(dim, sd, n)
        self.keys, self.slots = c.keys.to(DEV), c.slots.to(DEV)
        self.tk, self.tv = _table(c.table)
        self.hw, self.hs = _pin(c.host_w), _pin(c.host_s)
        self.W, self.S = c.weights.to(DEV), c.state.to(DEV)
        self.M = c.new_mask.to(DEV)
        self.F = _count(0)
        self.u = _count(c.live)
        self.hslots = c.spill_host.to(DEV)
        self.gslots = c.gather_slots.to(DEV)
        self.out = c.out.to(DEV)

    def fault_in(self, **kw):
        a = dict(keys=self.keys, u_dev=self.u, htk=self.tk, htv=self.tv,
                 host_w=self.hw, host_s=self.hs, weights=self.W,
                 state=self.S, slots=self.slots, new_mask=self.M,
                 faulted=self.F)
        a.update(kw)
        _ext().fault_in(*a.values())

    def spill_rows(self, **kw):
        a = dict(cache_slots=self.slots, host_slots=self.hslots,
                 weights=self.W, state=self.S, host_w=self.hw,
                 host_s=self.hs)
        a.update(kw)
        _ext().spill_rows(*a.values())

    def gather_host(self, **kw):
        a = dict(keys=self.keys, cache_slots=self.gslots, htk=self.tk,
                 htv=self.tv, host_w=self.hw, out=self.out)
        a.update(kw)
        _ext().gather_host(*a.values())

    def untouched(self):
        torch.cuda.synchronize()
        c = self.c
        return (ref.bits_equal(self.W.cpu(), c.weights)
                and ref.bits_equal(self.S.cpu(), c.state)
                and ref.bits_equal(self.hw, c.host_w)
                and ref.bits_equal(self.hs, c.host_s)
                and ref.bits_equal(self.out.cpu(), c.out)
                and torch.equal(self.M.cpu(), c.new_mask)
                and int(self.F.item()) == 0)


def _wider(t, by=1):
    return torch.zeros(t.shape[0], t.shape[1] + by, dtype=t.dtype)


def _bad_fault_in(a):
    i32 = torch.int32
    return {
        "keys on the host": dict(keys=a.keys.cpu()),
        "keys int32": dict(keys=a.keys.to(i32)),
        "u_dev int64": dict(u_dev=a.u.long()),
        "u_dev of two": dict(u_dev=torch.zeros(2, dtype=i32, device=DEV)),
        "u_dev on the host": dict(u_dev=a.u.cpu()),
        "htk int32": dict(htk=a.tk.to(i32)),
        "htk on the host": dict(htk=a.tk.cpu()),
        "table size not a power of two": dict(htk=a.tk[:24], htv=a.tv[:24]),
        "htv shorter than htk": dict(htv=a.tv[:16]),
        "htv int64": dict(htv=a.tv.long()),
        "host_w unpinned": dict(host_w=a.c.host_w.clone()),
        "host_w on the device": dict(host_w=a.hw.to(DEV)),
        "host_w wider": dict(host_w=_wider(a.hw).pin_memory()),
        "host_w narrower": dict(host_w=a.hw[:, :16].contiguous()
                                .pin_memory()),
        "host_w float64": dict(host_w=a.hw.double().pin_memory()),
        "host_s missing": dict(host_s=None),
        "host_s unpinned": dict(host_s=a.c.host_s.clone()),
        "host_s wider": dict(host_s=_wider(a.hs, 2).pin_memory()),
        "host_s as wide as dim": dict(host_s=a.hs[:, :17].contiguous()
                                      .pin_memory()),
        "weights on the host": dict(weights=a.W.cpu()),
        "weights float64": dict(weights=a.W.double()),
        "weights not contiguous": dict(weights=a.W.t().contiguous().t()),
        "state float64": dict(state=a.S.double()),
        "state with fewer rows": dict(state=a.S[:3]),
        "state on the host": dict(state=a.S.cpu()),
        "slots shorter": dict(slots=a.slots[:4]),
        "slots longer": dict(slots=torch.cat([a.slots, a.slots])),
        "slots int32": dict(slots=a.slots.to(i32)),
        "new_mask shorter": dict(new_mask=a.M[:4]),
        "new_mask bool": dict(new_mask=a.M.bool()),
        "new_mask on the host": dict(new_mask=a.M.cpu()),
        "faulted int64": dict(faulted=a.F.long()),
        "faulted of two": dict(faulted=torch.zeros(2, dtype=i32,
                                                   device=DEV)),
        "faulted on the host": dict(faulted=a.F.cpu()),
    }


def _bad_spill_rows(a):
    return {
        "cache_slots int32": dict(cache_slots=a.slots.to(torch.int32)),
        "cache_slots on the host": dict(cache_slots=a.slots.cpu()),
        "host_slots shorter": dict(host_slots=a.hslots[:4]),
        "host_slots on the host": dict(host_slots=a.hslots.cpu()),
        "host_slots int32": dict(host_slots=a.hslots.to(torch.int32)),
        "host_w unpinned": dict(host_w=a.c.host_w.clone()),
        "host_w wider": dict(host_w=_wider(a.hw).pin_memory()),
        "host_w float64": dict(host_w=a.hw.double().pin_memory()),
        "host_s missing": dict(host_s=None),
        "host_s unpinned": dict(host_s=a.c.host_s.clone()),
        "host_s narrower": dict(host_s=a.hs[:, :35].contiguous()
                                .pin_memory()),
        "weights float64": dict(weights=a.W.double()),
        "weights on the host": dict(weights=a.W.cpu()),
        "state float64": dict(state=a.S.double()),
        "state with fewer rows": dict(state=a.S[:3]),
    }


def _bad_gather_host(a):
    return {
        "keys int32": dict(keys=a.keys.to(torch.int32)),
        "cache_slots shorter": dict(cache_slots=a.gslots[:4]),
        "cache_slots on the host": dict(cache_slots=a.gslots.cpu()),
        "table size not a power of two": dict(htk=a.tk[:24], htv=a.tv[:24]),
        "htv shorter than htk": dict(htv=a.tv[:16]),
        "htv int64": dict(htv=a.tv.long()),
        "host_w unpinned": dict(host_w=a.c.host_w.clone()),
        "host_w wider than out": dict(host_w=_wider(a.hw).pin_memory()),
        "out narrower than host_w": dict(out=a.out[:, :16].contiguous()),
        "out with fewer rows": dict(out=a.out[:4]),
        "out on the host": dict(out=a.out.cpu()),
        "out float64": dict(out=a.out.double()),
    }


@pytest.mark.parametrize("binding,bad", [
    ("fault_in", _bad_fault_in), ("spill_rows", _bad_spill_rows),
    ("gather_host", _bad_gather_host)])
def test_mis_shaped_calls_are_refused(binding, bad):
    """Each mis-shaped call raises, and — the check coming before the
    launch — leaves every operand as it was. The valid call goes through."""
    a = _Args()
    assert a.c.cap == 32 and a.c.dim == 17 and a.c.sd == 36
    not_refused = []
    for name, kw in bad(a).items():
        try:
            getattr(a, binding)(**kw)
        except RuntimeError:
            continue
        not_refused.append(name)
    assert not not_refused, f"{binding} accepted: {not_refused}"
    assert a.untouched(), "a refused call wrote something"
    getattr(a, binding)()
    assert not a.untouched()


def test_state_free_call_takes_the_empty_state_as_the_shard_passes_it():
    """Without optimizer state the shard passes its [R, 0] state tensor and
    ``host_s=None``; a zero-width ``host_s`` is accepted too, any other
    width is not."""
    a = _Args(17, 0, 5)
    assert a.S.shape == (a.c.R, 0) and a.hs is None
    a.fault_in()
    a.spill_rows()
    a.fault_in(host_s=torch.zeros(a.c.host_rows, 0))
    with pytest.raises(RuntimeError, match="host_s"):
        a.fault_in(host_s=torch.zeros(a.c.host_rows, 2).pin_memory())
    with pytest.raises(RuntimeError, match="host_s"):
        a.spill_rows(host_s=torch.zeros(a.c.host_rows, 2).pin_memory())
