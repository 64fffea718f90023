"""Reference side of tests/test_gpu_tier_kernels.py: plain Python and CPU
torch, no GPU.

The capacity tier's three kernels (``k_fault_in``, ``k_spill_rows``,
``k_gather_host``) only probe a hash table and copy rows, so the model here
is exact: every comparison is bitwise and no tolerance appears anywhere.

  - ``build_table`` / ``probe``: an open-addressing table (home =
    ``splitmix64(k) & (cap - 1)``, linear probing, empty marker -1) built in
    insertion order by a Python loop, independent of ``k_ht_lookup``;
  - ``fault_in_reference`` / ``spill_reference`` / ``gather_host_reference``:
    the two-tier model, one row at a time;
  - ``check_fault_in`` / ``check_spill`` / ``check_gather_host``: compare
    every buffer a kernel was handed with the model — rows it must write,
    rows it must not touch, and the read-only operands — and return the list
    of violations (empty = pass);
  - ``make_case``: a hand-made case with every row class (module table
    below), canary rows, permuted slots and per-element codes.

The checkers themselves are tested without a GPU in
tests/test_tier_ref_checkers.py.

Row classes of a case's key vector (``TierCase.cls``):

  a  new (mask 1), key in the host table            -> copied
  b  new, key not in the host table                 -> untouched, mask stays 1
  c  mask 0, key in the host table with OTHER data  -> untouched
  d  slot -1 (key in the host table)                -> untouched
  e  key -1 with mask forced to 1                   -> untouched
  f  position >= live, key in the host, mask 1      -> untouched (copied when
                                                       no device count is given)
"""

from __future__ import annotations

import torch

import sparse_core_ref as scr
from openembedding_amd.core import rng

EMPTY = -1
TV_FILL = 0          # tv of an empty entry: host row 0, always a canary row
CANARY_BITS = 0x7FC0BEEF   # a quiet NaN with a payload

DIMS = [1, 16, 17, 32, 33, 64, 65, 130]   # G=16 up to 32, G=64 above
NS = [1, 5, 17, 67]    # BLOCK 256: 16 rows per block (G=16), 4 (G=64)


def state_dims(dim: int):
    """default, test, adagrad, adam."""
    return [0, 2, dim, 2 * dim + 2]


def case_n(dim: int, sd: int) -> int:
    """Row count of the (dim, sd) case. DIMS holds four dims per G, so for a
    fixed state layout the rotation gives every n to both G values."""
    return NS[(DIMS.index(dim) + state_dims(dim).index(sd)) % len(NS)]


def grid():
    """[(dim, sd, n)] of every kernel case."""
    return [(d, sd, case_n(d, sd)) for d in DIMS for sd in state_dims(d)]


def lane_group(dim: int) -> int:
    """Lanes per row of the three kernels' launchers."""
    return 16 if dim <= 32 else 64


def canary(*shape) -> torch.Tensor:
    return torch.full(shape, CANARY_BITS, dtype=torch.int32).view(
        torch.float32)


def bits_equal(a, b) -> bool:
    return scr.bits_equal(a, b)


def _rows_equal(a, b) -> torch.Tensor:
    """bool [rows]: row-wise bitwise equality of two float32 [rows, w]."""
    if a.shape[1] == 0:
        return torch.ones(a.shape[0], dtype=torch.bool)
    return (a.contiguous().view(torch.int32)
            == b.contiguous().view(torch.int32)).all(dim=1)


# ------------------------------------------------------------ the host map

def _home(key: int, cap: int) -> int:
    k = torch.tensor([key], dtype=torch.int64)
    return int(rng.splitmix64(k)[0]) & (cap - 1)


def build_table(keys, host_slots, cap: int):
    """(tk int64 [cap], tv int32 [cap]): ``keys`` inserted in the order
    given, each at the first empty entry from its home on, wrapping."""
    assert cap > 0 and cap & (cap - 1) == 0
    tk = [EMPTY] * cap
    tv = [TV_FILL] * cap
    for k, v in zip([int(k) for k in keys], [int(v) for v in host_slots]):
        assert k != EMPTY
        h = _home(k, cap)
        for _ in range(cap):
            if tk[h] == EMPTY or tk[h] == k:
                break
            h = (h + 1) & (cap - 1)
        else:
            raise AssertionError("table full")
        tk[h], tv[h] = k, v
    return (torch.tensor(tk, dtype=torch.int64),
            torch.tensor(tv, dtype=torch.int32))


def probe(table, key: int) -> int:
    """Host slot of ``key`` or -1."""
    tk, tv = table
    cap = tk.numel()
    if key == EMPTY:
        return -1
    h = _home(key, cap)
    for _ in range(cap):
        cur = int(tk[h])
        if cur == key:
            return int(tv[h])
        if cur == EMPTY:
            return -1
        h = (h + 1) & (cap - 1)
    return -1


def chain_lengths(tk):
    """Displacement of every occupied entry from its key's home."""
    cap = tk.numel()
    pos = torch.arange(cap)[tk != EMPTY]
    homes = rng.splitmix64(tk[tk != EMPTY]) & (cap - 1)
    return pos, homes, (pos - homes) & (cap - 1)


# --------------------------------------------------------------- the model

def _state(state, rows):
    return state if state is not None else torch.zeros(rows, 0)


def fault_in_reference(keys, live, table, host_w, host_s, weights, state,
                       slots, new_mask, probe=probe):
    """(weights', state', new_mask', n_faulted). ``live`` None = all."""
    n = keys.numel()
    live = n if live is None else int(live)
    w = weights.clone()
    s = _state(state, weights.shape[0]).clone()
    m = new_mask.clone()
    faulted = 0
    for g in range(n):
        if g >= live or int(m[g]) == 0 or int(slots[g]) < 0:
            continue
        k = int(keys[g])
        if k == EMPTY:
            continue
        hs = probe(table, k)
        if hs < 0:
            continue
        w[int(slots[g])] = host_w[hs]
        if s.shape[1]:
            s[int(slots[g])] = host_s[hs]
        m[g] = 0
        faulted += 1
    return w, s, m, faulted


def spill_reference(cache_slots, host_slots, weights, state, host_w, host_s):
    """(host_w', host_s')."""
    hw = host_w.clone()
    hs = _state(host_s, host_w.shape[0]).clone()
    for c, h in zip(cache_slots.tolist(), host_slots.tolist()):
        if c < 0 or h < 0:
            continue
        hw[h] = weights[c]
        if hs.shape[1]:
            hs[h] = state[c]
    return hw, hs


def gather_host_reference(keys, cache_slots, table, host_w, out,
                          probe=probe):
    o = out.clone()
    for g in range(keys.numel()):
        if int(cache_slots[g]) >= 0:
            continue
        k = int(keys[g])
        if k == EMPTY:
            continue
        hs = probe(table, k)
        if hs < 0:
            continue
        o[g] = host_w[hs]
    return o


# ------------------------------------------------------------ the checkers

def _compare(name, got, want, before, fails, written="written"):
    """Rows the model changed must match it; all others must be unchanged."""
    if got.shape != want.shape:
        fails.append(f"{name}: shape {tuple(got.shape)} != "
                     f"{tuple(want.shape)}")
        return
    ok = _rows_equal(got, want)
    moved = ~_rows_equal(want, before)
    if bool((~ok & moved).any()):
        r = int((~ok & moved).nonzero()[0])
        fails.append(f"{name}: a row that must be {written} differs from "
                     f"its source (row {r})")
    if bool((~ok & ~moved).any()):
        r = int((~ok & ~moved).nonzero()[0])
        fails.append(f"{name}: a row that must not be touched changed "
                     f"(row {r})")


def _readonly(name, got, before, fails):
    if got is None and (before is None or before.shape[1] == 0):
        return
    if not bits_equal(got, before):
        fails.append(f"{name}: read-only operand changed")


def check_fault_in(keys, live, table, host_w, host_s, weights, state, slots,
                   new_mask, got_weights, got_state, got_mask, got_faulted,
                   got_host_w, got_host_s):
    """Violations of one ``fault_in`` call. The first nine arguments are the
    operands BEFORE the call, ``got_*`` what came back; ``got_faulted`` is
    the counter's increment."""
    fails = []
    w, s, m, faulted = fault_in_reference(keys, live, table, host_w, host_s,
                                          weights, state, slots, new_mask)
    s0 = _state(state, weights.shape[0])
    _compare("weights", got_weights, w, weights, fails, "copied")
    _compare("state", _state(got_state, weights.shape[0]), s, s0, fails,
             "copied")
    if not torch.equal(got_mask, m):
        g = int((got_mask != m).nonzero()[0])
        fails.append(f"new_mask: position {g} is {int(got_mask[g])}, "
                     f"must be {int(m[g])}")
    if int(got_faulted) != faulted:
        fails.append(f"faulted: counted {int(got_faulted)}, must be "
                     f"{faulted}")
    _readonly("host_w", got_host_w, host_w, fails)
    _readonly("host_s", got_host_s, host_s, fails)
    return fails


def check_spill(cache_slots, host_slots, weights, state, host_w, host_s,
                got_host_w, got_host_s, got_weights, got_state):
    fails = []
    hw, hs = spill_reference(cache_slots, host_slots, weights, state, host_w,
                             host_s)
    _compare("host_w", got_host_w, hw, host_w, fails, "spilled")
    _compare("host_s", _state(got_host_s, host_w.shape[0]), hs,
             _state(host_s, host_w.shape[0]), fails, "spilled")
    _readonly("weights", got_weights, weights, fails)
    _readonly("state", got_state, state, fails)
    return fails


def check_gather_host(keys, cache_slots, table, host_w, out, got_out,
                      got_host_w):
    fails = []
    o = gather_host_reference(keys, cache_slots, table, host_w, out)
    _compare("out", got_out, o, out, fails, "gathered")
    _readonly("host_w", got_host_w, host_w, fails)
    return fails


# ---------------------------------------------------------------- the case

TIER_HOST_W, TIER_HOST_S, TIER_CACHE_W, TIER_CACHE_S, TIER_OUT = 1, 2, 3, 4, 5


def coded(tier: int, rows, width: int) -> torch.Tensor:
    """float32 [len(rows), width] holding tier * 2^19 + row * 2^9 + column:
    exact in float32 and distinct per (tier, row, column)."""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    assert width < 512 and (rows.numel() == 0 or int(rows.max()) < 1024)
    code = (tier << 19) + rows.view(-1, 1) * 512 + torch.arange(width)
    return code.to(torch.float32)


class TierCase:
    """See ``make_case``."""


def make_case(dim: int, sd: int, n: int, g) -> TierCase:
    """A hand-made tier case of ``n`` positions; ``g`` is a torch Generator.

    Cache slab (R rows) and host slab (H rows) both have more rows than the
    case names; unnamed rows — always including the first and the last — hold
    a NaN canary. Named rows hold ``coded`` values. ``slots`` is a random
    selection of cache rows, ``host_slots`` an unrelated one of host rows."""
    c = TierCase()
    c.dim, c.sd, c.n = dim, sd, n
    c.live = n - max(1, n // 4)          # < n; 0 for n == 1
    rot = dim + sd
    if n == 1:
        # the grid's n == 1 cases fall on every dim once per G: by dim
        # they cycle through all six classes
        c.cls = ["abcdef"[(DIMS.index(dim) if dim in DIMS else rot) % 6]]
    else:
        c.cls = ["abcde"[(i + rot) % 5] if i < c.live else "f"
                 for i in range(n)]
    in_host = [k in "acdf" for k in c.cls]
    n_host = sum(in_host)
    n_table = 8 + n_host
    cap = 16
    while cap < 2 * n_table:
        cap *= 2
    c.cap = cap
    # colliding keys: two homes at the table's end (their chain wraps to
    # entry 0) and one in the middle. Four fillers each go in first, so
    # that the case's own colliding keys sit deep in a chain.
    wrap = scr.colliding_keys(cap - 1, [cap - 2, cap - 1], 12).tolist()
    mid = scr.colliding_keys(cap - 1, [5], 12).tolist()
    fillers = wrap[:4] + mid[:4]
    deep_present = [k for pair in zip(wrap[4:8], mid[4:8]) for k in pair]
    deep_absent = [k for pair in zip(wrap[8:], mid[8:]) for k in pair]
    plain = [int(k) for k in scr.full_range_keys(n + 8, g)
             if int(k) not in set(wrap + mid)]
    keys = []
    for k in c.cls:
        if k == "e":
            keys.append(EMPTY)
        elif k == "b":
            keys.append(deep_absent.pop(0) if deep_absent else plain.pop(0))
        else:
            keys.append(deep_present.pop(0) if deep_present
                        else plain.pop(0))
    c.keys = torch.tensor(keys, dtype=torch.int64)
    distinct = [k for k in keys if k != EMPTY]
    assert len(set(distinct)) == len(distinct)
    table_keys = fillers + [k for k, h in zip(keys, in_host) if h]
    assert len(table_keys) == n_table

    # host slab: rows 1 .. H-2 in random order, first and last stay canaries
    H = 2 * n_table + 4
    c.host_rows = H
    hperm = (torch.randperm(H - 2, generator=g) + 1)
    c.table_slots = hperm[:n_table]
    c.table_keys = torch.tensor(table_keys, dtype=torch.int64)
    c.table = build_table(table_keys, c.table_slots, cap)
    c.host_w = canary(H, dim)
    c.host_w[c.table_slots] = coded(TIER_HOST_W, c.table_slots, dim)
    c.host_s = None
    if sd:
        c.host_s = canary(H, sd)
        c.host_s[c.table_slots] = coded(TIER_HOST_S, c.table_slots, sd)

    # cache slab
    R = 2 * n + 5
    c.R = R
    c.slots = (torch.randperm(R - 2, generator=g) + 1)[:n]
    named = c.slots.clone()
    c.slots[torch.tensor([k == "d" for k in c.cls])] = -1
    c.weights = canary(R, dim)
    c.weights[named] = coded(TIER_CACHE_W, named, dim)
    c.state = torch.zeros(R, 0)
    if sd:
        c.state = canary(R, sd)
        c.state[named] = coded(TIER_CACHE_S, named, sd)
    c.new_mask = torch.tensor([0 if k == "c" else 1 for k in c.cls],
                              dtype=torch.uint8)

    # read-only gather over the same keys: c rows are cache hits whose key
    # is also in the host (stale copy), every other b row a cache hit too
    c.gather_slots = torch.tensor(
        [int(s) if (k == "c" or (k == "b" and i % 2 == 0)) else -1
         for i, (k, s) in enumerate(zip(c.cls, named))], dtype=torch.int64)
    c.out = coded(TIER_OUT, torch.arange(n), dim)     # sentinel pattern

    # spill pairs: cache rows of the case against host rows unrelated to the
    # table's (never host row 0), with -1 entries on either side
    c.spill_cache = c.slots.clone()
    c.spill_host = (torch.randperm(H - 2, generator=g) + 1)[:n]
    c.spill_host[torch.arange(n) % 5 == 1] = -1
    return c


def assert_layout(c: TierCase) -> None:
    """The built table has a probe chain of length >= 4 and a chain that
    wraps from the last entry to entry 0."""
    tk = c.table[0]
    pos, homes, disp = chain_lengths(tk)
    assert int(disp.max()) >= 3, "no probe chain of length >= 4"
    wrapped = (pos < 8) & (homes >= c.cap - 2)
    assert bool(wrapped.any()), "no chain wraps past the table end"
    assert int((tk != EMPTY).sum()) == c.table_keys.numel()
