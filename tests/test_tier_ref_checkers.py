"""CPU tests of tests/tier_ref.py, the reference side of
tests/test_gpu_tier_kernels.py: the model passes its own checkers on every
case of the GPU grid, every mutant of a tier kernel that the GPU tests are
meant to catch is rejected with the violation that names it, and the table
builder agrees with a dict."""

import pytest
import torch

import tier_ref as ref


def _case(dim, sd, n):
    c = ref.make_case(dim, sd, n,
                      torch.Generator().manual_seed(1000 * dim + sd))
    ref.assert_layout(c)
    return c


def _fault_args(c, live):
    return (c.keys, live, c.table, c.host_w, c.host_s, c.weights, c.state,
            c.slots, c.new_mask)


def _check_fault(c, live, w, s, m, f, host_w=None, host_s=None):
    return ref.check_fault_in(*_fault_args(c, live), w, s, m, f,
                              c.host_w if host_w is None else host_w,
                              c.host_s if host_s is None else host_s)


def _has(fails, prefix):
    return any(f.startswith(prefix) for f in fails)


# ------------------------------------------------------ the model passes

@pytest.mark.parametrize("dim,sd,n", ref.grid())
def test_model_passes_its_checkers(dim, sd, n):
    c = _case(dim, sd, n)
    for live in (None, c.live):
        w, s, m, f = ref.fault_in_reference(*_fault_args(c, live))
        assert _check_fault(c, live, w, s, m, f) == []
        lim = n if live is None else live
        want = sum(1 for i, k in enumerate(c.cls)
                   if i < lim and k in "af")
        assert f == want, (f, want)
    hw, hs = ref.spill_reference(c.spill_cache, c.spill_host, c.weights,
                                 c.state, c.host_w, c.host_s)
    assert ref.check_spill(c.spill_cache, c.spill_host, c.weights, c.state,
                           c.host_w, c.host_s, hw, hs, c.weights,
                           c.state) == []
    o = ref.gather_host_reference(c.keys, c.gather_slots, c.table, c.host_w,
                                  c.out)
    assert ref.check_gather_host(c.keys, c.gather_slots, c.table, c.host_w,
                                 c.out, o, c.host_w) == []


def test_grid_covers_what_it_claims():
    grid = ref.grid()
    for G in (16, 64):
        mine = [c for c in grid if ref.lane_group(c[0]) == G]
        for i in range(4):      # every state layout meets every n
            assert {n for d, sd, n in mine
                    if ref.state_dims(d).index(sd) == i} == set(ref.NS)
        assert any(d > G for d, _, _ in mine), "no second stride trip"
    single = {_case(*c).cls[0] for c in grid if c[2] == 1}
    assert single == set("abcdef")


def test_case_holds_every_class_and_is_not_vacuous():
    c = _case(17, 2, 67)
    assert set(c.cls) == set("abcdef")
    w, s, m, f = ref.fault_in_reference(*_fault_args(c, c.live))
    assert f >= 4 and not ref.bits_equal(w, c.weights)
    # a copied element is identifiable: tier, host row and column
    g = c.cls.index("a")
    hs = ref.probe(c.table, int(c.keys[g]))
    assert w[int(c.slots[g])].tolist() == [
        float((ref.TIER_HOST_W << 19) + hs * 512 + j) for j in range(17)]
    # class c: the host copy differs from the cached row
    g = c.cls.index("c")
    hs = ref.probe(c.table, int(c.keys[g]))
    assert hs >= 0 and not ref.bits_equal(c.host_w[hs],
                                          c.weights[int(c.slots[g])])
    # canaries are NaNs that the bitwise comparison tells apart
    assert bool(torch.isnan(c.weights[0]).all())
    assert ref.bits_equal(c.weights[0], ref.canary(17))
    assert not ref.bits_equal(c.weights[0], torch.full((17,), float("nan")))


# --------------------------------------------------------------- mutants

def _probe_stops_at_mismatch(table, key):
    tk, tv = table
    h = ref._home(key, tk.numel())
    return int(tv[h]) if int(tk[h]) == key else -1


def _probe_no_wrap(table, key):
    tk, tv = table
    for h in range(ref._home(key, tk.numel()), tk.numel()):
        if int(tk[h]) == key:
            return int(tv[h])
        if int(tk[h]) == ref.EMPTY:
            return -1
    return -1


def _fault_mutant(c, live, kind):
    """The model's output with one defect."""
    keys, _, table, host_w, host_s, weights, state, slots, mask = \
        _fault_args(c, live)
    if kind == "ignores_live":
        return ref.fault_in_reference(keys, None, table, host_w, host_s,
                                      weights, state, slots, mask)
    if kind == "ignores_new_mask":
        return ref.fault_in_reference(keys, live, table, host_w, host_s,
                                      weights, state, slots,
                                      torch.ones_like(mask))
    if kind == "probe_stops":
        return ref.fault_in_reference(*_fault_args(c, live),
                                      probe=_probe_stops_at_mismatch)
    if kind == "probe_no_wrap":
        return ref.fault_in_reference(*_fault_args(c, live),
                                      probe=_probe_no_wrap)
    w, s, m, f = ref.fault_in_reference(*_fault_args(c, live))
    copied = slots[(m != mask)]
    G = ref.lane_group(c.dim)
    if kind == "state_skipped":
        s = state.clone()
    elif kind == "first_G_columns":
        w[copied, G:] = weights[copied, G:]
        s[copied, G:] = state[copied, G:]
    elif kind == "shifted":
        w[copied] = torch.roll(w[copied], 1, dims=1)
    elif kind == "mask_not_cleared":
        m = mask.clone()
    elif kind == "faulted_off_by_one":
        f += 1
    else:
        raise KeyError(kind)
    return w, s, m, f


FAULT_MUTANTS = [
    # kind, (dim, sd, n), the violation it must produce
    ("state_skipped", (17, 36, 17), "state: a row that must be copied"),
    ("state_skipped", (65, 2, 67), "state: a row that must be copied"),
    ("first_G_columns", (17, 0, 17), "weights: a row that must be copied"),
    ("first_G_columns", (65, 0, 17), "weights: a row that must be copied"),
    ("first_G_columns", (17, 36, 17), "state: a row that must be copied"),
    ("first_G_columns", (65, 132, 17), "state: a row that must be copied"),
    ("shifted", (17, 0, 17), "weights: a row that must be copied"),
    ("shifted", (65, 65, 17), "weights: a row that must be copied"),
    ("ignores_live", (16, 2, 17), "weights: a row that must not be touched"),
    ("ignores_live", (16, 2, 17), "faulted:"),
    ("mask_not_cleared", (33, 33, 17), "new_mask:"),
    ("ignores_new_mask", (17, 2, 67),
     "weights: a row that must not be touched"),
    ("ignores_new_mask", (17, 2, 67),
     "state: a row that must not be touched"),
    ("probe_stops", (32, 0, 67), "weights: a row that must be copied"),
    ("probe_stops", (32, 0, 67), "new_mask:"),
    ("probe_no_wrap", (64, 64, 67), "weights: a row that must be copied"),
    ("probe_no_wrap", (64, 64, 67), "state: a row that must be copied"),
    ("faulted_off_by_one", (1, 4, 67), "faulted:"),
]


@pytest.mark.parametrize("kind,shape,violation", FAULT_MUTANTS)
def test_fault_in_mutant_rejected(kind, shape, violation):
    c = _case(*shape)
    fails = _check_fault(c, c.live, *_fault_mutant(c, c.live, kind))
    assert _has(fails, violation), (kind, fails)


def test_stale_overwrite_is_what_the_new_mask_mutant_does():
    """The mutant that ignores new_mask replaces a cached row (class c) by
    its older host copy — the one failure the tier must never have."""
    c = _case(17, 2, 67)
    w, s, m, f = _fault_mutant(c, c.live, "ignores_new_mask")
    g = c.cls.index("c")
    hs = ref.probe(c.table, int(c.keys[g]))
    assert ref.bits_equal(w[int(c.slots[g])], c.host_w[hs])
    assert _has(_check_fault(c, c.live, w, s, m, f),
                "weights: a row that must not be touched")
    # that one row alone is enough, and the violation names it
    w, s, m, f = ref.fault_in_reference(*_fault_args(c, c.live))
    w[int(c.slots[g])] = c.host_w[hs]
    fails = _check_fault(c, c.live, w, s, m, f)
    assert fails == ["weights: a row that must not be touched changed "
                     f"(row {int(c.slots[g])})"]


def test_fault_in_writing_a_host_slab_rejected():
    c = _case(16, 16, 67)
    w, s, m, f = ref.fault_in_reference(*_fault_args(c, None))
    hw = c.host_w.clone()
    hw[0, 0] = 1.0
    assert _has(_check_fault(c, None, w, s, m, f, host_w=hw), "host_w: read")
    hs = c.host_s.clone()
    hs[-1, -1] = 1.0
    assert _has(_check_fault(c, None, w, s, m, f, host_s=hs), "host_s: read")


def _gather(c, out):
    return ref.check_gather_host(c.keys, c.gather_slots, c.table, c.host_w,
                                 c.out, out, c.host_w)


def test_gather_host_mutants_rejected():
    c = _case(33, 0, 67)
    kinds = [("h" if s >= 0 else k) for k, s in zip(c.cls, c.gather_slots)]
    # the case mixes cache hits, host hits, unknown keys and key -1
    assert "h" in kinds and "a" in kinds and "b" in kinds and "e" in kinds
    good = ref.gather_host_reference(c.keys, c.gather_slots, c.table,
                                     c.host_w, c.out)
    assert not ref.bits_equal(good, c.out)
    # overwrites a cache hit with the (stale) host copy
    bad = ref.gather_host_reference(c.keys, torch.full_like(c.gather_slots,
                                                            -1),
                                    c.table, c.host_w, c.out)
    assert not ref.bits_equal(bad, good)
    assert _has(_gather(c, bad), "out: a row that must not be touched")
    # zeros for an unknown key over the pre-filled out
    bad = good.clone()
    unknown = [i for i, k in enumerate(kinds) if k == "b"]
    bad[unknown] = 0.0
    assert _has(_gather(c, bad), "out: a row that must not be touched")
    # only the first G columns / a shift
    bad = good.clone()
    bad[:, 16:] = c.out[:, 16:]
    assert _has(_gather(c, bad), "out: a row that must be gathered")
    for p in (_probe_stops_at_mismatch, _probe_no_wrap):
        bad = ref.gather_host_reference(c.keys, c.gather_slots, c.table,
                                        c.host_w, c.out, probe=p)
        assert _has(_gather(c, bad), "out: a row that must be gathered")


def _spill(c, hw, hs, w=None, s=None):
    return ref.check_spill(c.spill_cache, c.spill_host, c.weights, c.state,
                           c.host_w, c.host_s, hw, hs,
                           c.weights if w is None else w,
                           c.state if s is None else s)


def test_spill_mutants_rejected():
    c = _case(65, 132, 67)
    assert int((c.spill_cache < 0).sum()) and int((c.spill_host < 0).sum())
    hw, hs = ref.spill_reference(c.spill_cache, c.spill_host, c.weights,
                                 c.state, c.host_w, c.host_s)
    assert not ref.bits_equal(hw, c.host_w)
    # a pair whose host slot is -1 goes to host row 0
    bad_w, bad_s = hw.clone(), hs.clone()
    g = int(((c.spill_host < 0) & (c.spill_cache >= 0)).nonzero()[0])
    bad_w[0] = c.weights[int(c.spill_cache[g])]
    assert _has(_spill(c, bad_w, hs), "host_w: a row that must not be")
    # writes the cache slab
    w = c.weights.clone()
    w[int(c.spill_cache[g])] = c.host_w[1]
    assert _has(_spill(c, hw, hs, w=w), "weights: read-only")
    s = c.state.clone()
    s[0, 0] = 0.0
    assert _has(_spill(c, hw, hs, s=s), "state: read-only")
    # the state copy is skipped / only G columns
    assert _has(_spill(c, hw, c.host_s), "host_s: a row that must be spilled")
    bad_w = hw.clone()
    bad_w[:, 64:] = c.host_w[:, 64:]
    assert _has(_spill(c, bad_w, hs), "host_w: a row that must be spilled")


# ------------------------------------------------------------ build_table

@pytest.mark.parametrize("cap", [16, 64, 256])
def test_build_table_against_dict(cap):
    g = torch.Generator().manual_seed(cap)
    n = cap // 2
    coll = ref.scr.colliding_keys(cap - 1, [cap - 1, 0], 6)
    keys = torch.cat([coll, ref.scr.full_range_keys(n - 6, g)])
    slots = torch.randperm(4 * n, generator=g)[:n]
    want = dict(zip(keys.tolist(), slots.tolist()))
    assert len(want) == n
    table = ref.build_table(keys, slots, cap)
    tk, tv = table
    assert int((tk != ref.EMPTY).sum()) == n
    for k, v in want.items():
        assert ref.probe(table, k) == v
    absent = ref.scr.colliding_keys(cap - 1, [cap - 1, 0], 12)[6:].tolist()
    absent += [ref.EMPTY, 123456789012345]
    for k in absent:
        assert k not in want and ref.probe(table, k) == -1
    # every key sits between its home and the first empty entry after it
    pos, homes, disp = ref.chain_lengths(tk)
    for p, d in zip(pos.tolist(), disp.tolist()):
        for step in range(d + 1):
            assert int(tk[(p - step) & (cap - 1)]) != ref.EMPTY
    # insertion order decides the layout: the first colliding key is home
    assert int(tk[ref._home(int(coll[0]), cap)]) == int(coll[0])
