"""The fused-MLP and CTR-head references of tests/mlp_ref.py, tested on the
CPU: they equal float64 autograd where nothing rounds, an exact emulation
of the kernels equals them on the integer cases while every mutant it
exists for does not, and the interval check keeps an fp32 evaluation of
the same chain inside while it rejects its mutants and stays non-vacuous.

The emulations below are the kernels' arithmetic written once more, in
float64 on integer data (exact, like the kernels' fp32 on that data) and
in float32 on random data, with one switch per mutant."""

import functools

import pytest
import torch

import mlp_ref as mr

f64 = torch.float64
SHAPE = (131, 400, 247)            # M, H, K0; K0p = 256


@functools.lru_cache(maxsize=None)
def _int():
    return mr.int_case(*SHAPE)


@functools.lru_cache(maxsize=None)
def _float():
    return mr.float_case(*SHAPE)


# ------------------------------------------------------------- roundings

def _bits(t):
    f = t.to(torch.float32).contiguous()
    assert torch.equal(f.to(t.dtype), t)
    return f.view(torch.int32)


trunc = mr.trunc_bf16


def half_away(t):
    """fp32 -> bf16, ties away from zero: add half an ulp to the
    magnitude, then drop the low bits."""
    return ((_bits(t) + 0x8000) & -65536).view(torch.float32).to(t.dtype)


def test_rounding_helpers():
    t = torch.tensor([257.0, 259.0, 258.5, -257.0, -259.0, 3.0, 0.0],
                     dtype=f64)
    assert mr.bf16_rne(t).tolist() == [256, 260, 258, -256, -260, 3, 0]
    assert trunc(t).tolist() == [256, 258, 258, -256, -258, 3, 0]
    assert half_away(t).tolist() == [258, 260, 258, -258, -260, 3, 0]
    assert mr.tie_share(t[:2]) == 1.0 and mr.inexact_share(t[:3]) == 1.0
    assert mr.tie_share(t[2:3]) == 0.0 and mr.inexact_share(t[5:]) == 0.0


# ------------------------------------------------------------ emulations

def emu_fwd(c, rnd=mr.bf16_rne, dtype=f64, drop=None, w2_t=False,
            bias_after=False, bias_shift=0):
    """k_mlp3_fwd's arithmetic: a1, a2, a3, out. ``drop`` = (layer, n, k)
    zeroes one weight element; ``bias_shift`` reads the bias of the
    column that many places on (a neighbouring 16-column chunk)."""
    ws = [c.w1.clone(), c.w2.t().clone() if w2_t else c.w2.clone(),
          c.w3.clone()]
    if drop is not None:
        ws[drop[0]][drop[1], drop[2]] = 0
    a, acts = c.x0.to(dtype), []
    for w, b in zip(ws, (c.b1, c.b2, c.b3)):
        b = torch.roll(b, -bias_shift).to(dtype)
        z = a @ w.to(dtype).t()
        if bias_after:
            a = torch.relu(rnd(z.to(f64)).to(dtype) + b)
        else:
            a = torch.relu(z + b)
        a = rnd(a.to(f64)).to(dtype)
        acts.append(a.to(f64))
    out = a @ c.w4.to(dtype) + c.b4.to(dtype) + c.partial.to(dtype)
    return acts + [out.to(f64)]


def emu_bwd(c, rnd=mr.bf16_rne, ge_mask=False, mask_dz3=True):
    """k_mlp3_bwd's arithmetic from the oracle's activations."""
    on = (lambda a: a >= 0) if ge_mask else (lambda a: a > 0)
    dz3 = c.dout.unsqueeze(1) * c.w4.unsqueeze(0)
    dz3 = rnd(dz3 * on(c.a3) if mask_dz3 else dz3)
    dz2 = rnd((dz3 @ c.w3) * on(c.a2))
    dz1 = rnd((dz2 @ c.w2) * on(c.a1))
    return [dz3, dz2, dz1, rnd(dz1 @ c.w1)]


def emu_wgrad(c, two_roundings=False, leak_pad=False):
    """k_mlp3_wgrad + finisher: dw1..dw3 after one call."""
    out = []
    for i, (dz, x, base) in enumerate(zip(c.dz, c.xs, c.base)):
        if i == 0 and leak_pad:
            # the finisher without its ``col >= K0`` test: scratch row r
            # is K0p wide and folds into the K0-wide dw1 at r * K0 + col
            full = dz.t() @ c.x0                               # [H, K0p]
            flat = torch.zeros(c.H * c.K0 + c.K0p, dtype=f64)
            idx = (torch.arange(c.H).unsqueeze(1) * c.K0
                   + torch.arange(c.K0p).unsqueeze(0))
            flat.index_add_(0, idx.reshape(-1), full.reshape(-1))
            p = flat[:c.H * c.K0].view(c.H, c.K0)
        else:
            p = dz.t() @ x
        out.append(mr.bf16_rne(base + mr.bf16_rne(p)) if two_roundings
                   else mr.bf16_rne(base + p))
    return out


def _same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


# ----------------------------------------------------- oracle == autograd

def test_oracle_equals_autograd_where_nothing_rounds():
    # small enough that every activation and grad is a bf16 integer:
    # then the oracle's roundings are identities and it IS the MLP
    M, H, K0 = 9, 16, 5
    c = mr.int_case(M, H, K0, seed=3)
    lin = torch.nn.Linear
    net = torch.nn.Sequential(lin(K0, H), torch.nn.ReLU(), lin(H, H),
                              torch.nn.ReLU(), lin(H, H), torch.nn.ReLU(),
                              lin(H, 1)).to(f64)
    ws = [c.w1, c.w2, c.w3, c.w4.view(1, H)]
    bs = [c.b1, c.b2, c.b3, c.b4]
    with torch.no_grad():
        for i, (w, b) in enumerate(zip(ws, bs)):
            net[2 * i].weight.copy_(w)
            net[2 * i].bias.copy_(b)
    x = c.x0.clone().requires_grad_(True)
    keep = []
    h = x
    for i, mod in enumerate(net):
        h = mod(h)
        if isinstance(mod, torch.nn.ReLU):
            h.retain_grad()
            keep.append(h)
    out = h.squeeze(1) + c.partial
    out.backward(c.dout)

    # the no-rounding precondition, on everything the oracle rounds
    pre = [torch.relu(mr.layer_pre(a, w, b)[0]) for a, w, b in
           zip((c.x0, c.a1, c.a2), ws, bs)]
    pre += [mr.dgrad_pre(c.dz3, c.w3)[0], mr.dgrad_pre(c.dz2, c.w2)[0],
            mr.dgrad_pre(c.dz1, c.w1)[0]]
    for t in pre:
        assert mr.is_bf16(t) and float(t.abs().max()) > 0
    assert float(c.a3.abs().max()) > 0 and float(c.dx0.abs().max()) > 0

    assert torch.equal(out.detach(), c.out)
    for got, want in zip(keep, (c.a1, c.a2, c.a3)):
        assert torch.equal(got.detach(), want)
    assert torch.equal(x.grad, c.dx0)
    # dz_i = grad at relu_i's output times its mask
    for got, a, want in zip(keep, (c.a1, c.a2, c.a3),
                            (c.dz1, c.dz2, c.dz3)):
        assert torch.equal(got.grad * (a > 0), want)
    grads, sums, _ = mr.param_grads_ref(c)
    auto = [p.grad for p in net.parameters()]          # w1, b1, ... b4
    for g, s, a in zip(grads, sums, auto):
        assert mr.is_bf16(s)
        assert torch.equal(g, a.reshape(g.shape))
    # wgrad_ref is the same sum on top of a base
    base = torch.full((H, K0), 7.0, dtype=f64)
    assert torch.equal(mr.wgrad_ref(c.dz1, c.x0, base), 7 + auto[0])


def test_take_rows_is_a_case_of_its_own():
    c = _int()
    s = mr.take_rows(c, 17)
    # not a fresh draw, so compare through the chain itself
    (a1, a2, a3, out), _ = mr.fwd_ref(s.x0, c.w1, c.b1, c.w2, c.b2, c.w3,
                                      c.b3, c.w4, c.b4, s.partial)
    assert _same([a1, a2, a3, out], [s.a1, s.a2, s.a3, s.out])
    r, _ = mr.bwd_ref(s.dout, s.a1, s.a2, s.a3, c.w4, c.w3, c.w2, c.w1)
    assert _same(r, [s.dz3, s.dz2, s.dz1, s.dx0, s.dw4, s.db4])
    assert s.M == 17 and not torch.equal(s.dw4, c.dw4)


# ------------------------------------------- exact comparison and mutants

def test_int_case_limits_and_rounding_shares():
    c = _int()
    assert c.max_mag < mr.LIMIT
    for name, t in mr.pre_rounding(c).items():
        assert mr.tie_share(t) >= 0.01, name
        assert mr.inexact_share(t) - mr.tie_share(t) >= 0.01, name
    with pytest.raises(AssertionError):
        mr.int_case(3000, 400, 247)        # dw4 outgrows 2^24 with M


def test_exact_emulation_equals_oracle():
    c = _int()
    assert _same(emu_fwd(c), [c.a1, c.a2, c.a3, c.out])
    assert _same(emu_bwd(c), [c.dz3, c.dz2, c.dz1, c.dx0])
    w = mr.wgrad_int_case(160, 400, 247, 256)
    assert _same(emu_wgrad(w), mr.wgrad_apply(w, w.base))


def _fwd_drop():
    c = _int()
    k = int((c.w1[5] * c.x0[0]).abs().argmax())     # a term that counts
    assert float(c.w1[5, k] * c.x0[0, k]) != 0
    return dict(drop=(0, 5, k))


FWD_MUTANTS = {
    "dropped element": _fwd_drop,
    "w2 transposed": lambda: dict(w2_t=True),
    "truncation": lambda: dict(rnd=trunc),
    "round half away": lambda: dict(rnd=half_away),
    "bias after rounding": lambda: dict(bias_after=True),
}


@pytest.mark.parametrize("name", list(FWD_MUTANTS))
def test_exact_rejects_forward_mutant(name):
    c = _int()
    got = emu_fwd(c, **FWD_MUTANTS[name]())
    want = [c.a1, c.a2, c.a3, c.out]
    assert not _same(got, want)
    if name == "dropped element":           # one row's one column of a1
        assert int((got[0] != c.a1).sum()) <= c.M


BWD_MUTANTS = {
    "truncation": dict(rnd=trunc),
    "round half away": dict(rnd=half_away),
    "mask >= 0": dict(ge_mask=True),
    "dz3 unmasked": dict(mask_dz3=False),
}


@pytest.mark.parametrize("name", list(BWD_MUTANTS))
def test_exact_rejects_backward_mutant(name):
    c = _int()
    got = emu_bwd(c, **BWD_MUTANTS[name])
    assert not _same(got, [c.dz3, c.dz2, c.dz1, c.dx0])
    if name == "mask >= 0":
        # caught only through activations that ARE zero: there must be
        # some with a live gradient, else the mutant would be invisible
        assert int(((c.a3 == 0) & (got[0] != 0)).sum()) > 0


@pytest.mark.parametrize("kw", [dict(two_roundings=True),
                                dict(leak_pad=True)],
                         ids=["+= in bf16", "x0 pad leaks into dw1"])
def test_exact_rejects_wgrad_mutant(kw):
    # M = 1056: below a few hundred rows the products dz^T . x stay under
    # 256, are bf16 integers, and a second rounding would change nothing
    w = mr.wgrad_int_case(1056, 400, 247, 256)
    want = mr.wgrad_apply(w, w.base)
    got = emu_wgrad(w, **kw)
    assert not _same(got, want)
    if "leak_pad" in kw:
        assert not torch.equal(got[0], want[0])
        assert _same(got[1:], want[1:])


def test_wgrad_case_properties():
    w = mr.wgrad_int_case(160, 400, 247, 256)
    assert bool((w.x0[:, 247:] != 0).all())           # pads nonzero
    once = mr.wgrad_apply(w, w.base)
    for b, o, d, x in zip(w.base, once, w.dz, w.xs):
        assert mr.is_bf16(b) and mr.inexact_share(b + d.t() @ x) > 0.2
    twice = mr.wgrad_apply(w, once)
    assert not _same(twice, once)
    b = mr.bias_int_case(200, 400)
    assert mr.inexact_share(b.preset + b.sums) > 0.2
    assert torch.equal(mr.bias_finish_ref(b.base[0], b.sums[:400]),
                       mr.bf16_rne(b.base[0] + b.dz[0].sum(0)))


# -------------------------------------------------------- interval check

def _layer_intervals(c, acts, K0p=256, Hp=416, scale=1.0):
    """Intervals of a1..a3, each from the PREVIOUS entry of ``acts``
    (stage-wise, as the GPU test does it)."""
    ins = [c.x0, acts[0], acts[1]]
    res = []
    for a, w, b, kp in zip(ins, (c.w1, c.w2, c.w3), (c.b1, c.b2, c.b3),
                           (K0p, Hp, Hp)):
        z, mag = mr.layer_pre(a, w, b)
        res.append(mr.interval(z, mag, kp + 2, relu=True, scale=scale))
    return res


def _violations(c, acts):
    return [mr.check_interval(a, lo, hi)[0]
            for a, (lo, hi) in zip(acts, _layer_intervals(c, acts))]


def test_interval_accepts_fp32_chain():
    # the honest result: the same chain in float32 torch
    c = _float()
    acts = emu_fwd(c, dtype=torch.float32)
    assert _violations(c, acts[:3]) == [0, 0, 0]
    z, mag = mr.out_pre(acts[2], c.w4, c.b4, c.partial)
    assert mr.err_ratio(acts[3], z, mag, c.H + 2) <= 1.0
    # backward and wgrad stages alike
    a1, a2, a3 = acts[:3]
    f32 = torch.float32
    dz3 = mr.dz3_ref(c.dout, a3, c.w4)
    p = (dz3.to(f32) @ c.w3.to(f32)).to(f64)
    dz2 = mr.bf16_rne(p * (a2 > 0))
    ref, mag = mr.dgrad_pre(dz3, c.w3)
    lo, hi = mr.interval(ref, mag, 416 + 2, mask=(a2 > 0))
    assert mr.check_interval(dz2, lo, hi)[0] == 0
    base = mr.int_base([(c.H, c.H)])[0] / 64
    dw = mr.bf16_rne(base + (dz2.to(f32).t() @ a1.to(f32)).to(f64))
    ref, mag = mr.wgrad_pre(dz2, a1, base)
    lo, hi = mr.interval(ref, mag, c.M + 8 + 2)
    assert mr.check_interval(dw, lo, hi)[0] == 0


def _first_live_k(c):
    return int((c.w1[5] * c.x0[0]).abs().argmax())


@pytest.mark.parametrize("name", ["truncation", "dropped element",
                                  "bias of the next chunk"])
def test_interval_rejects_mutant(name):
    c = _float()
    kw = {"truncation": dict(rnd=trunc),
          "dropped element": dict(drop=(0, 5, _first_live_k(c))),
          "bias of the next chunk": dict(bias_shift=16)}[name]
    acts = emu_fwd(c, dtype=torch.float32, **kw)[:3]
    bad = _violations(c, acts)
    assert bad[0] > 0, bad
    if name == "truncation":
        # every layer, and in numbers: about half of the inexact entries
        assert min(bad) > 0.1 * c.M * c.H, bad


def test_interval_is_not_vacuous():
    # the pinned share (lo == hi) is a property of reference and bound
    # alone. It falls as delta * 2^8 / |value| grows, i.e. with Kp: 0.86
    # for layer 1 at K0p = 256 here, about 0.8 for the Kp = 416 layers and
    # 0.37 for a layer 1 at K0p = 1696. The 0.8 is asserted where the
    # contraction is 256 long; at every length the interval still has to
    # reject truncation.
    c = _float()
    acts = emu_fwd(c, dtype=torch.float32)[:3]
    pins = [mr.check_interval(a, lo, hi)[1]
            for a, (lo, hi) in zip(acts, _layer_intervals(c, acts))]
    assert pins[0] >= 0.8, pins
    wide = mr.float_case(32, 400, 1677)
    z, mag = mr.layer_pre(wide.x0, wide.w1, wide.b1)
    lo, hi = mr.interval(z, mag, 1696 + 2, relu=True)
    assert mr.check_interval(mr.bf16_rne(torch.relu(z)), lo, hi)[0] == 0
    assert mr.check_interval(trunc(torch.relu(z).float().to(f64)),
                             lo, hi)[0] > 0
    # scaled-down deltas only ever pin more
    tight = _layer_intervals(c, acts, scale=1 / 64)
    for a, (lo, hi), p in zip(acts, tight, pins):
        assert mr.check_interval(a, lo, hi)[1] > p


# -------------------------------------------------------------- CTR head

def test_head_ref_equals_float64_autograd():
    c = mr.head_int_case(5, 26, 9, 13)
    for use_fm in (False, True):
        r = mr.head_ref(c, use_fm)
        e_all = c.e_all.to(f64).requires_grad_(True)
        dense = c.dense.to(f64).requires_grad_(True)
        w = c.w.to(f64).requires_grad_(True)
        b = c.b.to(f64).requires_grad_(True)
        e, lin = e_all[..., :c.dim], e_all[..., c.dim]
        deep_in = torch.cat([e.flatten(1), dense], dim=1)
        partial = lin.sum(1) + dense @ w + b
        if use_fm:
            s = e.sum(1)
            partial = partial + 0.5 * (s * s - (e * e).sum(1)).sum(1)
        assert torch.equal(deep_in.detach(), r.deep_in.to(f64))
        assert torch.equal(partial.detach(), r.partial.to(f64))
        ((deep_in * c.d_deep_in[:, :c.width].to(f64)).sum()
         + (partial * c.d_partial.to(f64)).sum()).backward()
        assert torch.equal(e_all.grad, r.de_all.to(f64))
        assert torch.equal(dense.grad, r.d_dense.to(f64))
        assert torch.equal(w.grad, r.dw.to(f64))
        assert torch.equal(b.grad, r.db.to(f64))
