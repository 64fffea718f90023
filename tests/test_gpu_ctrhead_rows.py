"""GPU: the row-staged CTR head kernels (k_ctr_head_fwd_rows,
k_ctr_head_bwd_rows) against the per-field kernels they replace (impl = 2
against impl = 1: bit for bit wherever the result is elementwise or summed
in a fixed order), against the float64 reference of tests/ctrhead_ref.py
for the atomically accumulated dw / db, and against the int64 oracle of
tests/mlp_ref.py for the accumulate-into-bound-grads route."""

import os
import subprocess
import sys

import pytest
import torch

import ctrhead_ref as hr
import mlp_fraglayout_ref as fl
import mlp_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64          # elements kept free on either side of a sliced operand


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _poison_allocator():
    # leave NaN / inf bit patterns (bf16 pairs; NaN and inf as fp32 too)
    # in freed memory, so that a pad tail nobody writes does not read as 0
    junk = torch.empty(8 << 20, device=DEV, dtype=torch.int32)
    junk[0::3] = 0x7FC07FC0
    junk[1::3] = 0x7F807F80
    junk[2::3] = -8323200            # 0xFF80FF80
    del junk


def _sliced(t, off):
    """A contiguous copy of t that starts `off` elements into a larger
    buffer (so its address is not 16-byte aligned for off % 4 != 0)."""
    t = t.to(DEV)
    buf = torch.full((t.numel() + 2 * GUARD,), 77.0, device=DEV,
                     dtype=t.dtype)
    view = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _stride(F, dim, nd, pad32):
    width = F * dim + nd
    return mr.ceil_to(width, 32) if pad32 else width


# (B, F, dim, nd, out_bf16, pad32, use_fm, slice offset of the inputs).
# k = 4 samples per block forward, 16 backward at the small shapes: B 3/4/5
# and 15/16/17; D1 64 -> 65 crosses into the second column of a lane; the
# dim-127 rows leave room for 2 (bwd) samples per block only; F 27 * D1 10
# is a row that is no multiple of 4 floats; offsets 1..3 misalign the spans.
CASES = [
    (1, 1, 1, 1, True, True, True, 0),
    (3, 2, 3, 13, False, False, True, 1),
    (4, 26, 9, 13, True, True, True, 0),
    (5, 27, 9, 13, True, False, False, 2),
    (15, 26, 9, 13, True, True, True, 3),
    (16, 27, 3, 32, False, True, True, 0),
    (17, 26, 9, 13, False, False, True, 1),
    (257, 26, 9, 13, True, True, True, 0),
    (257, 26, 9, 1, True, True, False, 0),
    (17, 26, 63, 13, True, True, True, 0),
    (17, 2, 64, 32, False, False, True, 3),
    (5, 26, 64, 13, True, True, True, 0),
    (5, 26, 127, 13, False, True, True, 0),
    (257, 1, 127, 1, True, False, True, 2),
]


@pytest.mark.parametrize("B,F,dim,nd,out_bf16,pad32,use_fm,off", CASES)
def test_forward_bit_identical(B, F, dim, nd, out_bf16, pad32, use_fm, off):
    """impl 2 == impl 1 for deep_in, partial and s on randn operands, the
    pad tail is zero whatever the allocator held, and sliced inputs at any
    4-byte offset neither change the result nor get written to."""
    ext = _ext()
    c = hr.float_case(B, F, dim, nd, _stride(F, dim, nd, pad32),
                      seed=B + 7 * F + dim)
    e_all, dense = _sliced(c.e_all, off), _sliced(c.dense, off)
    w, b = _sliced(c.w, off), _sliced(c.b, off)
    plan = ext.ctr_head_rows_plan(B, F, dim, nd, c.stride, out_bf16)
    assert plan[0] >= 1
    _poison_allocator()
    want = ext.ctr_head_fwd(e_all, dense, w, b, use_fm, out_bf16, pad32,
                            impl=1)
    _poison_allocator()
    got = ext.ctr_head_fwd(e_all, dense, w, b, use_fm, out_bf16, pad32,
                           impl=2)
    torch.cuda.synchronize()
    for name, g, x in zip(("deep_in", "partial", "s"), got, want):
        assert g.shape == x.shape and g.dtype == x.dtype, name
        assert torch.equal(g, x), name
    width = F * dim + nd
    assert got[0].shape == (B, c.stride)
    assert bool((got[0][:, width:] == 0).all())
    assert bool(torch.isfinite(got[0].float()).all())
    # the launcher's choice is the row-staged kernel here
    auto = ext.ctr_head_fwd(e_all, dense, w, b, use_fm, out_bf16, pad32)
    assert all(torch.equal(a, g) for a, g in zip(auto, got))
    # inputs and their guard regions are as they were
    for view, src in ((e_all, c.e_all), (dense, c.dense), (w, c.w),
                      (b, c.b)):
        assert torch.equal(view.cpu(), src)
        base = view._base
        assert bool((base[:GUARD + off] == 77).all())
        assert bool((base[GUARD + off + src.numel():] == 77).all())


def test_forward_outputs_stay_inside():
    """The outputs are allocated by the binding, so no guard can be laid
    behind them directly; the caching allocator carves small tensors out
    of one segment, so tensors made just before and just after the call
    are their neighbours, and must keep their contents."""
    ext = _ext()
    B, F, dim, nd = 5, 27, 9, 13
    c = hr.float_case(B, F, dim, nd, _stride(F, dim, nd, False), seed=1)
    ops = [t.to(DEV) for t in (c.e_all, c.dense, c.w, c.b)]
    guards = [torch.full((512,), 5.0, device=DEV) for _ in range(8)]
    out = ext.ctr_head_fwd(*ops, True, True, False, impl=2)
    more = [torch.full((512,), 5.0, device=DEV) for _ in range(8)]
    want = ext.ctr_head_fwd(*ops, True, True, False, impl=1)
    torch.cuda.synchronize()
    for g in guards + more:
        assert bool((g == 5).all())
    assert all(torch.equal(a, x) for a, x in zip(out, want))


def test_flagship_head_into_mlp_exact():
    """test_head_into_mlp_exact's chain with impl = 2 at B = 64: the
    row-staged head writes the 32-padded bf16 deep_in and the partial
    logit, mlp3_fwd takes both, a1..a3 and out equal the int64 oracle."""
    ext = _ext()
    M, H, K0, K0p, F, dim, nd = 64, 400, 247, 256, 26, 9, 13
    c = mr.int_case(M, H, K0)
    h = mr.head_int_case(M, F, dim, nd)
    x0 = c.x0.to(torch.int64)
    h.e_all[..., :dim] = x0[:, :F * dim].reshape(M, F, dim)
    h.dense = x0[:, F * dim:]
    r = mr.head_ref(h, True)
    assert torch.equal(r.deep_in, x0)
    f = lambda t: t.to(torch.float32).to(DEV)  # noqa: E731
    _poison_allocator()
    deep_in, partial, _ = ext.ctr_head_fwd(f(h.e_all), f(h.dense), f(h.w),
                                           f(h.b), True, True, True, impl=2)
    assert deep_in.shape == (M, K0p)
    ws = (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, c.w4, c.b4)
    (a1, a2, a3, out), mags = mr.fwd_ref(c.x0, *ws, r.partial.double())
    assert float(mags[3].max()) < mr.LIMIT
    b = lambda t: t.to(torch.bfloat16).to(DEV)  # noqa: E731
    Hp = mr.ceil_to(H, 32)
    img = lambda w, n, k: fl.pack(fl.pad(w.to(torch.bfloat16), n,  # noqa: E731
                                         k)).contiguous().to(DEV)
    got = ext.mlp3_fwd(deep_in, img(c.w1, H, K0p), b(c.b1),
                       img(c.w2, H, Hp), b(c.b2), img(c.w3, H, Hp), b(c.b3),
                       b(c.w4), b(c.b4), partial, frag=True)
    assert torch.equal(got[0].double().cpu(), out)
    for g, want in zip(got[1:], (a1, a2, a3)):
        assert torch.equal(g.double().cpu(), want)


def _bwd_operands(c, out_bf16, off):
    dt = torch.bfloat16 if out_bf16 else torch.float32
    d_in = _sliced(c.d_deep_in.to(dt), off)
    return (_sliced(c.e_all, off), _sliced(c.dense, off), _sliced(c.w, off),
            d_in, _sliced(c.d_partial, off))


@pytest.mark.parametrize("B,F,dim,nd,out_bf16,pad32,use_fm,off", CASES)
def test_backward_against_old_and_reference(B, F, dim, nd, out_bf16, pad32,
                                            use_fm, off):
    """de_all and d_dense of impl 2 equal impl 1 bit for bit; dw and db of
    both are inside the accumulation bound around the float64 reference
    (the old pair first: a case it misses would be a badly chosen case)."""
    ext = _ext()
    c = hr.float_case(B, F, dim, nd, _stride(F, dim, nd, pad32),
                      seed=B + 7 * F + dim + 1)
    e_all, dense, w, d_in, d_p = _bwd_operands(c, out_bf16, off)
    s = ext.ctr_head_fwd(e_all, dense, w, c.b.to(DEV), use_fm, out_bf16,
                         pad32, impl=1)[2]
    r = hr.head_bwd_ref(e_all, dense, w, d_in, d_p, use_fm)
    plan = ext.ctr_head_rows_plan(B, F, dim, nd, c.stride, out_bf16)
    assert plan[1] >= 1 and 1 <= plan[2] <= max(1, hr.old_blocks(B, nd))
    _poison_allocator()
    old = ext.ctr_head_bwd(e_all, dense, w, d_in, d_p, s, use_fm, impl=1)
    _poison_allocator()
    new = ext.ctr_head_bwd(e_all, dense, w, d_in, d_p, s, use_fm, impl=2)
    torch.cuda.synchronize()
    n_old = hr.n_terms(B, hr.old_blocks(B, nd))
    n_new = hr.n_terms(B, plan[2])
    ratios = {
        "old dw": hr.acc_ratio(old[2], r.dw, r.dw_mag, n_old),
        "old db": hr.acc_ratio(old[3], r.db, r.db_mag, n_old),
        "new dw": hr.acc_ratio(new[2], r.dw, r.dw_mag, n_new),
        "new db": hr.acc_ratio(new[3], r.db, r.db_mag, n_new),
        "old de_all": hr.elem_ratio(old[0], r.de_all, r.de_mag, F),
        "old d_dense": hr.elem_ratio(old[1], r.d_dense, r.d_dense_mag, F),
    }
    print(ratios)
    assert ratios["old dw"] <= 1 and ratios["old db"] <= 1, ratios
    assert ratios["old de_all"] <= 1 and ratios["old d_dense"] <= 1, ratios
    assert torch.equal(new[0], old[0]), "de_all"
    assert torch.equal(new[1], old[1]), "d_dense"
    assert new[2].shape == old[2].shape and new[3].shape == old[3].shape
    assert ratios["new dw"] <= 1 and ratios["new db"] <= 1, ratios
    auto = ext.ctr_head_bwd(e_all, dense, w, d_in, d_p, s, use_fm)
    assert torch.equal(auto[0], new[0]) and torch.equal(auto[1], new[1])
    for view, src in ((e_all, c.e_all), (dense, c.dense), (w, c.w),
                      (d_p, c.d_partial)):
        assert torch.equal(view.cpu(), src)
        assert bool((view._base[:GUARD + off] == 77).all())
        assert bool((view._base[GUARD + off + src.numel():] == 77).all())


# ------------------------------------------------------ ctr_head_bwd_acc

def _int_operands(c, out_bf16):
    f = lambda t: t.to(torch.float32).to(DEV)  # noqa: E731
    dt = torch.bfloat16 if out_bf16 else torch.float32
    return (f(c.e_all), f(c.dense), f(c.w), c.d_deep_in.to(dt).to(DEV),
            f(c.d_partial))


@pytest.mark.parametrize("B,F,dim,nd,out_bf16,use_fm", [
    (64, 26, 9, 13, True, True), (257, 26, 9, 13, False, False),
    (17, 27, 64, 32, True, True), (5, 1, 127, 1, False, True)])
def test_bwd_acc_exact(B, F, dim, nd, out_bf16, use_fm):
    """Integer operands: dw_acc / db_acc, preset to integer bases inside a
    larger buffer, equal base + the int64 oracle after one call and base +
    2 * oracle after two; the neighbours in the buffer are untouched;
    want_d_dense=False returns no d_dense and the same de_all, dw, db."""
    ext = _ext()
    c = mr.head_int_case(B, F, dim, nd, seed=B + dim)
    r = mr.head_ref(c, use_fm)
    e_all, dense, w, d_in, d_p = _int_operands(c, out_bf16)
    s = r.s.to(torch.float32).to(DEV)
    g = torch.Generator().manual_seed(nd)
    base = torch.randint(-600, 601, (nd + 1 + 2 * GUARD,), generator=g)
    assert int(base.abs().max()) + 2 * 3 * B * 3 < mr.LIMIT
    buf = base.to(torch.float32).to(DEV)
    dw_acc = buf[GUARD:GUARD + nd]
    db_acc = buf[GUARD + nd:GUARD + nd + 1]
    want = base.clone()
    for call in (1, 2):
        _poison_allocator()
        de_all, d_dense = ext.ctr_head_bwd_acc(e_all, dense, w, d_in, d_p,
                                               s, use_fm, dw_acc, db_acc,
                                               True)
        want[GUARD:GUARD + nd] += r.dw
        want[GUARD + nd] += r.db[0]
        assert torch.equal(buf.double().cpu(), want.double()), call
        assert torch.equal(de_all.double().cpu(), r.de_all.double())
        assert torch.equal(d_dense.double().cpu(), r.d_dense.double())
    buf2 = base.to(torch.float32).to(DEV)
    de2, none = ext.ctr_head_bwd_acc(e_all, dense, w, d_in, d_p, s, use_fm,
                                     buf2[GUARD:GUARD + nd],
                                     buf2[GUARD + nd:GUARD + nd + 1], False)
    assert none is None
    assert torch.equal(de2, de_all)
    want1 = base.clone()
    want1[GUARD:GUARD + nd] += r.dw
    want1[GUARD + nd] += r.db[0]
    assert torch.equal(buf2.double().cpu(), want1.double())


def test_bwd_acc_refuses_bad_accumulators():
    ext = _ext()
    c = mr.head_int_case(4, 2, 3, 5)
    e_all, dense, w, d_in, d_p = _int_operands(c, False)
    s = torch.zeros(4, 3, device=DEV)
    ok_w, ok_b = torch.zeros(5, device=DEV), torch.zeros(1, device=DEV)
    args = (e_all, dense, w, d_in, d_p, s, True)
    ext.ctr_head_bwd_acc(*args, ok_w, ok_b, True)
    bad = [
        (ok_w.bfloat16(), ok_b),                       # dtype
        (ok_w, ok_b.double()),
        (torch.zeros(6, device=DEV), ok_b),            # length
        (ok_w, torch.zeros(2, device=DEV)),
        (torch.zeros(10, device=DEV)[::2], ok_b),      # not contiguous
        (ok_w.cpu(), ok_b),                            # device
    ]
    for dw_acc, db_acc in bad:
        before = (dw_acc.clone(), db_acc.clone())
        with pytest.raises(RuntimeError):
            ext.ctr_head_bwd_acc(*args, dw_acc, db_acc, True)
        assert torch.equal(dw_acc, before[0])
        assert torch.equal(db_acc, before[1])
    with pytest.raises(RuntimeError):                  # d_partial too short
        ext.ctr_head_bwd_acc(e_all, dense, w, d_in, d_p[:3], s, True, ok_w,
                             ok_b, True)


# ------------------------------------------------------- _FusedCTRHeadFn

def _fn_case(B=64, F=26, dim=9, nd=13):
    c = mr.head_int_case(B, F, dim, nd, seed=11)
    r = mr.head_ref(c, True)
    f = lambda t: t.to(torch.float32).to(DEV)  # noqa: E731
    e_all = f(c.e_all).requires_grad_()
    dense = f(c.dense)
    w = torch.nn.Parameter(f(c.w).view(1, -1))
    b = torch.nn.Parameter(f(c.b))
    stride = mr.ceil_to(c.width, 32)
    return c, r, e_all, dense, w, b, stride


def _run_fn(c, e_all, dense, w, b):
    from openembedding_amd.models.ctr import _FusedCTRHeadFn
    deep_in, partial = _FusedCTRHeadFn.apply(e_all, dense, w, b, True, True,
                                             True)
    d_in = c.d_deep_in.to(torch.bfloat16).to(DEV)
    d_p = c.d_partial.to(torch.float32).to(DEV)
    torch.autograd.backward([deep_in, partial], [d_in, d_p])
    return deep_in, partial


def test_fn_bound_grads_accumulate_once():
    """w.grad / b.grad bound as views of one flat fp32 buffer: after
    backward the buffer is base + oracle, once — a route that accumulated
    in the kernel AND handed the grads to autograd would give twice."""
    c, r, e_all, dense, w, b, _ = _fn_case()
    base = torch.arange(-20, -20 + c.nd + 1 + 2 * GUARD, dtype=torch.float32)
    flat = base.to(DEV)
    w.grad = flat[GUARD:GUARD + c.nd].view(1, -1)
    b.grad = flat[GUARD + c.nd:GUARD + c.nd + 1]
    dense.requires_grad_(False)
    _run_fn(c, e_all, dense, w, b)
    want = base.double().clone()
    want[GUARD:GUARD + c.nd] += r.dw
    want[GUARD + c.nd] += r.db[0]
    assert torch.equal(flat.double().cpu(), want)
    assert w.grad.data_ptr() == flat[GUARD:].data_ptr()
    assert dense.grad is None
    assert torch.equal(e_all.grad.double().cpu(), r.de_all.double())


def test_fn_unbound_and_unfit_grads_take_autograd():
    """.grad = None: grads arrive through autograd and equal the oracle.
    A bf16 or non-contiguous .grad: the old route, correct as well. dense
    with requires_grad gets d_dense on every route."""
    c, r, e_all, dense, w, b, _ = _fn_case()
    dense.requires_grad_(True)
    _run_fn(c, e_all, dense, w, b)
    assert torch.equal(w.grad.double().cpu().reshape(-1), r.dw.double())
    assert torch.equal(b.grad.double().cpu(), r.db.double())
    assert torch.equal(dense.grad.double().cpu(), r.d_dense.double())
    assert torch.equal(e_all.grad.double().cpu(), r.de_all.double())
    # a bf16 .grad cannot be bound to dense_linear's fp32 parameters at
    # all (torch refuses the assignment), so the dtype clause of the
    # prebound rule can only ever send such a grad to the old route
    c, r, e_all, dense, w, b, _ = _fn_case(B=5)
    with pytest.raises((RuntimeError, TypeError)):
        w.grad = torch.zeros(1, c.nd, device=DEV, dtype=torch.bfloat16)
    # non-contiguous fp32 .grad
    c, r, e_all, dense, w, b, _ = _fn_case()
    wide = torch.zeros(1, 2 * c.nd, device=DEV)
    w.grad = wide[:, ::2]
    b.grad = torch.zeros(1, device=DEV)
    dense.requires_grad_(True)
    _run_fn(c, e_all, dense, w, b)
    assert torch.equal(w.grad.double().cpu().reshape(-1), r.dw.double())
    assert torch.equal(b.grad.double().cpu(), r.db.double())
    assert torch.equal(dense.grad.double().cpu(), r.d_dense.double())


# ------------------------------------------------------------- fallback

def test_unfit_shape_falls_back():
    """A row that cannot be staged (F 300, dim 127: 153 KB per sample):
    impl 0 takes the per-field kernels, impl 2 refuses."""
    ext = _ext()
    B, F, dim, nd = 2, 300, 127, 13
    c = hr.float_case(B, F, dim, nd, F * dim + nd, seed=5)
    ops = [t.to(DEV) for t in (c.e_all, c.dense, c.w, c.b)]
    assert ext.ctr_head_rows_plan(B, F, dim, nd, c.stride, False) == (
        0, 0, 0, False)
    want = ext.ctr_head_fwd(*ops, True, False, False, impl=1)
    got = ext.ctr_head_fwd(*ops, True, False, False, impl=0)
    assert all(torch.equal(a, x) for a, x in zip(got, want))
    with pytest.raises(RuntimeError):
        ext.ctr_head_fwd(*ops, True, False, False, impl=2)
    d_in, d_p = c.d_deep_in.to(DEV), c.d_partial.to(DEV)
    bw = (ops[0], ops[1], ops[2], d_in, d_p, want[2], True)
    old = ext.ctr_head_bwd(*bw, impl=1)
    new = ext.ctr_head_bwd(*bw, impl=0)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    r = hr.head_bwd_ref(ops[0], ops[1], ops[2], d_in, d_p, True)
    n = hr.n_terms(B, hr.old_blocks(B, nd))
    assert hr.acc_ratio(new[2], r.dw, r.dw_mag, n) <= 1
    with pytest.raises(RuntimeError):
        ext.ctr_head_bwd(*bw, impl=2)
    # the accumulating binding still serves the shape (old pair + add)
    base = torch.full((nd + 1,), 3.0, device=DEV)
    de, dd = ext.ctr_head_bwd_acc(*bw, base[:nd], base[nd:], True)
    assert torch.equal(de, old[0]) and torch.equal(dd, old[1])
    assert hr.acc_ratio(base[:nd], r.dw, r.dw_mag, n + 1,
                        torch.full((nd,), 3.0)) <= 1


def test_launchers_choice_for_the_backward():
    """impl 0 gives the backward to the merged kernel only where all 16
    samples of a block fit (the flagship rows), and to the pair at dim 64,
    where the merged kernel fits with 4 and measured slower; the forward
    takes the row-staged kernel at both."""
    ext = _ext()
    assert ext.ctr_head_rows_plan(4096, 26, 9, 13, 256, True) == (
        4, 16, 208, True)
    assert ext.ctr_head_rows_plan(4096, 26, 64, 13, 1696, True) == (
        4, 4, 208, False)


# -------------------------------------------------------------- capture

def test_graph_capture_forward_backward():
    """One torch.cuda.graph of head forward + backward with bound grads at
    the flagship row shape, replayed on two fresh input sets: deep_in,
    partial and de_all equal eager bit for bit, the grad buffer equals the
    eager accumulation within the bound."""
    ext = _ext()
    B, F, dim, nd, stride = 64, 26, 9, 13, 256
    cs = [hr.float_case(B, F, dim, nd, stride, seed=s) for s in (1, 2, 3)]
    st = [t.to(DEV).clone() for t in (cs[0].e_all, cs[0].dense, cs[0].w,
                                      cs[0].b,
                                      cs[0].d_deep_in.to(torch.bfloat16),
                                      cs[0].d_partial)]
    flat = torch.zeros(nd + 1, device=DEV)

    def step():
        deep_in, partial, s = ext.ctr_head_fwd(st[0], st[1], st[2], st[3],
                                               True, True, True)
        de_all, _ = ext.ctr_head_bwd_acc(st[0], st[1], st[2], st[4], st[5],
                                         s, True, flat[:nd], flat[nd:],
                                         False)
        return deep_in, partial, de_all

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    flat.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    mag = torch.zeros(nd + 1, dtype=torch.float64)
    total = torch.zeros(nd + 1, dtype=torch.float64)
    for c in cs[1:]:
        new = (c.e_all, c.dense, c.w, c.b, c.d_deep_in.to(torch.bfloat16),
               c.d_partial)
        for dst, src in zip(st, new):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        keep = flat.clone()
        want = step()                            # eager, same operands
        torch.cuda.synchronize()
        flat.copy_(keep)                         # undo the eager add
        for g, x in zip(got, want):
            assert torch.equal(g, x)
        r = hr.head_bwd_ref(st[0], st[1], st[2], st[4], st[5], True)
        total += torch.cat([r.dw, r.db])
        mag += torch.cat([r.dw_mag, r.db_mag])
    n = 2 * hr.n_terms(B, ext.ctr_head_rows_plan(B, F, dim, nd, stride,
                                                 True)[2])
    assert hr.acc_ratio(flat, total, mag, n) <= 1
    assert float(total.abs().max()) > 1


# --------------------------------------------------------------- switch

def test_switch_off_in_child_process(tmp_path):
    """OEAMD_HEAD_ROWS=0 (read once at import, hence a fresh process) runs
    one DeepFM step at batch 64 from the same seeds on the per-field
    kernels and AccumulateGrad: equal logits, dense_linear grads within
    the accumulation bound of each other."""
    out = tmp_path / "step.pt"
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests_dir)
    code = ("import sys; sys.path[:0] = [%r, %r]; import ctrhead_ref as h; "
            "h.step_child_main(%r)" % (root, tests_dir, str(out)))
    env = dict(os.environ, OEAMD_HEAD_ROWS="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True,
                   timeout=300)
    old = torch.load(out)
    from openembedding_amd.models import ctr
    assert ctr._HEAD_ROWS is True
    new = hr.deepfm_step(DEV)
    assert torch.equal(new["logits"], old["logits"])
    # both sides are fp32 sums of the same 64 terms per address in some
    # order: each is within bound(mag, n) of the exact sum, so they are
    # within twice that of each other
    n = hr.n_terms(64, 4)
    for k in ("dw", "db"):
        a, b = new[k].double().reshape(-1), old[k].double().reshape(-1)
        mag = new[k + "_mag"].double().reshape(-1)
        assert float(a.abs().max()) > 0
        assert bool(((a - b).abs() <= 2 * hr.cin_ref.bound(mag, n)).all()), k
