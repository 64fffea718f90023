"""k_cross_fwd / k_cross_bwd (ops/csrc/cross.hip) against cross_ref.py: bit
for bit on integer operands (the whole chain, both row tiles, both output
forms, the autograd function's fresh and prebound parameter gradients),
inside the derived intervals on random ones; the binding's refusals and
the torch route behind them; a captured step; the DCN model."""

import gc
import math

import pytest
import torch

import cross_ref as xr
from mlp_ref import bf16_rne, check_interval, err_ratio, interval

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf = torch.bfloat16
NAN = float("nan")
# dp = 32 (two chunks, idle waves), 64, the flagship 247 -> 256 and an
# unpadded 256 (KSM 8), 429 -> 448 (KS 14 of KSM 16), 512 (the limit)
GRID = [(d, L) for d in (20, 50, 247, 256, 429, 512) for L in (1, 3)] \
    + [(247, 4)]


def _pad(t, dp):
    return torch.nn.functional.pad(t, (0, dp - t.shape[-1]))


def _dev(t, dp=None, dt=bf):
    return (t if dp is None else _pad(t, dp)).to(dt).to(DEV).contiguous()


def _mirror(*shape):
    """A NaN-filled output with a canary row of 7s behind it."""
    n = math.prod(shape)
    buf = torch.full((n + shape[-1],), NAN, dtype=bf, device=DEV)
    buf[n:] = 7
    return buf, buf[:n].view(shape)


def _same(got, want, dp=None):
    """torch.equal on the padded reference: pads must be zero, not NaN."""
    want = torch.stack(want) if isinstance(want, list) else want
    return torch.equal(got.cpu().double(),
                       want if dp is None else _pad(want, dp))


def _kernels(ext, c, x0, bufs, b, logit, partial, gin, bm):
    """Both bindings over canary-backed mirrors -> (out, xs, us, qs, dx0)."""
    M, dp, L = c.M, c.dp, c.L
    held = [_mirror(L, M, dp), _mirror(L, M, dp), _mirror(L, M, dp),
            _mirror(M, dp)]
    (_, xs), (_, us), (_, qs), (_, dx0) = held
    out = torch.full((M,), NAN, device=DEV) if logit else None
    wo = _dev(c.w_out) if logit else None
    ext.cross_fwd(x0, bufs["w"], b, xs, us, wo,
                  _dev(c.b_out) if logit else None, partial, out, bm)
    ext.cross_bwd(x0, us, bufs["wt"], b, gin if logit else None, wo,
                  None if logit else gin, qs, dx0, bm)
    for buf, view in held:
        assert bool((buf[view.numel():] == 7).all())
    return out, xs, us, qs, dx0


@pytest.mark.parametrize("bm", [0, 16, 32])
@pytest.mark.parametrize("d,L", GRID)
def test_exact_on_integers(d, L, bm):
    """Every sum of |terms| is below 2^24 (cross_ref.solve asserts it), so
    every fp32 partial sum is an exact integer in any order and the kernels
    must equal the oracle's whole chain; at d >= 247, L >= 3 over 1 % of the
    last stage's values round, which pins nearest-even, the place of the
    bias add, the unrounded t in y and the residual."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    B = bm or 16                       # the launcher picks 16 at these M
    for M in sorted({1, 17, B - 1, B + 1, 2 * B + 3}):
        c = xr.int_case(M, d, L, seed=1000 * d + 10 * L + M)
        x0, b = _dev(c.x0, c.dp), _dev(c.b)
        W = _dev(c.W)
        bufs = dispatch._cross_images(W, c.dp, True, ext)
        for logit, part in ((True, True), (True, False), (False, False)):
            r = xr.solve(c, logit, part)
            partial = _dev(c.partial, dt=torch.float32) if part else None
            gin = _dev(c.dout, dt=torch.float32) if logit \
                else _dev(c.gx, c.dp)
            out, xs, us, qs, dx0 = _kernels(ext, c, x0, bufs, b, logit,
                                            partial, gin, bm)
            assert _same(xs, r.xs, c.dp) and _same(us, r.us, c.dp)
            assert _same(qs, r.qs, c.dp) and _same(dx0, r.dx0, c.dp)
            if logit:
                assert _same(out, r.out)
            # the autograd function: fresh gradients, then prebound ones
            # (zeroed, as the flat optimizer leaves them)
            ps = [W, b] + ([_dev(c.w_out), _dev(c.b_out)] if logit else [])
            want = [bf16_rne(torch.stack(r.dW)), bf16_rne(torch.stack(r.db))]
            if logit:
                want += [bf16_rne(r.dwo), bf16_rne(r.dbo).view(1)]
            for prebound in (False, True):
                leaves = [p.clone().requires_grad_() for p in ps]
                xg = x0.clone().requires_grad_()
                for p in leaves if prebound else []:
                    p.grad = torch.zeros_like(p)
                res = dispatch.cross_network(xg, *leaves, partial=partial,
                                             bm=bm)
                assert torch.equal(res, out if logit else xs[-1])
                res.backward(gin)
                assert torch.equal(xg.grad, dx0)
                for p, w in zip(leaves, want):
                    assert _same(p.grad, w)


@pytest.mark.parametrize("bm", [0, 32])
@pytest.mark.parametrize("d", [247, 512])
def test_random_within_intervals(d, bm):
    """M = 160, L = 6. Each stage is recomputed in float64 from the
    kernel's own previous bf16 outputs; delta = cin_ref.bound(mag, n) with
    mag = |x_0| (sum |W||x_l| + |b|) + |x_l| and n = dp + 4 (dp - 1 adds,
    bias, product, residual) forward, dp + 3 for a dgrad stage and the
    logit, L + 2 for a. No bf16 output may leave [bf16(ref - delta),
    bf16(ref + delta)]. Derived, nothing fitted."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    c = xr.float_case(160, d, 6, seed=d)
    x0, b, W = _dev(c.x0, c.dp), _dev(c.b), _dev(c.W)
    bufs = dispatch._cross_images(W, c.dp, True, ext)
    out, xs, us, qs, dx0 = _kernels(
        ext, c, x0, bufs, b, True, _dev(c.partial, dt=torch.float32),
        _dev(c.dout, dt=torch.float32), bm)
    xs, us, qs = (t.cpu().double()[..., :d] for t in (xs, us, qs))
    bad, worst = 0, 0.0
    xl = c.x0
    for l in range(6):
        t, y, mag_t, mag = xr.stage(c.x0, xl, c.W[l], c.b[l])
        bad += check_interval(us[l], *interval(t, mag_t, c.dp + 4))[0]
        bad += check_interval(xs[l], *interval(y, mag, c.dp + 4))[0]
        xl = xs[l]
    ref = xl @ c.w_out + c.b_out + c.partial
    mag = xl.abs() @ c.w_out.abs() + c.b_out.abs() + c.partial.abs()
    worst = err_ratio(out, ref, mag, c.dp + 3)
    gL = bf16_rne(c.dout.unsqueeze(1) * c.w_out)
    qiv, dxiv = xr.dgrad_intervals(gL, c.x0, us, qs, c.W, c.dp)
    for l in range(6):
        bad += check_interval(qs[l], *qiv[l])[0]
    bad += check_interval(dx0.cpu().double()[:, :d], *dxiv)[0]
    print(f"d={d} bm={bm}: logit err/delta {worst:.3f}, violations {bad}")
    assert bad == 0 and worst <= 1.0
    assert bool((dx0[:, d:] == 0).all())


@pytest.mark.parametrize("case", ["dp544", "L7", "fp32", "strided"])
def test_refusals_take_the_torch_route(case):
    """The torch route rounds after every op, so it is held to the float64
    formula only loosely: 3 L + 2 roundings of 2^-8 relative to the largest
    value (W ~ 1/(4 sqrt d): a layer amplifies an error by less than 2)."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    d, L = (530, 2) if case == "dp544" else (40, 7) if case == "L7" \
        else (40, 2)
    dp = (d + 31) // 32 * 32
    c = xr.float_case(9, d, L, seed=5)
    c.W = bf16_rne(c.W / 4)
    dt = torch.float32 if case == "fp32" else bf
    x0 = _dev(c.x0, dp, dt)
    if case == "strided":
        x0 = _dev(c.x0, 2 * dp)[:, :dp]
    W, b = _dev(c.W, dt=dt), _dev(c.b, dt=dt)
    img = torch.zeros(L, dp, dp, dtype=bf, device=DEV)
    with pytest.raises(RuntimeError):
        ext.cross_fwd(x0, img, b.to(bf), torch.empty(1, 9, dp, dtype=bf,
                                                     device=DEV),
                      None, None, None, None, None, 0)
    got = dispatch.cross_network(x0, W, b)
    assert got.shape == x0.shape and got.dtype == x0.dtype
    ref = xr.chain(c.x0, c.W, c.b).xs[-1]
    tol = (3 * L + 2) * 2.0 ** -8 * 2 ** L * float(ref.abs().max())
    assert float((got.cpu().double()[:, :d] - ref).abs().max()) <= tol
    assert bool((got[:, d:] == 0).all())


def test_captured_step_replays_bit_identically():
    from openembedding_amd.ops import dispatch
    c = xr.float_case(70, 247, 3, seed=9)
    x0 = _dev(c.x0, c.dp).requires_grad_()
    # frozen parameters: the capture holds the weight pack and the two
    # kernels, no library GEMM
    ps = [_dev(t) for t in (c.W, c.b, c.w_out, c.b_out)]
    partial = _dev(c.partial, dt=torch.float32)
    dout = _dev(c.dout, dt=torch.float32)

    def run():
        out = dispatch.cross_network(x0, *ps, partial=partial)
        return (out.detach(),) + torch.autograd.grad(out, [x0], dout)

    eager = [t.clone() for t in run()]
    assert all(bool(torch.isfinite(t).all()) for t in eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager):
            assert torch.equal(got, want)
    # hand the capture's private pool back before the next test runs
    del graph, static
    gc.collect()


@pytest.mark.parametrize("structure", ["parallel", "stacked"])
def test_dcn_is_head_cross_mlp(structure):
    from openembedding_amd.models import DCN, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16
    from openembedding_amd.ops import dispatch
    vocabs = [50, 3, 1000, 40, 7] + [100] * 21
    torch.manual_seed(0)
    m = convert_mlp_bf16(DCN(field_vocabs=vocabs, dim=9, cross_layers=3,
                             hidden=(64, 64, 64),
                             structure=structure).to(DEV))
    assert m.fused_mlp and m.fused_cross and m.cross_w.dtype == bf
    dense, sparse, _ = (t.to(DEV) for t in synthetic_batch(
        48, field_vocabs=vocabs, generator=torch.Generator().manual_seed(1)))
    with torch.no_grad():
        logits = m(dense, sparse)
        _, deep_in, partial = m._fused_head(dense, sparse, use_fm=False)
        assert deep_in.shape == (48, 256) and deep_in.dtype == bf
        if structure == "parallel":
            want = m._dnn_out(deep_in, dispatch.cross_network(
                deep_in, m.cross_w, m.cross_b,
                m.cross_out.weight.reshape(-1), m.cross_out.bias, partial))
        else:
            want = m._dnn_out(dispatch.cross_network(
                deep_in, m.cross_w, m.cross_b), partial)
    assert bool(torch.isfinite(logits).all()) and torch.equal(logits, want)
    m(dense, sparse).sum().backward()
    assert bool(torch.isfinite(m.cross_w.grad.float()).all())
