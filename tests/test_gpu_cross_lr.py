"""ops/csrc/cross_lr.hip against cross_lr_ref.py; the routing around it."""

import gc
import os
import subprocess
import sys

import pytest
import torch

import cross_lr_ref as lr
from cin_ref import bound
from mlp_ref import bf16_rne, check_interval, err_ratio, interval
from test_gpu_cross import DEV, NAN, _dev, _mirror, _same, bf

pytestmark = pytest.mark.gpu

GRID = [(d, r, L) for d, r in ((20, 3), (50, 16), (247, 33), (247, 64),
                               (256, 32), (429, 96), (512, 128))
        for L in (1, 3)] + [(247, 64, 4)]


def _kernels(ext, c, x0, bufs, b, logit, partial, gin, bm):
    M, big, rank = c.M, (c.L, c.M, c.dp), (c.L, c.M, c.rp)   # canary-backed
    held = [_mirror(*s) for s in (big, big, rank, big, rank, (M, c.dp))]
    xs, us, ps, qs, ss, dx0 = (v for _, v in held)
    out = torch.full((M,), NAN, device=DEV) if logit else None
    wo = _dev(c.w_out) if logit else None
    ext.cross_lr_fwd(x0, bufs["v"], bufs["u"], b, c.r, xs, us, ps, wo,
                     _dev(c.b_out) if logit else None, partial, out, bm)
    ext.cross_lr_bwd(x0, us, bufs["ut"], bufs["vt"], b, c.r,
                     gin if logit else None, wo, None if logit else gin,
                     qs, ss, dx0, bm)
    for buf, view in held:
        assert bool((buf[view.numel():] == 7).all())
    return out, xs, us, ps, qs, ss, dx0


@pytest.mark.parametrize("bm", [0, 16, 32])
@pytest.mark.parametrize("d,rk,L", GRID)
def test_exact_on_integers(d, rk, L, bm):
    """Sums of |terms| < 2^24 (solve): any order is exact, k-split too."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    B = bm or 16                       # the launcher picks 16 at these M
    for M in sorted({1, 17, B - 1, B + 1, 2 * B + 3}):
        c = lr.int_case(M, d, rk, L, seed=1000 * d + 10 * L + M)
        x0, b, U, V = _dev(c.x0, c.dp), _dev(c.b), _dev(c.U), _dev(c.V)
        bufs = dispatch._cross_lr_images(U, V, c.dp, c.rp, True, ext)
        for logit, part in ((True, True), (True, False), (False, False)):
            r = lr.solve(c, logit, part)
            partial = _dev(c.partial, dt=torch.float32) if part else None
            gin = _dev(c.dout, dt=torch.float32) if logit \
                else _dev(c.gx, c.dp)
            out, xs, us, ps, qs, ss, dx0 = _kernels(
                ext, c, x0, bufs, b, logit, partial, gin, bm)
            assert _same(xs, r.xs, c.dp) and _same(us, r.us, c.dp)
            assert _same(ps, r.ps, c.rp) and _same(ss, r.ss, c.rp)
            assert _same(qs, r.qs, c.dp) and _same(dx0, r.dx0, c.dp)
            if logit:
                assert _same(out, r.out)
            if L > 1:
                continue
            prm = [U, V, b] + ([_dev(c.w_out), _dev(c.b_out)] if logit
                               else [])
            want = [bf16_rne(torch.stack(t)) for t in (r.dU, r.dV, r.db)]
            if logit:
                want += [bf16_rne(r.dwo), bf16_rne(r.dbo).view(1)]
            for prebound in (False, True):
                leaves = [p.clone().requires_grad_() for p in prm]
                xg = x0.clone().requires_grad_()
                pg = partial.clone().requires_grad_() if part else None
                for p in leaves if prebound else []:
                    p.grad = torch.zeros_like(p)
                res = dispatch.cross_network_lr(xg, *leaves, partial=pg,
                                                bm=bm)
                assert torch.equal(res, out if logit else xs[-1])
                res.backward(gin)
                assert torch.equal(xg.grad, dx0)
                assert pg is None or torch.equal(pg.grad, gin)
                for p, w in zip(leaves, want):
                    assert _same(p.grad, w)


@pytest.mark.parametrize("bm", [0, 32])
@pytest.mark.parametrize("d,rk", [(256, 64), (512, 128)])
def test_random_within_intervals(d, rk, bm):
    """M = 160, L = 6. Each stage, recomputed in float64 from the kernel's
    own previous outputs, must lie in [bf16(ref - delta), bf16(ref + delta)],
    delta = cin_ref.bound(sum |terms|, n): n = dp + W + 2 for p_l (W k-split
    partials), rp + 4 for t and x_{l+1}, dp + 2 for s_l and the logit,
    rp + 3 for g_l (carried as an interval), L + 2 for a. Derived."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    L = 6
    c = lr.float_case(160, d, rk, L, seed=d)
    x0, b, U, V = _dev(c.x0, c.dp), _dev(c.b), _dev(c.U), _dev(c.V)
    bufs = dispatch._cross_lr_images(U, V, c.dp, c.rp, True, ext)
    out, xs, us, ps, qs, ss, dx0 = _kernels(
        ext, c, x0, bufs, b, True, _dev(c.partial, dt=torch.float32),
        _dev(c.dout, dt=torch.float32), bm)
    xs, us, qs = (t.cpu().double()[..., :d] for t in (xs, us, qs))
    ps, ss = (t.cpu().double()[..., :rk] for t in (ps, ss))
    W = {32: 4, 64: 2, 96: 4, 128: 1}[c.rp]    # k-split parts
    bad, xl = 0, c.x0
    for l in range(L):
        bad += check_interval(ps[l], *interval(
            xl @ c.V[l].t(), xl.abs() @ c.V[l].abs().t(), c.dp + W + 2))[0]
        t = ps[l] @ c.U[l].t() + c.b[l]
        mag_t = ps[l].abs() @ c.U[l].abs().t() + c.b[l].abs()
        bad += check_interval(xs[l], *interval(
            c.x0 * t + xl, c.x0.abs() * mag_t + xl.abs(), c.rp + 4))[0]
        xl = xs[l]
    ref = xl @ c.w_out + c.b_out + c.partial
    mag = xl.abs() @ c.w_out.abs() + c.b_out.abs() + c.partial.abs()
    worst = err_ratio(out, ref, mag, c.dp + 2)
    glo = ghi = bf16_rne(c.dout.unsqueeze(1) * c.w_out)
    alo = ahi = amag = torch.zeros_like(c.x0)
    for l in reversed(range(L)):
        e0, e1 = bf16_rne(glo * c.x0), bf16_rne(ghi * c.x0)
        bad += check_interval(qs[l], torch.minimum(e0, e1),
                              torch.maximum(e0, e1))[0]
        p0, p1 = glo * us[l], ghi * us[l]
        alo, ahi = alo + torch.minimum(p0, p1), ahi + torch.maximum(p0, p1)
        gabs = torch.maximum(glo.abs(), ghi.abs())
        amag = amag + gabs * us[l].abs()
        bad += check_interval(ss[l], *interval(
            qs[l] @ c.U[l], qs[l].abs() @ c.U[l].abs(), c.dp + 2))[0]
        s = ss[l] @ c.V[l]
        dl = bound(ss[l].abs() @ c.V[l].abs() + gabs, c.rp + 3)
        glo, ghi = bf16_rne(s + glo - dl), bf16_rne(s + ghi + dl)
    da = bound(amag + torch.maximum(glo.abs(), ghi.abs()), L + 2)
    bad += check_interval(dx0.cpu().double()[:, :d],
                          bf16_rne(alo + glo - da),
                          bf16_rne(ahi + ghi + da))[0]
    print(f"d={d} r={rk} bm={bm}: logit err/delta {worst:.3f}, bad {bad}")
    assert bad == 0 and worst <= 1.0


@pytest.mark.parametrize("case,msg", [
    ("dp544", "32..512"), ("rp160", "32..128"), ("L7", "L <= 6"),
    ("fp32", "must be bf16"), ("strided", "contiguous")])
def test_refusals_take_the_torch_route(case, msg):
    """Both bindings refuse, naming the limit; the operator returns the
    torch route's result, inside that route's derived rounding budget."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    d, rk, L = {"dp544": (530, 8, 2), "rp160": (200, 130, 2),
                "L7": (40, 8, 7)}.get(case, (40, 8, 2))
    c = lr.float_case(9, d, rk, L, seed=5)
    c.U = bf16_rne(c.U / 16)      # keeps L = 7 tame
    dt = torch.float32 if case == "fp32" else bf
    x0 = _dev(c.x0, c.dp, dt)
    if case == "strided":
        x0 = _dev(c.x0, 2 * c.dp)[:, :c.dp]
    U, V, b = (_dev(t, dt=dt) for t in (c.U, c.V, c.b))
    z = lambda *s: torch.zeros(*s, dtype=bf, device=DEV)  # noqa: E731
    down, up, bb = z(L, c.rp, c.dp), z(L, c.dp, c.rp), b.to(bf)
    with pytest.raises(RuntimeError, match=msg):
        ext.cross_lr_fwd(x0, down, up, bb, rk, z(1, 9, c.dp), None, None,
                         None, None, None, None, 0)
    with pytest.raises(RuntimeError, match=msg):
        ext.cross_lr_bwd(x0, z(L, 9, c.dp), down, up, bb, rk, None, None,
                         z(9, c.dp), z(L, 9, c.dp), z(L, 9, c.rp),
                         z(9, c.dp), 0)
    got = dispatch.cross_network_lr(x0, U, V, b)
    assert torch.equal(got, dispatch._cross_lr_torch(x0, U, V, b, None,
                                                     None, None))
    ref, e = lr.torch_route(c, 2.0 ** (-24 if case == "fp32" else -9))
    assert bool(((got.cpu().double()[:, :d] - ref).abs() <= e).all())
    assert float(e.max()) < float(ref.abs().max()) / 8    # below the signal
    assert bool((got[:, d:] == 0).all())


def test_captured_step_replays_bit_identically():
    from openembedding_amd.ops import dispatch
    c = lr.float_case(70, 247, 64, 3, seed=9)
    x0 = _dev(c.x0, c.dp).requires_grad_()
    prm = [_dev(t) for t in (c.U, c.V, c.b, c.w_out, c.b_out)]
    partial = _dev(c.partial, dt=torch.float32)
    dout = _dev(c.dout, dt=torch.float32)

    def run():
        out = dispatch.cross_network_lr(x0, *prm, partial=partial)
        return (out.detach(),) + torch.autograd.grad(out, [x0], dout)

    eager = [t.clone() for t in run()]
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
    del graph, static
    gc.collect()


@pytest.mark.parametrize("structure", ["parallel", "stacked"])
def test_dcn_low_rank_is_head_cross_mlp(structure):
    from openembedding_amd.models import DCN, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16
    from openembedding_amd.ops import dispatch
    vocabs = [50, 3, 1000, 40, 7] + [100] * 21
    m = convert_mlp_bf16(DCN(field_vocabs=vocabs, dim=9, cross_layers=3,
                             hidden=(64, 64, 64), structure=structure,
                             low_rank=64).to(DEV))
    assert m.fused_mlp and m.fused_cross and m.cross_u.dtype == bf
    dense, sparse, _ = (t.to(DEV) for t in synthetic_batch(
        48, field_vocabs=vocabs, generator=torch.Generator().manual_seed(1)))
    with torch.no_grad():
        logits = m(dense, sparse)
        _, deep_in, partial = m._fused_head(dense, sparse, use_fm=False)
        ws = (m.cross_u, m.cross_v, m.cross_b)
        if structure == "parallel":
            want = m._dnn_out(deep_in, dispatch.cross_network_lr(
                deep_in, *ws, m.cross_out.weight.reshape(-1),
                m.cross_out.bias, partial))
        else:
            want = m._dnn_out(dispatch.cross_network_lr(deep_in, *ws),
                              partial)
    assert bool(torch.isfinite(logits).all()) and torch.equal(logits, want)


def _switch_args():
    """Integers so small that neither route rounds (asserted below)."""
    c = lr.int_case(40, 50, 16, 2, seed=11)
    return c, [_dev(c.x0, c.dp)] + [_dev(t) for t in (
        c.U, c.V, c.b, c.w_out, c.b_out)] + [_dev(c.partial,
                                                  dt=torch.float32)]


def test_env_switch_keeps_the_torch_route():
    """A child with OEAMD_CROSS_LR=0 returns the torch route's logits bit
    for bit, within the interval test's bound of the fused ones: every
    intermediate is an integer <= 256, so the bf16 route rounds nothing."""
    from openembedding_amd.ops import dispatch
    assert dispatch._CROSS_LR
    c, args = _switch_args()
    r = lr.chain(c.x0, c.U, c.V, c.b)
    assert max(float(t.abs().max()) for t in r.ps + r.us + r.xs
               + [r.xs[-1] @ c.w_out]) <= 256
    fused = dispatch.cross_network_lr(*args).cpu().double()
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_cross_lr as t\n"
            "from openembedding_amd.ops import dispatch\n"
            "assert not dispatch._CROSS_LR\n"
            "print(*dispatch.cross_network_lr(*t._switch_args()[1])"
            ".tolist())\n" % [here, os.path.dirname(here)])
    res = subprocess.run([sys.executable, "-c", code], check=True,
                         capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, OEAMD_CROSS_LR="0"))
    child = torch.tensor([float(v) for v in res.stdout.split()],
                         dtype=torch.float64)
    assert torch.equal(child, dispatch._cross_lr_torch(*args).cpu().double())
    mag = r.xs[-1].abs() @ c.w_out.abs() + c.b_out.abs() + c.partial.abs()
    assert bool(((child - fused).abs() <= bound(mag, c.dp + 2)).all())
