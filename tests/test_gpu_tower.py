"""k_tower_fwd / k_tower_bwd (ops/csrc/tower.hip) against a float64
reference of the arithmetic at the head of that file: exact on integers,
inside derived intervals on random operands; autograd and routing."""

import gc
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from cin_ref import bound, ceil_to
from mlp_ref import bf16_rne, check_interval, interval

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf, f64 = torch.bfloat16, torch.float64
NAN, LIMIT = float("nan"), float(2 ** 24)
# one chunk; k-splits 2 and 4; the reference's WDL tower (KSM 8); DeepCTR's
# on an unpadded row; 3 chunks under KS 14 of KSM 16; every limit, split 7
GRID = [(20, (16,)), (50, (64, 32)), (247, (512, 256, 128, 32)),
        (256, (256, 128, 64)), (429, (48, 512)), (512, (416, 400, 16, 32))]
FOUR = [s for s in GRID if len(s[1]) == 4]


def _case(M, K0, widths, seed, integer=True):
    """Operands as float64: small integers (W_l at density 1/4), else random
    bf16 values at unit scale."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(  # noqa: E731
        lo, hi + 1, s, generator=g).to(f64)
    rn = lambda *s, sc=1.0: bf16_rne(  # noqa: E731
        (torch.randn(*s, generator=g) + 0.1) * sc)
    c = SimpleNamespace(M=M, K0=K0, K0p=ceil_to(K0, 32), widths=widths,
                        L=len(widths), W=[], b=[])
    k = K0
    for l, h in enumerate(widths):
        if integer:
            keep = (torch.rand(h, k, generator=g) < 0.25).to(f64)
            c.W.append(ri(-2, 2, h, k) * keep if l == 0
                       else ri(-1, 1, h, k) * keep)
            c.b.append(ri(-5, 5, h))
        else:
            c.W.append(rn(h, k, sc=k ** -0.5))
            c.b.append(rn(h, sc=0.3))
        k = h
    if integer:
        c.x0, c.dout = ri(-3, 3, M, K0), ri(-3, 3, M)
        c.w_out, c.b_out = ri(-2, 2, k), ri(-5, 5, 1)
        c.partial = ri(-9, 9, M)
    else:
        c.x0, c.w_out, c.b_out = rn(M, K0, sc=0.5), rn(k, sc=0.5), rn(1)
        c.dout = (torch.randn(M, generator=g) * 4 + 0.5).float().to(f64)
        c.partial = torch.randn(M, generator=g).float().to(f64)
    return c


def _layer(a, W, b):                   # -> (W a + b, the sum of |terms|)
    return a @ W.t() + b, a.abs() @ W.abs().t() + b.abs()


def _logit(a, c, part):
    z = a @ c.w_out + c.b_out
    mag = a.abs() @ c.w_out.abs() + c.b_out.abs()
    return (z + c.partial, mag + c.partial.abs()) if part else (z, mag)


def _solve(c):
    """The reference's whole chain; ``pre`` the unrounded a_l and dx0,
    ``mag`` the largest sum of |terms| of any stage and wgrad sum."""
    r = SimpleNamespace(a=[], dz=[None] * c.L, pre={}, mag=0.0)
    a = c.x0
    for l in range(c.L):
        z, mag = _layer(a, c.W[l], c.b[l])
        r.mag = max(r.mag, float(mag.max()))
        r.pre[f"a{l + 1}"] = torch.relu(z)
        a = bf16_rne(torch.relu(z))
        r.a.append(a)
    r.out, mag = _logit(a, c, True)
    r.out_nopartial = _logit(a, c, False)[0]
    r.fwd_mag = max(r.mag, float(mag.max()))
    dz = bf16_rne(c.dout.unsqueeze(1) * c.w_out * (a > 0))
    mags = [mag, (c.dout.unsqueeze(1) * a).abs().sum(0)]
    for l in range(c.L - 1, -1, -1):
        r.dz[l] = dz
        a_in = r.a[l - 1] if l else c.x0
        mags += [dz.abs().t() @ a_in.abs(), dz.abs().sum(0)]
        p, mag = dz @ c.W[l], dz.abs() @ c.W[l].abs()
        mags.append(mag)
        if l:
            dz = bf16_rne(p * (a_in > 0))
    r.pre["dx0"] = p
    r.dx0 = torch.nn.functional.pad(bf16_rne(p), (0, c.K0p - c.K0))
    r.mag = max([r.mag] + [float(m.max()) for m in mags])
    return r


def _dev(t, dt=bf, pad=0):
    return torch.nn.functional.pad(t, (0, pad)).to(dt).to(DEV).contiguous()


def _mirror(*shape):             # NaN-filled, a canary row of 7s behind it
    n = shape[0] * shape[1]
    buf = torch.full((n + shape[-1],), NAN, dtype=bf, device=DEV)
    buf[n:] = 7
    return buf, buf[:n].view(shape)


def _operands(c):
    return SimpleNamespace(
        x0=_dev(c.x0, pad=c.K0p - c.K0), W=[_dev(w) for w in c.W],
        b=[_dev(b) for b in c.b], w_out=_dev(c.w_out), b_out=_dev(c.b_out),
        partial=_dev(c.partial, torch.float32),
        dout=_dev(c.dout, torch.float32))


def _kernels(ext, c, o, part, bm):
    """Both bindings over canary-backed mirrors -> (out, acts, dzs, dx0)."""
    from openembedding_amd.ops import dispatch
    bufs = dispatch._tower_images(o.W, c.K0p, True, ext)
    held = [_mirror(c.M, h) for h in c.widths * 2] + [_mirror(c.M, c.K0p)]
    views = [v for _, v in held]
    acts, dzs, dx0 = views[:c.L], views[c.L:-1], views[-1]
    out = torch.full((c.M,), NAN, device=DEV)
    ext.tower_fwd(o.x0, c.K0, bufs["w"], o.b, acts, o.w_out, o.b_out,
                  o.partial if part else None, out, bm)
    ext.tower_bwd(c.K0, acts, bufs["wt"], o.dout, o.w_out, dzs, dx0, bm)
    for buf, view in held:
        assert bool((buf[view.numel():] == 7).all())
    return out, acts, dzs, dx0


def _same(got, want):
    return torch.equal(got.cpu().double(), want)


@pytest.mark.parametrize("bm", [0, 16, 32])
@pytest.mark.parametrize("K0,widths", GRID)
def test_exact_on_integers(K0, widths, bm):
    """Every sum of |terms| is below 2^24 (asserted): any summation order,
    the k-split's included, is exact. At the four-layer shapes over 10 % of
    a_3, a_L and dx0 round (asserted): equality pins nearest-even, the place
    of the bias add and the masks."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    B = bm or 16                       # the launcher picks 16 at these M
    for M in sorted({1, 17, B - 1, B + 1, 2 * B + 3}):
        c = _case(M, K0, widths, seed=1000 * K0 + 10 * len(widths) + M)
        r = _solve(c)
        assert r.mag < LIMIT
        if (K0, widths) in FOUR and M >= 17:
            for t in (r.pre[k] for k in ("a3", "a4", "dx0")):
                assert float((bf16_rne(t) != t).double().mean()) >= 0.10
        o = _operands(c)
        for part in (True, False):
            out, acts, dzs, dx0 = _kernels(ext, c, o, part, bm)
            assert _same(out, r.out if part else r.out_nopartial)
            for got, want in zip(acts + dzs + [dx0], r.a + r.dz + [r.dx0]):
                assert _same(got, want)


@pytest.mark.parametrize("bm", [0, 32])
@pytest.mark.parametrize("K0,widths", FOUR)
def test_random_within_intervals(K0, widths, bm):
    """M = 160, each stage recomputed in float64 from the kernel's own
    previous bf16 output; delta = cin_ref.bound(sum |terms|, n) with
    n = ceil32(K) + W + 2 for a stage whose contraction of K is cut W ways,
    H_L + 2 for the logit. Derived, nothing fitted."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    c = _case(160, K0, widths, seed=K0, integer=False)
    out, acts, dzs, dx0 = _kernels(ext, c, _operands(c), True, bm)
    acts, dzs = ([t.cpu().double() for t in ts] for ts in (acts, dzs))
    n = lambda nout, k: (ceil_to(k, 32)  # noqa: E731
                         + ext.tower_split(nout, k) + 2)
    bad, a = 0, c.x0
    for l in range(c.L):
        z, mag = _layer(a, c.W[l], c.b[l])
        bad += check_interval(acts[l], *interval(
            z, mag, n(widths[l], a.shape[1]), relu=True))[0]
        a = acts[l]
    ref, mag = _logit(a, c, True)
    worst = float(((out.cpu().double() - ref).abs()
                   / bound(mag, widths[-1] + 2)).max())
    assert _same(dzs[-1], bf16_rne(c.dout.unsqueeze(1) * c.w_out * (a > 0)))
    for l in range(c.L - 1, 0, -1):
        p, mag = dzs[l] @ c.W[l], dzs[l].abs() @ c.W[l].abs()
        bad += check_interval(dzs[l - 1], *interval(
            p, mag, n(widths[l - 1], widths[l]),
            mask=(acts[l - 1] > 0).to(f64)))[0]
    p, mag = dzs[0] @ c.W[0], dzs[0].abs() @ c.W[0].abs()
    bad += check_interval(dx0.cpu().double()[:, :K0], *interval(
        p, mag, n(c.K0p, widths[0])))[0]
    print(f"K0={K0} bm={bm}: logit err/delta {worst:.3f}, violations {bad}")
    assert bad == 0 and worst <= 1.0
    assert bool((dx0[:, K0:] == 0).all())


@pytest.mark.parametrize("K0,widths", [(50, (64, 32)),
                                       (247, (512, 256, 128, 32))])
def test_autograd_fresh_and_prebound(K0, widths):
    """Integers, M = 33: the wgrad sums are exact in fp32 too (asserted) and
    round once. Prebound bf16 grads accumulate in place: a second backward
    adds the same sums again, as it could not if autograd got them too."""
    from openembedding_amd.ops import dispatch
    c = _case(33, K0, widths, seed=7)
    r = _solve(c)
    assert r.mag < LIMIT
    o = _operands(c)
    ins = [c.x0] + r.a[:-1]
    sums = [dz.t() @ a for dz, a in zip(r.dz, ins)] \
        + [dz.sum(0) for dz in r.dz] \
        + [(c.dout.unsqueeze(1) * r.a[-1]).sum(0), c.dout.sum().view(1)]
    for prebound in (False, True):
        ps = [p.clone().requires_grad_() for p in o.W + o.b
              + [o.w_out, o.b_out]]
        xg = o.x0.clone().requires_grad_()
        pg = o.partial.clone().requires_grad_()
        for p in ps if prebound else []:
            p.grad = torch.zeros_like(p)
        acc = [torch.zeros_like(s) for s in sums]
        for _ in range(2 if prebound else 1):
            xg.grad = pg.grad = None
            out = dispatch.mlp_tower(xg, ps[:c.L], ps[c.L:2 * c.L], ps[-2],
                                     ps[-1], pg)
            assert _same(out, r.out)
            out.backward(o.dout)
            acc = [bf16_rne(a + s) for a, s in zip(acc, sums)]
            assert _same(xg.grad, r.dx0) and _same(pg.grad, c.dout)
            for p, w in zip(ps, acc):
                assert _same(p.grad, w)


REFUSALS = {                           # (K0, widths, what the message names)
    "K0p544": (530, (32,), "K0p"), "w528": (40, (528,), "multiple of 16"),
    "w24": (40, (24,), "multiple of 16"), "L5": (40, (16,) * 5, "L <= 4"),
    "fp32": (40, (32,), "bf16"), "strided": (40, (32,), "contiguous")}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_take_the_torch_route(case):
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    K0, widths, names = REFUSALS[case]
    c = _case(9, K0, widths, seed=5, integer=False)
    o = _operands(c)
    if case == "fp32":
        o.x0 = o.x0.float()
    if case == "strided":
        o.x0 = torch.cat([o.x0, o.x0], 1)[:, :c.K0p]
    kp = [c.K0p] + [ceil_to(h, 32) for h in widths[:-1]]
    imgs = [torch.zeros(h, k, dtype=bf, device=DEV)
            for h, k in zip(widths, kp)]
    with pytest.raises(RuntimeError, match=names):
        ext.tower_fwd(o.x0, K0, imgs, o.b, [], o.w_out, o.b_out, None,
                      torch.empty(9, device=DEV), 0)
    args = (o.x0, o.W, o.b, o.w_out, o.b_out, o.partial)
    got = dispatch.mlp_tower(*args)
    assert not dispatch._tower_fits(*args) and bool(torch.isfinite(got).all())
    assert torch.equal(got, dispatch._tower_torch(*args))


def test_models_route_to_the_tower():
    from openembedding_amd.models import WDL, DeepFM, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16
    from openembedding_amd.ops import dispatch
    vocabs = [50, 3, 1000, 40, 7] + [100] * 21
    torch.manual_seed(0)
    m = convert_mlp_bf16(WDL(field_vocabs=vocabs, dim=9,
                             hidden=(512, 256, 128, 32)).to(DEV))
    assert m.fused_tower and not m.fused_mlp
    dense, sparse, _ = (t.to(DEV) for t in synthetic_batch(
        48, field_vocabs=vocabs, generator=torch.Generator().manual_seed(1)))
    with torch.no_grad():
        logits = m(dense, sparse)
        _, deep_in, partial = m._fused_head(dense, sparse, use_fm=False)
        hidden = [m.dnn[i] for i in (0, 2, 4, 6)]
        want = dispatch.mlp_tower(
            deep_in, [h.weight for h in hidden], [h.bias for h in hidden],
            m.dnn[8].weight, m.dnn[8].bias, partial)
    assert bool(torch.isfinite(logits).all()) and torch.equal(logits, want)
    m(dense, sparse).sum().backward()
    assert bool(torch.isfinite(m.dnn[0].weight.grad.float()).all())
    m = convert_mlp_bf16(DeepFM(field_vocabs=vocabs, dim=9).to(DEV))
    assert m.fused_mlp and not m.fused_tower


def test_captured_step_replays_bit_identically():
    from openembedding_amd.ops import dispatch
    c = _case(70, 247, (512, 256, 128, 32), seed=9, integer=False)
    o = _operands(c)
    x0 = o.x0.requires_grad_()       # frozen parameters: no library GEMM

    def run():
        out = dispatch.mlp_tower(x0, o.W, o.b, o.w_out, o.b_out, o.partial)
        return (out.detach(),) + torch.autograd.grad(out, [x0], o.dout)

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
    del graph, static                # hand the capture's pool back
    gc.collect()


def _switch_args():              # integers so small that neither route rounds
    g =torch.Generator().manual_seed(11)
    c = _case(40, 50, (64, 32), seed=11)
    c.x0 = torch.randint(0, 2, c.x0.shape, generator=g).to(f64)
    c.W[0], c.b = c.W[0].sign(), [b.sign() for b in c.b]
    o = _operands(c)
    return c, (o.x0, o.W, o.b, o.w_out, o.b_out, o.partial)


def test_env_switch_keeps_the_torch_route():
    """Every intermediate is an integer <= 256, so the bf16 torch route of
    an OEAMD_TOWER=0 child rounds nothing and equals the fused logits."""
    from openembedding_amd.ops import dispatch
    assert dispatch._TOWER
    c, args = _switch_args()
    r = _solve(c)
    assert r.fwd_mag <= 256
    fused = dispatch.mlp_tower(*args).cpu().double()
    assert torch.equal(fused, r.out)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_gpu_tower as t\n"
            "from openembedding_amd.ops import dispatch\n"
            "assert not dispatch._TOWER\n"
            "print(*dispatch.mlp_tower(*t._switch_args()[1]).tolist())\n"
            % [here, os.path.dirname(here)])
    res = subprocess.run([sys.executable, "-c", code], check=True,
                         capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, OEAMD_TOWER="0"))
    child = torch.tensor([float(v) for v in res.stdout.split()], dtype=f64)
    assert torch.equal(child, fused)
