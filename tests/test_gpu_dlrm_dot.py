"""k_dot_interact_fwd / k_dot_interact_bwd (ops/csrc/dlrm.hip) through their
bindings against a float64 einsum: bit for bit on integer operands, inside
the derived fp32 bound (cin_ref.bound) on random ones; the binding's
refusals and the torch route behind them; the DLRM model captured."""

import os
import subprocess
import sys

import pytest
import torch

import cin_ref as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# T = 16 / 17 either side of the second row tile, D either side of a k-step
GRID = [(1, 1), (2, 9), (15, 16), (16, 33), (26, 31), (26, 32), (26, 64),
        (31, 128)]
# the launcher picks 4 samples per block (2 for the (31, 128) backward):
# 5 and 257 end in a partial block behind full ones, 1 is a lone partial
BATCHES = [1, 5, 257]
MODES = [(bf, pad) for bf in (False, True) for pad in (False, True)]


def _ref(e, x, g):
    """float64 (out, de, dx) and the sums of |terms| behind (tri, de, dx);
    e, x, g are the operands as the kernels see them, g unpadded."""
    D = x.shape[1]
    v = torch.cat([x.unsqueeze(1), e], 1)
    T = v.shape[1]
    li, lj = torch.tril_indices(T, T, -1)
    out = torch.cat([x, torch.einsum("bid,bjd->bij", v, v)[:, li, lj]], 1)
    mag = torch.einsum("bid,bjd->bij", v.abs(), v.abs())[:, li, lj]
    s = torch.zeros(e.shape[0], T, T, dtype=torch.float64)
    s[:, li, lj] = g[:, D:]
    s = s + s.transpose(1, 2)
    dv = torch.einsum("bij,bjd->bid", s, v)
    dmag = torch.einsum("bij,bjd->bid", s.abs(), v.abs())
    dv[:, 0] += g[:, :D]
    dmag[:, 0] += g[:, :D].abs()
    return out, dv[:, 1:], dv[:, 0], mag, dmag[:, 1:], dmag[:, 0]


def _poison_allocator(nbytes):
    """Free blocks of the size of the next ``out``, full of NaN patterns
    (as bf16 pairs and as fp32): the caching allocator hands a freed block
    of the same size class back, from the small pool too."""
    junk = [torch.full(((nbytes + 3) // 4,), 0x7FC07FC0, dtype=torch.int32,
                       device=DEV) for _ in range(4)]
    del junk


def _in_canaries(e):
    """e as a contiguous view between two canary rows of a larger buffer."""
    buf = torch.full((e.shape[0] + 2,) + e.shape[1:], 7.0, device=DEV)
    buf[1:-1] = e
    return buf, buf[1:-1]


def _pad(g, W):
    return torch.nn.functional.pad(g, (0, W - g.shape[1])).contiguous()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,D", GRID)
def test_exact_on_integers(F, D, B):
    """|dot| <= 9 D <= 1152 and |dV| <= 31 * 9 + 3: fp32 is exact in any
    order, so fp32 outputs equal the integer reference and bf16 ones its
    nearest-even rounding. At (31, 128) the operands are in {1, 2, 3}: the
    dots are in the hundreds, most are no bf16 values and many are ties."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    gen = torch.Generator().manual_seed(100 * F + D + B)
    lo = 1 if D == 128 else -3
    P = F * (F + 1) // 2
    e = torch.randint(lo, 4, (B, F, D), generator=gen).double()
    x = torch.randint(lo, 4, (B, D), generator=gen).double()
    g = torch.randint(-3, 4, (B, D + P), generator=gen).double()
    out_r, de_r, dx_r = _ref(e, x, g)[:3]
    if D == 128:
        t = out_r[:, D:]
        ulp = 2.0 ** (torch.frexp(t)[1] - 8).double()
        ties = (t - t.to(torch.bfloat16).double()).abs() * 2 == ulp
        assert ties.double().mean() >= 0.01
    buf, ed = _in_canaries(e.float())
    xd = x.float().to(DEV)
    for out_bf16, pad32 in MODES:
        dt = torch.bfloat16 if out_bf16 else torch.float32
        W = cr.ceil_to(D + P, 32) if pad32 else D + P
        _poison_allocator(B * W * (2 if out_bf16 else 4))
        out = ext.dot_interact_fwd(ed, xd, out_bf16, pad32)
        assert out.shape == (B, W) and out.dtype == dt
        assert torch.equal(out[:, :D + P].cpu(), out_r.to(dt))
        assert bool((out[:, D + P:] == 0).all())
        de, dx = ext.dot_interact_bwd(ed, xd, _pad(g, W).to(dt).to(DEV),
                                      pad32)
        assert de.dtype == dx.dtype == torch.float32 and de.is_contiguous()
        assert torch.equal(de.cpu().double(), de_r)
        assert torch.equal(dx.cpu().double(), dx_r)
    assert bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,D", GRID)
def test_random_within_bound(F, D, B):
    """randn operands against float64 on the bf16-rounded operands:
    delta = n 2^-23 sum|terms| + 2^-126, n = Dp + 2 forward and 32 + 3
    backward (one k-step and the g[:, :D] add)."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    gen = torch.Generator().manual_seed(7 * F + D + B)
    P = F * (F + 1) // 2
    e = torch.randn(B, F, D, generator=gen)
    x = torch.randn(B, D, generator=gen)
    g = torch.randn(B, D + P, generator=gen)
    out_r, de_r, dx_r, mag, de_m, dx_m = _ref(
        cr.bf16_rne(e), cr.bf16_rne(x), cr.bf16_rne(g))
    delta = cr.bound(mag, cr.ceil_to(D, 32) + 2)
    _, ed = _in_canaries(e)
    xd = x.to(DEV)
    for out_bf16, pad32 in MODES:
        dt = torch.bfloat16 if out_bf16 else torch.float32
        W = cr.ceil_to(D + P, 32) if pad32 else D + P
        out = ext.dot_interact_fwd(ed, xd, out_bf16, pad32).cpu()
        assert torch.equal(out[:, :D], x.to(dt))      # the unrounded x
        tri = out[:, D:D + P].double()
        # bf16: fp32 -> bf16 is monotone, so the rounded accumulator lies
        # between the rounded ends of [ref - delta, ref + delta]
        lo = (out_r[:, D:] - delta).float().to(dt).double()
        hi = (out_r[:, D:] + delta).float().to(dt).double()
        assert int(((tri < lo) | (tri > hi)).sum()) == 0
        # fp32 g is rounded by the kernel, bf16 g arrives rounded
        de, dx = ext.dot_interact_bwd(ed, xd, _pad(g, W).to(dt).to(DEV),
                                      pad32)
        r_de = cr.err_ratio(de, de_r, de_m, 35)
        r_dx = cr.err_ratio(dx, dx_r, dx_m, 35)
        # a bf16 out is judged by the interval above, an fp32 one by delta
        r_f = 0.0 if out_bf16 else cr.err_ratio(
            tri, out_r[:, D:], mag, cr.ceil_to(D, 32) + 2)
        print(f"F={F} D={D} B={B} bf16={out_bf16}: err/delta fwd "
              f"{r_f:.3f} de {r_de:.3f} dx {r_dx:.3f}")
        assert r_f <= 1.0 and r_de <= 1.0 and r_dx <= 1.0


@pytest.mark.parametrize("case", ["F32", "D129", "strided", "fp64"])
def test_refusals_take_the_torch_route(case):
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    F, D = {"F32": (32, 8), "D129": (3, 129)}.get(case, (5, 12))
    gen = torch.Generator().manual_seed(11)
    e = torch.randn(6, F, D, generator=gen).to(DEV)
    x = torch.randn(6, D, generator=gen).to(DEV)
    if case == "strided":
        e = torch.randn(6, D, F, generator=gen).to(DEV).transpose(1, 2)
    if case == "fp64":
        e, x = e.double(), x.double()
    with pytest.raises(RuntimeError):
        ext.dot_interact_fwd(e, x, False, False)
    with pytest.raises(RuntimeError):
        ext.dot_interact_bwd(e, x, torch.zeros(
            6, D + F * (F + 1) // 2, device=DEV), False)
    out = dispatch.dot_interact(e, x)
    out_r, _, _, mag = _ref(cr.bf16_rne(e.cpu().float()),
                            cr.bf16_rne(x.cpu().float()),
                            torch.zeros(6, out.shape[1],
                                        dtype=torch.float64))[:4]
    assert out.dtype == torch.float32 and out.shape == out_r.shape
    assert cr.err_ratio(out[:, D:], out_r[:, D:], mag,
                        cr.ceil_to(D, 32) + 2) <= 1.0


@pytest.mark.parametrize("out_bf16,pad32", MODES)
def test_autograd_is_the_backward_kernel(out_bf16, pad32):
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    gen = torch.Generator().manual_seed(5)
    e = torch.randn(9, 26, 16, generator=gen).to(DEV).requires_grad_()
    x = torch.randn(9, 16, generator=gen).to(DEV).requires_grad_()
    out = dispatch.dot_interact(e, x, out_bf16, pad32)
    assert torch.equal(out, ext.dot_interact_fwd(e, x, out_bf16, pad32))
    g = torch.randn(out.shape, generator=gen).to(DEV).to(out.dtype)
    out.backward(g)
    de, dx = ext.dot_interact_bwd(e.detach(), x.detach(), g, pad32)
    assert torch.equal(e.grad, de) and torch.equal(x.grad, dx)


_CHILD = """
import sys, torch
from openembedding_amd.ops import dispatch
assert not dispatch._DLRM_DOT
e, x = torch.load(sys.argv[1])
torch.save(dispatch.dot_interact(e.cuda(), x.cuda(), True, True).cpu(),
           sys.argv[2])
"""


def test_model_captured_and_torch_route_child(tmp_path):
    """DLRM(dim=16) with the bf16 fused MLP: one captured forward +
    backward, replayed twice on the same inputs, is bit-identical to itself
    and to eager; a child process with OEAMD_DLRM_DOT=0 builds deep_in from
    the same (e, x) inside the interval of the forward bound."""
    from openembedding_amd.models import DLRM, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16

    vocabs = [50, 3, 1000, 40, 7] + [100] * 21
    torch.manual_seed(0)
    model = convert_mlp_bf16(DLRM(field_vocabs=vocabs, dim=16,
                                  bottom=(32,), hidden=(64, 64, 64)).to(DEV))
    assert model.fused_mlp
    dense, sparse, labels = (t.to(DEV) for t in synthetic_batch(
        64, field_vocabs=vocabs, generator=torch.Generator().manual_seed(1)))
    kept = {}
    model.embedding.register_forward_hook(
        lambda m, i, o: kept.__setitem__("e", o))
    model.bottom_mlp.register_forward_hook(
        lambda m, i, o: kept.__setitem__("x", o))
    lossf = torch.nn.BCEWithLogitsLoss()

    def run():
        logits = model(dense, sparse)
        de, dx = torch.autograd.grad(lossf(logits, labels),
                                     [kept["e"], kept["x"]])
        return logits.detach(), de, dx

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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager):
            assert torch.equal(got, want)

    from openembedding_amd.ops import dispatch
    assert dispatch._DLRM_DOT
    deep_in = dispatch.dot_interact(kept["e"].detach(), kept["x"].detach(),
                                    True, True).cpu()
    e, x = kept["e"].detach().cpu(), kept["x"].detach().cpu()
    torch.save((e, x), tmp_path / "in.pt")
    env = dict(os.environ, OEAMD_DLRM_DOT="0")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD,
                        str(tmp_path / "in.pt"), str(tmp_path / "out.pt")],
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    child = torch.load(tmp_path / "out.pt")
    assert child.shape == deep_in.shape and child.dtype == torch.bfloat16
    out_r, _, _, mag = _ref(cr.bf16_rne(e), cr.bf16_rne(x),
                            torch.zeros(64, 16 + 351,
                                        dtype=torch.float64))[:4]
    delta = cr.bound(mag, 32 + 2)
    lo = (out_r[:, 16:] - delta).float().to(torch.bfloat16).double()
    hi = (out_r[:, 16:] + delta).float().to(torch.bfloat16).double()
    for t in (child, deep_in):
        tri = t[:, 16:16 + 351].double()
        assert int(((tri < lo) | (tri > hi)).sum()) == 0
        assert torch.equal(t[:, :16], x.to(torch.bfloat16))
        assert bool((t[:, 16 + 351:] == 0).all())
