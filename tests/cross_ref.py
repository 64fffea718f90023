"""Float64 oracle of the DCN-v2 cross network kernels (ops/csrc/cross.hip):
the arithmetic the kernels implement, written with plain torch ops.

Operands are bf16 values held in float64; every product and sum is exact
here and fp32 in the kernels, and ``bf16_rne`` stands wherever a kernel
rounds. On the integer cases every fp32 partial sum is an exact integer
(asserted), so a kernel must equal ``chain`` bit for bit; on random
operands ``stage``/``dgrad_intervals`` give, from the kernel's own previous
outputs, the bf16 values open to a kernel whose fp32 arithmetic stays
inside cin_ref.bound."""

from types import SimpleNamespace

import torch

from cin_ref import bound
from mlp_ref import bf16_rne

f64 = torch.float64


def stage(x0, xl, Wl, bl):
    """One forward layer from its inputs: (t, y, mag_t, mag_y) before
    rounding; u_l = bf16(t), x_{l+1} = bf16(y)."""
    t = xl @ Wl.t() + bl
    mag_t = xl.abs() @ Wl.abs().t() + bl.abs()
    return t, x0 * t + xl, mag_t, x0.abs() * mag_t + xl.abs()


def chain(x0, W, b, w_out=None, b_out=None, partial=None, gin=None):
    """The full forward and backward chain. gin: dout [M] in the logit form
    (w_out given), the incoming gradient [M, d] otherwise. ``mag`` is the
    largest sum of |terms| behind any value; ``inexact`` the share of x_L
    and of g_0 that are no bf16 values before rounding."""
    L = W.shape[0]
    r = SimpleNamespace(xs=[], us=[], qs=[], dW=[], db=[], mag=0.0)
    xl = x0
    for l in range(L):
        t, y, mag_t, mag = stage(x0, xl, W[l], b[l])
        r.mag = max(r.mag, float(mag.max()), float(mag_t.max()))
        r.us.append(bf16_rne(t))
        xn = bf16_rne(y)
        r.inexact_x = float((xn != y).double().mean())
        r.xs.append(xn)
        xl = xn
    if w_out is not None:
        r.out = xl @ w_out + b_out
        mag = xl.abs() @ w_out.abs() + b_out.abs()
        if partial is not None:
            r.out, mag = r.out + partial, mag + partial.abs()
        r.mag = max(r.mag, float(mag.max()))
    if gin is None:
        return r
    g = bf16_rne(gin.unsqueeze(1) * w_out) if w_out is not None \
        else bf16_rne(gin)
    a = torch.zeros_like(x0)
    amag = torch.zeros_like(x0)
    xin = [x0] + r.xs[:-1]
    for l in reversed(range(L)):
        q = bf16_rne(g * x0)
        a, amag = a + g * r.us[l], amag + (g * r.us[l]).abs()
        pre = q @ W[l] + g
        r.mag = max(r.mag, float((q.abs() @ W[l].abs() + g.abs()).max()),
                    float((q.abs().t() @ xin[l].abs()).max()),
                    float(q.abs().sum(0).max()))
        g = bf16_rne(pre)
        r.inexact_g = float((g != pre).double().mean())
        r.qs.insert(0, q)
        r.dW.insert(0, q.t() @ xin[l])
        r.db.insert(0, q.sum(0))
    r.mag = max(r.mag, float((amag + g.abs()).max()))
    r.dx0 = bf16_rne(a + g)
    if w_out is not None:
        r.dwo, r.dbo = gin @ xl, gin.sum()
        r.mag = max(r.mag, float((gin.abs() @ xl.abs()).max()))
    return r


def int_case(M, d, L, seed=0):
    """Integer operands in the ranges under which every sum of |terms|
    stays below 2^24 (asserted by ``solve``): x0, w_out in {-1, 0, 1}, W in
    {-1, 0, 1} at half density, b, dout in {-2..2}, partial in {-9..9}, and
    an incoming gradient in {-2..2} for the x_L form."""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(f64)
    c = SimpleNamespace(M=M, d=d, L=L, dp=(d + 31) // 32 * 32)
    c.x0 = ri(-1, 1, M, d)
    c.W = ri(-1, 1, L, d, d) * ri(0, 1, L, d, d)
    c.b, c.w_out, c.b_out = ri(-2, 2, L, d), ri(-1, 1, d), ri(-2, 2, 1)
    c.dout, c.partial, c.gx = ri(-2, 2, M), ri(-9, 9, M), ri(-2, 2, M, d)
    return c


def float_case(M, d, L, seed=0):
    """randn operands rounded to bf16, W ~ 1/sqrt(d): L = 6 does not grow."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, s=1.0):
        return bf16_rne(torch.randn(*shape, generator=g) * s)
    c = SimpleNamespace(M=M, d=d, L=L, dp=(d + 31) // 32 * 32)
    c.x0, c.W, c.b = rn(M, d), rn(L, d, d, s=d ** -0.5), rn(L, d, s=0.1)
    c.w_out, c.b_out = rn(d, s=d ** -0.5), rn(1)
    c.dout, c.partial = torch.randn(M, generator=g).float().to(f64), \
        torch.randn(M, generator=g).float().to(f64)
    return c


def solve(c, logit, with_partial=True):
    """``chain`` on an integer case, with the exactness limits asserted."""
    r = chain(c.x0, c.W, c.b, *((c.w_out, c.b_out,
                                 c.partial if with_partial else None)
                                if logit else ()),
              gin=c.dout if logit else c.gx)
    assert r.mag < 2 ** 24, r.mag
    if c.d >= 247 and c.L >= 3:
        assert r.inexact_x >= 0.01 and r.inexact_g >= 0.01
    return r


def dgrad_intervals(gL, x0, us, qs, W, dp):
    """[(q_lo, q_hi)] * L and (dx_lo, dx_hi): the values open to the
    backward kernel, each stage's sum recomputed from the KERNEL's q_l.
    g_l is no output, so it is carried as an interval [glo, ghi] (exact at
    g_L); products and roundings are monotone, sums get cin_ref.bound with
    n = dp + 3 (dp - 1 adds, the residual, margin of two) and L + 2 for a."""
    L = W.shape[0]
    glo = ghi = gL
    alo = ahi = amag = torch.zeros_like(x0)
    qiv = []
    for l in reversed(range(L)):
        e0, e1 = bf16_rne(glo * x0), bf16_rne(ghi * x0)
        qiv.insert(0, (torch.minimum(e0, e1), torch.maximum(e0, e1)))
        p0, p1 = glo * us[l], ghi * us[l]
        alo, ahi = alo + torch.minimum(p0, p1), ahi + torch.maximum(p0, p1)
        gabs = torch.maximum(glo.abs(), ghi.abs())
        amag = amag + gabs * us[l].abs()
        s = qs[l] @ W[l]
        dl = bound(qs[l].abs() @ W[l].abs() + gabs, dp + 3)
        glo, ghi = bf16_rne(s + glo - dl), bf16_rne(s + ghi + dl)
    da = bound(amag + torch.maximum(glo.abs(), ghi.abs()), L + 2)
    return qiv, (bf16_rne(alo + glo - da), bf16_rne(ahi + ghi + da))
