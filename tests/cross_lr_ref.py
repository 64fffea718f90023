"""Float64 oracle of the low-rank cross kernels (ops/csrc/cross_lr.hip):
``bf16_rne`` stands wherever a kernel rounds; ``mag`` is the largest sum of
|terms| behind any value of the chain."""

from types import SimpleNamespace

import torch

import cross_ref as xr
from cin_ref import bound
from mlp_ref import bf16_rne


def chain(x0, U, V, b, w_out=None, b_out=None, partial=None, gin=None):
    """Forward and, with gin (dout [M] or the gradient [M, d]), backward.
    ``inexact``: the shares of x_L, p, s, g_0 that round."""
    L = U.shape[0]
    r = SimpleNamespace(xs=[], us=[], ps=[], qs=[], ss=[], dU=[], dV=[],
                        db=[], mag=0.0, inexact={})

    def rnd(name, v, *mags):
        r.mag = max([r.mag] + [float(m.max()) for m in mags])
        out = bf16_rne(v)
        r.inexact[name] = float((out != v).double().mean())
        return out
    xl = x0
    for l in range(L):
        p = rnd("p", xl @ V[l].t(), xl.abs() @ V[l].abs().t())
        t = p @ U[l].t() + b[l]
        mag_t = p.abs() @ U[l].abs().t() + b[l].abs()
        r.us.append(bf16_rne(t))
        r.ps.append(p)
        xl = rnd("x", x0 * t + xl, mag_t, x0.abs() * mag_t + xl.abs())
        r.xs.append(xl)
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
    a = amag = torch.zeros_like(x0)
    xin = [x0] + r.xs[:-1]
    for l in reversed(range(L)):
        q = bf16_rne(g * x0)
        a, amag = a + g * r.us[l], amag + (g * r.us[l]).abs()
        s = rnd("s", q @ U[l], q.abs() @ U[l].abs())
        if L == 1:     # the parameter gradients are compared at L = 1 only
            r.mag = max(r.mag, float((q.abs().t() @ r.ps[l].abs()).max()),
                        float((s.abs().t() @ xin[l].abs()).max()),
                        float(q.abs().sum(0).max()))
        r.qs.insert(0, q)
        r.ss.insert(0, s)
        r.dU.insert(0, q.t() @ r.ps[l])
        r.dV.insert(0, s.t() @ xin[l])
        r.db.insert(0, q.sum(0))
        g = rnd("g", s @ V[l] + g, s.abs() @ V[l].abs() + g.abs())
    r.mag = max(r.mag, float((amag + g.abs()).max()))
    r.dx0 = bf16_rne(a + g)
    if w_out is not None:
        r.dwo, r.dbo = gin @ xl, gin.sum()
        if L == 1:
            r.mag = max(r.mag, float((gin.abs() @ xl.abs()).max()))
    return r


def _case(c, rk, seed, draw):
    """cross_ref's operands (W unused) with the factors U, V added."""
    g = torch.Generator().manual_seed(seed + 1)
    c.r, c.rp = rk, (rk + 31) // 32 * 32
    c.U, c.V = draw(g, c.L, c.d, rk), draw(g, c.L, rk, c.d)
    return c


def int_case(M, d, rk, L, seed=0):
    """cross_ref.int_case with U, V in {-1, 0, 1} at density 1/4."""
    def draw(g, *s):
        return (torch.randint(-1, 2, s, generator=g)
                * (torch.randint(0, 4, s, generator=g) == 0)).double()
    return _case(xr.int_case(M, d, L, seed), rk, seed, draw)


def float_case(M, d, rk, L, seed=0):
    """cross_ref.float_case with V ~ 1/sqrt(d), U ~ 1/sqrt(r)."""
    def draw(g, *s):
        return bf16_rne(torch.randn(*s, generator=g) * s[-1] ** -0.5)
    return _case(xr.float_case(M, d, L, seed), rk, seed, draw)


def solve(c, logit, with_partial=True):
    """``chain`` on an integer case, the exactness limits asserted; s and
    g_0 are exempt where one row's dout, which may be 0, is all there is."""
    r = chain(c.x0, c.U, c.V, c.b, *((c.w_out, c.b_out,
                                      c.partial if with_partial else None)
                                     if logit else ()),
              gin=c.dout if logit else c.gx)
    assert r.mag < 2 ** 24, r.mag
    if c.d >= 247 and c.L >= 3:
        keys = "xp" if logit and c.M < 15 else "xpsg"
        assert min(r.inexact[k] for k in keys) >= 0.01, r.inexact
    return r


def torch_route(c, u=2.0 ** -9):
    """(x_L, e): the unrounded float64 formula and a bound of the torch
    route's distance from it: each of its four ops a layer rounds once
    (relative u) after an fp32 sum; errors pass through |V|, |U|, |x0|."""
    def op(v, e_in, mag, n):
        e = e_in + bound(mag + e_in, n)
        return e + u * (v.abs() + e)
    x, e, a0 = c.x0, torch.zeros_like(c.x0), c.x0.abs()
    for l in range(c.L):
        Ua, Va = c.U[l].abs().t(), c.V[l].abs().t()
        p = x @ c.V[l].t()
        ep = op(p, e @ Va, x.abs() @ Va, c.d + 2)
        t = p @ c.U[l].t() + c.b[l]
        et = op(t, ep @ Ua, p.abs() @ Ua + c.b[l].abs(), c.r + 3)
        m = c.x0 * t
        em = op(m, a0 * et, m.abs(), 2)
        x, e = m + x, op(m + x, em + e, m.abs() + x.abs(), 2)
    return x, e
