"""Reference side of tests/test_gpu_cin_kernels.py: plain torch on the CPU,
float64 and int64, no GPU and no extension import.

The references take the operands exactly as the entry points of
ops/csrc/cin.hip take them (``x0p [N,F]`` and ``xkp [N,H]`` fp32, ``W [O,K]``
bf16-representable, ``doutp [N,O]`` fp32, columns ``n = dd*B + b``) and
perform the kernels' roundings, so that only the fp32 accumulation separates
a kernel from its reference:

  - ``fwd_ref``: V = bf16(bf16(x0) * bf16(xk)), out = V . W^T;
  - ``dw_ref``:  B' = bf16(xkt * x0t) from the bf16 transposed operands,
    dW = dzt . B';
  - ``dx_ref``:  P = W^T . bf16(dout), contracted with the UNROUNDED fp32
    x0 / xk (the kernel's consume phase reads them as fp32);
  - ``bound``:   the derived worst-case error of such an fp32 accumulation;
  - ``int_case`` / ``int_oracle``: small-integer operands on which every
    intermediate is exact, so a kernel must EQUAL the int64 einsum;
  - ``pack_wp`` / ``pack_wt`` / ``pack_t``: the operand layouts that
    ``_CINLayerFn._bufs`` and its backward build, ``wt_rows`` included.

Each ``*_ref`` returns the value and ``mag``, the same sum over absolute
values, which is what ``bound`` scales. The references are themselves
tested in tests/test_cin_ref_checkers.py.
"""

from __future__ import annotations

import torch

bf16 = torch.bfloat16
f64 = torch.float64


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even), returned as float64. The value goes
    through fp32 first, like the kernels' ``(bf16)float``; every caller
    here passes values that fp32 holds exactly, so nothing rounds twice."""
    f = t.to(torch.float32)
    assert torch.equal(f.to(t.dtype), t), "value not exact in fp32"
    return f.to(bf16).to(f64)


def _is_bf16(t: torch.Tensor) -> bool:
    return torch.equal(t.to(torch.float32).to(bf16).to(t.dtype), t)


# ------------------------------------------------------------- references

def vmat(x0p, xkp):
    """V [N, F*H] as k_cin_fwd builds it: operands staged as bf16, the
    product (exact in fp32: 8 x 8 significand bits) rounded to bf16."""
    N, F = x0p.shape
    H = xkp.shape[1]
    v = bf16_rne(x0p).unsqueeze(2) * bf16_rne(xkp).unsqueeze(1)
    return bf16_rne(v).reshape(N, F * H)


def fwd_ref(x0p, xkp, W):
    """out [N, O] and mag of cin_fwd."""
    assert _is_bf16(W), "W must be bf16-representable"
    v = vmat(x0p, xkp)
    w = W.to(f64)
    return v @ w.t(), v.abs() @ w.abs().t()


def dw_ref(dzt, x0t, xkt):
    """dW [O, F*H] and mag of cin_dw from its bf16 operands dzt [O, Np],
    x0t [F, Np], xkt [H, Np]."""
    assert dzt.dtype == x0t.dtype == xkt.dtype == bf16
    O = dzt.shape[0]
    F, H = x0t.shape[0], xkt.shape[0]
    b = bf16_rne(xkt.to(f64).unsqueeze(0) * x0t.to(f64).unsqueeze(1))
    b = b.reshape(F * H, -1)                                   # [F*H, Np]
    dz = dzt.to(f64)
    return dz @ b.t(), dz.abs() @ b.abs().t()


def dx_ref(doutp, W, x0p, xkp):
    """(dx0 [N,F], dxk [N,H]) and their mags of cin_dx."""
    assert _is_bf16(W), "W must be bf16-representable"
    N, F = x0p.shape
    H = xkp.shape[1]
    dz = bf16_rne(doutp)
    w = W.to(f64)
    p = (dz @ w).view(N, F, H)
    pm = (dz.abs() @ w.abs()).view(N, F, H)
    x0, xk = x0p.to(f64), xkp.to(f64)
    dx0 = (p * xk.unsqueeze(1)).sum(2)
    dxk = (p * x0.unsqueeze(2)).sum(1)
    m0 = (pm * xk.abs().unsqueeze(1)).sum(2)
    mk = (pm * x0.abs().unsqueeze(2)).sum(1)
    return (dx0, dxk), (m0, mk)


def bound(mag, n_terms: int):
    """Worst-case error of an fp32 accumulation of ``n_terms`` terms whose
    absolute values sum to ``mag``, in any order: gamma_n * sum|terms|.
    The unit roundoff is taken as 2^-23 instead of 2^-24, so that an MFMA
    accumulate that does not round to nearest stays inside; 2^-126 covers
    a flush to zero. Derived, not measured: nothing here is tuned to the
    kernels. n_terms: Kp + 2 for fwd, Np + n_split + 2 for dW, Op + H + 2
    for dx0 and Op + F + 2 for dxk."""
    return n_terms * 2.0 ** -23 * mag + 2.0 ** -126


def err_ratio(got, ref, mag, n_terms: int) -> float:
    """max |got - ref| / bound; a kernel passes when this is <= 1."""
    got = got.detach().to("cpu", f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bound(mag, n_terms)).max())


# ------------------------------------------------------------------ cases

def float_case(N, F, H, O, seed=0):
    """randn operands, W = 0.05 * randn rounded to bf16 (fp32 tensors)."""
    g = torch.Generator().manual_seed(seed)
    x0p = torch.randn(N, F, generator=g)
    xkp = torch.randn(N, H, generator=g)
    W = (torch.randn(O, F * H, generator=g) * 0.05).to(bf16).float()
    doutp = torch.randn(N, O, generator=g)
    return x0p, xkp, W, doutp


def int_case(N, F, H, O, seed=0):
    """x0, xk, dout in {-3..3} and W in {-2..2}, as fp32. Every value a
    kernel forms is then an integer that bf16 (|V| <= 9: 4 bits) or fp32
    (every sum < 2^24) holds exactly, in any summation order, atomics
    included; the limits are asserted here."""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    x0p, xkp = ri(-3, 3, N, F), ri(-3, 3, N, H)
    W, doutp = ri(-2, 2, O, F * H), ri(-3, 3, N, O)
    Np = ceil_to(N, 32)
    assert F <= 32 and H <= 128 and O <= 128
    vmax = int((x0p.abs().max() * xkp.abs().max()).item())
    assert vmax <= 9                                  # 4 of bf16's 8 bits
    assert vmax * 2 * F * H <= 18 * 4096 < 2 ** 24    # fwd: |V| |W| K
    assert 3 * vmax * Np <= 27 * Np < 2 ** 24         # dW: |dz| |V| Np
    assert 2 * 3 * O <= 768                           # P: |W| |dz| O
    assert 768 * 3 * max(F, H) <= 768 * 3 * 128 < 2 ** 24   # dx0, dxk
    return x0p, xkp, W, doutp


def int_oracle(x0p, xkp, W, doutp):
    """out, dW, dx0, dxk of an integer case as naive int64 einsums."""
    x0, xk, w, dz = (t.to(torch.int64) for t in (x0p, xkp, W, doutp))
    for a, b in ((x0, x0p), (xk, xkp), (w, W), (dz, doutp)):
        assert torch.equal(a.to(b.dtype), b), "not an integer case"
    N, F = x0.shape
    H = xk.shape[1]
    v = (x0.unsqueeze(2) * xk.unsqueeze(1)).reshape(N, F * H)
    out = v @ w.t()
    dw = dz.t() @ v
    p = (dz @ w).view(N, F, H)
    dx0 = (p * xk.unsqueeze(1)).sum(2)
    dxk = (p * x0.unsqueeze(2)).sum(1)
    return out, dw, dx0, dxk


def layer_autograd(x0, xk, W, dout, same=False):
    """The layer in its own layout (x0 [B,F,d], xk [B,H,d], dout [B,O,d]):
    float64 autograd through einsum("bfd,bhd->bfhd"). Returns out, dx0,
    dxk, dW; with ``same`` x0 is used for both operands, as on the first
    CIN layer, and dx0 is the sum of both paths (dxk is None)."""
    a = x0.detach().to("cpu", f64).requires_grad_(True)
    b = a if same else xk.detach().to("cpu", f64).requires_grad_(True)
    w = W.detach().to("cpu", f64).requires_grad_(True)
    B, F, d = a.shape
    z = torch.einsum("bfd,bhd->bfhd", a, b).reshape(B, F * b.shape[1], d)
    out = torch.einsum("ok,bkd->bod", w, z)
    out.backward(dout.detach().to("cpu", f64))
    return out.detach(), a.grad, None if same else b.grad, w.grad


def to_layer(xp, d):
    """Columns [d*B, C] (n = dd*B + b) -> the layer's [B, C, d]."""
    return xp.view(d, xp.shape[0] // d, -1).permute(1, 2, 0).contiguous()


def to_cols(x):
    """The layer's [B, C, d] -> columns [d*B, C], as _CINLayerFn lays
    them out."""
    return x.permute(2, 0, 1).reshape(-1, x.shape[1]).contiguous()


def equals_int(got, want) -> bool:
    """A kernel's fp32 output equals the int64 oracle, element for
    element."""
    got = got.detach().cpu()
    return (got.shape == want.shape
            and torch.equal(got.to(f64), want.to(f64)))


# ---------------------------------------------------------------- packers

def wt_rows(F: int, H: int) -> int:
    """Rows of the cin_dx operand ``wt``. k_cin_dx loads a whole 16-row
    fragment for every h-tile of every field, so its last read row is
    (F-1)*H + ceil16(H) - 1, which can lie past ceil32(F*H)."""
    return ceil_to(max(F * H, (F - 1) * H + ceil_to(H, 16)), 32)


def wt_rows_read(F: int, H: int) -> int:
    """1 + the highest wt row k_cin_dx reads, by walking its loops: rows
    f*H + kt*16 + (lane & 15) for every field, h-tile and lane."""
    return 1 + max(f * H + kt * 16 + r for f in range(F)
                   for kt in range((H + 15) // 16) for r in range(16))


def pack_wp(W):
    """cin_fwd's weight: [O, ceil32(K)] bf16, zero k tail."""
    O, K = W.shape
    wp = torch.zeros(O, ceil_to(K, 32), dtype=bf16)
    wp[:, :K] = W
    return wp


def pack_wt(W, F, H):
    """cin_dx's weight: [wt_rows(F, H), ceil32(O)] bf16 transposed, zero
    tails."""
    O, K = W.shape
    assert K == F * H
    wt = torch.zeros(wt_rows(F, H), ceil_to(O, 32), dtype=bf16)
    wt[:K, :O] = W.t()
    return wt


def pack_t(x, Np=None):
    """cin_dw's operands: x [N, C] fp32 -> [C, Np] bf16, zero n tail."""
    N, C = x.shape
    Np = ceil_to(N, 32) if Np is None else Np
    t = torch.zeros(C, Np, dtype=bf16)
    t[:, :N] = x.t()
    return t
