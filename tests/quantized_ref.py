"""Helpers of the quantized-table tests: the error bound of the int8 format,
the inputs the bound is checked on, and the slab comparison the GPU tests
use (tests/test_quantized.py shows on the CPU that it rejects what it
should)."""

import torch

from openembedding_amd.ops import dispatch as ops

U = 2.0 ** -24      # unit roundoff of float32

# (magnitude, offset) of the random rows the bound is checked on
INPUTS = [(1.0, 0.0), (1e-3, 5.0), (100.0, -1e4), (1e-30, 0.0)]
BOUND_DIMS = [2, 9, 64, 130]
BOUND_ROWS = 4096


def bound_rows(dim: int, mag: float, off: float, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(BOUND_ROWS, dim, generator=g) * mag + off).float()


def int8_fields(packed: torch.Tensor, dim: int):
    """(codes uint8 [n, dim], pad uint8 [n, p], scale f32 [n], lo f32 [n])
    of int8 packed rows."""
    cw = ops.row_stride("int8", dim) - 8
    scale = packed[:, cw:cw + 4].contiguous().view(torch.float32).view(-1)
    lo = packed[:, cw + 4:].contiguous().view(torch.float32).view(-1)
    return packed[:, :dim], packed[:, dim:cw], scale, lo


def int8_bound(w: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """Per-row bound (float64) on |dequantize(quantize(x)) - x| of the int8
    format, from its operation sequence with u = 2^-24:

      d = fl(x - lo)            |d - (x - lo)|  <= u (hi - lo)
      q = fl(d / scale)         relative error u, q <= 255 (1 + 2u)
      code = rint(q)            |code - q| <= 1/2: half a step, scale / 2,
                                and the two roundings before it move q by
                                at most 255 * 2u, another 510 u scale
      p = fl(scale * code)      |p - scale code| <= u (hi - lo) (1 + ...)
      x^ = fl(lo + p)           |x^ - (lo + p)| <= u max(|lo|, |hi|) (1 + ..)
                                 <= 2 u max|row| with the higher-order terms

    i.e. scale / 2 + 510 u scale + u (3 (hi - lo) + 2 max|row|)."""
    _, _, scale, _ = int8_fields(packed, w.shape[1])
    lo = w.amin(1).double()
    hi = w.amax(1).double()
    top = w.abs().amax(1).double()
    s = scale.double()
    return s / 2 + 510 * U * s + U * (3 * (hi - lo) + 2 * top)


def slab_violations(got: torch.Tensor, want: torch.Tensor, dim: int,
                    fmt: str):
    """Why packed rows ``got`` are not the rows ``want`` (both uint8
    [n, stride]); [] when they are byte-identical. Fields are compared one
    by one so that a failure names what differs."""
    stride = ops.row_stride(fmt, dim)
    if got.shape != want.shape or got.dtype != torch.uint8 \
            or got.shape[1] != stride:
        return [f"shape/dtype {tuple(got.shape)} {got.dtype}, want "
                f"{tuple(want.shape)} uint8"]
    got, want = got.cpu(), want.cpu()
    bad = []
    if fmt == "int8":
        gc, gp, gs, gl = int8_fields(got, dim)
        wc, wp, ws, wl = int8_fields(want, dim)
        if not torch.equal(gc, wc):
            n = int((gc != wc).sum())
            bad.append(f"{n} codes differ")
        if not torch.equal(gs.view(torch.int32), ws.view(torch.int32)):
            bad.append("scale bits differ")
        if not torch.equal(gl.view(torch.int32), wl.view(torch.int32)):
            bad.append("lo bits differ")
    else:
        gp, wp = got[:, 2 * dim:], want[:, 2 * dim:]
        if not torch.equal(got[:, :2 * dim], want[:, :2 * dim]):
            bad.append("half bits differ")
    if bool((gp != 0).any()):
        bad.append("non-zero pad byte")
    if not bad and not torch.equal(got, want):
        bad.append("bytes differ")
    return bad
