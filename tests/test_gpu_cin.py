"""CIN implicit-GEMM HIP kernels vs the chunked-torch oracle (all @gpu).

cin_fwd / cin_dw / cin_dx (ops/csrc/cin.hip) against _CINLayerFn's torch
path at identical bf16 operand precision, plus the end-to-end xDeepFM
training step."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _layer_io(B=512, F=26, H=128, O=128, d=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, F, d, generator=g).to(DEV)
    xk = torch.randn(B, H, d, generator=g).to(DEV)
    W = torch.randn(O, F * H, generator=g).to(DEV) * 0.05
    dout = torch.randn(B, O, d, generator=g).to(DEV)
    return x0, xk, W, dout


def _run(x0, xk, W, dout, force_torch):
    from openembedding_amd.models.ctr import _CINLayerFn
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    calls = []
    real = {n: getattr(ext, n) for n in ("cin_fwd", "cin_dx", "cin_dw")}

    def counted(name):
        def wrapper(*a):
            calls.append(name)
            return real[name](*a)
        return wrapper
    for name in real:
        setattr(ext, name, counted(name))
    x0 = x0.clone().requires_grad_(True)
    xk = xk.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    if force_torch:
        orig = _CINLayerFn._hip_ok
        _CINLayerFn._hip_ok = staticmethod(lambda *a: False)
    try:
        out = _CINLayerFn.apply(x0, xk, W, torch.bfloat16)
        out.backward(dout)
    finally:
        if force_torch:
            _CINLayerFn._hip_ok = orig
        for name, fn in real.items():
            setattr(ext, name, fn)
    # the HIP path was taken exactly when it was meant to be: without this
    # a False _hip_ok would compare the torch path with itself
    assert sorted(calls) == ([] if force_torch
                             else ["cin_dw", "cin_dx", "cin_fwd"]), calls
    return out.detach(), x0.grad, xk.grad, W.grad


@pytest.mark.parametrize("shape", [
    dict(),                              # benchmark layer 2
    dict(H=26, O=128),                   # benchmark layer 1 (xk = fields)
    dict(B=104, F=13, H=64, O=64, d=4),  # odd sizes, N=416 (%32==0)
])
def test_cin_kernels_match_torch(shape):
    io = _layer_io(**shape)
    out_h, dx0_h, dxk_h, dw_h = _run(*io, force_torch=False)
    out_t, dx0_t, dxk_t, dw_t = _run(*io, force_torch=True)
    # operands agree to bf16; the torch path additionally ROUNDS ITS
    # OUTPUTS to bf16 (library GEMM out dtype) while the kernels keep
    # fp32 accumulators, so the comparison tolerance is bf16-output-sized.
    # tests/test_gpu_cin_kernels.py holds the kernels to an exact oracle
    # (integer equality, derived fp32 bound) through their entry points;
    # this test pins end-to-end agreement of the two paths.
    torch.testing.assert_close(out_h, out_t, rtol=8e-2, atol=8e-2)
    torch.testing.assert_close(dx0_h, dx0_t, rtol=8e-2, atol=8e-2)
    torch.testing.assert_close(dxk_h, dxk_t, rtol=8e-2, atol=8e-2)
    torch.testing.assert_close(dw_h, dw_t, rtol=8e-2, atol=1.0)


def test_cin_kernels_match_fp32_reference():
    """Against the exact fp32 einsum (looser: the kernel stages bf16
    inputs and rounds the products to bf16, like the torch bf16 path)."""
    x0, xk, W, dout = _layer_io(B=256)
    out_h, dx0_h, dxk_h, dw_h = _run(x0, xk, W, dout, force_torch=False)
    z = torch.einsum("bfd,bhd->bfhd", x0, xk).reshape(256, -1, 9)
    ref = torch.einsum("ok,bkd->bod", W, z)
    torch.testing.assert_close(out_h, ref, rtol=8e-2, atol=8e-2)


def test_xdeepfm_trains_with_cin_kernels():
    import openembedding_amd.torch as embed
    from openembedding_amd.models import synthetic_batch, xDeepFM
    from openembedding_amd.models.ctr import convert_mlp_bf16

    torch.manual_seed(0)
    model = convert_mlp_bf16(xDeepFM(dim=9).to(DEV))
    assert model.cin.compute_dtype == torch.bfloat16
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01),
        flatten_dense=True)
    from openembedding_amd.ops.dispatch import bce_with_logits
    losses = []
    for _ in range(8):
        dense, sparse, labels = synthetic_batch(1024, device=DEV)
        opt.zero_grad(set_to_none=False)
        loss = bce_with_logits(model(dense, sparse).float(), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]
