"""DLRM on the CPU: the model trains, and the torch route of
``ops.dispatch.dot_interact`` equals a float64 double loop."""

import pytest
import torch

import cin_ref as cr
import openembedding_amd.torch as embed
from openembedding_amd.models import MODELS, synthetic_batch
from openembedding_amd.ops.dispatch import dot_interact

FIELD_VOCABS = [50, 3, 1000, 40, 7] + [100] * 21  # as tests/test_models.py


def test_dlrm_trains():
    torch.manual_seed(0)
    model = MODELS["dlrm"](field_vocabs=FIELD_VOCABS, dim=4)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad([p for p in model.parameters() if p.numel()],
                            lr=0.05))
    lossf = torch.nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(1)
    dense, sparse, labels = synthetic_batch(256, field_vocabs=FIELD_VOCABS,
                                            generator=g)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        out = model(dense, sparse)
        assert out.shape == (256,)
        loss = lossf(out, labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def test_tf_export_refuses_dlrm():
    from openembedding_amd import export_tf
    model = MODELS["dlrm"](field_vocabs=FIELD_VOCABS, dim=4)
    with pytest.raises(NotImplementedError, match="DLRM"):
        export_tf.build_graph(model)


def test_dot_interact_torch_route_matches_double_loop():
    B, F, D = 4, 3, 5
    T, P = F + 1, (F + 1) * F // 2
    gen = torch.Generator().manual_seed(3)
    e = torch.randn(B, F, D, generator=gen, requires_grad=True)
    x = torch.randn(B, D, generator=gen, requires_grad=True)
    g = torch.randn(B, D + P, generator=gen)
    out = dot_interact(e, x)
    assert out.shape == (B, D + P) and out.dtype == torch.float32
    out.backward(g)
    padded = dot_interact(e.detach(), x.detach(), out_bf16=True, pad32=True)
    assert padded.shape == (B, 32) and padded.dtype == torch.bfloat16
    assert bool((padded[:, D + P:] == 0).all())

    v = cr.bf16_rne(torch.cat([x.detach().unsqueeze(1), e.detach()], 1))
    gr = cr.bf16_rne(g)
    ref = torch.zeros(B, D + P, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    dv = torch.zeros(B, T, D, dtype=torch.float64)
    dmag = torch.zeros_like(dv)
    ref[:, :D] = x.detach().double()
    for i in range(T):
        for j in range(i):
            c = D + i * (i - 1) // 2 + j
            ref[:, c] = (v[:, i] * v[:, j]).sum(1)
            mag[:, c] = (v[:, i] * v[:, j]).abs().sum(1)
            dv[:, i] += gr[:, c:c + 1] * v[:, j]
            dv[:, j] += gr[:, c:c + 1] * v[:, i]
            dmag[:, i] += (gr[:, c:c + 1] * v[:, j]).abs()
            dmag[:, j] += (gr[:, c:c + 1] * v[:, i]).abs()
    dv[:, 0] += gr[:, :D]
    dmag[:, 0] += gr[:, :D].abs()
    assert torch.equal(out[:, :D].detach(), x.detach())
    assert cr.err_ratio(out[:, D:], ref[:, D:], mag[:, D:], D + 2) <= 1.0
    assert cr.err_ratio(e.grad, dv[:, 1:], dmag[:, 1:], T + 2) <= 1.0
    assert cr.err_ratio(x.grad, dv[:, 0], dmag[:, 0], T + 2) <= 1.0
