"""The cross network on the CPU: the torch route of ``ops.cross_network``
and the oracle of cross_ref.py against float64 autograd of the plain
formula; the DCN model trains and is refused by the TF export."""

import pytest
import torch

import cross_ref as xr
import openembedding_amd.torch as embed
from openembedding_amd.models import MODELS, synthetic_batch
from openembedding_amd.ops.dispatch import cross_network

FIELD_VOCABS = [50, 3, 1000, 40, 7] + [100] * 21  # as tests/test_models.py


def _plain(x0, W, b, w_out=None, b_out=None, partial=None):
    x = x0
    for l in range(W.shape[0]):
        x = x0 * (x @ W[l].t() + b[l]) + x
    return x if w_out is None else x @ w_out + b_out + partial


@pytest.mark.parametrize("logit", [True, False])
def test_torch_route_and_oracle_equal_float64_autograd(logit):
    """d = 50, L = 2, M = 17 on integers: every value stays below 256, so
    nothing rounds and the three must agree exactly."""
    c = xr.int_case(17, 50, 2, seed=3)
    r = xr.solve(c, logit)
    names = ["x0", "W", "b"] + (["w_out", "b_out", "partial"] if logit
                                else [])
    leaves = [getattr(c, n).clone().requires_grad_() for n in names]
    gin = c.dout if logit else c.gx
    _plain(*leaves).backward(gin)
    want = [t.grad for t in leaves]
    got_ref = [r.dx0, torch.stack(r.dW), torch.stack(r.db)] + (
        [r.dwo, r.dbo.view(1), c.dout] if logit else [])
    for n, w, g in zip(names, want, got_ref):
        assert torch.equal(w, g), n
    assert torch.equal(_plain(*leaves).detach(), r.out if logit else r.xs[-1])
    # the operator, on a 32-padded x0 as well
    for pad in (0, c.dp - c.d):
        ops = [t.detach().clone().requires_grad_() for t in leaves]
        x0p = torch.nn.functional.pad(ops[0], (0, pad))
        out = cross_network(x0p, *ops[1:])
        assert out.shape == ((17,) if logit else (17, c.d + pad))
        out.backward(gin if logit else torch.nn.functional.pad(gin, (0, pad)))
        assert torch.equal(out.detach()[..., :c.d] if not logit
                           else out.detach(),
                           (r.out if logit else r.xs[-1]).to(out.dtype))
        for n, w, t in zip(names, want, ops):
            assert torch.equal(w, t.grad), n
        if not logit:
            assert bool((out[:, c.d:] == 0).all())


@pytest.mark.parametrize("structure", ["parallel", "stacked"])
def test_dcn_trains_and_export_refuses(structure):
    torch.manual_seed(0)
    model = MODELS["dcn"](field_vocabs=FIELD_VOCABS, dim=4, cross_layers=2,
                          structure=structure)
    assert model.cross_w.shape == (2, 26 * 4 + 13, 26 * 4 + 13)
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad([p for p in model.parameters() if p.numel()],
                            lr=0.05))
    lossf = torch.nn.BCEWithLogitsLoss()
    dense, sparse, labels = synthetic_batch(
        256, field_vocabs=FIELD_VOCABS,
        generator=torch.Generator().manual_seed(1))
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
    from openembedding_amd import export_tf
    with pytest.raises(NotImplementedError, match="DCN"):
        export_tf.build_graph(model)
