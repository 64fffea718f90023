"""``ops.cross_network_lr`` on the CPU against ``ops.cross_network`` on
W = U V in float64, gradcheck, and the DCN model with ``low_rank``."""

import pytest
import torch

import cross_lr_ref as lr
from openembedding_amd.models import DCN, synthetic_batch
from openembedding_amd.ops.dispatch import cross_network, cross_network_lr

FIELD_VOCABS = [50, 3, 1000, 40, 7] + [100] * 21  # as tests/test_models.py


@pytest.mark.parametrize("logit", [True, False])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("d,rk", [(20, 3), (50, 16)])
def test_equals_full_rank_on_the_product(d, rk, L, pad, logit):
    c = lr.float_case(9, d, rk, L, seed=d + L)
    gen = torch.Generator().manual_seed(1)
    head = [c.w_out, c.b_out, c.partial] if logit else []
    gin = c.dout if logit else torch.randn(
        9, c.dp if pad else d, generator=gen).double()
    x0 = torch.nn.functional.pad(c.x0, (0, c.dp - d)) if pad else c.x0
    grads = []
    for low in (True, False):
        leaves = [t.clone().requires_grad_() for t in [x0, c.b] + head[:2]]
        ws = (c.U, c.V) if low else (c.U @ c.V,)
        fn = cross_network_lr if low else cross_network
        out = fn(leaves[0], *ws, leaves[1], *leaves[2:], *head[2:])
        out.backward(gin)
        grads.append([out.detach()] + [t.grad for t in leaves])
    assert grads[0][0].shape == ((9,) if logit else x0.shape)
    for got, want in zip(*grads):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_gradcheck_on_the_factors():
    """The x_L form: the logit form returns fp32, too coarse for finite
    differences."""
    c = lr.float_case(3, 6, 2, 2, seed=4)
    U, V = c.U.clone().requires_grad_(), c.V.clone().requires_grad_()
    assert torch.autograd.gradcheck(
        lambda u, v: cross_network_lr(c.x0, u, v, c.b), (U, V))
    with pytest.raises(ValueError):     # the factors swapped
        cross_network_lr(c.x0, c.V, c.U, c.b)


@pytest.mark.parametrize("structure", ["parallel", "stacked"])
def test_dcn_low_rank(structure):
    kw = dict(field_vocabs=FIELD_VOCABS, dim=4, cross_layers=2,
              structure=structure)
    d = 26 * 4 + 13
    model = DCN(low_rank=4, **kw)
    assert not hasattr(model, "cross_w")
    assert model.cross_u.shape == model.cross_v.mT.shape == (2, d, 4)
    dense, sparse, labels = synthetic_batch(
        32, field_vocabs=FIELD_VOCABS,
        generator=torch.Generator().manual_seed(1))
    out = model(dense, sparse)
    torch.nn.BCEWithLogitsLoss()(out, labels).backward()
    for p in (model.cross_u, model.cross_v, model.cross_b):
        assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.any())
    names = [n for n, _ in DCN(**kw).named_parameters() if "cross" in n]
    assert names[:2] == ["cross_w", "cross_b"]
