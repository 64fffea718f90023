"""The MLP tower on the CPU: the torch route of ``ops.mlp_tower`` against
``nn.Sequential``, its argument checks, and the towers for which
``convert_mlp_bf16`` sets ``fused_tower``."""

import pytest
import torch

from openembedding_amd.models import WDL
from openembedding_amd.models.ctr import _mlp, convert_mlp_bf16
from openembedding_amd.ops.dispatch import mlp_tower

FIELD_VOCABS = [50, 3, 1000, 40, 7] + [100] * 21  # as tests/test_models.py


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("pad", [0, 14])
def test_torch_route_equals_sequential(dtype, pad):
    """Integer operands whose sums stay below 2^24 (3 * 50 * 48 * 16 * 32):
    nothing rounds, so the two must agree exactly whatever the op order."""
    g = torch.Generator().manual_seed(0)
    seq = _mlp(50, (48, 16, 32)).to(dtype)
    for p in seq.parameters():
        p.data = torch.randint(-1, 2, p.shape, generator=g).to(dtype)
    x0 = torch.randint(-3, 4, (17, 50), generator=g).to(dtype)
    partial = torch.randint(-9, 10, (17,), generator=g).float()
    hidden = seq[0:-1:2]
    out = mlp_tower(torch.nn.functional.pad(x0, (0, pad)),
                    [m.weight for m in hidden], [m.bias for m in hidden],
                    seq[-1].weight, seq[-1].bias, partial)
    assert out.dtype == torch.float32 and out.shape == (17,)
    assert torch.equal(out, seq(x0).squeeze(1).float() + partial)
    dw, = torch.autograd.grad(out.sum(), [seq[0].weight])
    want, = torch.autograd.grad(seq(x0).sum(), [seq[0].weight])
    assert torch.equal(dw, want)


def test_mismatched_shapes_raise():
    w = [torch.zeros(16, 20), torch.zeros(32, 16)]
    b = [torch.zeros(16), torch.zeros(32)]
    wo, bo, x0 = torch.zeros(32), torch.zeros(1), torch.zeros(5, 20)
    mlp_tower(x0, w, b, wo, bo)
    for bad in (dict(x0=torch.zeros(5, 21)), dict(w=w[:1]),
                dict(w=[w[0], torch.zeros(32, 48)]),
                dict(b=[b[0], torch.zeros(16)]), dict(wo=torch.zeros(16)),
                dict(bo=torch.zeros(2)), dict(partial=torch.zeros(4))):
        a = {**dict(x0=x0, w=w, b=b, wo=wo, bo=bo, partial=None), **bad}
        with pytest.raises(ValueError):
            mlp_tower(a["x0"], a["w"], a["b"], a["wo"], a["bo"], a["partial"])


@pytest.mark.parametrize("in_dim,hidden,mlp3,tower", [
    (247, (400, 400, 400), True, False),        # the fused MLP keeps its own
    (247, (512, 256, 128, 32), False, True),
    (247, (256,), False, True),
    (247, (64, 24), False, False),              # no multiple of 16
    (247, (64, 64, 64, 64, 64), False, False),  # five hidden layers
    (1677, (256, 128, 64), False, False),       # the dim-64 row
])
def test_convert_sets_fused_tower(in_dim, hidden, mlp3, tower):
    model = WDL(field_vocabs=FIELD_VOCABS, dim=4)
    assert model.fused_tower is False
    model.dnn = _mlp(in_dim, hidden)
    convert_mlp_bf16(model)
    assert (model.fused_mlp, model.fused_tower) == (mlp3, tower)
