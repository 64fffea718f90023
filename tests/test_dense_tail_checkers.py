"""The dense-tail reference (dense_tail_ref.py) without a GPU: it is
self-consistent, and comparing against it rejects each mistake that a fused
tail kernel could make."""

from __future__ import annotations

import pytest
import torch

import dense_tail_ref as R
from mlp_fraglayout_ref import unpack

H, K0, K0P = 16, 20, 32
LR, CFG = 0.05, (1e-10, 0.0, 0.0)


@pytest.fixture(scope="module")
def case():
    start = R.make_state(H, K0, K0P, R.ADAGRAD, seed=3)
    want = R.tail(R.clone_state(start), R.ADAGRAD, H, K0, K0P, LR, *CFG)
    return start, want


def test_reference_accepts_itself(case):
    start, want = case
    again = R.tail(R.clone_state(start), R.ADAGRAD, H, K0, K0P, LR, *CFG)
    assert R.check(again, want) == []
    # the step moved every weight and the images stand for the new weights
    lay, n = R.layout(H, K0)
    assert not torch.equal(want["flat"], start["flat"])
    w1 = R.view(want["flat"], lay, "w1")
    assert torch.equal(unpack(want["w1p"])[:, :K0], w1)
    assert torch.equal(unpack(want["w1tp"])[:K0, :H], w1.t())
    assert not want["grad"].any() and not want["wscratch"].any()
    assert not want["bscratch"].any() and not want["g32"].any()


def test_rejects_unrounded_gradient(case):
    """fp32 sums straight into the optimizer, without the bf16 rounding of
    the finisher."""
    start, want = case
    st = R.clone_state(start)
    g32 = st["grad"].to(R.f32) + R.scratch_sums(st, H, K0, K0P)
    assert not torch.equal(g32, g32.to(R.bf16).to(R.f32))
    m = R.opt_step(R.ADAGRAD, st["master"], g32, st["s1"], None, None, LR,
                   *CFG)
    assert not torch.equal(m, want["master"])
    assert not torch.equal(st["s1"], want["s1"])
    assert not torch.equal(m.to(R.bf16), want["flat"])


def test_rejects_scratch_pads_left(case):
    start, want = case
    got = R.clone_state(want)
    got["wscratch"][:H * K0P].view(H, K0P)[:, K0:] = \
        start["wscratch"][:H * K0P].view(H, K0P)[:, K0:]
    assert start["wscratch"][:H * K0P].view(H, K0P)[:, K0:].any()
    assert R.check(got, want) == ["wscratch"]


def test_rejects_stale_transposed_image(case):
    start, want = case
    for name in ("w1tp", "w2tp", "w3tp"):
        got = R.clone_state(want)
        got[name] = start[name].clone()
        assert R.check(got, want) == [name]


def test_rejects_grads_not_zeroed(case):
    start, want = case
    got = R.clone_state(want)
    got["grad"] = start["grad"].clone()
    assert R.check(got, want) == ["grad"]
    got = R.clone_state(want)
    got["g32"] = start["g32"].clone()
    assert R.check(got, want) == ["g32"]


def test_rejects_image_pads_overwritten(case):
    """One element of a pad (a column >= K0 of w1's image, a row >= K0 of
    its transposed image) set to anything but the zero the pack wrote."""
    start, want = case
    got = R.clone_state(want)
    wp = unpack(got["w1p"])
    assert not wp[:, K0:].any()
    wp[3, K0 + 1] = 1.0
    from mlp_fraglayout_ref import pack
    got["w1p"] = pack(wp)
    assert R.check(got, want) == ["w1p"]
    got = R.clone_state(want)
    wt = unpack(got["w1tp"])
    assert not wt[K0:].any() and not wt[:, H:].any()
    wt[K0 + 2, 5] = 1.0
    got["w1tp"] = pack(wt)
    assert R.check(got, want) == ["w1tp"]


@pytest.mark.parametrize("opt,cfg", [
    (R.SGD, (0.0, 0.0, 0.0)), (R.SGD, (0.9, 0.0, 0.0)),
    (R.SGD, (0.9, 1.0, 0.0)), (R.ADAM, (0.9, 0.999, 1e-8))])
def test_other_optimizers_match_torch(opt, cfg):
    """opt_step against torch.optim on one fp32 vector, two steps."""
    g = torch.Generator().manual_seed(1)
    w0 = torch.randn(64, generator=g)
    grads = [torch.randn(64, generator=g) for _ in range(2)]
    p = torch.nn.Parameter(w0.clone())
    if opt == R.SGD:
        ref = torch.optim.SGD([p], lr=LR, momentum=cfg[0],
                              nesterov=bool(cfg[1]))
    else:
        ref = torch.optim.Adam([p], lr=LR, betas=cfg[:2], eps=cfg[2])
    w, s1, s2 = w0.clone(), torch.zeros(64), torch.zeros(64)
    sc = torch.zeros(3)
    for gr in grads:
        p.grad = gr.clone()
        ref.step()
        if opt == R.ADAM:
            R.step_scalars(sc, cfg[0], cfg[1])
        w = R.opt_step(opt, w, gr, s1, s2, sc, LR, *cfg)
    torch.testing.assert_close(w, p.detach(), rtol=1e-5, atol=1e-6)
