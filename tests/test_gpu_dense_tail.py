"""The fused dense-parameter tail (mlp.hip: k_dense_tail) against the five
launches it replaces, bit for bit, and the routing around it
(models/ctr.py, torch/__init__.py: _FlatDenseOptimizer).

The kernel cases start from dense_tail_ref.make_state: random scratch with
non-zero w1 pad columns, non-zero base grads (the accumulate case), images
written by a real pack, a canary behind every buffer. The routing cases
train a small _DNNHead on integer-valued operands whose loss touches two
rows only: every atomically accumulated sum then has at most two non-zero
terms and is the same in any order, so two routes that round alike must
agree with torch.equal, however many steps they take.

Run as a script (--child OUT) this file trains the small model for three
steps and saves parameters and logits; the parent test starts it with
OEAMD_DENSE_TAIL=0 in a fresh interpreter."""

from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import dense_tail_ref as R  # noqa: E402
from mlp_fraglayout_ref import image  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 64
LR = 0.05

SHAPES = [(400, 247, 256), (16, 20, 32), (64, 50, 64)]
OPTS = {
    "adagrad": (R.ADAGRAD, (1e-10, 0.0, 0.0), True),
    "sgd": (R.SGD, (0.0, 0.0, 0.0), False),
    "sgd_momentum": (R.SGD, (0.9, 0.0, 0.0), True),
    "sgd_nesterov": (R.SGD, (0.9, 1.0, 0.0), True),
    "adam": (R.ADAM, (0.9, 0.999, 1e-8), True),
}


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


# ------------------------------------------------------------------ kernel

def _fill(t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t.shape, generator=g).to(t.dtype)


def _to_dev(st):
    """Every buffer in front of a canary of its own; returns (views, bigs)."""
    views, bigs = {}, {}
    for k, v in st.items():
        if v is None:
            views[k] = None
            continue
        big = torch.empty(v.numel() + CANARY, dtype=v.dtype, device=DEV)
        big[:v.numel()] = v.reshape(-1).to(DEV)
        big[v.numel():] = 7.0
        bigs[k] = big
        views[k] = big[:v.numel()].view(v.shape)
    return views, bigs


def _five_launches(ext, d, opt, H, K0, K0p, cfg):
    lay, _ = R.layout(H, K0)
    gv = {k: R.view(d["grad"], lay, k) for k in lay}
    pv = {k: R.view(d["flat"], lay, k) for k in lay}
    ext.mlp3_finish(d["wscratch"], d["bscratch"], K0p,
                    [gv["w1"], gv["w2"], gv["w3"]],
                    [gv["b1"], gv["b2"], gv["b3"], gv["w4"].view(-1),
                     gv["b4"]])
    if d["p32"] is not None:
        ext.flat_opt(opt, d["p32"], None, d["s1_32"], d["s2_32"], d["g32"],
                     d["sc"], LR, *cfg)
    ext.flat_opt(opt, d["flat"], d["master"], d["s1"], d["s2"], d["grad"],
                 d["sc"], LR, *cfg)
    ws = [pv["w1"], pv["w2"], pv["w3"]]
    ext.mlp3_pack_frag(
        ws + ws[::-1],
        [d["w1p"], d["w2p"], d["w3p"], d["w3tp"], d["w2tp"], d["w1tp"]],
        [False] * 3 + [True] * 3)


def _one_launch(ext, d, opt, H, K0, K0p, cfg):
    lay, _ = R.layout(H, K0)
    pv = {k: R.view(d["flat"], lay, k) for k in lay}
    ext.dense_tail(
        opt, d["flat"], d["master"], d["s1"], d["s2"], d["grad"],
        [pv["w1"], pv["w2"], pv["w3"]],
        [pv["b1"], pv["b2"], pv["b3"], pv["w4"], pv["b4"]],
        d["wscratch"], d["bscratch"], [d["w1p"], d["w2p"], d["w3p"]],
        [d["w1tp"], d["w2tp"], d["w3tp"]], d["p32"], d["s1_32"],
        d["s2_32"], d["g32"], d["sc"], LR, *cfg)


def _run_case(H, K0, K0p, opt_name, n32):
    ext = _ext()
    opt, cfg, momentum = OPTS[opt_name]
    st = R.make_state(H, K0, K0p, opt, n32=max(n32, 1), seed=H + n32,
                      momentum=momentum)
    if n32 == 0:
        for k in ("p32", "g32", "s1_32", "s2_32"):
            st[k] = None
    a, abig = _to_dev(st)
    b, bbig = _to_dev(st)
    for step in range(2):       # two steps: Adam's device scalars advance
        if step:
            for k in ("wscratch", "bscratch", "grad", "g32"):
                if a[k] is not None:
                    fresh = _fill(st[k], 100 + step).to(DEV)
                    a[k].copy_(fresh)
                    b[k].copy_(fresh)
        for d, run in ((a, _five_launches), (b, _one_launch)):
            if opt == R.ADAM:
                ext.flat_step_scalars(d["sc"], cfg[0], cfg[1])
            run(ext, d, opt, H, K0, K0p, cfg)
        torch.cuda.synchronize()
        assert R.check(b, a) == [], (opt_name, step)
        for k in ("grad", "wscratch", "bscratch", "g32"):
            if b[k] is not None:
                assert not b[k].any(), k
        # the step moved the weights and the images
        assert not torch.equal(b["flat"].cpu(), st["flat"])
        assert not torch.equal(b["w3tp"].cpu(), st["w3tp"])
    for k, big in bbig.items():
        assert bool((big[-CANARY:] == 7.0).all()), k
    for k, big in abig.items():
        assert bool((big[-CANARY:] == 7.0).all()), k


@pytest.mark.parametrize("opt_name", list(OPTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tail_equals_five_launches(shape, opt_name):
    _run_case(*shape, opt_name, 14)


@pytest.mark.parametrize("n32", [0, 1, 300])
def test_fp32_group_sizes(n32):
    _run_case(16, 20, 32, "adagrad", n32)
    _run_case(64, 50, 64, "adam", n32)


# ----------------------------------------------------------------- routing

M, H_S, K0_S, K0P_S = 160, 64, 50, 64


def _small_model(seed=0):
    """A _DNNHead with integer-valued bf16 weights and one fp32 Linear
    (the fp32 group), converted and on the GPU."""
    from openembedding_amd.models.ctr import (_DNNHead, _mlp,
                                               convert_mlp_bf16)

    class Small(_DNNHead):
        def __init__(self):
            super().__init__()
            self.dnn = _mlp(K0_S, (H_S, H_S, H_S))
            self.lin = nn.Linear(3, 1)

        def forward(self, x0, extra):
            return self._dnn_out(x0) + self.lin(extra).squeeze(-1)

    model = Small()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            hi = 1 if i in (2, 4) else 2        # w2, w3 in {-1, 0, 1}
            p.copy_(torch.randint(-hi, hi + 1, p.shape, generator=g).float())
    model.to(DEV)
    convert_mlp_bf16(model)
    assert model.fused_mlp
    return model


def _optimizer(model, kind="adagrad"):
    from openembedding_amd.torch import _FlatDenseOptimizer
    if kind == "adagrad":
        base = torch.optim.Adagrad(model.parameters(), lr=LR)
    else:
        base = torch.optim.Adam(model.parameters(), lr=LR)
    return _FlatDenseOptimizer(base)


def _inputs(step):
    """Integer-valued x0 (padded to K0p, bf16), extra, and a dout with two
    non-zero rows."""
    g = torch.Generator().manual_seed(1000 + step)
    x0 = torch.zeros(M, K0P_S)
    x0[:, :K0_S] = torch.randint(-3, 4, (M, K0_S), generator=g).float()
    extra = torch.zeros(M, 3)
    dout = torch.zeros(M)
    for r in (5 + step, 133 - step):
        extra[r] = torch.randint(-3, 4, (3,), generator=g).float()
        dout[r] = float(1 + (r % 3))
    return x0.to(DEV).to(torch.bfloat16), extra.to(DEV), dout.to(DEV)


def _backward(model, inp):
    x0, extra, dout = inp
    out = model(x0, extra)
    (out * dout).sum().backward()
    return out.detach()


def _train(model, opt, steps, first=0):
    outs = []
    for s in range(first, first + steps):
        opt.zero_grad()
        outs.append(_backward(model, _inputs(s)))
        opt.step()
    return outs


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


class CountingExt:
    """Passes every attribute of the extension through, counting calls."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if not callable(fn):
            return fn

        def counted(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **kw)
        return counted


def _counted(monkeypatch, opt):
    import openembedding_amd.ops as ops
    proxy = CountingExt(_ext())
    monkeypatch.setattr(ops, "require_hip", lambda: proxy)
    opt._ext = proxy
    return proxy


def test_steady_state_is_one_launch(monkeypatch):
    import openembedding_amd.models.ctr as ctr
    assert ctr._DENSE_TAIL
    model = _small_model()
    opt = _optimizer(model)
    proxy = _counted(monkeypatch, opt)
    _train(model, opt, 1)
    # the first step packed (no stamp yet) and ran the tail
    assert proxy.calls.get("mlp3_pack_frag") == 1
    assert proxy.calls.get("dense_tail") == 1
    _train(model, opt, 1, first=1)
    proxy.calls.clear()
    _train(model, opt, 1, first=2)
    assert "mlp3_pack_frag" not in proxy.calls
    assert proxy.calls.get("dense_tail") == 1
    assert "flat_opt" not in proxy.calls and "mlp3_finish" not in proxy.calls
    # an in-place write to a weight moves its _version: the forward packs
    with torch.no_grad():
        model.dnn[2].weight.mul_(1)
    proxy.calls.clear()
    _train(model, opt, 1, first=3)
    assert proxy.calls.get("mlp3_pack_frag") == 1
    assert proxy.calls.get("dense_tail") == 1
    # eval under the stamp packs nothing; after load_state_dict it does
    proxy.calls.clear()
    with torch.no_grad():
        model(*_inputs(9)[:2])
    assert "mlp3_pack_frag" not in proxy.calls
    model.load_state_dict({k: v.clone()
                           for k, v in model.state_dict().items()})
    with torch.no_grad():
        model(*_inputs(9)[:2])
    assert proxy.calls.get("mlp3_pack_frag") == 1
    # the optimizer's own load_state_dict drops the stamp as well
    _train(model, opt, 1, first=4)
    opt.load_state_dict(opt.state_dict())
    proxy.calls.clear()
    with torch.no_grad():
        model(*_inputs(9)[:2])
    assert proxy.calls.get("mlp3_pack_frag") == 1


def test_tail_writes_its_own_transposed_set():
    """step() writes the forward images in place and the transposed ones
    into w1tq..w3tq; w1tp..w3tp stay what the last packing forward wrote."""
    model = _small_model()
    opt = _optimizer(model)
    ws = (model.dnn[0].weight, model.dnn[2].weight, model.dnn[4].weight)
    before = [w.detach().clone() for w in ws]
    _train(model, opt, 1)
    bufs = model._w1pad
    after = [w.detach().clone() for w in ws]
    assert not torch.equal(before[1], after[1])
    for l, wb, wa in zip(("w1", "w2", "w3"), before, after):
        for key, w, trans in ((l + "tp", wb, True), (l + "tq", wa, True),
                              (l + "p", wa, False)):
            want = image(w.cpu(), *bufs[key].shape, trans=trans)
            assert torch.equal(bufs[key].cpu(), want), key


def test_switch_off_keeps_the_five_launches(monkeypatch):
    import openembedding_amd.models.ctr as ctr
    monkeypatch.setattr(ctr, "_DENSE_TAIL", False)
    model = _small_model()
    opt = _optimizer(model)
    proxy = _counted(monkeypatch, opt)
    _train(model, opt, 2)
    assert "dense_tail" not in proxy.calls
    assert proxy.calls.get("mlp3_pack_frag") == 2
    assert proxy.calls.get("flat_opt") == 4


@pytest.mark.parametrize("kind", ["adagrad", "adam"])
def test_two_backwards_before_a_step(monkeypatch, kind):
    """Gradient accumulation: the second backward folds the first one's
    pending sums in bf16 before it adds its own, as the switch-off route
    does."""
    import openembedding_amd.models.ctr as ctr

    def run(fused):
        monkeypatch.setattr(ctr, "_DENSE_TAIL", fused)
        model = _small_model()
        opt = _optimizer(model, kind)
        proxy = _counted(monkeypatch, opt)
        outs = _train(model, opt, 1)
        opt.zero_grad()
        outs.append(_backward(model, _inputs(1)))
        outs.append(_backward(model, _inputs(2)))
        opt.step()
        outs += _train(model, opt, 1, first=3)
        return _params(model), outs, proxy.calls

    p_on, o_on, calls_on = run(True)
    p_off, o_off, calls_off = run(False)
    assert calls_on.get("dense_tail") == 3 and calls_on.get("mlp3_finish") == 1
    assert "dense_tail" not in calls_off
    for a, b in zip(p_on + o_on, p_off + o_off):
        assert torch.equal(a, b)
    assert not torch.equal(p_on[0], _params(_small_model())[0])


def test_discarded_backward_leaves_nothing_behind():
    """zero_grad after a deferred backward drops its sums with the grads."""
    model, ref = _small_model(), _small_model()
    opt, ropt = _optimizer(model), _optimizer(ref)
    _train(model, opt, 1)
    _train(ref, ropt, 1)
    opt.zero_grad()
    _backward(model, _inputs(7))
    opt.zero_grad()             # discards the extra backward
    _backward(model, _inputs(1))
    opt.step()
    _train(ref, ropt, 1, first=1)
    for a, b in zip(_params(model), _params(ref)):
        assert torch.equal(a, b)


def _three_steps():
    model = _small_model()
    opt = _optimizer(model)
    outs = _train(model, opt, 3)
    torch.cuda.synchronize()
    return [t.cpu() for t in _params(model) + outs]


def test_three_steps_equal_the_switch_off_child(tmp_path):
    import openembedding_amd.models.ctr as ctr
    assert ctr._DENSE_TAIL
    out = tmp_path / "child.pt"
    env = dict(os.environ, OEAMD_DENSE_TAIL="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child",
                    str(out)], env=env, check=True, timeout=300)
    child = torch.load(out)
    assert child["dense_tail"] is False
    mine = _three_steps()
    assert len(mine) == len(child["tensors"])
    for a, b in zip(mine, child["tensors"]):
        assert torch.equal(a, b)
    assert not torch.equal(mine[0], _params(_small_model())[0].cpu())


def test_captured_step_replays_like_eager():
    """Warm-up steps leave a valid stamp; the captured step holds no pack
    and one tail, and each replay's tail writes the images that the next
    replay's forward reads."""
    eager, graphed = _small_model(), _small_model()
    eopt, gopt = _optimizer(eager), _optimizer(graphed)
    want = _train(eager, eopt, 5)
    _train(graphed, gopt, 2)
    static = [t.clone() for t in _inputs(2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gopt.zero_grad()
            out = _backward(graphed, static)
            gopt.step()
    torch.cuda.current_stream().wait_stream(side)
    for s in range(2, 5):
        for dst, src in zip(static, _inputs(s)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[s]), s
    for a, b in zip(_params(graphed), _params(eager)):
        assert torch.equal(a, b)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    import openembedding_amd.models.ctr as ctr_child
    torch.save({"dense_tail": ctr_child._DENSE_TAIL,
                "tensors": _three_steps()}, sys.argv[2])
