"""k_tower_wgrad / k_tower_wgrad_fold (ops/csrc/tower.hip) against float64
sums of the same mirrors: exact on integers, inside the project's wgrad
interval on random operands; the route through ``mlp_tower``, capture and the
refusals."""

import gc
import os
import subprocess
import sys

import pytest
import torch

from cin_ref import bound, ceil_to
from mlp_ref import bf16_rne, check_interval, interval, trunc_bf16, wgrad_pre
from test_gpu_tower import FOUR, _case, _dev, _operands, _same, _solve, \
    _switch_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf, f64 = torch.bfloat16, torch.float64
NAN = float("nan")
WDL = (247, (512, 256, 128, 32))
SHAPES = [(20, (16,)), (50, (64, 32)), (429, (48, 512)), WDL]


def _ints(M, K0, widths, seed):
    """Arbitrary integer mirrors (no tower run): x0 with non-zero pad
    columns, a_l, dz_l, dout in {-3..3} as float64."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).to(f64)  # noqa: E731
    return (ri(M, ceil_to(K0, 32)), [ri(M, h) for h in widths],
            [ri(M, h) for h in widths], ri(M))


def _sums(x0, K0, acts, dzs, dout):
    """(sum, sum of |terms|) per gradient in the binding's order."""
    ins = [x0[:, :K0]] + acts[:-1]
    d = dout.unsqueeze(1) * acts[-1]
    zero = torch.zeros((), dtype=f64)
    return [wgrad_pre(dz, a, zero) for dz, a in zip(dzs, ins)] \
        + [(dz.sum(0), dz.abs().sum(0)) for dz in dzs] \
        + [(d.sum(0), d.abs().sum(0)),
           (dout.sum().view(1), dout.abs().sum().view(1))]


def _flat(bases):
    """One bf16 buffer of 7s that holds the gradients the way a flat
    optimizer's views lie: every second one off 16-byte alignment."""
    at, spans = 8, []
    for i, b in enumerate(bases):
        at = ceil_to(at, 8) + i % 2
        spans.append((at, b.numel()))
        at += b.numel() + 8
    buf = torch.full((at,), 7.0, dtype=bf, device=DEV)
    views = [buf[o:o + n].view(b.shape) for (o, n), b in zip(spans, bases)]
    for v, b in zip(views, bases):
        v.copy_(b)
    keep = torch.ones(at, dtype=torch.bool, device=DEV)
    for o, n in spans:
        keep[o:o + n] = False
    return buf, views, keep


def _call(ext, dev, K0, views, accumulate, m_split):
    x0, acts, dzs, dout = dev
    S, floats = ext.tower_wgrad_plan(x0.shape[0], K0,
                                     [a.shape[1] for a in acts], m_split)
    scratch = torch.full((floats,), NAN, device=DEV)    # nothing is zeroed
    ext.tower_wgrad(x0, K0, acts, dzs, dout, views, accumulate, scratch,
                    m_split)
    return S, scratch


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("K0,widths", SHAPES)
def test_exact_on_integers(K0, widths, accumulate):
    """Every sum of |terms| is at most 9 M + 600 < 2^24: any order is exact,
    so each gradient EQUALS bf16(base + sum), whatever m_split."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    g = torch.Generator().manual_seed(K0)
    for M in (1, 33, 127, 129, 300):
        assert 9 * M + 600 < 2 ** 24
        x0, acts, dzs, dout = host = _ints(M, K0, widths, 1000 * K0 + M)
        dev = (_dev(x0), [_dev(a) for a in acts], [_dev(d) for d in dzs],
               _dev(dout, torch.float32))
        before = [t.clone() for t in (dev[0], *dev[1], *dev[2], dev[3])]
        sums = [s for s, _ in _sums(x0, K0, *host[1:])]
        bases = [bf16_rne(torch.randint(-600, 601, s.shape, generator=g)
                          .to(f64)) if accumulate else torch.full_like(s, NAN)
                 for s in sums]
        once = [bf16_rne(s + b) if accumulate else bf16_rne(s)
                for s, b in zip(sums, bases)]
        for m_split in (0, 1, 3):
            buf, views, keep = _flat(bases)
            _call(ext, dev, K0, views, accumulate, m_split)
            for got, want in zip(views, once):
                assert _same(got, want)
            if accumulate:                  # the same sums on top, once more
                _call(ext, dev, K0, views, True, m_split)
                for got, want, s in zip(views, once, sums):
                    assert _same(got, bf16_rne(want + s))
            assert bool((buf[keep] == 7).all())
        for t, b in zip((dev[0], *dev[1], *dev[2], dev[3]), before):
            assert torch.equal(t, b)


@pytest.mark.parametrize("m_split", [0, 3])
@pytest.mark.parametrize("K0,widths", FOUR)
def test_random_within_interval(K0, widths, m_split):
    """M = 300, the mirrors of a float64 chain on random operands, random
    bf16 bases: every gradient inside [bf16(ref - delta), bf16(ref + delta)],
    delta = cin_ref.bound(sum |terms|, M + S + 2), the project's wgrad bound
    (docs/kernels.md, fused MLP). Derived, nothing fitted."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    M = 300
    c = _case(M, K0, widths, seed=K0 + 1, integer=False)
    r = _solve(c)
    g = torch.Generator().manual_seed(K0)
    x0 = torch.nn.functional.pad(c.x0, (0, c.K0p - K0), value=1.0)
    dev = (_dev(x0), [_dev(a) for a in r.a], [_dev(d) for d in r.dz],
           _dev(c.dout, torch.float32))
    sums = _sums(x0, K0, r.a, r.dz, c.dout)
    bases = [bf16_rne(torch.randn(s.shape, generator=g)) for s, _ in sums]
    S = ext.tower_wgrad_plan(M, K0, list(widths), m_split)[0]
    n = M + S + 2
    boxes = [interval(s + b, mag + b.abs(), n)
             for (s, mag), b in zip(sums, bases)]
    # the interval admits a plain fp32 reference and rejects a truncating fold
    for dz, a, b, box in zip(r.dz, [x0[:, :K0]] + r.a[:-1], bases, boxes):
        f32 = (b.float() + dz.float().t() @ a.float()).to(f64)
        assert check_interval(bf16_rne(f32), *box)[0] == 0
        assert check_interval(trunc_bf16(f32), *box)[0] > 0
    _, views, _ = _flat(bases)
    _call(ext, dev, K0, views, True, m_split)
    bad = sum(check_interval(v, *box)[0] for v, box in zip(views, boxes))
    # information: the fp32 slabs of dW_1, summed in float64, against delta
    _, views, _ = _flat(bases)
    _, scratch = _call(ext, dev, K0, views, False, m_split)
    slabs = scratch.view(S, -1)[:, :widths[0] * c.K0p].cpu().double()
    got = slabs.view(S, widths[0], c.K0p)[:, :, :K0].sum(0)
    worst = float(((got - sums[0][0]).abs() / bound(sums[0][1], n)).max())
    print(f"K0={K0} m_split={m_split} S={S}: violations {bad}, "
          f"dW_1 err/delta {worst:.4f}")
    assert bad == 0


def _leaves(args, frozen=()):
    x0, W, b, w_out, b_out, partial = args
    ps = [p.clone().requires_grad_(i not in frozen)
          for i, p in enumerate(W + b + [w_out, b_out])]
    return x0, ps, partial


def _step(x0, ps, partial, dout):
    """mlp_tower forward + backward into the parameters' .grad."""
    from openembedding_amd.ops import dispatch
    L = (len(ps) - 2) // 2
    out = dispatch.mlp_tower(x0, ps[:L], ps[L:2 * L], ps[-2], ps[-1], partial)
    out.backward(dout)


def test_captured_step_replays_bit_identically():
    """Prebound grads, re-zeroed inside the captured region: three replays
    equal eager, and eager equals eager (no atomics anywhere)."""
    c = _case(70, *WDL, seed=9, integer=False)
    o = _operands(c)
    x0, ps, partial = _leaves((o.x0, o.W, o.b, o.w_out, o.b_out, o.partial))
    for p in ps:
        p.grad = torch.zeros_like(p)

    def run():
        for p in ps:
            p.grad.zero_()
        _step(x0, ps, partial, o.dout)

    runs = []
    for _ in range(2):
        run()
        runs.append([p.grad.clone() for p in ps])
    assert hasattr(ps[0], "_tower_wgrad_buf")        # the fused route ran
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(t.float().abs().sum() > 0) for t in runs[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p.grad, w) for p, w in zip(ps, runs[0]))
    del graph                        # hand the capture's pool back
    gc.collect()


def _switch_grads(frozen=()):    # fresh gradients on test_gpu_tower's integers
    c, args = _switch_args()
    x0, ps, partial = _leaves(args, frozen)
    _step(x0, ps, partial, _dev(c.dout, torch.float32))
    return ps


def test_library_routes_agree_on_integers():
    """Sums exact in fp32 round once on either route: an OEAMD_TOWER_WGRAD=0
    child and a partly frozen tower (library ops) equal the fused wgrad."""
    from openembedding_amd.ops import dispatch
    assert dispatch._TOWER_WGRAD
    fused = _switch_grads()
    assert hasattr(fused[0], "_tower_wgrad_buf")
    part = _switch_grads(frozen=(1,))
    assert part[1].grad is None and not hasattr(part[0], "_tower_wgrad_buf")
    for i, (p, q) in enumerate(zip(part, fused)):
        assert i == 1 or torch.equal(p.grad, q.grad)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, test_gpu_tower_wgrad as t\n"
            "from openembedding_amd.ops import dispatch\n"
            "assert not dispatch._TOWER_WGRAD\n"
            "print(*torch.cat([p.grad.flatten().float()\n"
            "                  for p in t._switch_grads()]).tolist())\n"
            % [here, os.path.dirname(here)])
    res = subprocess.run([sys.executable, "-c", code], check=True,
                         capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, OEAMD_TOWER_WGRAD="0"))
    child = torch.tensor([float(v) for v in res.stdout.split()])
    assert torch.equal(child, torch.cat([p.grad.flatten().float().cpu()
                                         for p in fused]))


REFUSALS = {                     # what is wrong -> what the message names
    "m_split17": "m_split", "scratch_short": "scratch", "dz_fp32": "bf16",
    "grad_shape": "weight gradient", "mirror_strided": "contiguous",
    "K0p544": "K0p", "w24": "multiple of 16", "L5": "L <= 4"}
SHAPE_REFUSALS = {"K0p544": (530, (32,)), "w24": (40, (24,)),
                  "L5": (40, (16,) * 5)}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    """Nothing is launched (the NaN gradients stay), and behind a refused
    shape mlp_tower's gradients are torch's own."""
    from openembedding_amd.ops import dispatch, require_hip
    ext = require_hip()
    K0, widths = SHAPE_REFUSALS.get(case, (50, (64, 32)))
    M, L = 9, len(widths)
    x0, acts, dzs, dout = _ints(M, K0, widths, 3)
    dev = [_dev(x0), [_dev(a) for a in acts], [_dev(d) for d in dzs],
           _dev(dout, torch.float32)]
    shapes = [(h, k) for h, k in zip(widths, (K0,) + widths)] \
        + [(h,) for h in widths] + [(widths[-1],), (1,)]
    grads = [torch.full(s, NAN, dtype=bf, device=DEV) for s in shapes]
    floats = 16 * (sum(h * 512 for h in widths) + 2 * sum(widths) + 4)
    m_split = 17 if case == "m_split17" else 0
    if case == "scratch_short":
        floats = 64
    if case == "dz_fp32":
        dev[2][0] = dev[2][0].float()
    if case == "grad_shape":
        grads[0] = grads[0][:, :-1].contiguous()
    if case == "mirror_strided":
        dev[1][0] = torch.cat([dev[1][0]] * 2, 1)[:, :widths[0]]
    with pytest.raises(RuntimeError, match=REFUSALS[case]):
        ext.tower_wgrad(dev[0], K0, dev[1], dev[2], dev[3], grads, False,
                        torch.empty(floats, device=DEV), m_split)
    assert all(bool(g.isnan().all()) for g in grads)
    if case in SHAPE_REFUSALS:
        c = _case(M, K0, widths, seed=5, integer=False)
        o = _operands(c)
        args = (o.x0, o.W, o.b, o.w_out, o.b_out, o.partial)
        assert not dispatch._tower_fits(*args)
        got, want = _leaves(args), _leaves(args)
        _step(*got, o.dout)
        dispatch._tower_torch(want[0], want[1][:L], want[1][L:2 * L],
                              *want[1][-2:], want[2]).backward(o.dout)
        for p, q in zip(got[1], want[1]):
            assert torch.equal(p.grad, q.grad)
