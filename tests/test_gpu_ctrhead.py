"""GPU numerics: fused CTR head vs the plain fp32 torch composition
(forward values and every input gradient), and, on integer operands,
bit for bit against the int64 composition of tests/mlp_ref.py."""

import pytest
import torch

import mlp_fraglayout_ref as fl
import mlp_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _torch_head(e_all, dense, w, b, use_fm):
    dim = e_all.shape[2] - 1
    e = e_all[..., :dim]
    lin = e_all[..., dim]
    deep_in = torch.cat([e.flatten(1), dense], dim=1)
    partial = lin.sum(dim=1) + dense @ w.reshape(-1) + b.reshape(())
    if use_fm:
        s = e.sum(dim=1)
        partial = partial + 0.5 * (s * s - (e * e).sum(dim=1)).sum(dim=1)
    return deep_in, partial


@pytest.mark.parametrize("use_fm", [True, False])
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("dim,nd", [(9, 13), (4, 13), (63, 7), (64, 13), (127, 5)])
def test_head_matches_torch(use_fm, out_bf16, dim, nd):
    from openembedding_amd.models.ctr import _FusedCTRHeadFn

    torch.manual_seed(0)
    B, F = 257, 26
    e_all = torch.randn(B, F, dim + 1, device=DEV, requires_grad=True)
    dense = torch.rand(B, nd, device=DEV, requires_grad=True)
    w = torch.randn(1, nd, device=DEV, requires_grad=True)
    b = torch.randn(1, device=DEV, requires_grad=True)

    deep_in, partial = _FusedCTRHeadFn.apply(e_all, dense, w, b, use_fm,
                                             out_bf16)
    ref_in, ref_p = _torch_head(e_all, dense, w, b, use_fm)

    tol = 2e-2 if out_bf16 else 1e-5
    assert torch.allclose(deep_in.float(), ref_in, atol=tol, rtol=tol)
    assert torch.allclose(partial, ref_p, atol=2e-4, rtol=1e-4)

    g_in = torch.randn_like(ref_in)
    g_p = torch.randn_like(ref_p)
    (deep_in.float() * g_in).sum().backward(retain_graph=True)
    (partial * g_p).sum().backward()
    got = [t.grad.clone() for t in (e_all, dense, w, b)]
    for t in (e_all, dense, w, b):
        t.grad = None
    (ref_in * g_in).sum().backward(retain_graph=True)
    (ref_p * g_p).sum().backward()
    names = ["e_all", "dense", "w", "b"]
    for name, gg, t in zip(names, got, (e_all, dense, w, b)):
        atol = 5e-2 if out_bf16 else 1e-3  # atomic order + bf16 grad
        assert torch.allclose(gg, t.grad, atol=atol, rtol=1e-3), name


def test_deepfm_fused_matches_plain():
    """Whole-model check: DeepFM forward with fused head equals the torch
    path bit-for... closely (fp32 head)."""
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DeepFM, synthetic_batch

    torch.manual_seed(0)
    model = DeepFM(dim=9).to(DEV)
    dense, sparse, labels = synthetic_batch(512, device=DEV)
    with torch.no_grad():
        # materialize rows once so both paths read identical weights
        model.embedding.variable.sparse_read(
            sparse + model.embedding.field_offsets)
    out_fused = model(dense, sparse)
    try:
        model._use_fused_head = lambda t: False
        out_plain = model(dense, sparse)
    finally:
        del model._use_fused_head
    assert torch.allclose(out_fused, out_plain, atol=1e-4, rtol=1e-4)


# ---------------------------------------------------------- exact oracle

def _poison_allocator():
    # leave NaN / inf bit patterns (bf16 pairs; NaN and inf as fp32 too)
    # in freed memory, so that a pad tail nobody writes does not read as 0
    junk = torch.empty(8 << 20, device=DEV, dtype=torch.int32)
    junk[0::3] = 0x7FC07FC0
    junk[1::3] = 0x7F807F80
    junk[2::3] = -8323200            # 0xFF80FF80
    del junk


def _head_operands(c, out_dtype):
    f = lambda t: t.to(torch.float32).to(DEV)  # noqa: E731
    return (f(c.e_all), f(c.dense), f(c.w), f(c.b),
            c.d_deep_in.to(out_dtype).to(DEV), f(c.d_partial))


@pytest.mark.parametrize("F", [1, 26])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("nd", [1, 13, 32])
@pytest.mark.parametrize("dim", [1, 9, 63, 64, 127])
def test_head_exact(dim, nd, B, F):
    """ctr_head_fwd / ctr_head_bwd through the bindings on integer operands
    (mlp_ref.head_int_case): every sum is an integer far below 2^24 and
    0.5 * fm is one too, so deep_in, partial, s, de_all, d_dense, dw and
    db must EQUAL the int64 composition, float atomics included, for both
    output dtypes and with and without the FM term. dim 63 / 64 / 127 sit
    around the second column of a lane, nd 32 is the binding's maximum;
    nd = 0 is left out: the binding does not refuse it, but the dense-tail
    backward would be launched with an empty grid. The pad tail of the
    32-padded deep_in, which the fused MLP's 16-byte fragment loads rely
    on, must be zero although the allocator hands out NaN patterns."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    c = mr.head_int_case(B, F, dim, nd, seed=dim + 3 * nd + 5 * B + F)
    stride = mr.ceil_to(c.width, 32)
    for out_bf16 in (False, True):
        dt = torch.bfloat16 if out_bf16 else torch.float32
        e_all, dense, w, b, d_in, d_p = _head_operands(c, dt)
        for use_fm in (False, True):
            r = mr.head_ref(c, use_fm)
            tag = (out_bf16, use_fm)
            _poison_allocator()
            deep_in, partial, s = ext.ctr_head_fwd(e_all, dense, w, b,
                                                   use_fm, out_bf16, True)
            assert deep_in.shape == (B, stride) and deep_in.dtype == dt
            assert partial.shape == (B,) and s.shape == (B, dim)
            assert torch.equal(deep_in[:, :c.width].double().cpu(),
                               r.deep_in.double()), tag
            assert bool((deep_in[:, c.width:] == 0).all()), tag
            assert torch.equal(partial.double().cpu(),
                               r.partial.double()), tag
            assert torch.equal(s.double().cpu(), r.s.double()), tag
            # unpadded: exactly width columns, the same values
            plain, p2, _ = ext.ctr_head_fwd(e_all, dense, w, b, use_fm,
                                            out_bf16, False)
            assert plain.shape == (B, c.width)
            assert torch.equal(plain, deep_in[:, :c.width]), tag
            assert torch.equal(p2, partial), tag

            de_all, d_dense, dw, db = ext.ctr_head_bwd(
                e_all, dense, w, d_in, d_p, s, use_fm)
            for name, got, want in (("de_all", de_all, r.de_all),
                                    ("d_dense", d_dense, r.d_dense),
                                    ("dw", dw, r.dw), ("db", db, r.db)):
                assert got.shape == want.shape, (name, tag)
                assert torch.equal(got.double().cpu(), want.double()), (
                    name, tag)


def test_head_into_mlp_exact():
    """The flagship's dense path end to end on integers: the head at dim 9
    (K0 = 26 * 9 + 13 = 247) writes the 32-padded bf16 deep_in and the
    partial logit, mlp3_fwd takes both, and a1..a3 and out equal the
    oracle's chain."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    M, H, K0, K0p, F, dim, nd = 131, 400, 247, 256, 26, 9, 13
    c = mr.int_case(M, H, K0)
    h = mr.head_int_case(M, F, dim, nd)
    x0 = c.x0.to(torch.int64)
    h.e_all[..., :dim] = x0[:, :F * dim].reshape(M, F, dim)
    h.dense = x0[:, F * dim:]
    r = mr.head_ref(h, True)
    assert torch.equal(r.deep_in, x0)
    f = lambda t: t.to(torch.float32).to(DEV)  # noqa: E731
    _poison_allocator()
    deep_in, partial, _ = ext.ctr_head_fwd(f(h.e_all), f(h.dense), f(h.w),
                                           f(h.b), True, True, True)
    assert deep_in.shape == (M, K0p)
    ws = (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, c.w4, c.b4)
    (a1, a2, a3, out), mags = mr.fwd_ref(c.x0, *ws, r.partial.double())
    assert float(mags[3].max()) < mr.LIMIT
    b = lambda t: t.to(torch.bfloat16).to(DEV)  # noqa: E731
    Hp = mr.ceil_to(H, 32)
    img = lambda w, n, k: fl.pack(fl.pad(w.to(torch.bfloat16), n,  # noqa: E731
                                         k)).contiguous().to(DEV)
    got = ext.mlp3_fwd(deep_in, img(c.w1, H, K0p), b(c.b1),
                       img(c.w2, H, Hp), b(c.b2), img(c.w3, H, Hp), b(c.b3),
                       b(c.w4), b(c.b4), partial, frag=True)
    assert torch.equal(got[0].double().cpu(), out)
    for g, want in zip(got[1:], (a1, a2, a3)):
        assert torch.equal(g.double().cpu(), want)
