"""float64 reference of the fused CTR head's backward, with derived bounds.

The head backward (ops/csrc/ctrhead.hip) is elementwise for de_all and
d_dense and an fp32 accumulation over the batch for dw / db:

    de_all[b,f,c]  = d_deep_in[b, f*dim+c] + gp[b] * (s[b,c] - e[b,f,c])
    de_all[b,f,dim] = gp[b]                          (wide column)
    d_dense[b,j]   = d_deep_in[b, F*dim+j] + gp[b] * w[j]
    dw[j] = sum_b gp[b] * dense[b,j],   db = sum_b gp[b]

with gp = d_partial and s = sum_f e (the FM term only with use_fm).

Bounds. dw / db are sums of B fp32 terms that reach their address through
per-block partials and float atomics, in any order: cin_ref.bound(sum|terms|,
B + n_blocks + 2) — the terms, the block partials, the product's own
rounding and the add onto the base. de_all / d_dense are a handful of fp32
operations on top of the forward's F-term sum s: (F + 3) roundings of the
magnitude |d| + |gp| * (sum_f |e| + |e|). Nothing here is fitted to the
kernels."""

from types import SimpleNamespace

import torch

import cin_ref

f64 = torch.float64


def head_bwd_ref(e_all, dense, w, d_deep_in, d_partial, use_fm):
    """float64 de_all, d_dense, dw [nd], db [1] and the magnitudes the
    bounds need, from the operands the kernels get (any dtype/device;
    d_deep_in may be 32-padded)."""
    e_all, dense, w, d_in, gp = (t.detach().to("cpu", f64) for t in
                                 (e_all, dense, w, d_deep_in, d_partial))
    w = w.reshape(-1)
    B, F, D1 = e_all.shape
    dim, nd = D1 - 1, dense.shape[1]
    e = e_all[..., :dim]
    g = gp.view(-1, 1, 1)
    d_e = d_in[:, :F * dim].reshape(B, F, dim)
    r = SimpleNamespace(B=B, F=F, dim=dim, nd=nd)
    g_e = d_e
    mag_e = d_e.abs()
    if use_fm:
        g_e = d_e + g * (e.sum(1, keepdim=True) - e)
        mag_e = mag_e + g.abs() * (e.abs().sum(1, keepdim=True) + e.abs())
    r.de_all = torch.cat([g_e, g.expand(B, F, 1)], dim=2)
    r.de_mag = torch.cat([mag_e, g.abs().expand(B, F, 1)], dim=2)
    tail = d_in[:, F * dim:F * dim + nd]
    r.d_dense = tail + gp.unsqueeze(1) * w.unsqueeze(0)
    r.d_dense_mag = tail.abs() + (gp.unsqueeze(1) * w.unsqueeze(0)).abs()
    terms = gp.unsqueeze(1) * dense
    r.dw, r.dw_mag = terms.sum(0), terms.abs().sum(0)
    r.db, r.db_mag = gp.sum().reshape(1), gp.abs().sum().reshape(1)
    return r


def n_terms(B, n_blocks):
    """Roundings of one dw / db address: B terms, n_blocks block partials,
    in any order, + 2."""
    return B + n_blocks + 2


def old_blocks(B, nd):
    """Blocks (= global atomics per address) of k_ctr_head_bwd_d: one per
    256 (sample, feature) pairs."""
    return (B * nd + 255) // 256


def acc_ratio(got, want, mag, n, base=None):
    """max |got - (base + want)| / bound for an accumulated dw or db;
    passes when <= 1. base: what the buffer held before the launch."""
    got = got.detach().to("cpu", f64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    if base is not None:
        base = base.detach().to("cpu", f64).reshape(-1)
        want, mag = want + base, mag + base.abs()
    return float(((got - want).abs() / cin_ref.bound(mag, n)).max())


def elem_ratio(got, want, mag, F):
    """max |got - want| / bound for de_all or d_dense; passes when <= 1."""
    got = got.detach().to("cpu", f64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - want).abs() / cin_ref.bound(mag, F + 3)).max())


def float_case(B, F, dim, nd, stride, seed=0):
    """randn operands as fp32 CPU tensors; dense in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(B=B, F=F, dim=dim, nd=nd, stride=stride)
    c.e_all = torch.randn(B, F, dim + 1, generator=g)
    c.dense = torch.rand(B, nd, generator=g)
    c.w = torch.randn(nd, generator=g)
    c.b = torch.randn(1, generator=g)
    c.d_deep_in = torch.randn(B, stride, generator=g)
    c.d_partial = torch.randn(B, generator=g)
    return c


def deepfm_step(device="cuda:0", batch=64):
    """One seeded DeepFM training step on the flagship's dense path (bf16
    fused MLP, flat optimizer with bound grads), up to and including the
    backward: logits, dense_linear's grads and their magnitudes."""
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DeepFM, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16

    torch.manual_seed(0)
    model = convert_mlp_bf16(DeepFM(dim=9).to(device))
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01), flatten_dense=True)
    g = torch.Generator(device=device).manual_seed(1)
    dense, sparse, labels = synthetic_batch(batch, device=device, generator=g)
    opt.zero_grad()
    logits = model(dense, sparse)
    torch.nn.BCEWithLogitsLoss()(logits, labels).backward()
    torch.cuda.synchronize()
    gp = ((torch.sigmoid(logits.detach().double()) - labels.double())
          / batch).abs()
    lin = model.dense_linear
    return {"logits": logits.detach().cpu(),
            "dw": lin.weight.grad.detach().float().cpu().clone(),
            "db": lin.bias.grad.detach().float().cpu().clone(),
            "dw_mag": (gp.unsqueeze(1) * dense.double().abs()).sum(0).cpu(),
            "db_mag": gp.sum().reshape(1).cpu()}


def step_child_main(out_path):
    """Entry of the child process of the switch test (OEAMD_HEAD_ROWS=0)."""
    from openembedding_amd.models import ctr
    assert ctr._HEAD_ROWS is False
    torch.save(deepfm_step("cuda:0"), out_path)
