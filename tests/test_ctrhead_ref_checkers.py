"""CPU checks of tests/ctrhead_ref.py: the float64 reference equals float64
autograd through the torch composition of the head, and its checks reject
the mistakes a merged, accumulating backward can make."""

import pytest
import torch

import ctrhead_ref as hr
from test_gpu_ctrhead import _torch_head

f64 = torch.float64


def _autograd(c, use_fm):
    e_all, dense, w, b = (t.to(f64).requires_grad_() for t in
                          (c.e_all, c.dense, c.w, c.b))
    deep_in, partial = _torch_head(e_all, dense, w, b, use_fm)
    width = c.F * c.dim + c.nd
    loss = ((deep_in * c.d_deep_in[:, :width].to(f64)).sum()
            + (partial * c.d_partial.to(f64)).sum())
    loss.backward()
    return e_all.grad, dense.grad, w.grad, b.grad


@pytest.mark.parametrize("use_fm", [True, False])
@pytest.mark.parametrize("B,F,dim,nd", [(5, 3, 4, 2), (17, 26, 9, 13),
                                        (3, 1, 1, 1)])
def test_ref_equals_autograd(B, F, dim, nd, use_fm):
    c = hr.float_case(B, F, dim, nd, F * dim + nd + 5, seed=B + F)
    r = hr.head_bwd_ref(c.e_all, c.dense, c.w, c.d_deep_in, c.d_partial,
                        use_fm)
    de, dd, dw, db = _autograd(c, use_fm)
    for name, got, want in (("de_all", r.de_all, de), ("d_dense", r.d_dense,
                                                       dd),
                            ("dw", r.dw, dw), ("db", r.db, db.reshape(1))):
        assert got.shape == want.shape, name
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), name


def _case():
    c = hr.float_case(64, 26, 9, 13, 256, seed=3)
    r = hr.head_bwd_ref(c.e_all, c.dense, c.w, c.d_deep_in, c.d_partial, True)
    n = hr.n_terms(c.B, 4)
    return c, r, n


def test_checks_accept_fp32_evaluation():
    """An honest fp32 evaluation (torch on the CPU) is inside every bound,
    with and without a base."""
    c, r, n = _case()
    gp = c.d_partial
    dw32 = (gp.unsqueeze(1) * c.dense).sum(0)
    db32 = gp.sum().reshape(1)
    assert hr.acc_ratio(dw32, r.dw, r.dw_mag, n) <= 1
    assert hr.acc_ratio(db32, r.db, r.db_mag, n) <= 1
    base = torch.arange(13, dtype=torch.float32) * 7 - 40
    assert hr.acc_ratio(base + dw32, r.dw, r.dw_mag, n, base) <= 1
    e = c.e_all[..., :9]
    g_e = (c.d_deep_in[:, :234].reshape(64, 26, 9)
           + gp.view(-1, 1, 1) * (e.sum(1, keepdim=True) - e))
    de32 = torch.cat([g_e, gp.view(-1, 1, 1).expand(64, 26, 1)], dim=2)
    assert hr.elem_ratio(de32, r.de_all, r.de_mag, c.F) <= 1
    dd32 = c.d_deep_in[:, 234:247] + gp.unsqueeze(1) * c.w
    assert hr.elem_ratio(dd32, r.d_dense, r.d_dense_mag, c.F) <= 1


def test_checks_reject_mistakes():
    c, r, n = _case()
    # dw accumulated twice
    assert hr.acc_ratio(2 * r.dw, r.dw, r.dw_mag, n) > 1
    assert hr.acc_ratio(2 * r.db, r.db, r.db_mag, n) > 1
    # a base that was overwritten instead of accumulated into
    base = torch.full((13,), 100.0, dtype=f64)
    assert hr.acc_ratio(r.dw, r.dw, r.dw_mag, n, base) > 1
    assert hr.acc_ratio(base + r.dw, r.dw, r.dw_mag, n, base) <= 1
    # gp * w[j] dropped from d_dense
    assert hr.elem_ratio(c.d_deep_in[:, 234:247].to(f64), r.d_dense,
                         r.d_dense_mag, c.F) > 1
    # FM sign flipped in de_all
    e = c.e_all[..., :9].to(f64)
    gp = c.d_partial.to(f64).view(-1, 1, 1)
    flipped = torch.cat([c.d_deep_in[:, :234].to(f64).reshape(64, 26, 9)
                         - gp * (e.sum(1, keepdim=True) - e),
                         gp.expand(64, 26, 1)], dim=2)
    assert hr.elem_ratio(flipped, r.de_all, r.de_mag, c.F) > 1
    assert hr.elem_ratio(r.de_all, r.de_all, r.de_mag, c.F) <= 1
