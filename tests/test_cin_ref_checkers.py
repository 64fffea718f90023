"""The CIN references of tests/cin_ref.py, tested on the CPU: they equal a
naive int64 einsum on integer cases, agree with float64 autograd through
the einsum, keep an fp32 emulation of each kernel inside ``bound``, and
reject the mutants they exist for.

Where the rounding-mode assertions live: ``bound`` is a worst-case bound,
so it grows with K while a wrong rounding's error grows with sqrt(K). At
K = 4096 a V truncated to bf16 instead of rounded is only about 2x over
it; at K = 15 it is a thousand times over. The rounding mutants are
therefore asserted on the small-K shapes (32,3,5,16) and (96,16,18,48),
and the K = 4096 shape only has to stay inside the bound. Dropped, doubled
or mis-indexed elements are caught at every shape by integer equality,
which has no tolerance at all.
"""

import pytest
import torch

import cin_ref as cr

bf16 = torch.bfloat16

SMALL = [(32, 3, 5, 16), (96, 16, 18, 48)]          # (N, F, H, O)
SHAPES = SMALL + [(160, 32, 128, 128)]


# ------------------------------------------------- fp32 kernel emulations

def _trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _r(t, on=True):
    return t.to(bf16).float() if on else t


def emu_fwd(x0p, xkp, W, trunc_v=False, round_x0=True, round_xk=True,
            swap_fh=False, drop_last_k=False):
    """k_cin_fwd in fp32 on the CPU, from the packed weight."""
    N, F = x0p.shape
    H = xkp.shape[1]
    wp = cr.pack_wp(W).float()
    a, b = _r(x0p, round_x0), _r(xkp, round_xk)
    if swap_fh:                                    # k = h*F + f
        v = (b.unsqueeze(2) * a.unsqueeze(1)).reshape(N, F * H)
    else:
        v = (a.unsqueeze(2) * b.unsqueeze(1)).reshape(N, F * H)
    v = _trunc_bf16(v) if trunc_v else _r(v)
    vp = torch.zeros(N, wp.shape[1])
    vp[:, :F * H - (1 if drop_last_k else 0)] = \
        v[:, :F * H - (1 if drop_last_k else 0)]
    return torch.matmul(vp, wp.t())


def emu_dw(dzt, x0t, xkt, drop_chunk=None, spill=False):
    """k_cin_dw in fp32 on the CPU: per field a [O x ceil16(H)] tile over
    n, stored below h < H. ``spill`` is the kernel without its partial
    h-tile handling: rows past H hold the next rows of xkt and the store
    runs on into field f+1."""
    O, Np = dzt.shape
    F, H = x0t.shape[0], xkt.shape[0]
    Hp = cr.ceil_to(H, 16)
    dz = dzt.float().clone()
    if drop_chunk is not None:
        dz[:, drop_chunk * 32:(drop_chunk + 1) * 32] = 0
    xk = torch.zeros(Hp, Np)
    xk[:H] = xkt.float()
    if spill:
        xk[H:] = xkt.float()[torch.arange(Hp - H) % H]
    dw = torch.zeros(O, F * H + Hp)
    for f in range(F):
        b = _r(xk * x0t[f].float().unsqueeze(0))            # [Hp, Np]
        tile = torch.matmul(dz, b.t())                      # [O, Hp]
        width = Hp if spill else H
        dw[:, f * H:f * H + width] += tile[:, :width]
    return dw[:, :F * H]


def emu_dx(doutp, W, x0p, xkp, round_dout=True, pad_fill=0.0):
    """k_cin_dx in fp32 on the CPU, from the packed wt and a dZ tile Op
    wide. ``pad_fill`` puts a value into the pad columns [O, Op) of both,
    which the kernel and the packer keep at zero."""
    N, F = x0p.shape
    H = xkp.shape[1]
    O = doutp.shape[1]
    wt = cr.pack_wt(W, F, H).float()
    dz = torch.zeros(N, wt.shape[1])
    dz[:, :O] = _r(doutp, round_dout)
    wt[:, O:] = pad_fill
    dz[:, O:] = pad_fill
    p = torch.matmul(dz, wt[:F * H].t()).view(N, F, H)
    dx0 = (p * xkp.unsqueeze(1)).sum(2)
    dxk = (p * x0p.unsqueeze(2)).sum(1)
    return dx0, dxk


def _ratios(case, **mut):
    """|err| / bound of the three emulations on one case."""
    x0p, xkp, W, doutp = case
    N, F = x0p.shape
    H, O = xkp.shape[1], W.shape[0]
    Kp, Op, Np = cr.ceil_to(F * H, 32), cr.ceil_to(O, 32), cr.ceil_to(N, 32)
    out, mag = cr.fwd_ref(x0p, xkp, W)
    fwd_kw = {k: v for k, v in mut.items()
              if k in ("trunc_v", "round_x0", "round_xk")}
    r = {"fwd": cr.err_ratio(emu_fwd(x0p, xkp, W, **fwd_kw), out, mag,
                             Kp + 2)}
    ops = [cr.pack_t(t) for t in (doutp, x0p, xkp)]
    dw, mag = cr.dw_ref(*ops)
    r["dw"] = cr.err_ratio(emu_dw(*ops), dw, mag, Np + 1 + 2)
    (dx0, dxk), (m0, mk) = cr.dx_ref(doutp, W, x0p, xkp)
    g0, gk = emu_dx(doutp, W, x0p, xkp,
                    round_dout=mut.get("round_dout", True))
    r["dx0"] = cr.err_ratio(g0, dx0, m0, Op + H + 2)
    r["dxk"] = cr.err_ratio(gk, dxk, mk, Op + F + 2)
    return r


# ------------------------------------------------------- integer equality

@pytest.mark.parametrize("shape", SHAPES + [(64, 1, 16, 16), (160, 8, 8, 48)])
def test_references_equal_int64_einsum(shape):
    x0p, xkp, W, doutp = case = cr.int_case(*shape)
    out, dw, dx0, dxk = cr.int_oracle(*case)
    # the oracle against the einsum written out, independent of its code
    N, F = x0p.shape
    H = xkp.shape[1]
    z = torch.einsum("nf,nh->nfh", x0p.long(), xkp.long()).reshape(N, -1)
    assert torch.equal(out, torch.einsum("ok,nk->no", W.long(), z))
    assert torch.equal(dw, torch.einsum("no,nk->ok", doutp.long(), z))
    p = torch.einsum("no,ok->nk", doutp.long(), W.long()).view(N, F, H)
    assert torch.equal(dx0, torch.einsum("nfh,nh->nf", p, xkp.long()))
    assert torch.equal(dxk, torch.einsum("nfh,nf->nh", p, x0p.long()))
    # the float64 references hit it exactly, and so do the emulations
    assert cr.equals_int(cr.fwd_ref(x0p, xkp, W)[0], out)
    ops = [cr.pack_t(t) for t in (doutp, x0p, xkp)]
    assert cr.equals_int(cr.dw_ref(*ops)[0], dw)
    (r0, rk), _ = cr.dx_ref(doutp, W, x0p, xkp)
    assert cr.equals_int(r0, dx0) and cr.equals_int(rk, dxk)
    assert cr.equals_int(emu_fwd(x0p, xkp, W), out)
    assert cr.equals_int(emu_dw(*ops), dw)
    g0, gk = emu_dx(doutp, W, x0p, xkp)
    assert cr.equals_int(g0, dx0) and cr.equals_int(gk, dxk)


def test_int_case_asserts_its_limits():
    with pytest.raises(AssertionError):
        cr.int_case(32, 33, 5, 16)
    with pytest.raises(AssertionError):
        cr.int_case(32, 3, 129, 16)
    with pytest.raises(AssertionError):
        cr.int_oracle(*cr.float_case(32, 3, 5, 16))


@pytest.mark.parametrize("shape", SMALL)
def test_integer_equality_rejects_index_mutants(shape):
    x0p, xkp, W, doutp = case = cr.int_case(*shape, seed=1)
    out, dw, dx0, dxk = cr.int_oracle(*case)
    F, H = x0p.shape[1], xkp.shape[1]
    assert not cr.equals_int(emu_fwd(x0p, xkp, W, drop_last_k=True), out)
    assert not cr.equals_int(emu_fwd(x0p, xkp, W, swap_fh=True), out)
    ops = [cr.pack_t(t) for t in (doutp, x0p, xkp)]
    for chunk in range(ops[0].shape[1] // 32):
        assert not cr.equals_int(emu_dw(*ops, drop_chunk=chunk), dw)
    assert H % 16 and F > 1
    assert not cr.equals_int(emu_dw(*ops, spill=True), dw)
    g0, gk = emu_dx(doutp, W, x0p, xkp, pad_fill=1.0)
    assert not cr.equals_int(g0, dx0) and not cr.equals_int(gk, dxk)


def test_equals_int_wants_every_element_and_the_shape():
    want = torch.arange(12).view(3, 4)
    assert cr.equals_int(want.float(), want)
    off = want.float()
    off[2, 3] += 1
    assert not cr.equals_int(off, want)
    assert not cr.equals_int(want.float().view(4, 3), want)
    assert not cr.equals_int(want.float() + 0.5, want)


# ------------------------------------------------ float64 autograd oracle

def _autograd(x0p, xkp, W, doutp, d):
    """cr.layer_autograd from and to the d-leading column layout
    n = dd*B + b: out, dW, dx0, dxk."""
    out, dx0, dxk, dw = cr.layer_autograd(
        cr.to_layer(x0p, d), cr.to_layer(xkp, d), W, cr.to_layer(doutp, d))
    return cr.to_cols(out), dw, cr.to_cols(dx0), cr.to_cols(dxk)


@pytest.mark.parametrize("shape", SMALL)
def test_references_agree_with_float64_autograd(shape):
    x0p, xkp, W, doutp = cr.float_case(*shape, seed=2)
    # inputs rounded the way the references round them: x0, xk to 4
    # significant bits (so bf16 holds them and their products exactly),
    # dout to bf16
    x0p = (x0p * 4).round().clamp(-15, 15) / 4
    xkp = (xkp * 4).round().clamp(-15, 15) / 4
    doutp = doutp.to(bf16).float()
    out, dw, dx0, dxk = _autograd(x0p, xkp, W, doutp, d=2)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(cr.fwd_ref(x0p, xkp, W)[0], out, **tol)
    ops = [cr.pack_t(t) for t in (doutp, x0p, xkp)]
    torch.testing.assert_close(cr.dw_ref(*ops)[0], dw, **tol)
    (r0, rk), _ = cr.dx_ref(doutp, W, x0p, xkp)
    torch.testing.assert_close(r0, dx0, **tol)
    torch.testing.assert_close(rk, dxk, **tol)


def test_dx_ref_keeps_x0_and_xk_unrounded():
    # with plain fp32 x0 / xk the input gradients still equal autograd's:
    # only dout is rounded on that path
    shape = SMALL[1]
    x0p, xkp, W, doutp = cr.float_case(*shape, seed=3)
    doutp = doutp.to(bf16).float()
    _, _, dx0, dxk = _autograd(x0p, xkp, W, doutp, d=2)
    (r0, rk), _ = cr.dx_ref(doutp, W, x0p, xkp)
    torch.testing.assert_close(r0, dx0, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rk, dxk, rtol=1e-12, atol=1e-12)
    assert not torch.equal(x0p.to(bf16).float(), x0p)


def test_mag_dominates_the_value():
    x0p, xkp, W, doutp = cr.float_case(*SMALL[1], seed=4)
    out, mag = cr.fwd_ref(x0p, xkp, W)
    assert bool((out.abs() <= mag).all()) and bool((mag > 0).all())
    dw, mag = cr.dw_ref(*[cr.pack_t(t) for t in (doutp, x0p, xkp)])
    assert bool((dw.abs() <= mag).all())
    (dx0, dxk), (m0, mk) = cr.dx_ref(doutp, W, x0p, xkp)
    assert bool((dx0.abs() <= m0).all()) and bool((dxk.abs() <= mk).all())


# -------------------------------------------------------------- the bound

def test_bound_formula():
    assert cr.bound(torch.tensor(0.0, dtype=torch.float64), 10) == 2.0 ** -126
    got = cr.bound(torch.tensor(8.0, dtype=torch.float64), 34)
    assert got == 34 * 2.0 ** -23 * 8.0 + 2.0 ** -126


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_emulation_stays_inside_bound(shape):
    r = _ratios(cr.float_case(*shape, seed=5))
    print(shape, r)
    assert max(r.values()) < 0.5, r


@pytest.mark.parametrize("shape", SMALL)
def test_bound_rejects_rounding_mutants(shape):
    case = cr.float_case(*shape, seed=5)
    r = _ratios(case, trunc_v=True)
    print(shape, "V truncated", r["fwd"])
    assert r["fwd"] > 1
    for kw in ("round_x0", "round_xk"):
        r = _ratios(case, **{kw: False})
        print(shape, kw, "off", r["fwd"])
        assert r["fwd"] > 1
    r = _ratios(case, round_dout=False)
    print(shape, "dout unrounded", r["dx0"], r["dxk"])
    assert r["dx0"] > 1 and r["dxk"] > 1


# ---------------------------------------------------------------- packers

def test_wt_rows_covers_every_row_the_kernel_reads():
    for F in range(1, 33):
        for H in range(1, 129):
            rows = cr.wt_rows(F, H)
            assert rows % 32 == 0 and rows >= cr.ceil_to(F * H, 32)
            assert rows >= cr.wt_rows_read(F, H), (F, H)
            assert rows - cr.wt_rows_read(F, H) < 32, (F, H)


def test_first_layer_shapes_that_ceil32_left_short():
    short = [n for n in range(1, 33)
             if cr.ceil_to(n * n, 32) < cr.wt_rows_read(n, n)]
    assert short == [5, 8, 21, 24]
    assert cr.wt_rows_read(8, 8) == 72 and cr.wt_rows(8, 8) == 96
    assert cr.ceil_to(16 * 18, 32) < cr.wt_rows_read(16, 18)
    # the benchmark shapes pad past it
    assert cr.wt_rows(26, 26) == 704 and cr.wt_rows(26, 128) == 26 * 128


def test_wt_rows_is_the_layer_rule():
    from openembedding_amd.models.ctr import _CINLayerFn
    for F, H in [(8, 8), (5, 5), (16, 18), (26, 26), (26, 128), (1, 16)]:
        assert _CINLayerFn._wt_rows(F, H) == cr.wt_rows(F, H)
        W = torch.randn(16, F * H)
        bufs = _CINLayerFn._bufs(W, F, H)
        assert torch.equal(bufs["wp"], cr.pack_wp(W))
        assert torch.equal(bufs["wt"], cr.pack_wt(W, F, H))


def test_packers_zero_their_tails():
    x0p, xkp, W, doutp = cr.int_case(40, 3, 5, 16, seed=6)
    wp, wt = cr.pack_wp(W), cr.pack_wt(W, 3, 5)
    assert wp.shape == (16, 32) and wt.shape == (32, 32)
    assert torch.equal(wp[:, :15].float(), W) and not wp[:, 15:].any()
    assert torch.equal(wt[:15, :16].float(), W.t())
    assert not wt[15:].any() and not wt[:, 16:].any()
    t = cr.pack_t(doutp)
    assert t.shape == (16, 64) and t.dtype == bf16
    assert torch.equal(t[:, :40].float(), doutp.t()) and not t[:, 40:].any()
    assert cr.pack_t(doutp, 96).shape == (16, 96)
