"""k_cin_fwd / k_cin_dw / k_cin_dx of ops/csrc/cin.hip through their direct
entry points, against the exact oracle of tests/cin_ref.py (all @gpu). The
reference side is tested without a GPU in tests/test_cin_ref_checkers.py.

Two kinds of check on every shape:

  - integer operands (x0, xk, dout in {-3..3}, W in {-2..2}): every value a
    kernel forms is exact in bf16 and fp32 in any order, atomics included,
    so the output must be torch.equal to the int64 einsum. A dropped,
    doubled or mis-indexed element, k-tile or n-chunk fails;
  - randn operands: the output must lie within cin_ref.bound of the float64
    reference that performs the kernel's own roundings. The bound is the
    worst case of an fp32 accumulation, derived and not fitted; a wrong
    rounding of V, x0, xk or dout is far outside it at the small-K shapes
    (test_cin_ref_checkers.py).

The shapes (N, F, H, O) are the smallest that reach each path: K inside an
8-element pack, a partial or single K-chunk, spare waves at O < 128, the
generic Op != 128 loop of k_cin_dx next to its prefetch path, partial
h-tiles, empty and uneven n-splits of k_cin_dw, column tails, F = 1 and the
maximum geometry F = 32, H = 128. (160, 8, 8) and (96, 16, 18) are shapes
at which k_cin_dx's last fragment reads past ceil32(F*H) rows of wt; they
are legal because wt carries cin_ref.wt_rows(F, H) rows, which the binding
requires.

Worst |err| / bound observed on an MI355X over the float cases below
(information only; the bound is not adjusted to it):
fwd 1.6e-2 at (32, 3, 5, 16); dW 2.8e-2 at (F, H, O) = (2, 128, 128),
Np = 32, n_split = 1; dx0 1.4e-2 at (160, 8, 8), O = 16; dxk 1.8e-2 at
(96, 3, 5), O = 16. Every integer case was equal.
"""

import functools

import pytest
import torch

import cin_ref as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf16 = torch.bfloat16


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


@functools.lru_cache(maxsize=None)
def _case(kind, N, F, H, O):
    """One case, built once and shared unchanged: its operands on the CPU
    and the same on the GPU."""
    make = cr.int_case if kind == "int" else cr.float_case
    cpu = make(N, F, H, O, seed=N + 7 * F + 11 * H + 13 * O)
    dev = tuple(t.to(DEV) for t in cpu)
    return cpu, dev


@functools.lru_cache(maxsize=None)
def _int_oracle(N, F, H, O):
    return cr.int_oracle(*_case("int", N, F, H, O)[0])


def _report(kernel, shape, ratio):
    print(f"cin-ratio {kernel} {shape} {ratio:.3e}")


# ---------------------------------------------------------------- forward

FWD_SHAPES = [
    (32, 3, 5, 16),       # K=15, Kp=32: one partial chunk, K ends mid-pack,
                          # 7 spare waves, N < 128
    (160, 8, 8, 48),      # K=Kp=64, no pad; second block, 32-column tail
    (288, 5, 26, 128),    # Kp=160: full chunk then a 32-wide one; K=130
                          # ends 2 into it; H no power of two; 3 blocks
    (96, 26, 26, 128),    # benchmark layer 1: 676 -> 704, 5 chunks then 64
    (64, 32, 128, 128),   # maximum geometry, 32 chunks, prefetch carried
    (64, 1, 16, 16),      # F = 1
]


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_fwd_integer_exact(shape):
    (_, _, W, _), (x0d, xkd, _, _) = _case("int", *shape)
    out = _ext().cin_fwd(x0d, xkd, cr.pack_wp(W).to(DEV))
    assert cr.equals_int(out, _int_oracle(*shape)[0])


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_fwd_float_within_bound(shape):
    (x0p, xkp, W, _), (x0d, xkd, _, _) = _case("float", *shape)
    wp = cr.pack_wp(W).to(DEV)
    out = _ext().cin_fwd(x0d, xkd, wp)
    again = _ext().cin_fwd(x0d, xkd, wp)
    ref, mag = cr.fwd_ref(x0p, xkp, W)
    ratio = cr.err_ratio(out, ref, mag, wp.shape[1] + 2)
    _report("fwd", shape, ratio)
    assert ratio <= 1.0
    assert torch.equal(out, again)          # no atomics: bit-identical


# --------------------------------------------------------------------- dW

DW_SHAPES = [(3, 5, 16), (8, 8, 48), (5, 26, 128), (2, 128, 128)]  # F, H, O
DW_SPLITS = [
    (32, 1),      # one half chunk
    (96, 8),      # five empty splits
    (160, 3),     # splits of 64 / 64 / 32
    (416, 1),     # six full chunks and a half chunk, one block per field
    (416, 16),    # 13 chunks over 16 splits
]


def _dw_operands(kind, Np, F, H, O):
    (x0p, xkp, _, doutp), _ = _case(kind, Np, F, H, O)
    return [cr.pack_t(t) for t in (doutp, x0p, xkp)]


@pytest.mark.parametrize("split", DW_SPLITS)
@pytest.mark.parametrize("shape", DW_SHAPES)
def test_dw_integer_exact(shape, split):
    F, H, O = shape
    Np, n_split = split
    ops = _dw_operands("int", Np, F, H, O)
    dw = _ext().cin_dw(*[t.to(DEV) for t in ops], O, n_split)
    assert cr.equals_int(dw, _int_oracle(Np, F, H, O)[1])


@pytest.mark.parametrize("split", DW_SPLITS)
@pytest.mark.parametrize("shape", DW_SHAPES)
def test_dw_float_within_bound(shape, split):
    F, H, O = shape
    Np, n_split = split
    ops = _dw_operands("float", Np, F, H, O)
    dw = _ext().cin_dw(*[t.to(DEV) for t in ops], O, n_split)
    ref, mag = cr.dw_ref(*ops)
    ratio = cr.err_ratio(dw, ref, mag, Np + n_split + 2)
    _report("dw", shape + split, ratio)
    assert ratio <= 1.0


# --------------------------------------------------------------------- dx

DX_SHAPES = [(32, 1, 16), (96, 3, 5), (160, 8, 8), (96, 16, 18),
             (96, 26, 26), (64, 32, 128)]                       # N, F, H
DX_O = [16, 48, 80,      # generic loop, Op = 32, 64, 96
        112, 128]        # Op == 128 prefetch path; 112 has 16 pad columns


@pytest.mark.parametrize("O", DX_O)
@pytest.mark.parametrize("shape", DX_SHAPES)
def test_dx_integer_exact(shape, O):
    N, F, H = shape
    (_, _, W, _), (x0d, xkd, _, dzd) = _case("int", N, F, H, O)
    wt = cr.pack_wt(W, F, H).to(DEV)
    dx0, dxk = _ext().cin_dx(dzd, wt, x0d, xkd)
    _, _, want0, wantk = _int_oracle(N, F, H, O)
    assert cr.equals_int(dx0, want0)
    assert cr.equals_int(dxk, wantk)


@pytest.mark.parametrize("O", DX_O)
@pytest.mark.parametrize("shape", DX_SHAPES)
def test_dx_float_within_bound(shape, O):
    N, F, H = shape
    (x0p, xkp, W, doutp), (x0d, xkd, _, dzd) = _case("float", N, F, H, O)
    wt = cr.pack_wt(W, F, H).to(DEV)
    dx0, dxk = _ext().cin_dx(dzd, wt, x0d, xkd)
    a0, ak = _ext().cin_dx(dzd, wt, x0d, xkd)
    (r0, rk), (m0, mk) = cr.dx_ref(doutp, W, x0p, xkp)
    Op = wt.shape[1]
    ratio0 = cr.err_ratio(dx0, r0, m0, Op + H + 2)
    ratiok = cr.err_ratio(dxk, rk, mk, Op + F + 2)
    _report("dx0", shape + (O,), ratio0)
    _report("dxk", shape + (O,), ratiok)
    assert ratio0 <= 1.0 and ratiok <= 1.0
    assert torch.equal(dx0, a0) and torch.equal(dxk, ak)


# -------------------------------------------------------------- refusals

def _dx_args(N=32, F=8, H=8, O=16):
    (_, _, W, _), (x0d, xkd, _, dzd) = _case("int", N, F, H, O)
    return dzd, cr.pack_wt(W, F, H).to(DEV), x0d, xkd


def test_dx_refuses_wt_without_the_fragment_rows():
    dzd, wt, x0d, xkd = _dx_args(F=8, H=8)
    assert wt.shape[0] == 96
    short = wt[:64].contiguous()            # ceil32(F*H): the old rule
    with pytest.raises(RuntimeError, match="cin_dx shapes"):
        _ext().cin_dx(dzd, short, x0d, xkd)


def test_dx_refuses_op_wider_than_its_tile():
    dzd, wt, x0d, xkd = _dx_args(O=128)
    wide = torch.zeros(wt.shape[0], 160, dtype=bf16, device=DEV)
    with pytest.raises(RuntimeError, match="cin_dx shapes"):
        _ext().cin_dx(dzd, wide, x0d, xkd)


def test_dx_refuses_mismatched_rows_and_dtypes():
    dzd, wt, x0d, xkd = _dx_args()
    with pytest.raises(RuntimeError, match="cin_dx shapes"):
        _ext().cin_dx(dzd, wt, x0d[:16].contiguous(), xkd)
    with pytest.raises(RuntimeError, match="cin_dx shapes"):
        _ext().cin_dx(dzd, wt, x0d, xkd[:16].contiguous())
    with pytest.raises(RuntimeError, match="cin_dx dtypes"):
        _ext().cin_dx(dzd, wt, x0d.to(bf16), xkd)
    with pytest.raises(RuntimeError, match="cin_dx dtypes"):
        _ext().cin_dx(dzd, wt, x0d, xkd.double())
    with pytest.raises(RuntimeError, match="cin_dx shapes"):
        _ext().cin_dx(dzd[:, :0].contiguous(), wt, x0d, xkd)


def test_dw_refusals():
    def operands(O, Np=32, F=3, H=5):
        return [torch.zeros(r, Np, dtype=bf16, device=DEV)
                for r in (O, F, H)]
    ext = _ext()
    with pytest.raises(RuntimeError, match="cin_dw shapes"):
        ext.cin_dw(*operands(24), 24, 1)            # O no multiple of 16
    with pytest.raises(RuntimeError, match="cin_dw shapes"):
        ext.cin_dw(*operands(16), 32, 1)            # dzt rows != O
    with pytest.raises(RuntimeError, match="cin_dw shapes"):
        ext.cin_dw(*operands(16), 16, 0)            # n_split = 0
    with pytest.raises(RuntimeError, match="cin_dw shapes"):
        ext.cin_dw(*operands(16, F=33), 16, 1)
    assert ext.cin_dw(*operands(16), 16, 1).shape == (16, 15)


def test_fwd_refusals():
    (_, _, W, _), (x0d, xkd, _, _) = _case("int", 32, 3, 5, 16)
    ext = _ext()
    wp = cr.pack_wp(W).to(DEV)
    with pytest.raises(RuntimeError, match="cin_fwd shapes"):
        ext.cin_fwd(x0d, xkd[:16].contiguous(), wp)         # N mismatch
    with pytest.raises(RuntimeError, match="cin_fwd shapes"):
        ext.cin_fwd(x0d, xkd, wp[:0].contiguous())          # O < 16
    with pytest.raises(RuntimeError, match="cin_fwd shapes"):
        ext.cin_fwd(x0d, torch.cat([xkd] * 3, 1).contiguous(), wp)  # Kp < F*H


# ------------------------------------------------------------- layer level

@pytest.fixture
def hip_calls(monkeypatch):
    """Counts the calls _CINLayerFn makes into the three entry points."""
    ext = _ext()
    calls = {"cin_fwd": 0, "cin_dx": 0, "cin_dw": 0}

    def counted(name):
        real = getattr(ext, name)

        def wrapper(*a):
            calls[name] += 1
            return real(*a)
        return wrapper
    for name in calls:
        monkeypatch.setattr(ext, name, counted(name))
    return calls


def _layer(x0, xk, W, dout, same):
    from openembedding_amd.models.ctr import _CINLayerFn
    a = x0.to(DEV).requires_grad_(True)
    b = a if same else xk.to(DEV).requires_grad_(True)
    w = W.to(DEV).requires_grad_(True)
    out = _CINLayerFn.apply(a, b, w, bf16)
    out.backward(dout.to(DEV))
    return out.detach(), a.grad, None if same else b.grad, w.grad


@pytest.mark.parametrize("shape,same", [
    ((8, 4, 8, 8, 16), True),       # first layer; wt needs the extra rows
    ((8, 4, 5, 5, 32), True),       # first layer; K = 25 inside a pack
    ((32, 9, 26, 26, 128), False),  # benchmark layer 1, d = 9
])
def test_layer_integer_exact_and_on_the_hip_path(shape, same, hip_calls):
    B, d, F, H, O = shape
    x0p, xkp, W, doutp = cr.int_case(B * d, F, H, O, seed=B)
    x0, xk, dout = (cr.to_layer(t, d) for t in (x0p, xkp, doutp))
    got = _layer(x0, xk, W, dout, same)
    want = cr.layer_autograd(x0, xk, W, dout, same)
    assert hip_calls == {"cin_fwd": 1, "cin_dx": 1, "cin_dw": 1}
    for g, w_ in zip(got, want):
        if w_ is None:
            assert g is None
            continue
        assert g.dtype == torch.float32
        assert cr.equals_int(g, w_)


def test_layer_falls_back_when_columns_are_no_multiple_of_32(hip_calls):
    from openembedding_amd.models.ctr import _CINLayerFn
    B, d, F, H, O = 5, 3, 3, 4, 16
    g = torch.Generator().manual_seed(0)
    # {-1, 0, 1}: every value of the torch bf16 path stays an integer
    # below 256, which its bf16 outputs hold exactly
    x0, xk, W, dout = (
        torch.randint(-1, 2, s, generator=g).float()
        for s in ((B, F, d), (B, H, d), (O, F * H), (B, O, d)))
    assert not _CINLayerFn._hip_ok(x0.to(DEV), W.to(DEV), bf16)
    got = _layer(x0, xk, W, dout, same=False)
    want = cr.layer_autograd(x0, xk, W, dout)
    assert hip_calls == {"cin_fwd": 0, "cin_dx": 0, "cin_dw": 0}
    # the tolerances of tests/test_cin.py
    torch.testing.assert_close(got[0].cpu().double(), want[0],
                               rtol=1e-5, atol=1e-6)
    for g_, w_ in zip(got[1:], want[1:]):
        torch.testing.assert_close(g_.cpu().double(), w_,
                                   rtol=1e-4, atol=1e-5)
