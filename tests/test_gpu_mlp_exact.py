"""k_mlp3_fwd, k_mlp3_bwd, k_mlp3_wgrad + finisher and k_mlp3_bias_bwd +
k_mlp3_bias_finish of ops/csrc/mlp.hip through their direct entry points,
and _FusedMLP3Fn through every backward branch, against the oracle of
tests/mlp_ref.py (all @gpu). The reference side is tested without a GPU in
tests/test_mlp_ref_checkers.py, mutant by mutant.

Two kinds of check:

  - integer operands (mlp_ref.int_case and its kin): every fp32 partial sum
    is an exact integer below 2^24 in any order, float atomics and the
    MFMA's internal order included, so every output must be torch.equal to
    the oracle's FULL chain (its own a1, not the kernel's), roundings to
    bf16 included. The activations outgrow bf16's 8 bits on purpose: ties
    and inexact values make up several per cent of a2, a3, dz1 and dx0
    (asserted in int_case), which pins round-to-nearest-even, the place of
    the bias add, the mask ``> 0`` and the one fp32 ``+=`` of the
    finishers. Every row tile, both weight layouts and all m_splits are
    held to the SAME oracle, not to each other;
  - random operands (mlp_ref.float_case): each stage is recomputed in
    float64 from the kernel's own previous bf16 output, and the kernel's
    bf16 must lie in the interval that the derived bound of an fp32
    accumulation (cin_ref.bound) leaves open after the epilogue; fp32
    outputs must lie within the bound itself. dz3 is one fp32 product per
    element and must be equal. Only the derived delta is asserted; the
    smallest fraction of it that still passes is printed as measured
    tightness (docs/kernels.md).

Shapes (H, K0, K0p) are the smallest that reach each path: the unrolled
Kp == 256 and Kp == 416 layers at (400, 247, 256) and (416, 256, 256), the
generic k-loop at (16, 20, 32) and (64, 50, 64), the dim-64 width (400,
1677, 1696), where the forward has BM = 16 only; rows around one and two
tiles of every BM.

test_function_paths_exact: the branches that this project's kernels
compute (prebound grads with M % 32 == 0: fused wgrad with its bias rider,
head sums from the dgrad kernel, finisher) are held to equality. The
library-GEMM branches (autograd's ``dz^T @ x``, ``addmm_`` at M = 130 and
at K0p = 1696) are held to equality as well: their sums are integers
below 2^24, which a GEMM that accumulates in fp32 and rounds once
reproduces.
"""

import functools

import pytest
import torch

import mlp_fraglayout_ref as fl
import mlp_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf16 = torch.bfloat16
f32 = torch.float32
f64 = torch.float64

SHAPES = [(400, 247, 256), (416, 256, 256), (16, 20, 32), (64, 50, 64)]
WIDE = (400, 1677, 1696)
BMS = [0, 16, 32, 64]              # 0 = the launcher's choice


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _rows(bm, shape):
    if shape == WIDE:
        return [1, 17]
    b = bm or 16
    return sorted({1, 17, b - 1, b + 1, 2 * b + 3})


def _hp(H):
    return mr.ceil_to(H, 32)


def _bm_kw(bm, frag):
    kw = {"frag": frag}
    if bm:
        kw["bm"] = bm
    return kw


@functools.lru_cache(maxsize=None)
def _int(M, H, K0):
    return mr.int_case(M, H, K0)


def _weights(c, K0p, frag):
    """The padded weight operands of mlp3_fwd and mlp3_bwd in one layout,
    built on the CPU by the helpers of mlp_fraglayout_ref."""
    H, Hp = c.H, _hp(c.H)
    lay = fl.pack if frag else (lambda t: t)

    def img(w, n, k):
        return lay(fl.pad(w.to(bf16), n, k)).contiguous().to(DEV)

    fwd = [img(c.w1, H, K0p), img(c.w2, H, Hp), img(c.w3, H, Hp)]
    bwd = [img(c.w3.t(), H, Hp), img(c.w2.t(), H, Hp),
           img(c.w1.t(), K0p, Hp)]
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _dev(shape):
    """One integer case per shape, built once and shared unchanged: the
    operands and the oracle's chain on the GPU, in the kernels' dtypes.
    Smaller M are row slices (mlp_ref.take_rows)."""
    H, K0, K0p = shape
    c = _int(17 if shape == WIDE else 131, H, K0)
    d = {"case": c}
    for frag in (False, True):
        d["fwd", frag], d["bwd", frag] = _weights(c, K0p, frag)
    for k in ("b1", "b2", "b3", "w4", "b4", "a1", "a2", "a3", "dz1", "dz2",
              "dz3"):
        d[k] = getattr(c, k).to(bf16).to(DEV)
    d["x0"] = mr.padded(c.x0, c.M, K0p).to(DEV)
    d["dx0"] = mr.padded(c.dx0, c.M, K0p).to(DEV)
    for k in ("partial", "dout", "out", "out_nopartial"):
        d[k] = getattr(c, k).to(f32).to(DEV)
    return d


def _is(got, want, shape, dtype):
    """Exact shape and dtype, then every bit."""
    assert tuple(got.shape) == tuple(shape) and got.dtype == dtype
    return torch.equal(got, want)


def _run_fwd(d, M, bm, frag, partial=True):
    w1, w2, w3 = d["fwd", frag]
    return _ext().mlp3_fwd(
        d["x0"][:M].contiguous(), w1, d["b1"], w2, d["b2"], w3, d["b3"],
        d["w4"], d["b4"], d["partial"][:M].contiguous() if partial else None,
        **_bm_kw(bm, frag))


def _check_fwd(d, M, bm, frag):
    H = d["case"].H
    for partial in (True, False):
        out, a1, a2, a3 = _run_fwd(d, M, bm, frag, partial)
        tag = (M, bm, frag, partial)
        for name, got in (("a1", a1), ("a2", a2), ("a3", a3)):
            assert _is(got, d[name][:M], (M, H), bf16), (name, tag)
        want = d["out" if partial else "out_nopartial"][:M]
        assert _is(out, want, (M,), f32), ("out", tag)


def _run_bwd(d, M, bm, frag, bs):
    w3t, w2t, w1t = d["bwd", frag]
    return _ext().mlp3_bwd(
        d["dout"][:M].contiguous(), d["a1"][:M].contiguous(),
        d["a2"][:M].contiguous(), d["a3"][:M].contiguous(), d["w4"],
        w3t, w2t, w1t, bs, **_bm_kw(bm, frag))


def _check_bwd(d, M, bm, frag):
    c = d["case"]
    H, K0p = c.H, d["x0"].shape[1]
    s = mr.take_rows(c, M)
    buf = torch.zeros(4 * H + 1 + 32, device=DEV)
    buf[4 * H + 1:] = 7.0                       # canary behind the scratch
    bs = buf[:4 * H + 1]
    res = _run_bwd(d, M, bm, frag, bs)
    tag = (M, bm, frag)
    for name, got in zip(("dx0", "dz1", "dz2", "dz3"), res):
        shape = (M, K0p if name == "dx0" else H)
        assert _is(got, d[name][:M], shape, bf16), (name, tag)
    assert torch.equal(bs[3 * H:4 * H], s.dw4.to(f32).to(DEV)), tag
    assert float(bs[4 * H]) == float(s.db4), tag
    assert float(bs[:3 * H].abs().sum()) == 0.0, tag   # not this kernel's
    assert bool((buf[4 * H + 1:] == 7.0).all()), tag
    # without the scratch: the same dgrad chain
    for got, want in zip(_run_bwd(d, M, bm, frag, None), res):
        assert torch.equal(got, want), tag


FWD_CASES = [(s, bm) for s in SHAPES for bm in BMS] + [(WIDE, 0), (WIDE, 16)]
BWD_CASES = [(s, bm) for s in SHAPES + [WIDE] for bm in BMS]


@pytest.mark.parametrize("frag", [False, True])
@pytest.mark.parametrize("shape,bm", FWD_CASES)
def test_fwd_exact(shape, bm, frag):
    d = _dev(shape)
    for M in _rows(bm, shape):
        _check_fwd(d, M, bm, frag)


@pytest.mark.parametrize("frag", [False, True])
@pytest.mark.parametrize("shape,bm", BWD_CASES)
def test_bwd_exact(shape, bm, frag):
    d = _dev(shape)
    for M in _rows(bm, shape):
        _check_bwd(d, M, bm, frag)


def test_exact_with_images_from_pack_kernel():
    # the same oracle once more, the six images written by mlp3_pack_frag
    shape = SHAPES[0]
    H, K0, K0p = shape
    d = dict(_dev(shape))
    c = d["case"]
    Hp = _hp(H)
    w1, w2, w3 = (t.to(bf16).to(DEV) for t in (c.w1, c.w2, c.w3))
    junk = lambda *s: torch.full(s, float("nan"), device=DEV,  # noqa: E731
                                 dtype=bf16)
    dsts = [junk(H, K0p), junk(H, Hp), junk(H, Hp), junk(H, Hp),
            junk(H, Hp), junk(K0p, Hp)]
    _ext().mlp3_pack_frag([w1, w2, w3, w3, w2, w1], dsts,
                          [False, False, False, True, True, True])
    for got, want in zip(dsts, d["fwd", True] + d["bwd", True]):
        assert torch.equal(got, want)
    d["fwd", True], d["bwd", True] = dsts[:3], dsts[3:]
    _check_fwd(d, 131, 0, True)
    _check_bwd(d, 131, 0, True)


# ---------------------------------------------------------------- wgrad

def _b(t):
    return t.to(bf16).to(DEV)


@pytest.mark.parametrize("rider", [False, True])
@pytest.mark.parametrize("H,K0,K0p", SHAPES[:3])
@pytest.mark.parametrize("M", [32, 160, 1056])
def test_wgrad_exact(M, H, K0, K0p, rider):
    # M = 32: one chunk shorter than 128; M = 160 with 8 splits: three
    # empty splits; M = 1056: uneven splits, and sums past 256 that the
    # finisher has to round. Every m_split must give the oracle's bits.
    ext = _ext()
    c = mr.wgrad_int_case(M, H, K0, K0p)
    once = mr.wgrad_apply(c, c.base)
    twice = mr.wgrad_apply(c, once)
    ops = [_b(t) for t in c.dz + [c.x0, c.a1, c.a2]]
    colsum = torch.cat(c.colsum).to(f32).to(DEV)
    for m_split in (0, 1, 2, 8):
        guard = torch.full((H * K0 + 64,), 7.0, device=DEV, dtype=bf16)
        dw1 = guard[:H * K0].view(H, K0)
        dw1.copy_(_b(c.base[0]))
        got = [dw1, _b(c.base[1]), _b(c.base[2])]
        scratch = torch.zeros(H * K0p + 2 * H * H, device=DEV)
        bs = torch.zeros(4 * H + 1, device=DEV) if rider else None
        kw = {"m_split": m_split} if m_split else {}
        for n, want in enumerate((once, twice)):
            ext.mlp3_wgrad(*ops, scratch, *got, bs, **kw)
            for i in range(3):
                assert torch.equal(got[i], _b(want[i])), (
                    f"dw{i + 1}", m_split, n)
            assert float(scratch.abs().sum()) == 0.0      # self-cleaned
            assert bool((guard[H * K0:] == 7.0).all())
            if rider:
                assert torch.equal(bs[:3 * H], colsum), (m_split, n)
                assert float(bs[3 * H:].abs().sum()) == 0.0
                bs.zero_()


# ------------------------------------------------------------ bias pass

@pytest.mark.parametrize("H", [16, 400])
@pytest.mark.parametrize("M", [1, 33, 200])
def test_bias_bwd_exact(M, H):
    # emb_mlp3_bias_bwd gives a block 32 rows: M = 1 and 33 sit on either
    # side of one block, 200 is six blocks and a quarter; H = 400 takes a
    # thread through two columns. Parts that the flags leave out fold a
    # scratch preset by hand, as the fused wgrad / dgrad kernels leave it.
    ext = _ext()
    c = mr.bias_int_case(M, H)
    ops = [c.dout.to(f32).to(DEV)] + [_b(t) for t in c.dz] + [_b(c.a3)]
    base = torch.cat(c.base)
    idx = torch.arange(4 * H + 1)
    for with_dz in (False, True):
        for with_head in (False, True):
            sel = ((idx < 3 * H) & with_dz) | ((idx >= 3 * H) & with_head)
            buf = torch.zeros(4 * H + 1 + 32, device=DEV)
            buf[4 * H + 1:] = 7.0
            scratch = buf[:4 * H + 1]
            scratch.copy_(torch.where(sel, 0.0, c.preset).to(f32))
            want = mr.bias_finish_ref(base, torch.where(sel, c.sums,
                                                        c.preset))
            got = [_b(t) for t in c.base]
            ext.mlp3_bias_bwd(*ops, scratch, *got, with_dz, with_head)
            tag = (with_dz, with_head)
            assert torch.equal(torch.cat(got), _b(want)), tag
            assert float(scratch.abs().sum()) == 0.0, tag
            assert bool((buf[4 * H + 1:] == 7.0).all()), tag


# ------------------------------------------------- the autograd function

PATHS = {
    # name: (shape, M, prebound)
    "autograd": (SHAPES[0], 131, False),
    "prebound_fused_wgrad": (SHAPES[0], 160, True),
    "prebound_library_wgrad": (SHAPES[0], 130, True),
    "prebound_wide": (WIDE, 32, True),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_function_paths_exact(path):
    """Equality on every branch (see the module docstring): grads not
    prebound (library GEMMs and GEMVs); prebound with M % 32 == 0 (fused
    wgrad with bias rider, finisher only); prebound with M = 130 (addmm_
    wgrads, fused bias pass); K0p = 1696 (addmm_ by the K0p <= 512
    rule)."""
    from openembedding_amd.models.ctr import _FusedMLP3Fn
    (H, K0, K0p), M, prebound = PATHS[path]
    c = _int(M, H, K0)
    Hp = _hp(H)
    srcs = [c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, c.w4.view(1, H), c.b4]
    params = [_b(t).requires_grad_(True) for t in srcs]
    base = None
    if prebound:
        base = mr.int_base([tuple(t.shape) for t in srcs])
        for p, b in zip(params, base):
            p.grad = _b(b)
    want, _, _ = mr.param_grads_ref(c, base)
    x0 = mr.padded(c.x0, M, K0p).to(DEV).requires_grad_(True)
    partial = c.partial.to(f32).to(DEV).requires_grad_(True)
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=bf16)  # noqa: E731
    bufs = {"w1p": z(H, K0p), "w2p": z(H, Hp), "w3p": z(H, Hp),
            "w3tp": z(H, Hp), "w2tp": z(H, Hp), "w1tp": z(K0p, Hp)}
    out = _FusedMLP3Fn.apply(x0, partial, *params, bufs)
    assert torch.equal(out, c.out.to(f32).to(DEV))
    dout = c.dout.to(f32).to(DEV)
    out.backward(dout)
    wrong = []
    names = ["w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4"]
    for n, p, w in zip(names, params, want):
        assert p.grad.shape == p.shape and p.grad.dtype == bf16
        bad = int((p.grad != _b(w)).sum())
        if bad:
            wrong.append((n, bad, p.grad.numel()))
    print(f"mlp-paths {path} mismatching grads: {wrong}")
    assert not wrong, wrong
    assert torch.equal(x0.grad, mr.padded(c.dx0, M, K0p).to(DEV))
    assert torch.equal(partial.grad, dout)
    for k in ("bscratch", "wscratch"):
        if k in bufs:
            assert float(bufs[k].abs().sum()) == 0.0, k


# ------------------------------------------------------ random operands

SCALES = [2.0 ** -i for i in range(7)]          # 1 ... 1/64


def _tightness(got, ref, mag, n, **kw):
    """Violations at the derived delta, the pinned share there, and the
    smallest scale of delta (1, 1/2, ... 1/64) that still has none."""
    bad, pinned = mr.check_interval(got, *mr.interval(ref, mag, n, **kw))
    tight = None
    for s in SCALES:
        if mr.check_interval(got, *mr.interval(ref, mag, n, scale=s,
                                               **kw))[0]:
            break
        tight = s
    return bad, pinned, tight


@pytest.mark.parametrize("bm", [0, 64])
@pytest.mark.parametrize("shape,M", [(SHAPES[0], 160), (WIDE, 32)])
def test_float_intervals(shape, M, bm):
    """Asserted: zero interval violations at the derived delta for a1..a3,
    dz2, dz1, dx0 and dw1..dw3, dz3 equal, out and the scratch sums within
    the bound. The share of entries that the interval pins to one bf16
    value depends on reference and delta alone and falls with delta * 2^8
    / |value|, i.e. with Kp. It is asserted >= 0.8 for the three forward
    layers of the K0p = 256 shape (0.86, 0.82, 0.80). At K0p = 1696 layer
    1 cannot reach it (0.39: delta exceeds half an ulp of most entries)
    and layer 3 sits at 0.797, so there the shares are printed, and every
    layer of both shapes is shown to reject a truncated reference
    instead. The forward of the wide shape has BM = 16 only; its backward
    and the other shape run the given bm. frag = True."""
    ext = _ext()
    H, K0, K0p = shape
    Hp = _hp(H)
    c = mr.float_case(M, H, K0, seed=M + K0)
    fwd, bwd = _weights(c, K0p, True)
    cpu = lambda t: t.detach().to("cpu", f64)  # noqa: E731
    x0 = mr.padded(c.x0, M, K0p).to(DEV)
    bias = [_b(t) for t in (c.b1, c.b2, c.b3)]
    fbm = 0 if shape == WIDE else bm
    out, a1, a2, a3 = ext.mlp3_fwd(
        x0, fwd[0], bias[0], fwd[1], bias[1], fwd[2], bias[2], _b(c.w4),
        _b(c.b4), c.partial.to(f32).to(DEV), **_bm_kw(fbm, True))
    tag = f"{shape} M={M} bm={bm}"

    def report(name, bad, pinned, tight):
        print(f"mlp-interval {tag} {name}: violations {bad}, pinned "
              f"{pinned:.3f}, smallest passing scale {tight}")

    acts = [cpu(a1), cpu(a2), cpu(a3)]
    ins = [c.x0] + acts[:2]
    for i, (w, b, kp) in enumerate(((c.w1, c.b1, K0p), (c.w2, c.b2, Hp),
                                    (c.w3, c.b3, Hp))):
        z, mag = mr.layer_pre(ins[i], w, b)
        bad, pinned, tight = _tightness(acts[i], z, mag, kp + 2, relu=True)
        report(f"a{i + 1}", bad, pinned, tight)
        assert bad == 0
        if shape != WIDE:
            assert pinned >= 0.8
        lo, hi = mr.interval(z, mag, kp + 2, relu=True)
        wrong = mr.trunc_bf16(torch.relu(z).float().to(f64))
        assert mr.check_interval(wrong, lo, hi)[0] > 0     # not vacuous
    z, mag = mr.out_pre(acts[2], c.w4, c.b4, c.partial)
    ratio = mr.err_ratio(out, z, mag, H + 2)
    print(f"mlp-ratio {tag} out: {ratio:.3e}")
    assert ratio <= 1.0

    bs = torch.zeros(4 * H + 1, device=DEV)
    dout = c.dout.to(f32).to(DEV)
    dx0, dz1, dz2, dz3 = ext.mlp3_bwd(dout, a1, a2, a3, _b(c.w4), *bwd, bs,
                                      **_bm_kw(bm, True))
    g3, g2, g1, g0 = cpu(dz3), cpu(dz2), cpu(dz1), cpu(dx0)
    assert torch.equal(g3, mr.dz3_ref(c.dout, acts[2], c.w4))
    for name, got, dz, w, mask in (("dz2", g2, g3, c.w3, acts[1] > 0),
                                   ("dz1", g1, g2, c.w2, acts[0] > 0),
                                   ("dx0", g0[:, :K0], g1, c.w1, None)):
        ref, mag = mr.dgrad_pre(dz, w)
        bad, pinned, tight = _tightness(got, ref, mag, Hp + 2, mask=mask)
        report(name, bad, pinned, tight)
        assert bad == 0
    assert float(g0[:, K0:].abs().sum()) == 0.0
    (dw4, db4), (mw4, mb4) = mr.head_sums(c.dout, acts[2])
    n_at = mr.atomic_terms(M)
    r4 = mr.err_ratio(bs[3 * H:4 * H], dw4, mw4, n_at)
    rb = mr.err_ratio(bs[4 * H], db4, mb4, n_at)
    print(f"mlp-ratio {tag} dw4: {r4:.3e} db4: {rb:.3e}")
    assert r4 <= 1.0 and rb <= 1.0
    assert float(bs[:3 * H].abs().sum()) == 0.0
    bs.zero_()

    base = [t / 64 for t in mr.int_base([(H, K0), (H, H), (H, H)])]
    got = [_b(t) for t in base]
    scratch = torch.zeros(H * K0p + 2 * H * H, device=DEV)
    ext.mlp3_wgrad(dz1, dz2, dz3, x0, a1, a2, scratch, *got, bs)
    for i, (dz, x) in enumerate(((g1, c.x0), (g2, acts[0]),
                                 (g3, acts[1]))):
        ref, mag = mr.wgrad_pre(dz, x, base[i])
        bad, pinned, tight = _tightness(got[i], ref, mag, M + 8 + 2)
        report(f"dw{i + 1}", bad, pinned, tight)
        assert bad == 0
        rs = mr.err_ratio(bs[i * H:(i + 1) * H], dz.sum(0),
                          dz.abs().sum(0), n_at)
        print(f"mlp-ratio {tag} db{i + 1} (rider): {rs:.3e}")
        assert rs <= 1.0
    assert float(scratch.abs().sum()) == 0.0
    assert float(bs[3 * H:].abs().sum()) == 0.0
