"""GPU checks of the fragment-major weight path of the fused MLP:

* mlp3_pack_frag writes, bit for bit and pads included, the image that the
  pure-torch helper (mlp_fraglayout_ref, itself tested on the CPU) builds;
* mlp3_fwd / mlp3_bwd with frag=True equal the same call with frag=False on
  row-major copies of the same weights — torch.equal, tolerance zero: only
  the address of a weight element differs, its (lane, element) slot and
  the k-order do not, so every fp32 sum is the same. The one exception are
  the head sums in bias_scratch: float atomics across blocks, compared with
  the tolerance tests/test_gpu_mlp.py uses for them (atol 5e-3, rtol 3e-2);
* the DeepFM train step packs all six images in its forward, and only the
  three forward ones under no_grad."""

import pytest
import torch

import mlp_fraglayout_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _pads(N, K):
    return (N + 15) // 16 * 16, (K + 31) // 32 * 32


def _src(rows, cols, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(rows, cols, device=DEV, generator=g) + 0.1).to(BF)


def _nan_dst(N, Kp):
    # NaN bit patterns everywhere: a pad the kernel does not write, or
    # multiplies into, shows
    return torch.full((N, Kp), float("nan"), device=DEV, dtype=BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_pack(jobs):
    """jobs: (src, trans, N, Kp) per matrix; ONE mlp3_pack_frag call."""
    dsts = [_nan_dst(N, Kp) for _, _, N, Kp in jobs]
    _ext().mlp3_pack_frag([j[0] for j in jobs], dsts, [j[1] for j in jobs])
    for i, ((src, trans, N, Kp), dst) in enumerate(zip(jobs, dsts)):
        want = ref.image(src, N, Kp, trans=trans)
        assert torch.equal(_bits(dst), _bits(want)), (i, trans, N, Kp)


# ------------------------------------------------------------------ pack

def test_pack_six_in_one_call():
    # the train step's set: w1 [400, 247] (rows not 16-byte aligned), w2,
    # w3, and the dgrad operands w3^T, w2^T, w1^T (image [256, 416])
    w1, w2, w3 = _src(400, 247, 1), _src(400, 400, 2), _src(400, 400, 3)
    _check_pack([(w1, False, 400, 256), (w2, False, 400, 416),
                 (w3, False, 400, 416), (w3, True, 400, 416),
                 (w2, True, 400, 416), (w1, True, 256, 416)])


def test_pack_three_in_one_call():
    # (N, K) = (16, 8), (48, 40) plain and (48, 40) as a transposed source;
    # chunk counts and k-steps differ inside one launch
    _check_pack([(_src(16, 8, 4), False, 16, 32),
                 (_src(48, 40, 5), False, 48, 64),
                 (_src(40, 48, 6), True, 48, 64)])


@pytest.mark.parametrize("N,K", [(16, 8), (48, 40), (400, 247), (256, 400)])
@pytest.mark.parametrize("trans", [False, True])
def test_pack_shapes(N, K, trans):
    Np, Kp = _pads(N, K)
    src = _src(K, N, N + K) if trans else _src(N, K, N + K)
    _check_pack([(src, trans, Np, Kp)])


def test_pack_source_strides_and_alignment():
    # sources as a flat parameter buffer hands them out: a row stride above
    # the width, and a start that is not 16-byte aligned (the aligned
    # 16-byte source read must not be taken there)
    flat = _src(1, 48 * 72 + 8, 7).reshape(-1)
    strided = flat[:48 * 72].view(48, 72)[:, :40]           # ld 72, aligned
    odd = flat[3:3 + 48 * 40].view(48, 40)                  # 6 bytes off
    assert odd.data_ptr() % 16 != 0 and strided.stride(0) == 72
    _check_pack([(strided, False, 48, 64), (odd, False, 48, 64),
                 (strided, True, 48, 64), (odd, True, 48, 64)])


# --------------------------------------------------------------- kernels

_CACHE = {}


def _problem(M, H, K0p):
    """Seeded asymmetric operands, row-major padded weights and their
    fragment-major images. Cached and never modified."""
    key = (M, H, K0p)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator(device=DEV)
    g.manual_seed(7000 * H + 10 * K0p + M)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale
                + 0.1 * scale).to(BF)

    K0 = {64: 50, 256: 247, 1696: 1677}[K0p]
    Hp = (H + 31) // 32 * 32
    sc = 1.0 / (H ** 0.5)
    x0 = torch.zeros(M, K0p, device=DEV, dtype=BF)
    x0[:, :K0] = rn(M, K0, scale=0.5)
    w1 = rn(H, K0, scale=1.0 / (K0 ** 0.5))
    w2, w3 = rn(H, H, scale=sc), rn(H, H, scale=sc)
    row = {"w1": ref.pad(w1, H, K0p), "w2": ref.pad(w2, H, Hp),
           "w3": ref.pad(w3, H, Hp), "w3t": ref.pad(w3.t(), H, Hp),
           "w2t": ref.pad(w2.t(), H, Hp), "w1t": ref.pad(w1.t(), K0p, Hp)}
    frag = {k: ref.pack(v) for k, v in row.items()}
    p = dict(M=M, H=H, x0=x0, row=row, frag=frag,
             b=[rn(H, scale=0.3) for _ in range(3)],
             w4=rn(H, scale=0.5), b4=rn(1, scale=0.3),
             partial=torch.randn(M, device=DEV, generator=g),
             dout=torch.randn(M, device=DEV, generator=g) * 4.0 + 0.5)
    _CACHE[key] = p
    return p


def _fwd(p, bm, frag, partial=False):
    w = p["frag" if frag else "row"]
    return _ext().mlp3_fwd(p["x0"], w["w1"], p["b"][0], w["w2"], p["b"][1],
                           w["w3"], p["b"][2], p["w4"], p["b4"],
                           p["partial"] if partial else None, bm=bm,
                           frag=frag)


def _bwd(p, acts, bm, frag, bias):
    w = p["frag" if frag else "row"]
    bs = torch.zeros(4 * p["H"] + 1, device=DEV) if bias else None
    r = _ext().mlp3_bwd(p["dout"], *acts, p["w4"], w["w3t"], w["w2t"],
                        w["w1t"], bs, bm=bm, frag=frag)
    return r, bs


def _check_equal(M, H, K0p, bm_fwd, bm_bwd):
    p = _problem(M, H, K0p)
    for partial in (False, True):
        want = _fwd(p, bm_fwd, False, partial)
        got = _fwd(p, bm_fwd, True, partial)
        for name, g, w in zip(("out", "a1", "a2", "a3"), got, want):
            assert torch.equal(g, w), (name, partial)
    acts = want[1:]
    for bias in (False, True):
        want_b, ws = _bwd(p, acts, bm_bwd, False, bias)
        got_b, gs = _bwd(p, acts, bm_bwd, True, bias)
        for name, g, w in zip(("dx0", "dz1", "dz2", "dz3"), got_b, want_b):
            assert torch.equal(g, w), (name, bias)
        if bias:
            # float atomics over blocks: order-dependent, layout-independent
            assert torch.allclose(gs, ws, atol=5e-3, rtol=3e-2), (
                (gs - ws).abs().max().item())
            assert float(gs[:3 * H].abs().sum()) == 0.0


@pytest.mark.parametrize("H,K0p", [(400, 256), (64, 64)])
@pytest.mark.parametrize("bm", [16, 32, 64])
@pytest.mark.parametrize("M", [1, 17, 33, 130])
def test_frag_equals_row_major(M, bm, H, K0p):
    # (400, 256): the unrolled KS = 8 / 13 layers; (64, 64): the generic
    # fallback (KS = 2). M: one row, a partial last block, several row tiles
    _check_equal(M, H, K0p, bm, bm)


@pytest.mark.parametrize("bm", [16, 32, 64])
def test_frag_equals_row_major_dim64(bm):
    # K0p = 1696 (dim 64): layer 1 through the generic fallback at KS = 53,
    # the dgrad's last layer with 106 column chunks. The forward stages x0
    # in LDS for BM > 16, so it has BM = 16 only at this width.
    _check_equal(17, 400, 1696, 16, bm)


def test_frag_auto_tile_and_kernel_packed_images():
    # the launcher's own row tile, on images written by mlp3_pack_frag
    p = _problem(130, 400, 256)
    row = p["row"]
    srcs = [row["w1"][:, :247], row["w2"][:, :400], row["w3"][:, :400]]
    srcs = [s.contiguous() for s in srcs]
    keys = ["w1", "w2", "w3", "w3t", "w2t", "w1t"]
    dsts = [_nan_dst(*row[k].shape) for k in keys]
    _ext().mlp3_pack_frag(srcs + srcs[::-1], dsts,
                          [False] * 3 + [True] * 3)
    q = dict(p)
    q["frag"] = dict(zip(keys, dsts))
    want = _fwd(p, 0, False, True)
    got = _fwd(q, 0, True, True)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    want_b, _ = _bwd(p, want[1:], 0, False, False)
    got_b, _ = _bwd(q, want[1:], 0, True, False)
    for g, w in zip(got_b, want_b):
        assert torch.equal(g, w)
        assert bool(torch.isfinite(g.float()).all())


# ----------------------------------------------------------------- model

def test_deepfm_step_packs_in_forward():
    import openembedding_amd.torch as embed
    from openembedding_amd.models import DeepFM, synthetic_batch
    from openembedding_amd.models.ctr import convert_mlp_bf16

    torch.manual_seed(0)
    model = convert_mlp_bf16(DeepFM(dim=9).to(DEV))
    assert model.fused_mlp
    opt = embed.distributed_optimizer(
        torch.optim.Adagrad(model.parameters(), lr=0.01),
        flatten_dense=True)
    lossf = torch.nn.BCEWithLogitsLoss()
    dense, sparse, labels = synthetic_batch(64, device=DEV)
    tkeys = ("w3tp", "w2tp", "w1tp")

    def weights():
        return [model.dnn[i].weight.detach().clone() for i in (0, 2, 4)]

    def images(ws, trans):
        bufs = model._w1pad
        keys = tkeys if trans else ("w1p", "w2p", "w3p")
        ws = ws[::-1] if trans else ws
        return [ref.image(w, *bufs[k].shape, trans=trans)
                for w, k in zip(ws, keys)]

    # grad step: all six images are of the weights the forward ran with
    w_before = weights()
    opt.zero_grad()
    loss = lossf(model(dense, sparse), labels)
    bufs = model._w1pad
    for k, want in zip(tkeys, images(w_before, True)):
        assert torch.equal(_bits(bufs[k]), _bits(want)), k
    for k, want in zip(("w1p", "w2p", "w3p"), images(w_before, False)):
        assert torch.equal(_bits(bufs[k]), _bits(want)), k
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss))
    for k, want in zip(tkeys, images(w_before, True)):
        assert torch.equal(_bits(bufs[k]), _bits(want)), k   # bwd packs none

    # no_grad: the weights have moved; only the forward images follow
    w_after = weights()
    assert not torch.equal(w_after[1], w_before[1])
    t_before = [bufs[k].clone() for k in tkeys]
    with torch.no_grad():
        out = model(dense, sparse)
    assert bool(torch.isfinite(out).all())
    for k, t in zip(tkeys, t_before):
        assert torch.equal(_bits(bufs[k]), _bits(t)), k
    for k, want in zip(("w1p", "w2p", "w3p"), images(w_after, False)):
        assert torch.equal(_bits(bufs[k]), _bits(want)), k
