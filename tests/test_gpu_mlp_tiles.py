"""GPU numerics of the retiled fused-MLP kernels: every row-tile variant
(bm 16/32/64 and the launcher's own choice) of the forward and the dgrad
chain on partial last tiles, row independence bit for bit, LDS zeroing,
the vector-staged wgrad kernel (short chunks, empty and uneven m-splits,
bias rider) and the 2-D repack kernel.

References are stage-wise, as in test_gpu_mlp.py: every layer is recomputed
in fp32 from the KERNEL's own previous bf16 output, so bf16 rounding does
not compound. Tolerances are that file's: 2e-2/2e-2 for activations, dz and
wgrads, atol 3e-2 for the logit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
BMS = [0, 16, 32, 64]          # 0 = the launcher's choice


def _ext():
    from openembedding_amd.ops import require_hip
    return require_hip()


def _bm_kw(bm):
    return {} if bm == 0 else {"bm": bm}


def _close(got, ref, name, atol=2e-2, rtol=2e-2):
    got, ref = got.float(), ref.float()
    assert torch.allclose(got, ref, atol=atol, rtol=rtol), (
        name, (got - ref).abs().max().item())


def _rows(bm):
    b = bm or 16
    return sorted({1, 17, b - 1, b + 1, 2 * b + 3})


_CACHE = {}


def _problem(M, H, K0p):
    """Seeded asymmetric operands; weights carry the zero pads the kernels
    rely on. Cached: several tests share one problem, none modifies it."""
    key = (M, H, K0p)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * H + 10 * K0p + M)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale
                + 0.1 * scale).to(BF)

    K0 = {32: 20, 64: 64, 256: 247}[K0p]
    Hp = (H + 31) // 32 * 32
    sc = 1.0 / (H ** 0.5)
    x0 = torch.zeros(M, K0p, device=DEV, dtype=BF)
    x0[:, :K0] = rn(M, K0, scale=0.5)
    w1 = torch.zeros(H, K0p, device=DEV, dtype=BF)
    w1[:, :K0] = rn(H, K0, scale=1.0 / (K0 ** 0.5))
    w2, w3 = rn(H, H, scale=sc), rn(H, H, scale=sc)
    w2p = torch.zeros(H, Hp, device=DEV, dtype=BF)
    w3p = torch.zeros(H, Hp, device=DEV, dtype=BF)
    w2p[:, :H], w3p[:, :H] = w2, w3
    w3tp = torch.zeros(H, Hp, device=DEV, dtype=BF)
    w2tp = torch.zeros(H, Hp, device=DEV, dtype=BF)
    w1tp = torch.zeros(K0p, Hp, device=DEV, dtype=BF)
    w3tp[:, :H], w2tp[:, :H], w1tp[:, :H] = w3.t(), w2.t(), w1.t()
    p = dict(M=M, H=H, K0p=K0p, Hp=Hp, x0=x0, w1=w1, w2=w2, w3=w3,
             w2p=w2p, w3p=w3p, w3tp=w3tp, w2tp=w2tp, w1tp=w1tp,
             b=[rn(H, scale=0.3) for _ in range(3)],
             w4=rn(H, scale=0.5), b4=rn(1, scale=0.3),
             dout=torch.randn(M, device=DEV, generator=g) * 4.0 + 0.5)
    _CACHE[key] = p
    return p


def _fwd(p, bm):
    return _ext().mlp3_fwd(p["x0"], p["w1"], p["b"][0], p["w2p"], p["b"][1],
                           p["w3p"], p["b"][2], p["w4"], p["b4"], None,
                           **_bm_kw(bm))


def _bwd(p, acts, bm, bias=True):
    H = p["H"]
    bs = torch.zeros(4 * H + 1, device=DEV) if bias else None
    a1, a2, a3 = acts
    r = _ext().mlp3_bwd(p["dout"], a1, a2, a3, p["w4"], p["w3tp"],
                        p["w2tp"], p["w1tp"], bs, **_bm_kw(bm))
    return r, bs


def _check_fwd_bwd(M, H, K0p, bm):
    p = _problem(M, H, K0p)
    out, a1, a2, a3 = _fwd(p, bm)
    f = torch.Tensor.float
    b = p["b"]
    _close(a1, torch.relu(f(p["x0"]) @ f(p["w1"]).t() + f(b[0])), "a1")
    _close(a2, torch.relu(f(a1) @ f(p["w2"]).t() + f(b[1])), "a2")
    _close(a3, torch.relu(f(a2) @ f(p["w3"]).t() + f(b[2])), "a3")
    _close(out, f(a3) @ f(p["w4"]) + f(p["b4"]), "out", atol=3e-2)

    (dx0, dz1, dz2, dz3), bs = _bwd(p, (a1, a2, a3), bm)
    dout = p["dout"]
    _close(dz3, (dout[:, None] * f(p["w4"])[None, :]) * (f(a3) > 0), "dz3")
    _close(dz2, (f(dz3) @ f(p["w3"])) * (f(a2) > 0), "dz2")
    _close(dz1, (f(dz2) @ f(p["w2"])) * (f(a1) > 0), "dz1")
    _close(dx0, f(dz1) @ f(p["w1"]), "dx0")
    _close(bs[3 * H:4 * H], (dout[:, None] * f(a3)).sum(0), "dw4")
    _close(bs[4 * H], dout.sum(), "db4")
    assert float(bs[:3 * H].abs().sum()) == 0.0   # not this kernel's part


@pytest.mark.parametrize("K0p", [32, 256])
@pytest.mark.parametrize("H", [16, 400, 416])
@pytest.mark.parametrize("bm", BMS)
def test_fwd_bwd_partial_tiles(bm, H, K0p):
    for M in _rows(bm):
        _check_fwd_bwd(M, H, K0p, bm)


@pytest.mark.parametrize("bm", BMS)
def test_fwd_bwd_generic_k(bm):
    # K0p = 64 has no unrolled layer: the generic-Kp path, every row tile
    _check_fwd_bwd(2 * (bm or 16) + 3, 400, 64, bm)


def test_fwd_bwd_auto_at_batch_sizes():
    # the launcher's own choice at the sizes its rule distinguishes
    for M in (1024 + 5, 4096 + 3):
        _check_fwd_bwd(M, 400, 256, 0)


@pytest.mark.parametrize("H,K0p", [(400, 256), (16, 32), (416, 64)])
def test_row_independence_bitwise(H, K0p):
    # no atomics and the same k-order in every variant: results must not
    # depend on the row tile, nor on which other rows share the launch
    p = _problem(200, H, K0p)
    ref_f = _fwd(p, 16)
    acts = ref_f[1:]
    ref_b, _ = _bwd(p, acts, 16)
    for bm in (0, 32, 64):
        for g, r in zip(_fwd(p, bm), ref_f):
            assert torch.equal(g, r), bm
        got_b, _ = _bwd(p, acts, bm)
        for g, r in zip(got_b, ref_b):
            assert torch.equal(g, r), bm
    # first 100 rows alone == first 100 rows of the 200-row run
    q = dict(p)
    q["x0"] = p["x0"][:100].contiguous()
    q["dout"] = p["dout"][:100].contiguous()
    for bm in BMS:
        for g, r in zip(_fwd(q, bm), ref_f):
            assert torch.equal(g, r[:100]), bm
        got_b, _ = _bwd(q, tuple(a[:100].contiguous() for a in acts), bm)
        for g, r in zip(got_b, ref_b):
            assert torch.equal(g, r[:100]), bm


@pytest.mark.parametrize("bm", BMS)
def test_nonfinite_poison_stays_out(bm):
    # LDS zeroing: pad columns meet zero weight pads, and 0 * inf = NaN.
    # Dirty freed memory with NaN/inf bit patterns first, then a partial
    # tile must still come out finite everywhere.
    junk = torch.empty(8 << 20, device=DEV, dtype=torch.int32)
    junk[0::3] = 0x7FC07FC0          # bf16 NaN pairs
    junk[1::3] = 0x7F807F80          # +inf
    junk[2::3] = -8323200            # 0xFF80FF80: -inf
    del junk
    p = _problem(17, 400, 256)
    out, a1, a2, a3 = _fwd(p, bm)
    (dx0, dz1, dz2, dz3), bs = _bwd(p, (a1, a2, a3), bm)
    for t in (out, a1, a2, a3, dx0, dz1, dz2, dz3, bs):
        assert bool(torch.isfinite(t.float()).all())


# ---------------------------------------------------------------- wgrad

@pytest.mark.parametrize("m_split", [0, 2, 8])
@pytest.mark.parametrize("rider", [False, True])
@pytest.mark.parametrize("H,K0,K0p", [(400, 247, 256), (16, 20, 32),
                                      (416, 256, 256)])
@pytest.mark.parametrize("M", [32, 160, 1056])
def test_wgrad_vector_staged(M, H, K0, K0p, rider, m_split):
    # M=32: one chunk shorter than 128; M=160 with 8 splits: three splits
    # empty (block-uniform early return); M=1056: uneven splits
    ext = _ext()
    g = torch.Generator(device=DEV)
    g.manual_seed(M + H)

    def rn(*s):
        return (torch.randn(*s, device=DEV, generator=g) + 0.1).to(BF)

    dz = [rn(M, H) for _ in range(3)]
    # x0's pad columns K0..K0p deliberately NON-zero: nothing of them may
    # reach dw1, whose rows are K0 wide
    x0, a1, a2 = rn(M, K0p), rn(M, H), rn(M, H)
    base = [rn(H, K0), rn(H, H), rn(H, H)]
    guard = torch.full((H * K0 + 64,), 7.0, device=DEV, dtype=BF)
    dw1 = guard[:H * K0].view(H, K0)
    dw1.copy_(base[0])
    got = [dw1, base[1].clone(), base[2].clone()]
    scratch = torch.zeros(H * K0p + 2 * H * H, device=DEV)
    bs = torch.zeros(4 * H + 1, device=DEV) if rider else None
    kw = {} if m_split == 0 else {"m_split": m_split}
    f = torch.Tensor.float
    prods = [f(dz[0]).t() @ f(x0[:, :K0]), f(dz[1]).t() @ f(a1),
             f(dz[2]).t() @ f(a2)]

    ext.mlp3_wgrad(*dz, x0, a1, a2, scratch, *got, bs, **kw)
    for i in range(3):
        _close(got[i], f(base[i]) + prods[i], f"dw{i + 1}")
    assert float(scratch.abs().sum()) == 0.0       # self-cleaned
    assert bool((guard[H * K0:] == 7.0).all())
    if rider:
        for i in range(3):
            _close(bs[i * H:(i + 1) * H], f(dz[i]).sum(0), f"db{i + 1}")
        assert float(bs[3 * H:].abs().sum()) == 0.0
        bs.zero_()
    # a second call accumulates again (beta = 1)
    first = [t.clone() for t in got]
    ext.mlp3_wgrad(*dz, x0, a1, a2, scratch, *got, bs, **kw)
    for i in range(3):
        _close(got[i], f(first[i]) + prods[i], f"dw{i + 1} second")
    assert float(scratch.abs().sum()) == 0.0
    if rider:
        _close(bs[H:2 * H], f(dz[1]).sum(0), "db2 second")


# ----------------------------------------------------------------- pack

@pytest.mark.parametrize("H,K0,K0p", [(400, 247, 256), (16, 20, 32)])
def test_pack_2d(H, K0, K0p):
    ext = _ext()
    torch.manual_seed(7)
    Hp = (H + 31) // 32 * 32
    w1 = (torch.randn(H, K0, device=DEV) + 0.1).to(BF)
    w2 = (torch.randn(H, H, device=DEV) + 0.1).to(BF)
    w3 = (torch.randn(H, H, device=DEV) + 0.1).to(BF)
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=BF)  # noqa: E731
    w1p, w2p, w3p = z(H, K0p), z(H, Hp), z(H, Hp)
    ext.mlp3_pack(w1, w1p, False, w2, w2p, False, w3, w3p, False)
    assert torch.equal(w1p[:, :K0], w1)
    assert float(w1p[:, K0:].abs().sum()) == 0
    assert torch.equal(w2p[:, :H], w2) and torch.equal(w3p[:, :H], w3)
    assert float(w2p[:, H:].abs().sum()) == 0
    assert float(w3p[:, H:].abs().sum()) == 0

    w3tp, w2tp, w1tp = z(H, Hp), z(H, Hp), z(K0p, Hp)
    ext.mlp3_pack(w3, w3tp, True, w2, w2tp, True, w1p, w1tp, True)
    assert torch.equal(w3tp[:, :H], w3.t())
    assert torch.equal(w2tp[:, :H], w2.t())
    assert torch.equal(w1tp[:, :H], w1p.t())   # incl. zero K0..K0p rows
    for t in (w3tp, w2tp, w1tp):
        assert float(t[:, H:].abs().sum()) == 0
