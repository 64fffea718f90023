"""Reference side of tests/test_gpu_mlp_exact.py and of test_head_exact in
tests/test_gpu_ctrhead.py: plain torch on the CPU, float64 and int64, no
GPU and no extension import.

The references take the operands as the entry points of ops/csrc/mlp.hip
take them (float64 tensors that hold bf16-representable weights, biases
and activations, fp32-representable ``dout`` and ``partial``) and perform
the kernels' roundings, so that only the fp32 accumulation separates a
kernel from its reference:

  - ``fwd_ref``:  a_i = bf16(relu(a_{i-1} . w_i^T + b_i)), and
    out = a3 . w4 + b4 + partial (fp32, not rounded);
  - ``bwd_ref``:  dz3 = bf16(dout * w4 * [a3 > 0]), dz2 = bf16((dz3 . w3)
    * [a2 > 0]), dz1 alike, dx0 = bf16(dz1 . w1); the mask is "bf16 value
    > 0", as mlp_epilogue applies it; head sums dw4 = sum_m dout * a3 and
    db4 = sum dout stay fp32;
  - ``wgrad_ref``: bf16(base + dz^T . x): the += of k_mlp3_wgrad_finish
    happens in fp32 and rounds once;
  - ``bias_finish_ref``: bf16(base + sums), k_mlp3_bias_finish;
  - ``bound``: cin_ref's derived worst case of an fp32 accumulation, and
    ``interval``: the bf16 values a kernel whose fp32 value lies within
    that bound of the exact one can round to;
  - ``int_case`` / ``wgrad_int_case`` / ``bias_int_case``: small-integer
    operands on which every fp32 partial sum is exact in any order, so a
    kernel must EQUAL the reference, roundings to bf16 included;
  - ``head_int_case`` / ``head_ref``: the same for ops/csrc/ctrhead.hip,
    as an int64 composition.

Each ``*_pre`` function returns the value before the epilogue and ``mag``,
the same sum over absolute values, which is what ``bound`` scales. The
references are themselves tested in tests/test_mlp_ref_checkers.py.
"""

from __future__ import annotations

from types import SimpleNamespace

import torch

from cin_ref import bound, ceil_to

bf16 = torch.bfloat16
f64 = torch.float64
LIMIT = float(2 ** 24)       # integers below it are exact in fp32


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even), returned as float64. The value goes
    through fp32 first, like the kernels' ``(bf16)float``. On the integer
    cases every value is exact in fp32 (asserted there), so nothing rounds
    twice; on float64 references the map is still monotone and equals the
    kernel's rounding on every fp32 value, which is all ``interval``
    needs."""
    return t.to(torch.float32).to(bf16).to(f64)


def is_bf16(t: torch.Tensor) -> bool:
    return torch.equal(bf16_rne(t).to(t.dtype), t)


def _low16(t: torch.Tensor) -> torch.Tensor:
    """The 16 bits of an fp32-exact value that a bf16 cannot keep."""
    f = t.to(torch.float32)
    assert torch.equal(f.to(t.dtype), t), "value not exact in fp32"
    return f.contiguous().view(torch.int32) & 0xFFFF


def trunc_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): the
    wrong epilogue that the checks must reject."""
    f = t.to(torch.float32).contiguous()
    assert torch.equal(f.to(t.dtype), t), "value not exact in fp32"
    return (f.view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def tie_share(t: torch.Tensor) -> float:
    """Share of entries exactly halfway between two bf16 values: the ones
    that tell round-to-nearest-even from round-half-away."""
    return float((_low16(t) == 0x8000).double().mean())


def inexact_share(t: torch.Tensor) -> float:
    """Share of entries that no bf16 holds: the ones that tell rounding
    from truncation (half of them round up)."""
    return float((_low16(t) != 0).double().mean())


# ------------------------------------------------------------- references

def layer_pre(a, w, b=None):
    """a . w^T (+ b) of one forward layer, before ReLU and rounding, and
    its mag. a [M, K], w [N, K], b [N]."""
    z, mag = a @ w.t(), a.abs() @ w.abs().t()
    if b is not None:
        z, mag = z + b, mag + b.abs()
    return z, mag


def out_pre(a3, w4, b4, partial=None):
    """out [M] = a3 . w4 + b4 (+ partial) and its mag."""
    z = a3 @ w4 + b4.reshape(())
    mag = a3.abs() @ w4.abs() + b4.abs().reshape(())
    if partial is not None:
        z, mag = z + partial, mag + partial.abs()
    return z, mag


def dgrad_pre(dz, w):
    """dz . w of one dgrad stage, before mask and rounding, and its mag.
    dz [M, N], w [N, K] (the layer's own [out, in] weight)."""
    return dz @ w, dz.abs() @ w.abs()


def fwd_ref(x0, w1, b1, w2, b2, w3, b3, w4, b4, partial=None):
    """(a1, a2, a3, out) and their mags, as k_mlp3_fwd forms them."""
    vals, mags, a = [], [], x0
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        z, mag = layer_pre(a, w, b)
        a = bf16_rne(torch.relu(z))
        vals.append(a)
        mags.append(mag)
    out, mag = out_pre(a, w4, b4, partial)
    return tuple(vals) + (out,), tuple(mags) + (mag,)


def dz3_ref(dout, a3, w4):
    """dz3: ONE fp32 product per element, rounded to bf16. No sum is
    involved, so a kernel equals this on any data."""
    return bf16_rne(dout.unsqueeze(1) * w4.unsqueeze(0) * (a3 > 0))


def head_sums(dout, a3):
    """dw4 [H] = sum_m dout * a3, db4 = sum dout, and their mags."""
    d = dout.unsqueeze(1)
    return ((d * a3).sum(0), dout.sum()), \
           ((d * a3).abs().sum(0), dout.abs().sum())


def bwd_ref(dout, a1, a2, a3, w4, w3, w2, w1):
    """(dz3, dz2, dz1, dx0, dw4, db4) and their mags, as k_mlp3_bwd forms
    them from the saved activations."""
    dz3 = dz3_ref(dout, a3, w4)
    p2, m2 = dgrad_pre(dz3, w3)
    dz2 = bf16_rne(p2 * (a2 > 0))
    p1, m1 = dgrad_pre(dz2, w2)
    dz1 = bf16_rne(p1 * (a1 > 0))
    p0, m0 = dgrad_pre(dz1, w1)
    dx0 = bf16_rne(p0)
    (dw4, db4), (mw4, mb4) = head_sums(dout, a3)
    m3 = (dout.unsqueeze(1) * w4.unsqueeze(0)).abs()
    return (dz3, dz2, dz1, dx0, dw4, db4), (m3, m2, m1, m0, mw4, mb4)


def wgrad_pre(dz, x, base):
    """base + dz^T . x before the finisher's one rounding, and its mag."""
    return base + dz.t() @ x, base.abs() + dz.abs().t() @ x.abs()


def wgrad_ref(dz, x, base):
    return bf16_rne(wgrad_pre(dz, x, base)[0])


def bias_finish_ref(base, sums):
    return bf16_rne(base + sums)


# --------------------------------------------------------------- interval

def interval(ref, mag, n_terms: int, relu=False, mask=None, scale=1.0):
    """(lo, hi): the bf16 values open to a kernel whose fp32 value lies
    within delta = scale * bound(mag, n_terms) of ``ref`` before its
    epilogue f (ReLU and / or mask). f and the rounding are monotone, so
    such a kernel lands in [bf16(f(ref - delta)), bf16(f(ref + delta))].
    Only scale = 1 is derived; smaller scales measure tightness.
    n_terms (cin_ref.bound): Kp + 2 for a layer or a dgrad stage, H + 2
    for out, M + m_split + 2 for a wgrad, M + ceil(M / 16) + 2 for sums
    that cross blocks through atomics."""
    d = scale * bound(mag, n_terms)
    lo, hi = ref - d, ref + d
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    if mask is not None:
        lo, hi = lo * mask, hi * mask
    return bf16_rne(lo), bf16_rne(hi)


def check_interval(got, lo, hi):
    """(number of entries outside [lo, hi], share of entries that the
    interval pins to a single bf16 value)."""
    got = got.detach().to("cpu", f64)
    assert got.shape == lo.shape, (got.shape, lo.shape)
    bad = ~((got >= lo) & (got <= hi))          # a NaN is a violation
    return int(bad.sum()), float((lo == hi).double().mean())


def err_ratio(got, ref, mag, n_terms: int) -> float:
    """max |got - ref| / bound of an fp32 output; passes when <= 1."""
    got = got.detach().to("cpu", f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bound(mag, n_terms)).max())


def atomic_terms(M: int) -> int:
    return M + (M + 15) // 16 + 2


# ------------------------------------------------------------------ cases

def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(f64)


def _solve(c):
    """Attach the oracle's forward and backward chain to a case."""
    ws = (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, c.w4, c.b4)
    (c.a1, c.a2, c.a3, c.out), c.fwd_mag = fwd_ref(c.x0, *ws, c.partial)
    c.out_nopartial = out_pre(c.a3, c.w4, c.b4)[0]
    (c.dz3, c.dz2, c.dz1, c.dx0, c.dw4, c.db4), c.bwd_mag = bwd_ref(
        c.dout, c.a1, c.a2, c.a3, c.w4, c.w3, c.w2, c.w1)
    return c


def int_case(M, H, K0, seed=1):
    """x0, dout in {-3..3}, w1, w4 in {-2..2}, w2, w3 in {-1, 0, 1},
    biases and b4 in {-5..5}, partial in {-9..9}, with the oracle's whole
    chain attached (a1..a3, out, out_nopartial, dz3..dz1, dx0, dw4, db4).

    Every sum of absolute values (the mag of each layer, of out, of each
    dgrad, of dw4 and of the bias sums) is asserted below 2^24, so every
    fp32 partial sum is an exact integer in any order, atomics and the
    MFMA's internal order included, and a kernel differs from the oracle
    only by what it rounds, masks or indexes differently. dw4 grows with
    M: keep M <= 256 where head sums are compared.

    The activations outgrow bf16's 8 bits, which is the point: at H >= 400
    ties and inexact values are asserted to make up at least 1 % each of
    the pre-rounding a2, a3, dz1 and dx0 (M >= 16: fewer rows are too few
    entries for a share), so equality pins round-to-nearest-even against
    truncation and round-half-away."""
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(M=M, H=H, K0=K0)
    c.x0, c.dout = _ri(g, -3, 3, M, K0), _ri(g, -3, 3, M)
    c.w1, c.w4 = _ri(g, -2, 2, H, K0), _ri(g, -2, 2, H)
    c.w2, c.w3 = _ri(g, -1, 1, H, H), _ri(g, -1, 1, H, H)
    c.b1, c.b2, c.b3 = (_ri(g, -5, 5, H) for _ in range(3))
    c.b4, c.partial = _ri(g, -5, 5, 1), _ri(g, -9, 9, M)
    _solve(c)
    bias_mag = [t.abs().sum(0) for t in (c.dz1, c.dz2, c.dz3)]
    for m in list(c.fwd_mag) + list(c.bwd_mag) + bias_mag:
        assert float(m.max()) < LIMIT, float(m.max()) / LIMIT
    c.max_mag = max(float(m.max()) for m in
                    list(c.fwd_mag) + list(c.bwd_mag) + bias_mag)
    if H >= 400 and M >= 16:
        for name, t in pre_rounding(c).items():
            assert tie_share(t) >= 0.01, (name, tie_share(t))
            assert inexact_share(t) >= 0.01, (name, inexact_share(t))
    return c


def pre_rounding(c):
    """The exact values that the oracle rounds into a2, a3, dz1, dx0."""
    return {
        "a2": torch.relu(layer_pre(c.a1, c.w2, c.b2)[0]),
        "a3": torch.relu(layer_pre(c.a2, c.w3, c.b3)[0]),
        "dz1": dgrad_pre(c.dz2, c.w2)[0] * (c.a1 > 0),
        "dx0": dgrad_pre(c.dz1, c.w1)[0],
    }


def take_rows(c, M):
    """The first M rows of a case as a case of its own. Rows do not see
    each other, so the chain is a slice; the head sums are formed anew."""
    assert M <= c.M
    s = SimpleNamespace(**vars(c))
    s.M = M
    for k in ("x0", "dout", "partial", "a1", "a2", "a3", "out",
              "out_nopartial", "dz3", "dz2", "dz1", "dx0"):
        setattr(s, k, getattr(c, k)[:M].contiguous())
    (s.dw4, s.db4), _ = head_sums(s.dout, s.a3)
    return s


def param_grads_ref(c, base=None):
    """The eight parameter grads of a case, each bf16(base + exact sum),
    in the order w1, b1, w2, b2, w3, b3, w4 [1, H], b4. The sums are
    asserted below 2^24, so a kernel or a GEMM that accumulates in fp32
    and rounds once must equal them."""
    sums = [c.dz1.t() @ c.x0, c.dz1.sum(0), c.dz2.t() @ c.a1, c.dz2.sum(0),
            c.dz3.t() @ c.a2, c.dz3.sum(0), c.dw4.unsqueeze(0),
            c.db4.reshape(1)]
    mags = [c.dz1.abs().t() @ c.x0.abs(), c.dz2.abs().t() @ c.a1.abs(),
            c.dz3.abs().t() @ c.a2.abs()]
    base = [torch.zeros_like(s) for s in sums] if base is None else base
    for m, b in zip(mags, base[0::2]):
        assert float((m + b.abs()).max()) < LIMIT
    return [bf16_rne(b + s) for b, s in zip(base, sums)], sums, mags


def int_base(shapes, seed=5):
    """bf16(randint(-600, 600)) tensors: grads that a += has to round."""
    g = torch.Generator().manual_seed(seed)
    return [bf16_rne(_ri(g, -600, 600, *s)) for s in shapes]


def wgrad_int_case(M, H, K0, K0p, seed=2):
    """Operands of mlp3_wgrad: dz1..dz3, a1, a2 [M, H] and x0 [M, K0p] in
    {-3..3}; x0's pad columns K0..K0p are NONZERO on purpose (nothing of
    them may reach dw1). base = bf16(randint(-600, 600)), so the final +=
    rounds. Asserted: 9 M + 600 < 2^24."""
    assert 9 * M + 600 < LIMIT
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(M=M, H=H, K0=K0, K0p=K0p)
    c.dz = [_ri(g, -3, 3, M, H) for _ in range(3)]
    c.x0 = _ri(g, -3, 3, M, K0p)
    if K0p > K0:
        c.x0[:, K0:] = _ri(g, 1, 3, M, K0p - K0)
    c.a1, c.a2 = _ri(g, -3, 3, M, H), _ri(g, -3, 3, M, H)
    c.base = int_base([(H, K0), (H, H), (H, H)], seed + 1)
    c.xs = [c.x0[:, :K0], c.a1, c.a2]
    c.colsum = [d.sum(0) for d in c.dz]
    return c


def wgrad_apply(c, base):
    """One call of mlp3_wgrad on ``base`` = [dw1, dw2, dw3]."""
    return [wgrad_ref(d, x, b) for d, x, b in zip(c.dz, c.xs, base)]


def bias_int_case(M, H, seed=3):
    """Operands of mlp3_bias_bwd: dout [M], dz1..dz3, a3 [M, H] in
    {-3..3}; base (db1, db2, db3, dw4, db4) and a preset for the scratch
    [4H + 1] in bf16(randint(-600, 600)). 9 M + 1200 < 2^24."""
    assert 9 * M + 1200 < LIMIT
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(M=M, H=H)
    c.dout = _ri(g, -3, 3, M)
    c.dz = [_ri(g, -3, 3, M, H) for _ in range(3)]
    c.a3 = _ri(g, -3, 3, M, H)
    c.base = int_base([(H,), (H,), (H,), (H,), (1,)], seed + 1)
    c.preset = int_base([(4 * H + 1,)], seed + 2)[0]
    (dw4, db4), _ = head_sums(c.dout, c.a3)
    c.sums = torch.cat([d.sum(0) for d in c.dz] + [dw4, db4.reshape(1)])
    return c


def float_case(M, H, K0, seed=0):
    """Asymmetric random bf16 operands, scaled as ``_problem`` of
    tests/test_gpu_mlp_tiles.py scales them; dout and partial fp32."""
    g = torch.Generator().manual_seed(seed)

    def rn(*s, scale=1.0):
        return bf16_rne(torch.randn(*s, generator=g) * scale + 0.1 * scale)

    sc = 1.0 / H ** 0.5
    c = SimpleNamespace(M=M, H=H, K0=K0)
    c.x0 = rn(M, K0, scale=0.5)
    c.w1 = rn(H, K0, scale=1.0 / K0 ** 0.5)
    c.w2, c.w3 = rn(H, H, scale=sc), rn(H, H, scale=sc)
    c.b1, c.b2, c.b3 = (rn(H, scale=0.3) for _ in range(3))
    c.w4, c.b4 = rn(H, scale=0.5), rn(1, scale=0.3)
    c.dout = (torch.randn(M, generator=g) * 4.0 + 0.5).to(f64)
    c.partial = torch.randn(M, generator=g).to(f64)
    return c


# ------------------------------------------------------- operand layouts

def padded(t, rows, cols):
    """Zero-padded [rows, cols] bf16 copy of a float64 matrix."""
    p = torch.zeros(rows, cols, dtype=bf16)
    p[:t.shape[0], :t.shape[1]] = t.to(bf16)
    return p


# -------------------------------------------------------------- CTR head

def head_int_case(B, F, dim, nd, seed=4):
    """Operands of ctr_head_fwd / ctr_head_bwd as int64: e_all [B, F,
    dim + 1] and d_deep_in, d_partial in {-3..3}, dense in {0..3}, w in
    {-2..2}, b in {-5..5}. With dim <= 127 and F <= 26 every sum stays
    below 127 * 78^2 < 2^24 (asserted), and (sum e)^2 - sum e^2 = 2 *
    sum_{i<j} e_i e_j is even, so 0.5 * fm is an integer."""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g)

    c = SimpleNamespace(B=B, F=F, dim=dim, nd=nd, width=F * dim + nd)
    c.e_all, c.dense = ri(-3, 3, B, F, dim + 1), ri(0, 3, B, nd)
    c.w, c.b = ri(-2, 2, nd), ri(-5, 5, 1)
    c.d_deep_in = ri(-3, 3, B, ceil_to(c.width, 32))
    c.d_partial = ri(-3, 3, B)
    assert dim * (3 * F) ** 2 + 3 * F + 6 * nd + 5 < LIMIT
    assert 3 * B * 3 < LIMIT and 3 + 3 * (3 * F + 3) < LIMIT
    return c


def head_ref(c, use_fm: bool):
    """int64 composition of the head: deep_in [B, width], partial [B],
    s [B, dim], de_all, d_dense, dw [nd], db [1]."""
    dim, F = c.dim, c.F
    e, lin = c.e_all[..., :dim], c.e_all[..., dim]
    r = SimpleNamespace()
    r.deep_in = torch.cat([e.flatten(1), c.dense], dim=1)
    r.s = e.sum(1)
    r.partial = lin.sum(1) + c.dense @ c.w + c.b
    if use_fm:
        fm = (r.s * r.s - (e * e).sum(1)).sum(1)
        assert bool((fm % 2 == 0).all())
        r.partial = r.partial + fm // 2
    gp = c.d_partial
    g_e = c.d_deep_in[:, :F * dim].reshape(c.B, F, dim)
    if use_fm:
        g_e = g_e + gp.view(-1, 1, 1) * (r.s.unsqueeze(1) - e)
    r.de_all = torch.cat([g_e, gp.view(-1, 1, 1).expand(c.B, F, 1)], dim=2)
    r.d_dense = (c.d_deep_in[:, F * dim:c.width]
                 + gp.unsqueeze(1) * c.w.unsqueeze(0))
    r.dw = (gp.unsqueeze(1) * c.dense).sum(0)
    r.db = gp.sum().reshape(1)
    return r
