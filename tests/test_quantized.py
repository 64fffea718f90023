"""Quantized serving tables on the CPU: the row formats of
ops.dispatch.quantize_rows / dequantize_rows (the oracle of the HIP
kernels), their error bound, the import-time rejections, QuantizedShard's
torch form, and the slab checker the GPU tests rely on."""

import pytest
import torch

import quantized_ref as qref
from openembedding_amd.core.quantized import QuantizedShard
from openembedding_amd.core.variable import VariableMeta, VariableShard
from openembedding_amd.ops import dispatch as ops

FMTS = ["int8", "fp16"]
MODES = ["sum", "mean", "sqrtn"]


# ------------------------------------------------------------------ formats

def test_row_stride():
    assert [ops.row_stride("int8", d) for d in (1, 4, 5, 9, 64, 100)] \
        == [12, 12, 16, 20, 72, 108]
    assert [ops.row_stride("fp16", d) for d in (1, 2, 3, 9, 64, 100)] \
        == [4, 4, 8, 20, 128, 200]
    for fmt in FMTS:
        assert all(ops.row_stride(fmt, d) % 4 == 0 for d in range(1, 70))
    with pytest.raises(ValueError):
        ops.row_stride("int4", 8)


@pytest.mark.parametrize("fmt", FMTS)
def test_constant_rows_and_dim_1_are_exact(fmt):
    vals = torch.tensor([0.0, 1.0, -3.25, 1e-30, 0.37, -1234.5, 1e-42])
    if fmt == "fp16":
        vals = vals.to(torch.float16).float()
    for dim in (1, 5, 64):
        w = vals.unsqueeze(1).expand(-1, dim).contiguous()
        p = ops.quantize_rows(w, fmt)
        assert p.shape == (vals.numel(), ops.row_stride(fmt, dim))
        assert torch.equal(ops.dequantize_rows(p, dim, fmt), w)
        if fmt == "int8":
            codes, pad, scale, lo = qref.int8_fields(p, dim)
            assert not bool(codes.any()) and not bool(scale.any())
            assert torch.equal(lo, vals)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(100, 1, generator=g)
    if fmt == "fp16":
        w = w.to(torch.float16).float()
    assert torch.equal(ops.dequantize_rows(ops.quantize_rows(w, fmt), 1, fmt),
                       w)


def test_subnormal_scale_is_zero_and_negative_zero_lo_is_positive():
    w = torch.tensor([[0.0, 1e-41, 3e-41], [0.0, 1e-38, 2e-36],
                      [-0.0, 0.0, 1.0]])
    p = ops.quantize_rows(w, "int8")
    codes, _, scale, lo = qref.int8_fields(p, 3)
    assert float(scale[0]) == 0 and float(scale[1]) == 0
    assert not bool(codes[:2].any())
    assert float(scale[2]) > 0 and codes[2].tolist() == [0, 0, 255]
    assert lo.view(torch.int32).tolist() == [0, 0, 0]      # +0.0 bits


@pytest.mark.parametrize("mag,off", qref.INPUTS)
@pytest.mark.parametrize("dim", qref.BOUND_DIMS)
def test_int8_error_within_derived_bound(dim, mag, off):
    """err <= scale/2 + 510 u scale + u (3 (hi - lo) + 2 max|row|), u =
    2^-24 (quantized_ref.int8_bound derives it). The worst err / bound of
    these inputs on the CPU is 0.99985."""
    w = qref.bound_rows(dim, mag, off, seed=dim)
    p = ops.quantize_rows(w, "int8")
    back = ops.dequantize_rows(p, dim, "int8")
    err = (back.double() - w.double()).abs().amax(1)
    ratio = err / qref.int8_bound(w, p)
    print(f"dim {dim} mag {mag} off {off}: worst err/bound "
          f"{float(ratio.max()):.5f}")
    assert float(ratio.max()) <= 1.0
    codes, pad, scale, _ = qref.int8_fields(p, dim)
    both = (codes == 0).any(1) & (codes == 255).any(1)
    assert float(both.float().mean()) >= 0.5        # vacuity guard
    assert not bool(pad.any())


@pytest.mark.parametrize("mag,off", [(1.0, 0.0), (1e-3, 5.0), (100.0, -1e4),
                                     (1e-6, 0.0)])
@pytest.mark.parametrize("dim", qref.BOUND_DIMS)
def test_fp16_is_torch_half(dim, mag, off):
    w = qref.bound_rows(dim, mag, off, seed=dim)
    p = ops.quantize_rows(w, "fp16")
    assert torch.equal(ops.dequantize_rows(p, dim, "fp16"),
                       w.to(torch.float16).float())
    assert not bool(p[:, 2 * dim:].any())


# --------------------------------------------------------------- rejections

def _meta(dim, table="hash", vocab=64):
    return VariableMeta(variable_id=1, embedding_dim=dim) if table == "hash" \
        else VariableMeta(variable_id=1, embedding_dim=dim,
                          vocabulary_size=vocab)


BAD_ROWS = {
    "nan": ([1.0, float("nan"), 2.0], FMTS),
    "inf": ([1.0, float("inf"), 2.0], FMTS),
    "neg_inf": ([float("-inf"), 0.0, 2.0], FMTS),
    "span": ([3e38, -3e38, 0.0], ["int8"]),
    "half_range": ([1.0, 65520.0, 0.0], ["fp16"]),
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", sorted(BAD_ROWS))
@pytest.mark.parametrize("table", ["hash", "array"])
def test_bad_block_is_rejected_whole(table, case, fmt):
    row, fmts = BAD_ROWS[case]
    sh = QuantizedShard(_meta(3, table), fmt)
    sh.import_rows(torch.tensor([4, 9]), torch.ones(2, 3))
    n0, slab0 = sh.num_rows, sh.slab.clone()
    w = torch.tensor([[0.5, 0.25, 0.0], row])
    if fmt in fmts:
        with pytest.raises(ValueError):
            sh.import_rows(torch.tensor([11, 12]), w)
        with pytest.raises(ValueError):
            ops.quantize_rows(w, fmt)
        assert sh.num_rows == n0 and torch.equal(sh.slab, slab0)
        assert not bool(sh.pull_readonly(torch.tensor([11])).any())
    elif case == "span":        # fits a half? no: 3e38 is beyond it
        with pytest.raises(ValueError):
            sh.import_rows(torch.tensor([11, 12]), w)
    else:                       # 65520 is fine for int8
        sh.import_rows(torch.tensor([11, 12]), w)
        assert sh.num_rows == n0 + 2


def test_reserved_and_out_of_range_keys_are_rejected():
    sh = QuantizedShard(_meta(3), "int8")
    with pytest.raises(ValueError):
        sh.import_rows(torch.tensor([3, -1]), torch.ones(2, 3))
    assert sh.num_rows == 0
    arr = QuantizedShard(_meta(3, "array", vocab=10), "int8")
    for bad in (-2, 10):
        with pytest.raises(ValueError):
            arr.import_rows(torch.tensor([3, bad]), torch.ones(2, 3))
    assert arr.num_rows == 0 and not bool(arr.slab.any())


def test_float64_variable_and_unknown_format_are_refused():
    meta = VariableMeta(variable_id=1, embedding_dim=4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float64"):
        QuantizedShard(meta, "int8")
    with pytest.raises(ValueError):
        QuantizedShard(_meta(4), "int4")


# ----------------------------------------------------------- QuantizedShard

def _filled(table, fmt, dim=9, vocab=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    keys = torch.randperm(vocab, generator=g)[:40]
    if table == "hash":
        keys = keys * 1_000_003 - 17_000_000     # negative keys too
    rows = torch.randn(40, dim, generator=g)
    sh = QuantizedShard(_meta(dim, table, vocab), fmt)
    sh.import_rows(keys[:25], rows[:25])
    sh.import_rows(keys[25:], rows[25:])
    return sh, keys, rows


def _oracle(rows, fmt):
    return ops.dequantize_rows(ops.quantize_rows(rows, fmt), rows.shape[1],
                               fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("table", ["hash", "array"])
def test_pull_readonly_and_misses(table, fmt):
    sh, keys, rows = _filled(table, fmt)
    assert sh.num_rows == 40 and sh.dim == 9 and sh.dtype == torch.float32
    assert sh.device.type == "cpu"
    got = sh.pull_readonly(keys)
    assert torch.equal(got, _oracle(rows, fmt))
    absent = torch.tensor([-1, 1 << 50, -9, 64, 65])
    if table == "array":
        free = sorted(set(range(64)) - set(keys.tolist()))[:3]
        absent = torch.cat([absent, torch.tensor(free)])
    assert not bool(sh.pull_readonly(absent).any())
    assert sh.num_rows == 40
    assert torch.equal(sh.get_weights(keys[:3]), got[:3])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("table", ["hash", "array"])
def test_duplicate_key_last_wins_and_overwrite(table, fmt):
    sh = QuantizedShard(_meta(4, table), fmt)
    rows = torch.arange(20.0).view(5, 4)
    sh.import_rows(torch.tensor([7, 3, 7, 5, 3]), rows)
    assert sh.num_rows == 3
    got = sh.pull_readonly(torch.tensor([7, 3, 5]))
    assert torch.equal(got, _oracle(rows[[2, 4, 3]], fmt))
    new = torch.full((1, 4), -2.5)
    sh.import_rows(torch.tensor([3]), new)
    assert sh.num_rows == 3
    assert torch.equal(sh.pull_readonly(torch.tensor([3, 7])),
                       _oracle(torch.cat([new, rows[2:3]]), fmt))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("table", ["hash", "array"])
def test_pooled_equals_pool_over_dequantized_rows(table, fmt, mode, weighted):
    sh, keys, rows = _filled(table, fmt)
    g = torch.Generator().manual_seed(5)
    pick = torch.randint(0, 40, (30,), generator=g)
    values = keys[pick].clone()
    values[4], values[11] = -1, 1 << 45          # misses inside bags
    values = torch.cat([values, torch.full((6,), -1, dtype=torch.int64)])
    offsets = torch.tensor([0, 3, 3, 10, 11, 30])        # an empty bag
    w = torch.randn(values.numel(), generator=g) if weighted else None
    elems = _oracle(rows, fmt)[pick]
    elems[4] = 0
    elems[11] = 0
    elems = torch.cat([elems, torch.zeros(6, 9)])
    if weighted:
        want = ops.pool_fwd_weighted(elems, None, None, offsets, w, mode)[0]
    else:
        want = ops.pool_fwd(elems, None, None, offsets, mode, False)[0]
    got = sh.pull_pooled_readonly(values, offsets, mode, w)
    assert got.shape == (5, 9) and torch.equal(got, want)
    assert not bool(got[1].any()) and bool(got[4].any())
    with pytest.raises(ValueError):
        sh.pull_pooled_readonly(values, offsets, "max")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("table", ["hash", "array"])
def test_export_matches_pull_and_from_shard_matches_import(table, fmt):
    sh, keys, rows = _filled(table, fmt)
    ek, ew, es = sh.export_rows()
    assert es is None and ek.numel() == 40
    assert sorted(ek.tolist()) == sorted(keys.tolist())
    assert torch.equal(sh.pull_readonly(ek), ew)

    src = VariableShard(_meta(9, table))
    src.import_rows(keys, rows)
    old = QuantizedShard.IMPORT_BLOCK
    QuantizedShard.IMPORT_BLOCK = 16            # several blocks
    try:
        conv = QuantizedShard.from_shard(src, fmt)
    finally:
        QuantizedShard.IMPORT_BLOCK = old
    assert conv.fmt == fmt and conv.num_rows == 40
    assert torch.equal(conv.pull_readonly(keys), sh.pull_readonly(keys))
    if table == "hash":
        assert conv.slab.shape[0] == 40         # reserved exactly


def test_reserve_rows_is_exact_and_nbytes_counts_slab_and_key_map():
    sh = QuantizedShard(_meta(64), "int8")
    sh.reserve_rows(100)
    assert sh.slab.shape == (100, 72)
    g = torch.Generator().manual_seed(1)
    for s in range(0, 100, 30):
        n = min(30, 100 - s)
        sh.import_rows(torch.arange(s, s + n), torch.randn(n, 64,
                                                           generator=g))
        assert sh.slab.shape == (100, 72)
    assert sh.num_rows == 100 and sh.nbytes == 100 * 72 + 100 * 8
    sh.import_rows(torch.arange(40, 50), torch.ones(10, 64))    # overwrites
    assert sh.slab.shape == (100, 72) and sh.num_rows == 100
    sh.import_rows(torch.arange(95, 105), torch.ones(10, 64))   # 5 new keys
    assert sh.slab.shape == (105, 72) and sh.num_rows == 105
    arr = QuantizedShard(_meta(9, "array", vocab=50), "fp16")
    assert arr.nbytes == 50 * 20 + 50


def test_write_methods_raise():
    sh, keys, _ = _filled("hash", "int8")
    for call in (lambda: sh.pull(keys), lambda: sh.update_weights(),
                 lambda: sh.push(keys, torch.zeros(40, 9),
                                 torch.ones(40, dtype=torch.int64)),
                 lambda: sh.set_optimizer("sgd", learning_rate=0.1)):
        with pytest.raises(RuntimeError, match="read-only"):
            call()


# ------------------------------------------------------------- slab checker

@pytest.mark.parametrize("dim", [5, 9, 64])
def test_slab_checker_accepts_equal_and_rejects_mutants(dim):
    g = torch.Generator().manual_seed(2)
    w = torch.randn(8, dim, generator=g)
    cw = ops.row_stride("int8", dim) - 8
    want = ops.quantize_rows(w, "int8")
    assert qref.slab_violations(want.clone(), want, dim, "int8") == []

    off_by_one = want.clone()
    c = int(off_by_one[3, 2])
    off_by_one[3, 2] = c + 1 if c < 255 else c - 1
    assert any("codes" in m for m in
               qref.slab_violations(off_by_one, want, dim, "int8"))

    swapped = want.clone()
    swapped[:, cw:cw + 4] = want[:, cw + 4:]
    swapped[:, cw + 4:] = want[:, cw:cw + 4]
    bad = qref.slab_violations(swapped, want, dim, "int8")
    assert "scale bits differ" in bad and "lo bits differ" in bad

    if dim % 4:
        pad = want.clone()
        pad[5, dim] = 1
        assert "non-zero pad byte" in qref.slab_violations(pad, want, dim,
                                                           "int8")
    assert qref.slab_violations(want[:, :-4], want, dim, "int8")

    half = ops.quantize_rows(w, "fp16")
    assert qref.slab_violations(half.clone(), half, dim, "fp16") == []
    flipped = half.clone()
    flipped[0, 0] ^= 1
    assert qref.slab_violations(flipped, half, dim, "fp16") \
        == ["half bits differ"]
    if dim % 2:
        pad = half.clone()
        pad[2, 2 * dim] = 7
        assert "non-zero pad byte" in qref.slab_violations(pad, half, dim,
                                                           "fp16")
