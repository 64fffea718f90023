"""GPU tests of the quantized serving tables (all @gpu): k_quantize_rows
writes the CPU oracle's bytes; k_pool_lookup_q and k_gather_lookup_q equal
the CPU QuantizedShard bit for bit on the hard tables of
tests/test_gpu_pooled_readonly.py; malformed offsets are clamped; the table
is only read; the lookup captures into a hipGraph; a block-wise load never
holds an fp32 table; and a model is served from a packed table in HBM."""

import functools

import pytest
import torch

import quantized_ref as qref
import sparse_core_ref as ref
from test_gpu_pooled_readonly import (DEV, TABLES, VOCAB, _keymap, _present)

pytestmark = pytest.mark.gpu

FMTS = ["int8", "fp16"]
# the issue's dims, and 600: more than 128 dwords a row in either format,
# the only size at which a group loops over column passes
DIMS = [1, 3, 4, 5, 9, 16, 17, 64, 65, 128, 130, 600]
ROW_COUNTS = [1, 63, 64, 65, 1025]      # around the group, wave and block
MODES = ["sum", "mean", "sqrtn"]
TAIL = 37
# bag lengths 0, 1, G-1, G, G+1 for the lookup's groups of 16, 32 and 64
# lanes (3, 4, 5: around the ILP of its widest rung), and one bag of several
# chunks for every group
EDGE = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 600, 0]


def _classes():
    from openembedding_amd.core.quantized import QuantizedShard
    from openembedding_amd.core.variable import (HASH_VOCAB_THRESHOLD,
                                                 VariableMeta)
    return QuantizedShard, VariableMeta, HASH_VOCAB_THRESHOLD


def _ops():
    from openembedding_amd.ops import dispatch as ops
    return ops


# ------------------------------------------------------------ quantize_rows

def _source_rows(n: int, dim: int, fmt: str, seed: int) -> torch.Tensor:
    """Random rows of mixed magnitude; among the first ones a constant row,
    a row whose span is subnormal and a row whose span is normal but whose
    scale is not, a row of both zeros, and for fp16 the largest half."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** torch.randint(-3, 3, (n, 1), generator=g).float()
    w = torch.randn(n, dim, generator=g) * mag + torch.randn(n, 1,
                                                             generator=g)
    step = torch.arange(dim, dtype=torch.float32) % 7
    special = [torch.full((dim,), 0.37), step * 1e-41, step * 1e-38,
               torch.where(step % 2 == 0, 0.0, -0.0) * torch.ones(dim),
               step * (65504.0 / 6.0)]
    for i, row in enumerate(special):
        if 1 + i < n:
            w[1 + i] = row
    if fmt == "fp16":
        w = w.clamp(-65504.0, 65504.0)
    return w.float()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_rows_writes_the_oracle_bytes(fmt, dim):
    """The whole slab, pad bytes included, equals the CPU oracle's rows at
    the named slots; slots -1 and R are skipped; rows no slot names and the
    canary rows before and after the slab keep their bytes."""
    from openembedding_amd.ops import require_hip
    ext = require_hip()
    ops = _ops()
    stride = ops.row_stride(fmt, dim)
    for n in ROW_COUNTS:
        w = _source_rows(n, dim, fmt, seed=dim * 7 + n)
        want_rows = ops.quantize_rows(w, fmt)
        assert want_rows.device.type == "cpu"
        R = n + 3
        g = torch.Generator().manual_seed(n)
        slots = torch.randperm(R, generator=g)[:n]
        skipped = []
        if n >= 3:
            slots[0], slots[n // 2] = -1, R
            skipped = [0, n // 2]
        buf = torch.full((R + 2, stride), 0xA5, dtype=torch.uint8, device=DEV)
        slab = buf[1:R + 1]
        ext.quantize_rows(w.to(DEV), slots.to(DEV), slab,
                          ops.QUANT_FORMATS[fmt])
        want = torch.full((R + 2, stride), 0xA5, dtype=torch.uint8)
        keep = torch.ones(n, dtype=torch.bool)
        keep[skipped] = False
        want[1 + slots[keep]] = want_rows[keep]
        got = buf.cpu()
        assert qref.slab_violations(got[1 + slots[keep]], want_rows[keep],
                                    dim, fmt) == [], (n,)
        assert torch.equal(got, want), (n,)
        if fmt == "int8" and n > 3:
            codes, _, scale, _ = qref.int8_fields(want_rows, dim)
            assert float(scale[1]) == 0 and float(scale[2]) == 0 \
                and float(scale[3]) == 0 and not bool(codes[1:4].any())
    # the dispatch form routes a cuda tensor to the kernel
    assert torch.equal(ops.quantize_rows(w.to(DEV), fmt).cpu(), want_rows)


# ------------------------------------------------------------------ lookups

@functools.lru_cache(maxsize=None)
def _rows(dim: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(300 + dim)
    return torch.randn(VOCAB, dim, generator=g)


def _shards(table: str, dim: int, fmt: str):
    """(gpu, cpu) QuantizedShards holding row i under key _keymap[i] for
    the present ids, imported in two calls."""
    QuantizedShard, VariableMeta, hash_vocab = _classes()
    meta = VariableMeta(variable_id=1, embedding_dim=dim,
                        vocabulary_size=(VOCAB if table == "array"
                                         else hash_vocab))
    keys = _keymap(table)[_present()]
    live = _rows(dim)[_present()]
    out = []
    for dev in (DEV, "cpu"):
        sh = QuantizedShard(meta, fmt, device=dev)
        half = keys.numel() // 2
        sh.import_rows(keys[:half], live[:half])
        sh.import_rows(keys[half:], live[half:])
        out.append(sh)
    gpu, cpu = out
    assert gpu.num_rows == cpu.num_rows == keys.numel()
    if table == "hash_colliding":
        cap = gpu._cap          # the chain occupies both table ends
        assert cap == QuantizedShard.MIN_TABLE_CAP
        assert int(gpu.tk[cap - 1]) != -1 and int(gpu.tk[0]) != -1
    return gpu, cpu


@functools.lru_cache(maxsize=None)
def _problem(table: str, B: int):
    """(keys [nnz + TAIL], offsets [B + 1], weights): the edge lengths,
    then short random bags; ids over the whole vocabulary (one in nine
    absent), some -1 inside the bags, keys outside every table, and a tail
    of -1 behind offsets[B]."""
    g = torch.Generator().manual_seed(B)
    lens = ([5] if B == 1 else EDGE[:B]) + torch.randint(
        0, 7, (max(B - len(EDGE), 0),), generator=g).tolist()
    lens = lens[:B]
    offsets = torch.tensor([0] + lens).cumsum(0)
    nnz = int(offsets[-1])
    ids = torch.randint(0, VOCAB, (nnz,), generator=g, dtype=torch.int64)
    keys = _keymap(table)[ids]
    odd = torch.tensor([-1, -5, VOCAB, VOCAB + 1, 1 << 40, -1],
                       dtype=torch.int64)
    pos = torch.randperm(nnz, generator=g)[:min(nnz // 3, 4 * odd.numel())]
    keys[pos] = odd.repeat(4)[:pos.numel()]
    keys = torch.cat([keys, torch.full((TAIL,), -1, dtype=torch.int64)])
    w = torch.randn(keys.numel(), generator=g)
    return keys, offsets, w


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fmt", FMTS)
def test_lookups_equal_the_cpu_shard(fmt, dim):
    """pull_pooled_readonly (three modes, weighted or not, B = 1, 16, 257)
    and pull_readonly on array, hash, full-range and wrapping-chain tables
    are bit-identical to the CPU QuantizedShard holding the same imports,
    and leave every table buffer as it was."""
    for table in TABLES:
        gpu, cpu = _shards(table, dim, fmt)
        if table == "array":    # same rows at the same slots
            assert torch.equal(gpu.slab.cpu(), cpu.slab)
        before = [t.clone() for t in _buffers(gpu)]
        for B in (1, 16, 257):
            keys, offsets, w = _problem(table, B)
            kd, od, wd = keys.to(DEV), offsets.to(DEV), w.to(DEV)
            for mode in MODES:
                for weights, wdev in ((None, None), (w, wd)):
                    want = cpu.pull_pooled_readonly(keys, offsets, mode,
                                                    weights)
                    got = gpu.pull_pooled_readonly(kd, od, mode, wdev)
                    assert got.shape == (B, dim) and got.is_cuda
                    assert torch.equal(got.cpu(), want), (table, B, mode,
                                                          weights is None)
            assert bool((want != 0).any())
        flat = gpu.pull_readonly(kd)
        want_flat = cpu.pull_readonly(keys)
        assert torch.equal(flat.cpu(), want_flat), table
        assert bool((want_flat[-1] == 0).all())
        assert bool((want_flat != 0).any())
        for a, b in zip(_buffers(gpu), before):
            assert torch.equal(a, b), table
        ek, ew, _ = gpu.export_rows()
        assert torch.equal(gpu.pull_readonly(ek), ew)


@pytest.mark.parametrize("fmt", FMTS)
def test_empty_table_reads_zeros(fmt):
    """A shard nothing was imported into has a slab of no rows; both reads
    answer zeros without touching it."""
    QuantizedShard, VariableMeta, _ = _classes()
    sh = QuantizedShard(VariableMeta(variable_id=1, embedding_dim=9), fmt,
                        device=DEV)
    assert sh.slab.shape[0] == 0 and sh.num_rows == 0
    keys = torch.tensor([3, -1, 1 << 40, 3], device=DEV)
    assert torch.equal(sh.pull_readonly(keys), torch.zeros(4, 9, device=DEV))
    out = sh.pull_pooled_readonly(keys, torch.tensor([0, 2, 2, 4],
                                                     device=DEV), "mean")
    assert torch.equal(out, torch.zeros(3, 9, device=DEV))


def _buffers(sh):
    if sh.meta.use_hash_table:
        return [sh.slab, sh.tk, sh.tv, sh.slot_keys, sh.nrows_dev]
    return [sh.slab, sh.valid_u8]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("table", ["array", "hash"])
def test_unsanitised_offsets_are_clamped(table, fmt):
    """offsets below 0 or above nnz are clamped and a decreasing pair is an
    empty bag. Reference: the CPU shard, one bag at a time, on the clamped
    bounds."""
    nnz = 48
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, VOCAB, (nnz,), generator=g, dtype=torch.int64)
    keys = _keymap(table)[ids]
    w = torch.randn(nnz, generator=g)
    offsets = torch.tensor([-3, 4, 12, 8, 16, 80], dtype=torch.int64)
    bounds = [(0, 4), (4, 12), (12, 12), (8, 16), (16, 48)]
    for dim in (9, 64):
        gpu, cpu = _shards(table, dim, fmt)
        for mode in MODES:
            for weights in (None, w):
                want = torch.stack([
                    cpu.pull_pooled_readonly(
                        keys[s:e], torch.tensor([0, e - s]), mode,
                        None if weights is None else weights[s:e])[0]
                    for s, e in bounds])
                got = gpu.pull_pooled_readonly(
                    keys.to(DEV), offsets.to(DEV), mode,
                    None if weights is None else weights.to(DEV))
                assert torch.equal(got.cpu(), want), (dim, mode)
                assert bool((want[2] == 0).all())
                assert bool((want[4] != 0).any())


# ------------------------------------------------------------ graph capture

@pytest.mark.parametrize("table,dim,fmt,weighted",
                         [("hash", 64, "int8", True),
                          ("array", 9, "fp16", False)])
def test_pooled_lookup_is_graph_capturable(table, dim, fmt, weighted):
    """One captured pull_pooled_readonly replayed over two fresh batches
    written into the same buffers equals the eager result on each."""
    gpu, _ = _shards(table, dim, fmt)
    B = 16
    batches = []
    for seed in range(3):
        g = torch.Generator().manual_seed(50 + seed)
        lens = torch.randint(0, 40, (B,), generator=g)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64),
                             lens.cumsum(0)])
        ids = torch.randint(0, VOCAB, (int(offsets[-1]),), generator=g,
                            dtype=torch.int64)
        batches.append((_keymap(table)[ids], offsets,
                        torch.randn(ids.numel(), generator=g)))
    cap = max(k.numel() for k, _, _ in batches) + TAIL
    s_keys = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    s_off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    s_w = torch.zeros(cap, device=DEV) if weighted else None

    def load(i):
        keys, offsets, w = batches[i]
        s_keys.fill_(-1)
        s_keys[:keys.numel()].copy_(keys)
        s_off.copy_(offsets)
        if weighted:
            s_w.zero_()
            s_w[:w.numel()].copy_(w)

    load(0)
    gpu.pull_pooled_readonly(s_keys, s_off, "mean", s_w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            gpu.pull_pooled_readonly(s_keys, s_off, "mean", s_w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu.pull_pooled_readonly(s_keys, s_off, "mean", s_w)
    outs = []
    for i in (1, 2):
        load(i)
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    for i, got in zip((1, 2), outs):
        load(i)
        eager = gpu.pull_pooled_readonly(s_keys, s_off, "mean", s_w)
        assert bool((eager != 0).any())
        assert torch.equal(got, eager)
    assert not torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------- memory

def test_blockwise_load_never_holds_an_fp32_table():
    """N = 20 000 rows of dim 64 loaded in blocks of 2 048 into a reserved
    int8 shard: the allocator's peak stays below slab + key map + four fp32
    blocks (the fp32 table alone, 5.1 MB, is above that), and the shard
    ends at exactly N * stride + key-map bytes."""
    QuantizedShard, VariableMeta, _ = _classes()
    ops = _ops()
    N, dim, blk, fmt = 20_000, 64, 2048, "int8"
    stride = ops.row_stride(fmt, dim)
    g = torch.Generator().manual_seed(1)
    keys = ref.full_range_keys(N, g)
    keys = torch.unique(keys)
    assert keys.numel() == N
    rows = torch.randn(N, dim, generator=g)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    sh = QuantizedShard(VariableMeta(variable_id=1, embedding_dim=dim), fmt,
                        device=DEV)
    sh.reserve_rows(N)
    for s in range(0, N, blk):
        sh.import_rows(keys[s:s + blk], rows[s:s + blk])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    keymap = sh.tk.numel() * 8 + sh.tv.numel() * 4 + N * 8
    block_bytes = blk * dim * 4
    bound = N * stride + keymap + 4 * block_bytes
    print(f"peak rise {rise} B, bound {bound} B, slab {N * stride} B, "
          f"key map {keymap} B, fp32 table {N * dim * 4} B")
    assert N * dim * 4 > bound - N * stride     # the bound has teeth
    assert rise < bound
    assert sh.num_rows == N
    assert sh.slab.shape == (N, stride)
    assert sh.nbytes == N * stride + keymap
    probe = torch.arange(0, N, 97)
    want = ops.dequantize_rows(ops.quantize_rows(rows[probe], fmt), dim, fmt)
    assert torch.equal(sh.pull_readonly(keys[probe]).cpu(), want)


# ------------------------------------------------------------------ serving

def test_serve_quantized_from_gpu(tmp_path):
    """ServedModel.load(quantize="int8") on the GPU answers pull_weights and
    pull_pooled exactly like the same load on the CPU."""
    import openembedding_amd.torch as embed
    from openembedding_amd.core.quantized import QuantizedShard
    from openembedding_amd.serving import ServedModel

    torch.manual_seed(3)
    embed.get_context("cpu")            # train and dump on the CPU
    emb = embed.EmbeddingBag(-1, 24, mode="mean")
    emb.variable.set_initializer("uniform", minval=-0.5, maxval=0.5)
    emb.variable.set_optimizer("adagrad", learning_rate=0.1)
    vals = torch.randint(0, 200, (300,))
    off = torch.arange(0, 301, 5)
    for _ in range(2):
        emb(vals, off).sum().backward()
        embed.get_context().update_all_weights()
    uri = str(tmp_path / "dump")
    embed.save_server_model(uri)

    gpu, cpu = ServedModel("m", uri), ServedModel("m", uri)
    gpu.load(device=DEV, quantize="int8")
    cpu.load(device="cpu", quantize="int8")
    gv, cv = gpu.variables[0], cpu.variables[0]
    assert isinstance(gv.shard, QuantizedShard) and gv.shard.slab.is_cuda
    assert gpu.describe()["variables"][0]["storage"] == "int8"
    q = torch.tensor([[3, 250, 7], [-1, 9, 9]])        # 250 never trained
    got = gv.pull_weights(q)
    assert got.is_cuda and torch.equal(got.cpu(), cv.pull_weights(q))
    assert bool((got[0, 0] != 0).any()) and bool((got[0, 1] == 0).all())
    w = torch.randn(vals.numel())
    for weights in (None, w):
        got = gv.pull_pooled(vals, off, "sqrtn", weights)
        want = cv.pull_pooled(vals, off, "sqrtn", weights)
        assert got.is_cuda and torch.equal(got.cpu(), want)
        assert bool((want != 0).any())
