"""Backend dispatch for the engine's hot ops.

Each op has a pure-torch implementation (CPU oracle; exact reference
semantics) and routes to the HIP extension on ROCm devices. The HIP kernels
are tested against the torch versions in tests/test_gpu_numerics.py.
"""

from __future__ import annotations

from typing import Tuple

import torch

from . import require_hip


def _use_hip(t: torch.Tensor) -> bool:
    return t.is_cuda


# --------------------------------------------------------------------- unique

def unique_inverse(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batch-local dedup: keys int64 [n] -> (unique [u], inverse [n]).

    GPU: hash-based (no sort) CDNA4 kernel — the reference's client-side
    dedup (EmbeddingPullOperator.cpp:67-79) moved on-device. Unique order is
    unspecified (GPU: first-probe order; CPU: sorted)."""
    if keys.numel() == 0:
        return keys.clone(), torch.empty(0, dtype=torch.int64, device=keys.device)
    if _use_hip(keys):
        ext = require_hip()
        if ext is not None:
            return ext.unique_inverse(keys)
    return torch.unique(keys, return_inverse=True)


# ------------------------------------------------------------- reduce-by-key

def reduce_by_inverse(inverse: torch.Tensor, grads: torch.Tensor, u: int
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sum gradients per unique id + occurrence counts (the reference's
    client pre-aggregation, EmbeddingPushOperator.cpp:39-58).

    inverse int64 [n], grads [n, dim] -> (ugrads [u, dim], counts int64 [u]).
    """
    if _use_hip(grads) and grads.dtype == torch.float32:
        ext = require_hip()   # f64 variables use the torch path below
        if ext is not None:
            return ext.reduce_by_inverse(inverse, grads, u)
    ugrads = torch.zeros((u, grads.shape[1]), dtype=grads.dtype,
                         device=grads.device)
    ugrads.index_add_(0, inverse, grads)
    counts = torch.bincount(inverse, minlength=u).to(torch.int64)
    return ugrads, counts


def seg_reduce_covers(grads: torch.Tensor) -> bool:
    """True when ``reduce_by_index`` has a kernel for ``grads``: float32 on
    the GPU with a dim on the kernel's ladder. Everything else (float64
    variables, wider rows, CPU tensors) keeps ``reduce_by_inverse``."""
    if not (_use_hip(grads) and grads.dtype == torch.float32):
        return False
    ext = require_hip()
    return ext is not None and grads.shape[1] <= ext.seg_reduce_max_dim()


def reduce_by_index(index, grads: torch.Tensor, u_dev
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``reduce_by_inverse(inverse, grads, n)`` summed through the batch's
    inverted index instead of atomics.

    index = (seg_off, seg_cnt, perm, long_list, n_long) as
    ``unique_bounded_indexed`` returns it: uid's elements are
    ``perm[seg_off[uid] : seg_off[uid] + seg_cnt[uid]]``; ``u_dev`` is the
    live unique count (int32 [1] tensor, or an int on the torch path).
    grads [n, dim] -> (ugrads [n, dim], counts int64 [n]); rows at and
    beyond ``u_dev`` are zero with count 0. Rows are added in list order
    (arrival order on the GPU: not bitwise reproducible from run to run,
    like the atomic reduce it replaces)."""
    seg_off, seg_cnt, perm, long_list, n_long = index
    if seg_reduce_covers(grads):
        return require_hip().reduce_by_index(seg_off, seg_cnt, perm,
                                             long_list, n_long, grads, u_dev)
    n = grads.shape[0]
    u = int(u_dev)
    dev = grads.device
    cnt = seg_cnt[:u].to(dev, torch.int64)
    start = seg_off[:u].to(dev, torch.int64)
    uid = torch.repeat_interleave(torch.arange(u, device=dev), cnt)
    first = torch.cumsum(cnt, 0) - cnt      # of each list in the flat walk
    pos = (torch.arange(uid.numel(), device=dev)
           + torch.repeat_interleave(start - first, cnt))
    elems = perm.to(dev, torch.int64).index_select(0, pos)
    ugrads = torch.zeros((n, grads.shape[1]), dtype=grads.dtype, device=dev)
    ugrads.index_add_(0, uid, grads.index_select(0, elems))
    counts = torch.zeros(n, dtype=torch.int64, device=dev)
    counts[:u] = cnt
    return ugrads, counts


def reduce_apply_by_index(opt_id: int, weights: torch.Tensor,
                          state: torch.Tensor, slots: torch.Tensor, index,
                          grads: torch.Tensor, cfg, u_dev) -> None:
    """``reduce_by_index`` and the sparse optimizer step on its result: the
    rows of ``weights`` / ``state`` behind ``slots`` (int64 [n], -1 = skip)
    are updated in place from the per-unique sums of ``grads`` [n, dim].

    One launch where ``seg_reduce_covers(grads)``: the sums are applied where
    they are formed and never written out. Everything else on the GPU (a dim
    above the ladder) takes the two launches, ``reduce_by_index`` then
    ``apply_optimizer``. ``opt_id`` / ``cfg`` as ``apply_optimizer`` takes
    them (core/variable_gpu.py)."""
    ext = require_hip() if _use_hip(grads) else None
    if ext is None or weights.dtype != torch.float32:
        raise NotImplementedError(
            "reduce_apply_by_index serves float32 GPU tables; other "
            "variables reduce at push time and commit through their shard")
    grads = grads.contiguous()
    if seg_reduce_covers(grads):
        ext.reduce_apply_by_index(opt_id, weights, state, slots, *index,
                                  grads, list(cfg), u_dev)
        return
    ugrads, counts = reduce_by_index(index, grads, u_dev)
    ext.apply_optimizer(opt_id, weights, state, slots, ugrads, counts,
                        list(cfg), u_dev)


# ---------------------------------------------------------- feature admission
# The count-min filter in front of a hashed row's creation. ``sketch`` is one
# flat int32 tensor of ``depth`` rows of ``width`` counters, width a power of
# two. The torch forms are the CPU path and the oracle of k_admit_note /
# k_admit_resolve / k_admit_age (ops/csrc/embops.hip).

def admit_cells(keys: torch.Tensor, width: int, depth: int, seed: int
                ) -> torch.Tensor:
    """The sketch cells of ``keys`` (int64 [n]) -> int64 [depth, n]: row j
    holds ``j*width + (splitmix64(splitmix64(k) ^ (seed + j)) & (width-1))``
    in wrap-around int64 arithmetic."""
    from ..core.rng import splitmix64
    hk = splitmix64(keys.to(torch.int64))
    rows = []
    for j in range(depth):
        sj = ((int(seed) + j + (1 << 63)) % (1 << 64)) - (1 << 63)
        rows.append(j * width + (splitmix64(hk ^ sj) & (width - 1)))
    return torch.stack(rows) if rows else hk.new_empty((0, keys.numel()))


def admit_note(sketch: torch.Tensor, keys: torch.Tensor, depth: int,
               seed: int) -> torch.Tensor:
    """One sighting of each of ``keys`` (unique int64 [n], all missing from
    the table): add 1 to every key's cells, then return the estimates
    (int32 [n]), each the minimum of the key's cells AFTER all adds."""
    cells = admit_cells(keys, sketch.numel() // depth, depth, seed)
    sketch.index_add_(0, cells.reshape(-1),
                      torch.ones(cells.numel(), dtype=sketch.dtype,
                                 device=sketch.device))
    return sketch[cells].min(dim=0).values


def admit_age(sketch: torch.Tensor, shift: int) -> None:
    """Every counter ``>> shift`` in place; ``shift >= 31`` zeroes."""
    shift = int(shift)
    if shift < 0:
        raise ValueError("shift must not be negative")
    if _use_hip(sketch):
        ext = require_hip()
        if ext is not None:
            ext.admit_age(sketch, shift)
            return
    if shift >= 31:
        sketch.zero_()
    else:
        sketch.copy_(sketch >> shift)


# ------------------------------------------------------------ multi-hot bags

POOL_MODES = {"sum": 0, "mean": 1, "sqrtn": 2}


def _sqrt(t: torch.Tensor) -> torch.Tensor:
    """Correctly rounded square root, like the kernels' ``sqrtf``. torch's
    float32 sqrt on the CPU is off by an ulp for about 0.7 % of inputs
    (the bag length 267 is the first integer), which would make this
    oracle differ from the kernels it defines; the float64 root of a
    float32 rounds to the correct float32."""
    if t.dtype == torch.float32:
        return t.double().sqrt().to(torch.float32)
    return t.sqrt()


def _bag_scale(offsets: torch.Tensor, nnz: int, mode: str,
               dtype: torch.dtype) -> torch.Tensor:
    """Combiner scale per bag: 1 (sum), 1/len (mean), 1/sqrt(len) (sqrtn);
    0 for an empty bag. ``offsets`` is clamped to [0, nnz] like the
    kernels do."""
    off = offsets.clamp(0, nnz)
    length = (off[1:] - off[:-1]).clamp(min=0).to(dtype)
    if mode == "sum":
        scale = torch.ones_like(length)
    elif mode == "mean":
        scale = 1.0 / length
    else:
        scale = 1.0 / _sqrt(length)
    return torch.where(length > 0, scale, torch.zeros_like(scale))


def _bag_of(offsets: torch.Tensor, nnz: int) -> torch.Tensor:
    """Bag of every element (int32 [nnz]); -1 at or beyond offsets[-1]."""
    off = offsets.clamp(0, nnz)
    pos = torch.arange(nnz, device=offsets.device)
    bag = torch.bucketize(pos, off[1:].contiguous(), right=True)
    bag = torch.where(bag < off.numel() - 1, bag, torch.full_like(bag, -1))
    return bag.to(torch.int32)


def pool_fwd(rows: torch.Tensor, inverse, row_map, offsets: torch.Tensor,
             mode: str, want_bag_of: bool = True
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Segment-pooled gather over ragged bags (the reference's ragged
    sparse_read, exb.py:315-321, with the combiner fused in).

    Bag b pools elements [offsets[b], offsets[b+1]). Element j reads
    ``rows[row_map[inverse[j]]]``; ``inverse`` None is the identity,
    ``row_map`` None reads ``rows[inverse[j]]``; a mapped row < 0 is a zero
    row. rows [R, dim], inverse int64 [nnz], row_map int64/int32 [u],
    offsets int64 [B+1] -> (out [B, dim], bag_of int32 [nnz]); bag_of is -1
    for elements at or beyond offsets[-1] and feeds
    ``reduce_bags_by_inverse``."""
    if mode not in POOL_MODES:
        raise ValueError(f"unknown pooling mode {mode!r}")
    if _use_hip(rows) and rows.dtype == torch.float32:
        ext = require_hip()   # f64 variables use the torch path below
        if ext is not None:
            return ext.pool_fwd(rows, inverse, row_map, offsets,
                                POOL_MODES[mode], want_bag_of)
    if inverse is not None:
        nnz = inverse.numel()
        idx = inverse
    else:
        nnz = row_map.numel() if row_map is not None else rows.shape[0]
        idx = torch.arange(nnz, device=rows.device)
    if row_map is not None:
        idx = row_map.long().index_select(0, idx)
    elems = rows.index_select(0, idx.clamp(min=0))
    return pool_rows(elems, offsets, mode, live=idx >= 0)


def pool_rows(elems: torch.Tensor, offsets: torch.Tensor, mode: str,
              live: torch.Tensor = None, weights: torch.Tensor = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pool already-gathered element rows [nnz, dim] per bag with plain
    torch ops (differentiable w.r.t. ``elems``; sums in element order).
    ``live`` [nnz] bool masks elements out. ``weights`` [nnz] (optional)
    are per-sample weights with the semantics of ``pool_fwd_weighted``,
    differentiable too. Returns (out [B, dim], bag_of)."""
    nnz = elems.shape[0]
    bag_of = _bag_of(offsets, nnz)
    bag = bag_of.long()
    keep = bag >= 0
    if live is not None:
        keep = keep & live
    elems = torch.where(keep.unsqueeze(1), elems, torch.zeros_like(elems))
    if weights is not None:
        w, scale = _weighted_scale(weights.to(elems.dtype), bag,
                                   offsets.numel() - 1, mode)
        elems = elems * w.unsqueeze(1)
    else:
        scale = _bag_scale(offsets, nnz, mode, elems.dtype)
    out = torch.zeros((offsets.numel() - 1, elems.shape[1]),
                      dtype=elems.dtype, device=elems.device)
    out = out.index_add(0, bag.clamp(min=0), elems)
    out = out * scale.unsqueeze(1)
    return out, bag_of


def reduce_bags_by_inverse(inverse: torch.Tensor, grad_out: torch.Tensor,
                           bag_of: torch.Tensor, offsets: torch.Tensor,
                           mode: str, u: int
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of ``pool_fwd``: the (ugrads [u, dim], counts int64 [u])
    that ``reduce_by_inverse`` gives for the expanded gradient
    ``grad_out[bag_of[e]] * scale[bag_of[e]]``. The HIP kernels never
    build that [nnz, dim] expansion. Elements with bag_of < 0 add neither
    gradient nor count; counts are value occurrences over all bags (the
    reference's flat-value semantics)."""
    if mode not in POOL_MODES:
        raise ValueError(f"unknown pooling mode {mode!r}")
    if _use_hip(grad_out) and grad_out.dtype == torch.float32:
        ext = require_hip()
        if ext is not None:
            return ext.reduce_bags_by_inverse(inverse, grad_out, bag_of,
                                              offsets, POOL_MODES[mode], u)
    nnz = inverse.numel()
    bag = bag_of.long()
    live = bag >= 0
    b = bag.clamp(min=0)
    scale = _bag_scale(offsets, nnz, mode, grad_out.dtype)
    g = grad_out.index_select(0, b) * scale.index_select(0, b).unsqueeze(1)
    g = torch.where(live.unsqueeze(1), g, torch.zeros_like(g))
    ugrads = torch.zeros((u, grad_out.shape[1]), dtype=grad_out.dtype,
                         device=grad_out.device)
    ugrads.index_add_(0, inverse, g)
    counts = torch.zeros(u, dtype=torch.int64, device=grad_out.device)
    counts.index_add_(0, inverse, live.to(torch.int64))
    return ugrads, counts


# ------------------------------------------------------- per-sample weights

def _weighted_scale(weights: torch.Tensor, bag: torch.Tensor, B: int,
                    mode: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w [nnz] with the tail zeroed, scale [B]) of a weighted pool: scale
    is 1 (sum), 1 / sum w (mean), 1 / sqrt(sum w^2) (sqrtn), and 0 where
    that denominator is 0 (TF's divide_no_nan). The denominators run over
    every position of the bag, a missed row included; weights of the tail
    (bag < 0) are masked out before any use."""
    w = torch.where(bag >= 0, weights, torch.zeros_like(weights))
    if mode == "sum":
        return w, torch.ones(B, dtype=w.dtype, device=w.device)
    den = torch.zeros(B, dtype=w.dtype, device=w.device)
    den = den.index_add(0, bag.clamp(min=0), w if mode == "mean" else w * w)
    nz = den != 0
    safe = torch.where(nz, den, torch.ones_like(den))
    scale = 1.0 / safe if mode == "mean" else 1.0 / _sqrt(safe)
    return w, torch.where(nz, scale, torch.zeros_like(scale))


def _gather_rows(rows: torch.Tensor, inverse, row_map, nnz: int
                 ) -> torch.Tensor:
    """[nnz, dim] rows element j reads through inverse -> row_map; a mapped
    row < 0 is a zero row (torch path only)."""
    idx = inverse if inverse is not None \
        else torch.arange(nnz, device=rows.device)
    if row_map is not None:
        idx = row_map.long().index_select(0, idx)
    elems = rows.index_select(0, idx.clamp(min=0))
    return torch.where((idx >= 0).unsqueeze(1), elems,
                       torch.zeros_like(elems))


def pool_fwd_weighted(rows: torch.Tensor, inverse, row_map,
                      offsets: torch.Tensor, weights: torch.Tensor, mode: str
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``pool_fwd`` with per-sample weights (TF's embedding_lookup_sparse
    with ``sp_weights``): ``out[b] = scale_b * sum_j w_j * row_j`` with
    scale_b = 1 (sum) | 1 / sum_j w_j (mean) | 1 / sqrt(sum_j w_j^2)
    (sqrtn), 0 when that denominator is 0. weights float [nnz] (float32 on
    the HIP path); weights at or beyond offsets[-1] are never used.
    Returns (out [B, dim], bag_of int32 [nnz], bag_scale [B]); the last two
    feed ``reduce_bags_weighted_by_inverse`` and ``pool_wgrad``."""
    if mode not in POOL_MODES:
        raise ValueError(f"unknown pooling mode {mode!r}")
    if _use_hip(rows) and rows.dtype == torch.float32:
        ext = require_hip()   # f64 variables use the torch path below
        if ext is not None:
            return ext.pool_fwd_weighted(rows, inverse, row_map, offsets,
                                         weights, POOL_MODES[mode])
    nnz = weights.numel()
    B = offsets.numel() - 1
    elems = _gather_rows(rows, inverse, row_map, nnz)
    bag_of = _bag_of(offsets, nnz)
    bag = bag_of.long()
    w, scale = _weighted_scale(weights.to(rows.dtype), bag, B, mode)
    out = torch.zeros((B, rows.shape[1]), dtype=rows.dtype,
                      device=rows.device)
    out.index_add_(0, bag.clamp(min=0), elems * w.unsqueeze(1))
    return out * scale.unsqueeze(1), bag_of, scale


def reduce_bags_weighted_by_inverse(inverse: torch.Tensor,
                                    grad_out: torch.Tensor,
                                    bag_of: torch.Tensor,
                                    weights: torch.Tensor,
                                    bag_scale: torch.Tensor, u: int
                                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of ``pool_fwd_weighted`` w.r.t. the rows: element e adds
    ``grad_out[bag_of[e]] * (weights[e] * bag_scale[bag_of[e]])`` to its
    key. Counts do not depend on the weights: a weight-0 element counts 1,
    a tail element (bag_of < 0) 0."""
    if _use_hip(grad_out) and grad_out.dtype == torch.float32:
        ext = require_hip()
        if ext is not None:
            return ext.reduce_bags_weighted_by_inverse(
                inverse, grad_out, bag_of, weights, bag_scale, u)
    bag = bag_of.long()
    live = bag >= 0
    b = bag.clamp(min=0)
    w = torch.where(live, weights.to(grad_out.dtype),
                    torch.zeros((), dtype=grad_out.dtype,
                                device=grad_out.device))
    f = w * bag_scale.index_select(0, b)
    g = grad_out.index_select(0, b) * f.unsqueeze(1)
    g = torch.where(live.unsqueeze(1), g, torch.zeros_like(g))
    ugrads = torch.zeros((u, grad_out.shape[1]), dtype=grad_out.dtype,
                         device=grad_out.device)
    ugrads.index_add_(0, inverse, g)
    counts = torch.zeros(u, dtype=torch.int64, device=grad_out.device)
    counts.index_add_(0, inverse, live.to(torch.int64))
    return ugrads, counts


def pool_wgrad(rows: torch.Tensor, inverse, row_map, weights: torch.Tensor,
               bag_of: torch.Tensor, bag_scale: torch.Tensor,
               out: torch.Tensor, grad_out: torch.Tensor, mode: str
               ) -> torch.Tensor:
    """Backward of ``pool_fwd_weighted`` w.r.t. the weights, dw [nnz]:
    ``dw_j = scale_b * (<g_b, r_j> - c_j * <g_b, out_b>)`` with c_j = 0
    (sum) | 1 (mean) | w_j * scale_b (sqrtn); r_j is the row element j read
    (zero for a miss), g_b = grad_out[b]. 0 for tail elements. ``rows``,
    ``inverse`` and ``row_map`` are those of the forward (both None: rows
    are the gathered [nnz, dim] elements)."""
    if mode not in POOL_MODES:
        raise ValueError(f"unknown pooling mode {mode!r}")
    if _use_hip(rows) and rows.dtype == torch.float32:
        ext = require_hip()
        if ext is not None:
            return ext.pool_wgrad(rows, inverse, row_map, weights, bag_of,
                                  bag_scale, out, grad_out, POOL_MODES[mode])
    bag = bag_of.long()
    live = bag >= 0
    b = bag.clamp(min=0)
    r = _gather_rows(rows, inverse, row_map, weights.numel())
    g = grad_out.index_select(0, b)
    s = bag_scale.index_select(0, b)
    gr = (g * r).sum(1)
    if mode == "sum":
        dw = s * gr
    else:
        go = (g * out.index_select(0, b)).sum(1)
        c = 1.0 if mode == "mean" else weights.to(rows.dtype) * s
        dw = s * (gr - c * go)
    return torch.where(live, dw, torch.zeros_like(dw))


# ------------------------------------------------ quantized serving tables

QUANT_FORMATS = {"int8": 0, "fp16": 1}
FP16_MAX = 65504.0
_FLT_MIN = 1.1754943508222875e-38     # 2**-126, smallest normal float32


def _check_fmt(fmt: str) -> None:
    if fmt not in QUANT_FORMATS:
        raise ValueError(f"unknown row format {fmt!r}; expected one of "
                         f"{sorted(QUANT_FORMATS)}")


def row_stride(fmt: str, dim: int) -> int:
    """Bytes per packed row, a multiple of 4. int8: ``dim`` codes padded to
    a dword, then fp32 scale and fp32 lo. fp16: ``dim`` halves padded to a
    dword."""
    _check_fmt(fmt)
    if dim < 1:
        raise ValueError("dim must be >= 1")
    if fmt == "int8":
        return 4 * ((dim + 3) // 4) + 8
    return 4 * ((dim + 1) // 2)


def quantize_problems(w: torch.Tensor, fmt: str):
    """Why a block of fp32 rows cannot be stored in ``fmt``, or None: a
    non-finite value, a non-finite ``max - min`` of a row (int8 needs the
    span), or for fp16 a magnitude above 65504. Reads row minima and maxima
    only — no [n, dim] temporary. One host sync; import-time use."""
    _check_fmt(fmt)
    if w.numel() == 0:
        return None
    lo = w.amin(dim=1)          # amin / amax propagate NaN
    hi = w.amax(dim=1)
    if not bool((torch.isfinite(lo) & torch.isfinite(hi)).all()):
        return "a row holds a non-finite value"
    if not bool(torch.isfinite(hi - lo).all()):
        return "max - min of a row overflows float32"
    if fmt == "fp16" and bool((torch.maximum(hi, -lo) > FP16_MAX).any()):
        return f"a value exceeds the float16 range (|x| > {FP16_MAX:g})"
    return None


def quantize_rows(w: torch.Tensor, fmt: str) -> torch.Tensor:
    """fp32 rows [n, dim] -> packed rows uint8 [n, row_stride(fmt, dim)].

    int8, all in float32 and in this order: ``lo = min(row)`` (a -0.0
    minimum is stored as +0.0), ``hi = max(row)``,
    ``scale = (hi - lo) / 255``; a scale below FLT_MIN (zero or subnormal)
    becomes 0 with every code 0, otherwise
    ``code = clamp(rint((x - lo) / scale), 0, 255)`` (half to even).
    fp16: round-to-nearest-even halves. Pad bytes are zero. Rows that
    ``quantize_problems`` names raise ValueError. This torch form is the
    CPU path and the oracle of ``k_quantize_rows``, which fills the same
    bytes on a cuda tensor."""
    _check_fmt(fmt)
    if w.dim() != 2 or w.dtype != torch.float32:
        raise ValueError("quantize_rows takes float32 [n, dim] rows")
    bad = quantize_problems(w, fmt)
    if bad is not None:
        raise ValueError(f"cannot quantize to {fmt}: {bad}")
    n, dim = w.shape
    stride = row_stride(fmt, dim)
    if _use_hip(w):
        ext = require_hip()
        if ext is not None:
            slab = torch.empty((n, stride), dtype=torch.uint8,
                               device=w.device)
            ext.quantize_rows(w.contiguous(),
                              torch.arange(n, device=w.device), slab,
                              QUANT_FORMATS[fmt])
            return slab
    out = torch.zeros((n, stride), dtype=torch.uint8, device=w.device)
    if n == 0:
        return out
    if fmt == "fp16":
        out[:, :2 * dim] = w.to(torch.float16).contiguous() \
            .view(torch.uint8).view(n, 2 * dim)
        return out
    lo = w.amin(dim=1) + 0.0
    hi = w.amax(dim=1)
    # a tensor divisor: every backend then does a true division, not a
    # multiply by a rounded reciprocal
    scale = (hi - lo) / torch.full_like(lo, 255.0)
    live = scale >= _FLT_MIN
    scale = torch.where(live, scale, torch.zeros_like(scale))
    safe = torch.where(live, scale, torch.ones_like(scale))
    q = torch.round((w - lo.unsqueeze(1)) / safe.unsqueeze(1)).clamp(0, 255)
    q = torch.where(live.unsqueeze(1), q, torch.zeros_like(q))
    cw = stride - 8
    out[:, :dim] = q.to(torch.uint8)
    out[:, cw:cw + 4] = scale.contiguous().view(torch.uint8).view(n, 4)
    out[:, cw + 4:] = lo.contiguous().view(torch.uint8).view(n, 4)
    return out


def dequantize_rows(packed: torch.Tensor, dim: int, fmt: str) -> torch.Tensor:
    """Packed rows uint8 [n, row_stride(fmt, dim)] -> fp32 [n, dim]:
    ``lo + scale * float(code)`` (one multiply, then one add) for int8,
    ``float(half)`` for fp16. Plain torch on every device — the oracle of
    the dequantizing lookups, which never materialise this tensor."""
    stride = row_stride(fmt, dim)
    if packed.dim() != 2 or packed.dtype != torch.uint8 \
            or packed.shape[1] != stride:
        raise ValueError(f"packed rows must be uint8 [n, {stride}]")
    n = packed.shape[0]
    if fmt == "fp16":
        return packed[:, :2 * dim].contiguous().view(torch.float16) \
            .view(n, dim).float()
    cw = stride - 8
    scale = packed[:, cw:cw + 4].contiguous().view(torch.float32).view(n, 1)
    lo = packed[:, cw + 4:].contiguous().view(torch.float32).view(n, 1)
    return lo + scale * packed[:, :dim].float()


# ----------------------------------------------------------------- fused loss

class _FusedBCEFn(torch.autograd.Function):
    """BCEWithLogitsLoss(mean) in one kernel per direction at bench-size
    batches — a single-block forward with a plain store (no pre-fill, no
    atomics) up to n=64k, the fill+atomic grid form above that
    (torch spends ~5 launches per
    step on it inside the captured train graph: log_sigmoid + mean reduce +
    grad fill + the sigmoid-sub-scale chain). Same stable formulation, so
    it matches torch to fp32 atomic-order noise."""

    @staticmethod
    def forward(ctx, logits, labels, ext):
        logits = logits.contiguous()
        labels = labels.contiguous()
        ctx.save_for_backward(logits, labels)
        return ext.bce_fwd(logits, labels)

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels = ctx.saved_tensors
        ext = require_hip()
        g = ext.bce_bwd(logits, labels, grad_out)
        return g, None, None


def bce_with_logits(logits: torch.Tensor, labels: torch.Tensor
                    ) -> torch.Tensor:
    """Mean binary-cross-entropy-with-logits; fused HIP kernels on GPU,
    torch elsewhere. Differentiable w.r.t. logits."""
    if _use_hip(logits) and logits.dtype == torch.float32:
        ext = require_hip()
        if ext is not None:
            return _FusedBCEFn.apply(logits, labels.float(), ext)
    return torch.nn.functional.binary_cross_entropy_with_logits(
        logits, labels.to(logits.dtype))
