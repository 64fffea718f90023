"""Backend dispatch for the engine's hot ops.

Each op has a pure-torch implementation (CPU oracle; exact reference
semantics) and routes to the HIP extension on ROCm devices. The HIP kernels
are tested against the torch versions in tests/test_gpu_numerics.py.
"""

from __future__ import annotations

import os
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


# ------------------------------------------------- DLRM dot interaction
# out[b] = [x[b] | <v_i, v_j> for 0 <= j < i < T (tril_indices order) | pad]
# with v_0 = x[b], v_1.. = e[b]; x and e rounded to bf16 once as operands
# of the dots, fp32 sums. ops/csrc/dlrm.hip does it in one launch each way;
# OEAMD_DLRM_DOT=0 keeps the torch route on the GPU in the same build (A/B
# runs). Read once at import.
_DLRM_DOT = os.environ.get("OEAMD_DLRM_DOT", "1") != "0"


class _RoundGradBF16Fn(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16 once (what d_out is when
    it comes out of the fused MLP backward)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _dot_interact_torch(e: torch.Tensor, x: torch.Tensor, out_bf16: bool,
                        pad32: bool) -> torch.Tensor:
    B, F, D = e.shape
    T = F + 1
    v = torch.cat([x.unsqueeze(1), e], dim=1)
    # straight-through rounding: v + (r - v) is r exactly, and the gradient
    # passes unrounded
    vr = (v + (v.to(torch.bfloat16).to(v.dtype) - v).detach()).float()
    gram = torch.bmm(vr, vr.transpose(1, 2))
    li, lj = torch.tril_indices(T, T, -1, device=e.device)
    out = torch.cat([x.float(), gram[:, li, lj]], dim=1)
    out = _RoundGradBF16Fn.apply(out)
    if out_bf16:
        out = out.to(torch.bfloat16)
    if pad32:
        out = torch.nn.functional.pad(out, (0, -out.shape[1] % 32))
    return out


class _DotInteractFn(torch.autograd.Function):
    """k_dot_interact_fwd / k_dot_interact_bwd. Nothing extra is saved: the
    backward recomputes the bf16 operands from e and x."""

    @staticmethod
    def forward(ctx, e, x, out_bf16, pad32):
        ctx.save_for_backward(e, x)
        ctx.pad32 = pad32
        return require_hip().dot_interact_fwd(e, x, out_bf16, pad32)

    @staticmethod
    def backward(ctx, d_out):
        e, x = ctx.saved_tensors
        de, dx = require_hip().dot_interact_bwd(e, x, d_out.contiguous(),
                                                ctx.pad32)
        return de, dx, None, None


def _dot_interact_fits(e: torch.Tensor, x: torch.Tensor) -> bool:
    """The limits the binding checks (it refuses everything else)."""
    if not (_use_hip(e) and x.device == e.device and e.dim() == 3
            and x.dim() == 2 and e.dtype == x.dtype == torch.float32
            and e.is_contiguous() and x.is_contiguous()):
        return False
    B, F, D = e.shape
    Kp = (D + F * (F + 1) // 2 + 31) // 32 * 32
    return (1 <= F <= 31 and 1 <= D <= 128 and B * F * D < 2 ** 31
            and B * Kp < 2 ** 31)


def dot_interact(e: torch.Tensor, x: torch.Tensor, out_bf16: bool = False,
                 pad32: bool = False) -> torch.Tensor:
    """DLRM's pairwise dot interaction, differentiable w.r.t. e and x.

    e [B, F, D] embedding rows, x [B, D] bottom-MLP output ->
    [B, D + T(T-1)/2] (T = F + 1; 32-padded with zeros when ``pad32``),
    bf16 when ``out_bf16`` else fp32: x in front (unrounded), then the
    strictly lower triangle of the Gram matrix of (x, e_1 .. e_F) in
    ``torch.tril_indices(T, T, -1)`` order. x and e enter the dots rounded
    to bf16, the sums are fp32; the gradient coming in is rounded to bf16
    once. GPU: one HIP launch each way for contiguous fp32 operands with
    F <= 31 and D <= 128; everything else, and the CPU, takes torch ops."""
    if e.dim() != 3 or x.dim() != 2 or x.shape != (e.shape[0], e.shape[2]):
        raise ValueError("dot_interact takes e [B, F, D] and x [B, D]")
    if _DLRM_DOT and _dot_interact_fits(e, x) and require_hip() is not None:
        return _DotInteractFn.apply(e, x, out_bf16, pad32)
    return _dot_interact_torch(e, x, out_bf16, pad32)


# ------------------------------------------------- DCN-v2 cross network
# x_{l+1} = x_0 * (W_l x_l + b_l) + x_l for l = 0 .. L-1, optionally followed
# by the head w_out . x_L + b_out (+ partial). ops/csrc/cross.hip runs all L
# layers in one launch each way; OEAMD_CROSS=0 keeps the torch route on the
# GPU in the same build (A/B runs). Read once at import.
_CROSS = os.environ.get("OEAMD_CROSS", "1") != "0"


def _cross_torch(x0, W, b, w_out, b_out, partial):
    """The definition of the operator: plain differentiable ops in the
    parameters' dtype."""
    L, d = b.shape
    x0v = x0[:, :d].to(W.dtype)
    x = x0v
    for l in range(L):
        x = x0v * torch.nn.functional.linear(x, W[l], b[l]) + x
    return _cross_torch_tail(x, x0, w_out, b_out, partial)


def _cross_torch_tail(x, x0, w_out, b_out, partial):
    """x_L [M, d] of a torch route -> x_L in x0's shape and dtype, or the
    fp32 logit."""
    if w_out is None:
        x = x.to(x0.dtype)
        return torch.nn.functional.pad(x, (0, x0.shape[1] - x.shape[1]))
    out = (x @ w_out.reshape(-1, 1)).squeeze(1).float() + b_out.float()
    return out if partial is None else out + partial


def _cross_images(W: torch.Tensor, dp: int, with_t: bool, ext):
    """The fragment-major images of W_l and (with_t) of W_l^T, padded to
    [dp, dp], in two [L, dp, dp] buffers cached on the parameter and
    rewritten every forward: one mlp3_pack_frag launch for both sets while
    they are six matrices or fewer, else one per set."""
    L = W.shape[0]
    bufs = getattr(W, "_cross_bufs", None)
    if (bufs is None or bufs["w"].shape != (L, dp, dp)
            or bufs["w"].device != W.device):
        bufs = {k: torch.empty(L, dp, dp, dtype=torch.bfloat16,
                               device=W.device) for k in ("w", "wt")}
        W._cross_bufs = bufs
    srcs = [W[l] for l in range(L)]
    fwd = [bufs["w"][l] for l in range(L)]
    if not with_t:
        ext.mlp3_pack_frag(srcs, fwd, [False] * L)
    elif 2 * L <= 6:
        ext.mlp3_pack_frag(srcs + srcs, fwd + [bufs["wt"][l]
                                               for l in range(L)],
                           [False] * L + [True] * L)
    else:
        ext.mlp3_pack_frag(srcs, fwd, [False] * L)
        ext.mlp3_pack_frag(srcs, [bufs["wt"][l] for l in range(L)],
                           [True] * L)
    return bufs


def _cross_fn_forward(fn, ctx, x0, weights, r, b, w_out, b_out, partial,
                      save, bm):
    """The forward of _CrossNetFn and _CrossLRFn (``fn``): the mirrors xs,
    us and, at rank r > 0, ps; the head's arguments; what the backward
    needs, on ctx. ``fn.launch_fwd`` packs the weight images and launches."""
    ext = require_hip()
    M, dp = x0.shape
    L = b.shape[0]
    logit = w_out is not None
    save = bool(save) and any(ctx.needs_input_grad)
    weights = tuple(w.contiguous() for w in weights)
    b = b.contiguous()
    new = lambda *s, dt=torch.bfloat16: torch.empty(  # noqa: E731
        *s, dtype=dt, device=x0.device)
    us = new(L, M, dp) if save else None
    ps = new(L, M, (r + 31) // 32 * 32) if save and r else None
    xs = new(L, M, dp) if save else None if logit else new(1, M, dp)
    out = new(M, dt=torch.float32) if logit else None
    wo = w_out.reshape(-1).contiguous() if logit else None
    bufs = fn.launch_fwd(
        ext, x0, weights, b, save, xs, us, ps, wo,
        b_out.reshape(-1).contiguous() if logit else None,
        partial.contiguous() if partial is not None else None, out, bm)
    if save:
        ctx.save_for_backward(x0, xs, us, ps, b, wo)
        ctx.bufs = bufs
        ctx.bm = bm
        ctx._params = (*weights, b, w_out, b_out)
        ctx._has_partial = partial is not None
    return out if logit else xs[-1]


def _cross_fn_backward(fn, ctx, g):
    """The backward of _CrossNetFn and _CrossLRFn (``fn``). The kernel
    (``fn.launch_bwd``) gives dx0, q_l and, at low rank, s_l; the weight
    gradients are ``fn.wgrads``, db_l = sum_m q_l and the head's gradients
    are library ops here. When every parameter's .grad is bound (the flat
    optimizer's views) they accumulate in place and autograd gets None, as
    in _FusedMLP3Fn."""
    ext = require_hip()
    x0, xs, us, ps, b, wo = ctx.saved_tensors
    *weights, _, w_out, b_out = ctx._params
    nw = len(weights)
    L, d = b.shape
    logit = wo is not None
    qs = torch.empty_like(us)
    ss = None if ps is None else torch.empty_like(ps)
    dx0 = torch.empty_like(x0)
    dout = g.contiguous().float() if logit else None
    gl = None if logit else g.to(torch.bfloat16).contiguous()
    fn.launch_bwd(ext, ctx, weights, x0, us, b, dout, wo, gl, qs, ss, dx0)
    xl = [x0[:, :d]] + [xs[l][:, :d] for l in range(L - 1)]
    q = qs[:, :, :d]
    params = [p for p in ctx._params if p is not None]
    prebound = all(p.is_leaf and p.requires_grad and p.grad is not None
                   and p.grad.dtype == torch.bfloat16
                   and p.grad.is_contiguous() for p in params)
    dpart = dout if ctx._has_partial else None
    dvec = dout.to(torch.bfloat16).unsqueeze(0) if logit else None
    if prebound:
        fn.wgrads(weights, None, q, xl, ss, ps)
        b.grad.add_(q.sum(1))
        if logit:
            w_out.grad.view(1, d).addmm_(dvec, xs[L - 1][:, :d])
            b_out.grad.add_(dout.sum().to(b_out.grad.dtype))
        return (dx0,) + (None,) * (nw + 3) + (dpart, None, None)
    need = ctx.needs_input_grad
    dws = fn.wgrads(weights, need, q, xl, ss, ps)
    db = dwo = dbo = None
    if need[nw + 1]:
        db = q.sum(1)
    if logit and need[nw + 2]:
        dwo = (dvec @ xs[L - 1][:, :d]).view_as(w_out)
    if logit and need[nw + 3]:
        dbo = dout.sum().to(b_out.dtype).view_as(b_out)
    return (dx0, *dws, db, dwo, dbo, dpart, None, None)


class _CrossNetFn(torch.autograd.Function):
    """k_cross_fwd / k_cross_bwd. Saved for the backward: x_0, the kernel's
    mirrors x_1 .. x_L and u_0 .. u_{L-1}, and the transposed weight images
    packed by the forward (the weights cannot change before the backward
    runs). The kernel gives dx0 and q_l; dW_l = q_l^T x_l."""

    @staticmethod
    def forward(ctx, x0, W, b, w_out, b_out, partial, save, bm):
        return _cross_fn_forward(_CrossNetFn, ctx, x0, (W,), 0, b, w_out,
                                 b_out, partial, save, bm)

    @staticmethod
    def backward(ctx, g):
        return _cross_fn_backward(_CrossNetFn, ctx, g)

    @staticmethod
    def launch_fwd(ext, x0, weights, b, save, xs, us, ps, wo, bo, partial,
                   out, bm):
        bufs = _cross_images(weights[0], x0.shape[1], save, ext)
        ext.cross_fwd(x0, bufs["w"], b, xs, us, wo, bo, partial, out, bm)
        return bufs

    @staticmethod
    def launch_bwd(ext, ctx, weights, x0, us, b, dout, wo, gl, qs, ss, dx0):
        ext.cross_bwd(x0, us, ctx.bufs["wt"], b, dout, wo, gl, qs, dx0,
                      ctx.bm)

    @staticmethod
    def wgrads(weights, need, q, xl, ss, ps):
        """Into W.grad when ``need`` is None, else (dW,)."""
        (W,), L = weights, q.shape[0]
        if need is None:
            for l in range(L):
                W.grad[l].addmm_(q[l].t(), xl[l])
            return None
        return (torch.stack([q[l].t() @ xl[l] for l in range(L)])
                if need[1] else None,)


def _cross_fits(x0, weights, b, w_out, b_out, partial, rp=0) -> bool:
    """The limits the bindings check (they refuse everything else), for the
    full-rank network (rp = 0) and the low-rank one (rp = ceil32(r))."""
    bf = torch.bfloat16
    if not (_use_hip(x0) and x0.is_contiguous()
            and all(t.dtype == bf and t.device == x0.device
                    for t in (x0, b, *weights))):
        return False
    M, dp = x0.shape
    L, d = b.shape
    if not (dp == (d + 31) // 32 * 32 and 32 <= dp <= 512 and rp <= 128
            and 1 <= L <= 6 and M * max(dp, rp) * (L + 1) < 2 ** 31
            and x0.data_ptr() % 16 == 0):
        return False
    if w_out is None:
        return True
    return (w_out.dtype == b_out.dtype == bf
            and w_out.device == b_out.device == x0.device
            and (partial is None or (partial.dtype == torch.float32
                                     and partial.device == x0.device)))


def cross_network(x0: torch.Tensor, W: torch.Tensor, b: torch.Tensor,
                  w_out: torch.Tensor = None, b_out: torch.Tensor = None,
                  partial: torch.Tensor = None, bm: int = 0) -> torch.Tensor:
    """DCN-v2 cross network, differentiable w.r.t. every tensor argument.

    x0 [M, d], or [M, ceil32(d)] with zero pad columns; W [L, d, d], each
    W[l] stored [out, in] like nn.Linear; b [L, d]. Computes
    x_{l+1} = x_0 * (W_l x_l + b_l) + x_l for l = 0 .. L-1 and returns x_L in
    x0's shape and dtype, or with w_out [d] and b_out [1] the fp32 logit [M]
    = w_out . x_L + b_out (+ partial [M]).

    GPU: one HIP launch each way (ops/csrc/cross.hip) for contiguous bf16
    x0 [M, dp], dp = ceil32(d) in 32..512, bf16 parameters, 1 <= L <= 6 and
    M*dp*(L+1) < 2^31: bf16 operands, fp32 arithmetic, each stored value
    rounded to bf16 once. Everything else, and the CPU, takes torch ops in
    the parameters' dtype. ``bm`` forces the kernels' row tile (16 or 32;
    0 = the launcher's choice)."""
    if (x0.dim() != 2 or W.dim() != 3 or b.dim() != 2
            or W.shape != (b.shape[0], b.shape[1], b.shape[1])
            or x0.shape[1] not in (b.shape[1], (b.shape[1] + 31) // 32 * 32)
            or (w_out is None) != (b_out is None)
            or (partial is not None and w_out is None)):
        raise ValueError("cross_network takes x0 [M, d or ceil32(d)], "
                         "W [L, d, d], b [L, d], w_out [d] with b_out [1]")
    if (_CROSS and _cross_fits(x0, (W,), b, w_out, b_out, partial)
            and require_hip() is not None):
        return _CrossNetFn.apply(x0, W, b, w_out, b_out, partial,
                                 torch.is_grad_enabled(), bm)
    return _cross_torch(x0, W, b, w_out, b_out, partial)


# --------------------------------------- DCN-v2 low-rank cross network
# x_{l+1} = x_0 * (U_l (V_l x_l) + b_l) + x_l: W_l = U_l V_l of rank r << d.
# ops/csrc/cross_lr.hip runs all L layers in one launch each way;
# OEAMD_CROSS_LR=0 keeps the torch route on the GPU in the same build (A/B
# runs). Read once at import.
_CROSS_LR = os.environ.get("OEAMD_CROSS_LR", "1") != "0"


def _cross_lr_torch(x0, U, V, b, w_out, b_out, partial):
    """The definition of the operator: plain differentiable ops in the
    parameters' dtype."""
    L, d = b.shape
    x0v = x0[:, :d].to(U.dtype)
    x = x0v
    lin = torch.nn.functional.linear
    for l in range(L):
        x = x0v * lin(lin(x, V[l]), U[l], b[l]) + x
    return _cross_torch_tail(x, x0, w_out, b_out, partial)


def _cross_lr_images(U: torch.Tensor, V: torch.Tensor, dp: int, rp: int,
                     with_t: bool, ext):
    """The fragment-major images of V_l [rp, dp] and U_l [dp, rp], and
    (with_t) of U_l^T [rp, dp] and V_l^T [dp, rp], zero-padded, in buffers
    cached on U and rewritten every forward by mlp3_pack_frag, six matrices
    per launch."""
    L = U.shape[0]
    bufs = getattr(U, "_cross_lr_bufs", None)
    if (bufs is None or bufs["v"].shape != (L, rp, dp)
            or bufs["v"].device != U.device):
        new = lambda *s: torch.empty(*s, dtype=torch.bfloat16,  # noqa: E731
                                     device=U.device)
        bufs = {"v": new(L, rp, dp), "u": new(L, dp, rp),
                "ut": new(L, rp, dp), "vt": new(L, dp, rp)}
        U._cross_lr_bufs = bufs
    jobs = []
    for l in range(L):
        jobs += [(V[l], bufs["v"][l], False), (U[l], bufs["u"][l], False)]
    for l in range(L if with_t else 0):
        jobs += [(U[l], bufs["ut"][l], True), (V[l], bufs["vt"][l], True)]
    for i in range(0, len(jobs), 6):
        src, dst, tr = zip(*jobs[i:i + 6])
        ext.mlp3_pack_frag(list(src), list(dst), list(tr))
    return bufs


class _CrossLRFn(torch.autograd.Function):
    """k_cross_lr_fwd / k_cross_lr_bwd. Saved for the backward: x_0, the
    kernel's mirrors x_1 .. x_L, u_l and p_l, and the transposed weight
    images packed by the forward. The kernel gives dx0, q_l and s_l;
    dU_l = q_l^T p_l, dV_l = s_l^T x_l. The rest as in _CrossNetFn."""

    @staticmethod
    def forward(ctx, x0, U, V, b, w_out, b_out, partial, save, bm):
        return _cross_fn_forward(_CrossLRFn, ctx, x0, (U, V), V.shape[1], b,
                                 w_out, b_out, partial, save, bm)

    @staticmethod
    def backward(ctx, g):
        return _cross_fn_backward(_CrossLRFn, ctx, g)

    @staticmethod
    def launch_fwd(ext, x0, weights, b, save, xs, us, ps, wo, bo, partial,
                   out, bm):
        U, V = weights
        r = V.shape[1]
        bufs = _cross_lr_images(U, V, x0.shape[1], (r + 31) // 32 * 32, save,
                                ext)
        ext.cross_lr_fwd(x0, bufs["v"], bufs["u"], b, r, xs, us, ps, wo, bo,
                         partial, out, bm)
        return bufs

    @staticmethod
    def launch_bwd(ext, ctx, weights, x0, us, b, dout, wo, gl, qs, ss, dx0):
        ext.cross_lr_bwd(x0, us, ctx.bufs["ut"], ctx.bufs["vt"], b,
                         weights[1].shape[1], dout, wo, gl, qs, ss, dx0,
                         ctx.bm)

    @staticmethod
    def wgrads(weights, need, q, xl, ss, ps):
        """Into U.grad and V.grad when ``need`` is None, else (dU, dV)."""
        (U, V), L = weights, q.shape[0]
        r = V.shape[1]
        s, p = ss[:, :, :r], ps[:, :, :r]
        if need is None:
            for l in range(L):
                U.grad[l].addmm_(q[l].t(), p[l])
                V.grad[l].addmm_(s[l].t(), xl[l])
            return None
        dU = dV = None
        if need[1]:
            dU = torch.stack([q[l].t() @ p[l] for l in range(L)])
        if need[2]:
            dV = torch.stack([s[l].t() @ xl[l] for l in range(L)])
        return dU, dV


def cross_network_lr(x0: torch.Tensor, U: torch.Tensor, V: torch.Tensor,
                     b: torch.Tensor, w_out: torch.Tensor = None,
                     b_out: torch.Tensor = None,
                     partial: torch.Tensor = None,
                     bm: int = 0) -> torch.Tensor:
    """DCN-v2 cross network with low-rank layers W_l = U_l V_l,
    differentiable w.r.t. every tensor argument.

    x0 [M, d], or [M, ceil32(d)] with zero pad columns; V [L, r, d] the
    down-projection and U [L, d, r] the up-projection, each stored
    [out, in] like nn.Linear; b [L, d]. Computes
    x_{l+1} = x_0 * (U_l (V_l x_l) + b_l) + x_l for l = 0 .. L-1 and returns
    x_L in x0's shape and dtype, or with w_out [d] and b_out [1] the fp32
    logit [M] = w_out . x_L + b_out (+ partial [M]): ``cross_network``'s two
    forms. Out of scope: the paper's mixture of experts with its gate, and
    the non-linearity inside the projection.

    GPU: one HIP launch each way (ops/csrc/cross_lr.hip) for contiguous bf16
    x0 [M, dp], dp = ceil32(d) in 32..512, rp = ceil32(r) <= 128, bf16
    parameters, 1 <= L <= 6 and M*max(dp, rp)*(L+1) < 2^31: bf16 operands,
    fp32 arithmetic, each stored value (the rank activation included)
    rounded to bf16 once. Everything else, and the CPU, takes torch ops in
    the parameters' dtype. ``bm`` forces the kernels' row tile (16 or 32;
    0 = the launcher's choice)."""
    if (x0.dim() != 2 or U.dim() != 3 or V.dim() != 3 or b.dim() != 2
            or V.shape[1] < 1
            or U.shape != (b.shape[0], b.shape[1], V.shape[1])
            or V.shape != (b.shape[0], V.shape[1], b.shape[1])
            or x0.shape[1] not in (b.shape[1], (b.shape[1] + 31) // 32 * 32)
            or (w_out is None) != (b_out is None)
            or (partial is not None and w_out is None)):
        raise ValueError("cross_network_lr takes x0 [M, d or ceil32(d)], "
                         "U [L, d, r], V [L, r, d], b [L, d], w_out [d] "
                         "with b_out [1]")
    if (_CROSS_LR and _cross_fits(x0, (U, V), b, w_out, b_out, partial,
                                  (V.shape[1] + 31) // 32 * 32)
            and require_hip() is not None):
        return _CrossLRFn.apply(x0, U, V, b, w_out, b_out, partial,
                                torch.is_grad_enabled(), bm)
    return _cross_lr_torch(x0, U, V, b, w_out, b_out, partial)


# ------------------------------------------------------- fused MLP tower
# a_l = relu(W_l a_{l-1} + b_l) for l = 1 .. L, then w_out . a_L + b_out
# (+ partial). ops/csrc/tower.hip runs 1 to 4 hidden layers of unequal widths
# in one launch each way; OEAMD_TOWER=0 keeps the torch route on the GPU in
# the same build (A/B runs). Read once at import.
_TOWER = os.environ.get("OEAMD_TOWER", "1") != "0"
# OEAMD_TOWER_WGRAD=0 keeps the library wgrads behind k_tower_bwd
_TOWER_WGRAD = os.environ.get("OEAMD_TOWER_WGRAD", "1") != "0"


def _ceil32(v: int) -> int:
    return (v + 31) // 32 * 32


def _tower_torch(x0, weights, biases, w_out, b_out, partial):
    """The definition of the operator: plain differentiable ops in the
    parameters' dtype."""
    a = x0[:, :weights[0].shape[1]].to(weights[0].dtype)
    for W, b in zip(weights, biases):
        a = torch.relu(torch.nn.functional.linear(a, W, b))
    out = (a @ w_out.reshape(-1, 1)).squeeze(1).float() + b_out.float()
    return out if partial is None else out + partial


def _tower_images(weights, K0p: int, with_t: bool, ext):
    """The fragment-major images of W_l padded to [H_l, ceil32(H_{l-1})] and
    (with_t) of W_l^T padded to [H_{l-1}, ceil32(H_l)] ([K0p, ..] for the
    first layer), cached on the first weight and rewritten every forward by
    mlp3_pack_frag, six matrices per launch."""
    W1 = weights[0]
    key = (K0p, tuple(w.shape for w in weights), W1.device)
    bufs = getattr(W1, "_tower_bufs", None)
    if bufs is None or bufs["key"] != key:
        new = lambda *s: torch.empty(*s, dtype=torch.bfloat16,  # noqa: E731
                                     device=W1.device)
        kp = [K0p] + [_ceil32(w.shape[0]) for w in weights[:-1]]
        rows = [K0p] + [w.shape[0] for w in weights[:-1]]
        bufs = {"key": key,
                "w": [new(w.shape[0], k) for w, k in zip(weights, kp)],
                "wt": [new(r, _ceil32(w.shape[0]))
                       for w, r in zip(weights, rows)]}
        W1._tower_bufs = bufs
    jobs = [(w, d, False) for w, d in zip(weights, bufs["w"])]
    if with_t:
        jobs += [(w, d, True) for w, d in zip(weights, bufs["wt"])]
    for i in range(0, len(jobs), 6):
        src, dst, tr = zip(*jobs[i:i + 6])
        ext.mlp3_pack_frag(list(src), list(dst), list(tr))
    return bufs


def _tower_wgrad_scratch(weights, M: int, ext):
    """The fp32 slabs of k_tower_wgrad, beside ``_tower_bufs`` on the first
    weight and keyed like them (plus M, which sets the slices): allocated on
    the first call, so a captured step replays on the buffer its warm-up
    made."""
    W1 = weights[0]
    key = (M, tuple(w.shape for w in weights), W1.device)
    held = getattr(W1, "_tower_wgrad_buf", None)
    if held is None or held[0] != key:
        floats = ext.tower_wgrad_plan(M, W1.shape[1],
                                      [w.shape[0] for w in weights], 0)[1]
        held = (key, torch.empty(floats, dtype=torch.float32,
                                 device=W1.device))
        W1._tower_wgrad_buf = held
    return held[1]


class _TowerFn(torch.autograd.Function):
    """k_tower_fwd / k_tower_bwd / k_tower_wgrad. Saved for the backward:
    x_0, the kernel's mirrors a_1 .. a_L, and the transposed weight images
    packed by the forward (the weights cannot change before the backward
    runs). k_tower_bwd gives dx0 and dz_l. When every parameter needs a
    gradient, k_tower_wgrad and its fold give dW_l = dz_l^T a_{l-1}, db_l =
    sum_m dz_l and the head's gradients (OEAMD_TOWER_WGRAD=0: library ops, as
    for a partly frozen tower). When every parameter's .grad is bound (the
    flat optimizer's views) they accumulate in place and autograd gets None,
    as in _CrossNetFn."""

    @staticmethod
    def forward(ctx, x0, w_out, b_out, partial, save, bm, *wb):
        ext = require_hip()
        L = len(wb) // 2
        weights = [w.contiguous() for w in wb[:L]]
        biases = [b.contiguous() for b in wb[L:]]
        M = x0.shape[0]
        save = bool(save) and any(ctx.needs_input_grad)
        acts = [torch.empty(M, w.shape[0], dtype=torch.bfloat16,
                            device=x0.device) for w in weights] if save else []
        out = torch.empty(M, dtype=torch.float32, device=x0.device)
        wo = w_out.reshape(-1).contiguous()
        bufs = _tower_images(weights, x0.shape[1], save, ext)
        ext.tower_fwd(x0, weights[0].shape[1], bufs["w"], biases, acts, wo,
                      b_out.reshape(-1).contiguous(),
                      partial.contiguous() if partial is not None else None,
                      out, bm)
        if save:
            ctx.save_for_backward(x0, wo, *acts)
            ctx.bufs = bufs
            ctx.bm = bm
            ctx._params = (wb[:L], wb[L:], w_out, b_out)
            ctx._has_partial = partial is not None
        return out

    @staticmethod
    def backward(ctx, g):
        ext = require_hip()
        x0, wo, *acts = ctx.saved_tensors
        weights, biases, w_out, b_out = ctx._params
        L, K0 = len(weights), weights[0].shape[1]
        dout = g.contiguous().float()
        dzs = [torch.empty_like(a) for a in acts]
        dx0 = torch.empty_like(x0)
        ext.tower_bwd(K0, acts, ctx.bufs["wt"], dout, wo, dzs, dx0, ctx.bm)
        ins = [x0[:, :K0]] + acts[:-1]
        params = (*weights, *biases, w_out, b_out)
        prebound = all(p.is_leaf and p.requires_grad and p.grad is not None
                       and p.grad.dtype == torch.bfloat16
                       and p.grad.is_contiguous() for p in params)
        dpart = dout if ctx._has_partial else None
        need = ctx.needs_input_grad
        if _TOWER_WGRAD and all(need[1:3]) and all(need[6:]):
            # k_tower_wgrad + fold: every parameter gradient in two launches,
            # in place when every .grad is bound, else into fresh tensors
            grads = ([p.grad for p in params] if prebound else
                     [torch.empty(p.shape, dtype=torch.bfloat16,
                                  device=x0.device) for p in params])
            ext.tower_wgrad(x0, K0, acts, dzs, dout, grads, prebound,
                            _tower_wgrad_scratch(weights, x0.shape[0], ext), 0)
            if prebound:
                return (dx0, None, None, dpart, None, None) + (None,) * (2 * L)
            return (dx0, grads[-2], grads[-1], dpart, None, None, *grads[:-2])
        dvec = dout.to(torch.bfloat16).unsqueeze(0)
        if prebound:
            for W, b, dz, a in zip(weights, biases, dzs, ins):
                W.grad.addmm_(dz.t(), a)
                b.grad.add_(dz.sum(0))
            w_out.grad.view(1, -1).addmm_(dvec, acts[-1])
            b_out.grad.add_(dout.sum().to(b_out.grad.dtype))
            return (dx0, None, None, dpart, None, None) + (None,) * (2 * L)
        dwo =(dvec @ acts[-1]).view_as(w_out) if need[1] else None
        dbo = (dout.sum().to(b_out.dtype).view_as(b_out) if need[2]
               else None)
        dws = [dz.t() @ a if need[6 + l] else None
               for l, (dz, a) in enumerate(zip(dzs, ins))]
        dbs = [dz.sum(0) if need[6 + L + l] else None
               for l, dz in enumerate(dzs)]
        return (dx0, dwo, dbo, dpart, None, None, *dws, *dbs)


def _tower_fits(x0, weights, biases, w_out, b_out, partial) -> bool:
    """The limits the bindings check (they refuse everything else)."""
    bf = torch.bfloat16
    if not (_use_hip(x0) and x0.is_contiguous()
            and all(t.dtype == bf and t.device == x0.device
                    for t in (x0, *weights, *biases, w_out, b_out))):
        return False
    M, K0p = x0.shape
    L = len(weights)
    return (K0p == _ceil32(weights[0].shape[1]) and K0p <= 512
            and 1 <= L <= 4
            and all(w.shape[0] % 16 == 0 and 16 <= w.shape[0] <= 512
                    for w in weights)
            and M * 512 * (L + 1) < 2 ** 31 and x0.data_ptr() % 16 == 0
            and (partial is None or (partial.dtype == torch.float32
                                     and partial.device == x0.device)))


def mlp_tower(x0: torch.Tensor, weights, biases, w_out: torch.Tensor,
              b_out: torch.Tensor, partial: torch.Tensor = None,
              bm: int = 0) -> torch.Tensor:
    """MLP tower with a logit head, differentiable w.r.t. every tensor
    argument.

    x0 [M, K0], or [M, ceil32(K0)] with zero pad columns; weights[l]
    [H_l, H_{l-1}] (H_0 = K0) stored like nn.Linear, biases[l] [H_l];
    w_out [H_L] or [1, H_L], b_out [1]. Computes
    a_l = relu(W_l a_{l-1} + b_l) and returns the fp32 logit [M]
    = w_out . a_L + b_out (+ partial [M]).

    GPU: one HIP launch each way (ops/csrc/tower.hip) for contiguous bf16
    x0 [M, K0p], K0p = ceil32(K0) <= 512, bf16 parameters, 1 to 4 hidden
    layers, every width a multiple of 16 in 16..512 and M*512*(L+1) < 2^31:
    bf16 operands, fp32 arithmetic, each activation rounded to bf16 once;
    the parameter gradients come from one more launch and a fold when every
    parameter needs one (OEAMD_TOWER_WGRAD=0: library ops).
    Everything else, and the CPU, takes torch ops in the parameters' dtype.
    ``bm`` forces the kernels' row tile (16 or 32; 0 = the launcher's
    choice)."""
    weights, biases = list(weights), list(biases)
    ok = (x0.dim() == 2 and len(weights) == len(biases) >= 1
          and all(w.dim() == 2 for w in weights))
    if ok:
        widths = [weights[0].shape[1]] + [w.shape[0] for w in weights]
        ok = (all(w.shape[1] == k and b.shape == (w.shape[0],)
                  for w, b, k in zip(weights, biases, widths))
              and x0.shape[1] in (widths[0], _ceil32(widths[0]))
              and tuple(w_out.shape) in ((widths[-1],), (1, widths[-1]))
              and b_out.numel() == 1
              and (partial is None or partial.shape == (x0.shape[0],)))
    if not ok:
        raise ValueError("mlp_tower takes x0 [M, K0 or ceil32(K0)], "
                         "weights[l] [H_l, H_{l-1}] with biases[l] [H_l], "
                         "w_out [H_L] or [1, H_L], b_out [1], partial [M]")
    if (_TOWER and _tower_fits(x0, weights, biases, w_out, b_out, partial)
            and require_hip() is not None):
        return _TowerFn.apply(x0, w_out, b_out, partial,
                              torch.is_grad_enabled(), bm, *weights, *biases)
    return _tower_torch(x0, weights, biases, w_out, b_out, partial)


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
