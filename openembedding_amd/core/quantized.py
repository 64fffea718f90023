"""Quantized serving table: one read-only shard stored as packed rows.

A serving replica only receives rows (a load, a delta's upserts and
tombstones) and never trains them, so it needs neither fp32 rows nor an
optimizer-state slab nor a grow-by-doubling policy.
``QuantizedShard`` owns exactly two things: a key -> row map (the hash
``tk`` / ``tv`` / ``slot_keys`` or the array ``valid_u8`` of the training
shards, built with the same kernels) and a ``torch.uint8`` slab
``[R, row_stride(fmt, dim)]`` of packed rows in one of the formats of
``ops.dispatch.quantize_rows`` ("int8": 8-bit codes with a per-row fp32
scale and offset; "fp16": IEEE halves).

On a cuda device rows are quantized into place by ``k_quantize_rows`` and
read by the dequantizing lookups ``k_gather_lookup_q`` / ``k_pool_lookup_q``
(ops/csrc/embops.hip) — the extension is required there. On the CPU the
torch forms of ``ops.dispatch`` do the same arithmetic op for op; that path
is the oracle of the kernels (bit-identical results).

Not combined with the capacity tier (core/tiered_gpu.py): every packed row
lives in the device slab.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from ..ops import dispatch as ops
from ..ops import require_hip
from .variable import VariableMeta, hole_fill_plan


class QuantizedShard:
    """Read-only quantized table of one variable (hash or array keyed)."""

    MIN_TABLE_CAP = 1 << 16     # probe table floor, as HipVariableShard
    IMPORT_BLOCK = 1 << 16      # rows per block in from_shard
    # every row is in the slab: the pooled read is one fused launch
    fused_pooled_readonly = True

    def __init__(self, meta: VariableMeta, fmt: str, device: str = "cpu",
                 shard_id: int = 0, shard_num: int = 1):
        if fmt not in ops.QUANT_FORMATS:
            raise ValueError(f"unknown row format {fmt!r}; expected one of "
                             f"{sorted(ops.QUANT_FORMATS)}")
        if meta.dtype != torch.float32:
            raise NotImplementedError(
                "quantized tables hold float32 variables; a "
                f"{meta.datatype_str()} variable cannot be quantized")
        self.meta = meta
        self.fmt = fmt
        self.shard_id = shard_id
        self.shard_num = shard_num
        self.device = torch.device(device)
        self.dim = meta.embedding_dim
        self.dtype = torch.float32
        self.stride = ops.row_stride(fmt, self.dim)
        self._hip = self.device.type == "cuda"
        self.ext = None
        if self._hip:
            self.ext = require_hip()
            if self.ext is None:
                raise RuntimeError("HIP extension missing: a quantized "
                                   "table on a GPU needs its kernels")
        self._fmt_id = ops.QUANT_FORMATS[fmt]
        self._reserved = False
        self._nrows = 0
        dev = self.device
        if meta.use_hash_table:
            self._array_cap = 0
            self.slab = torch.zeros((0, self.stride), dtype=torch.uint8,
                                    device=dev)
            self.slot_keys = torch.empty(0, dtype=torch.int64, device=dev)
            if self._hip:
                self._cap = self.MIN_TABLE_CAP
                self.tk = torch.full((self._cap,), -1, dtype=torch.int64,
                                     device=dev)
                self.tv = torch.empty(self._cap, dtype=torch.int32,
                                      device=dev)
                self.nrows_dev = torch.zeros(1, dtype=torch.int32,
                                             device=dev)
            else:
                self._index: Dict[int, int] = {}
        else:
            vocab = meta.vocabulary_size
            self._array_cap = (vocab - shard_id + shard_num - 1) // shard_num
            self.slab = torch.zeros((self._array_cap, self.stride),
                                    dtype=torch.uint8, device=dev)
            self.valid_u8 = torch.zeros(self._array_cap, dtype=torch.uint8,
                                        device=dev)

    # ------------------------------------------------------------- capacity

    def reserve_rows(self, n: int) -> None:
        """Size the slab for exactly ``n`` rows (and the hash map for ``n``
        keys), so that a load of ``n`` rows never regrows either. An array
        table is sized by its vocabulary already."""
        if not self.meta.use_hash_table:
            return
        n = int(n)
        self._reserved = True
        self._resize_rows(max(n, self._nrows))
        if self._hip:
            self._grow_table(n)

    def _resize_rows(self, cap: int) -> None:
        if cap == self.slab.shape[0]:
            return
        slab = torch.zeros((cap, self.stride), dtype=torch.uint8,
                           device=self.device)
        sk = torch.empty(cap, dtype=torch.int64, device=self.device)
        n = self._nrows
        slab[:n] = self.slab[:n]
        sk[:n] = self.slot_keys[:n]
        self.slab, self.slot_keys = slab, sk

    def _ensure_rows(self, need: int) -> None:
        """Room for ``need`` rows: exact once reserve_rows was called (a
        load that outgrows its reservation still works), doubling
        otherwise."""
        cap = self.slab.shape[0]
        if need <= cap:
            return
        self._resize_rows(need if self._reserved
                          else max(need, 2 * cap, 1024))

    def _grow_table(self, rows: int) -> None:
        """Probe table at load factor <= 0.5 for ``rows`` keys."""
        want = max(self.MIN_TABLE_CAP, 1 << max(0, 2 * rows - 1).bit_length())
        if want <= self._cap:
            return
        tk = torch.empty(want, dtype=torch.int64, device=self.device)
        tv = torch.empty(want, dtype=torch.int32, device=self.device)
        self.ext.ht_rehash(self.tk, self.tv, tk, tv)
        self.tk, self.tv, self._cap = tk, tv, want

    # --------------------------------------------------------------- import

    def _check_keys(self, keys: torch.Tensor) -> None:
        if self.meta.use_hash_table:
            if bool((keys == -1).any()):
                raise ValueError("key -1 is reserved in hash mode (table "
                                 "empty marker)")
            return
        if bool((keys % self.shard_num != self.shard_id).any()):
            raise ValueError("keys not owned by this shard")
        slots = keys // self.shard_num
        if bool(((slots < 0) | (slots >= self._array_cap)).any()):
            raise ValueError("key out of vocabulary range")

    @staticmethod
    def _last_of_each(keys: torch.Tensor) -> Optional[torch.Tensor]:
        """Positions of the last occurrence of every distinct key, or None
        when the keys are distinct already."""
        n = keys.numel()
        uk, inv = torch.unique(keys, return_inverse=True)
        if uk.numel() == n:
            return None
        last = torch.zeros(uk.numel(), dtype=torch.int64, device=keys.device)
        last.scatter_reduce_(0, inv, torch.arange(n, device=keys.device),
                             reduce="amax", include_self=False)
        return last

    def _slots_for_import(self, keys: torch.Tensor) -> torch.Tensor:
        """Rows of distinct, validated keys; new keys get the next rows."""
        n = keys.numel()
        if not self.meta.use_hash_table:
            if self._hip:
                slots, _ = self.ext.array_touch(self.valid_u8, keys,
                                                self.shard_num, None)
            else:
                slots = keys // self.shard_num
                self.valid_u8[slots] = 1
            self._nrows = int((self.valid_u8 != 0).sum())
            return slots
        need = self._nrows + n
        if need > self.slab.shape[0]:
            # some of the keys may be overwrites: count the new ones before
            # growing, so that a full reservation is not outgrown by them
            if self._hip:
                old, _ = self.ext.ht_lookup(self.tk, self.tv, keys,
                                            self.nrows_dev, self.slot_keys,
                                            False, None)
                need = self._nrows + int((old < 0).sum())
            else:
                need = self._nrows + sum(k not in self._index
                                         for k in keys.tolist())
        self._ensure_rows(need)
        if self._hip:
            self._grow_table(need)
            slots, _ = self.ext.ht_lookup(self.tk, self.tv, keys,
                                          self.nrows_dev, self.slot_keys,
                                          True, None)
            self._nrows = int(self.nrows_dev.item())
            return slots
        idx = self._index
        out = []
        for k in keys.tolist():
            s = idx.get(k)
            if s is None:
                s = self._nrows
                idx[k] = s
                self.slot_keys[s] = k
                self._nrows += 1
            out.append(s)
        return torch.tensor(out, dtype=torch.int64, device=self.device)

    def import_rows(self, keys: torch.Tensor, weights: torch.Tensor,
                    state: Optional[torch.Tensor] = None) -> None:
        """Store fp32 rows under ``keys``, quantized into place; a key
        already present is overwritten, and of a key that occurs twice in
        one call the last row wins. The block is validated first
        (``ops.quantize_problems``, reserved / out-of-range keys): a
        rejected block raises ValueError and changes nothing. ``state`` is
        accepted for the interface of the training shards and ignored."""
        keys = keys.to(self.device, torch.int64).reshape(-1)
        w = weights.to(self.device, torch.float32)
        if w.dim() != 2 or w.shape != (keys.numel(), self.dim):
            raise ValueError(f"weights must be [{keys.numel()}, {self.dim}]"
                             f", got {tuple(w.shape)}")
        if keys.numel() == 0:
            return
        bad = ops.quantize_problems(w, self.fmt)
        if bad is not None:
            raise ValueError(f"cannot quantize to {self.fmt}: {bad}")
        self._check_keys(keys)
        last = self._last_of_each(keys)
        if last is not None:
            keys = keys.index_select(0, last)
            w = w.index_select(0, last)
        slots = self._slots_for_import(keys.contiguous())
        if self._hip:
            self.ext.quantize_rows(w.contiguous(), slots, self.slab,
                                   self._fmt_id)
        else:
            self.slab[slots] = ops.quantize_rows(w, self.fmt)

    @classmethod
    def from_shard(cls, shard, fmt: str) -> "QuantizedShard":
        """Quantized copy of a loaded fp32 shard (any backend), on the
        shard's device, imported block by block."""
        q = cls(shard.meta, fmt, device=str(shard.device),
                shard_id=shard.shard_id, shard_num=shard.shard_num)
        keys, w, _ = shard.export_rows(include_state=False)
        q.reserve_rows(keys.numel())
        for s in range(0, keys.numel(), cls.IMPORT_BLOCK):
            q.import_rows(keys[s:s + cls.IMPORT_BLOCK],
                          w[s:s + cls.IMPORT_BLOCK])
        return q

    # ---------------------------------------------------------------- reads

    def _table_args(self) -> dict:
        if self.meta.use_hash_table:
            return {"tk": self.tk, "tv": self.tv}
        return {"valid": self.valid_u8, "shard_num": self.shard_num}

    def _lookup_readonly(self, keys: torch.Tensor) -> torch.Tensor:
        """Torch form: rows of ``keys``, -1 for a miss."""
        if self.meta.use_hash_table:
            idx = self._index
            return torch.tensor([idx.get(k, -1) for k in keys.tolist()],
                                dtype=torch.int64, device=self.device)
        slots = torch.div(keys, self.shard_num, rounding_mode="floor")
        ok = (keys >= 0) & (slots < self._array_cap)
        hit = ok & (self.valid_u8[slots.clamp(0, max(self._array_cap - 1,
                                                     0))] != 0)
        return torch.where(hit, slots, torch.full_like(slots, -1))

    def pull_readonly(self, keys: torch.Tensor) -> torch.Tensor:
        """keys int64 [n] -> dequantized fp32 rows [n, dim]; key -1 and an
        absent key give a zero row. One ``gather_lookup_q`` launch on a
        GPU (resolve and dequantize in the kernel)."""
        keys = keys.to(self.device, torch.int64).reshape(-1).contiguous()
        if self._hip:
            return self.ext.gather_lookup_q(self.slab, self.dim,
                                            self._fmt_id, keys,
                                            **self._table_args())
        slots = self._lookup_readonly(keys)
        hit = slots >= 0
        rows = ops.dequantize_rows(self.slab[slots.clamp(min=0)], self.dim,
                                   self.fmt)
        return torch.where(hit.unsqueeze(1), rows, torch.zeros_like(rows))

    def pull_pooled_readonly(self, values: torch.Tensor,
                             offsets: torch.Tensor, mode: str,
                             weights: torch.Tensor = None) -> torch.Tensor:
        """Read-only pooled pull over ragged bags, the contract of
        ``VariableShard.pull_pooled_readonly`` over dequantized rows: on a
        GPU one ``pool_lookup_q`` launch from keys to [B, dim]; on the CPU
        ``pull_readonly`` then the identity pool, which is the kernel's
        oracle (bit-identical)."""
        if mode not in ops.POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode!r}")
        if weights is not None:
            weights = weights.to(self.device, torch.float32).contiguous()
        values = values.to(self.device, torch.int64).contiguous()
        offsets = offsets.to(self.device, torch.int64).contiguous()
        if self._hip:
            return self.ext.pool_lookup_q(self.slab, self.dim, self._fmt_id,
                                          values, offsets,
                                          ops.POOL_MODES[mode], weights,
                                          **self._table_args())
        rows = self.pull_readonly(values)
        if weights is None:
            return ops.pool_fwd(rows, None, None, offsets, mode, False)[0]
        return ops.pool_fwd_weighted(rows, None, None, offsets, weights,
                                     mode)[0]

    def get_weights(self, keys: torch.Tensor) -> torch.Tensor:
        return self.pull_readonly(keys)

    # ------------------------------------------------------------- snapshot

    @property
    def num_rows(self) -> int:
        return self._nrows

    @property
    def nbytes(self) -> int:
        """Bytes of the slab plus the key map (hash: probe table and
        row -> key list; array: the valid bitmap). The CPU hash form counts
        its row -> key list only (the index is a Python dict)."""
        def size(t):
            return t.numel() * t.element_size()
        total = size(self.slab)
        if not self.meta.use_hash_table:
            return total + size(self.valid_u8)
        total += size(self.slot_keys)
        if self._hip:
            total += size(self.tk) + size(self.tv)
        return total

    def export_rows(self, include_state: bool = True
                    ) -> Tuple[torch.Tensor, torch.Tensor, None]:
        """(keys [n], dequantized fp32 rows [n, dim], None) in row order —
        what ``pull_readonly`` returns for those keys."""
        if self.meta.use_hash_table:
            n = self._nrows
            keys = self.slot_keys[:n].clone()
            packed = self.slab[:n]
        else:
            slots = (self.valid_u8 != 0).nonzero(as_tuple=True)[0]
            keys = slots * self.shard_num + self.shard_id
            packed = self.slab[slots]
        return keys, ops.dequantize_rows(packed, self.dim, self.fmt), None

    # -------------------------------------------------------------- removal

    def remove_rows(self, keys: torch.Tensor) -> torch.Tensor:
        """Remove the rows of ``keys`` (a delta's tombstones; unknown keys,
        duplicates and the reserved key -1 are ignored), with the layout
        rule of ``VariableShard.remove_rows``: a hash table moves its last
        rows into the holes, an array table clears the valid byte. On a GPU
        the expiry kernels of the training shards run over ``slab`` /
        ``slot_keys`` / ``tk`` / ``tv`` / ``nrows_dev`` in place; the CPU
        form is their oracle (equal slab bytes). Returns the removed keys,
        int64 on the shard's device, in ascending old-slot order."""
        keys = keys.to(self.device, torch.int64).reshape(-1).contiguous()
        if self.meta.use_hash_table:
            return self._remove_hashed(keys)
        # array table: keys of another shard or outside the vocabulary miss
        ok = ((keys >= 0) & (keys % self.shard_num == self.shard_id)
              & (keys // self.shard_num < self._array_cap))
        slots = torch.where(ok, keys // self.shard_num,
                            torch.full_like(keys, -1))
        if self._hip:
            dead = self.ext.flag_slots(slots, self._array_cap)
            gone = self.ext.remove_flagged_array(dead, self.valid_u8,
                                                 self.shard_num,
                                                 self.shard_id)
        else:
            slots = torch.unique(slots[ok])
            slots = slots[self.valid_u8[slots] != 0]
            self.valid_u8[slots] = 0
            gone = slots * self.shard_num + self.shard_id
        self._nrows -= int(gone.numel())
        return gone

    def _remove_hashed(self, keys: torch.Tensor) -> torch.Tensor:
        if self._hip:
            slots, _ = self.ext.ht_lookup(self.tk, self.tv, keys,
                                          self.nrows_dev, self.slot_keys,
                                          False, None)
            dead = self.ext.flag_slots(slots, self.slot_keys.numel())
            gone, n2 = self.ext.remove_flagged(
                dead, [self.slab, self.slot_keys], self.slot_keys, self.tk,
                self.tv, self.nrows_dev)
            self._nrows = int(n2)
            return gone
        idx = self._index
        dead = torch.zeros(self._nrows, dtype=torch.bool, device=self.device)
        dead[[idx[k] for k in keys.tolist() if k in idx]] = True
        dead_slots, holes, movers = hole_fill_plan(dead, self._nrows)
        gone = self.slot_keys[dead_slots]
        for k in gone.tolist():
            del idx[k]
        for k, h in zip(self.slot_keys[movers].tolist(), holes.tolist()):
            idx[k] = h
        self.slab[holes] = self.slab[movers]
        self.slot_keys[holes] = self.slot_keys[movers]
        self._nrows -= int(dead_slots.numel())
        return gone

    # ---------------------------------------------------------------- writes

    def _read_only(self, what: str):
        raise RuntimeError(f"QuantizedShard is read-only: {what} is not "
                           "supported (train on an fp32 shard and quantize "
                           "at load time)")

    def pull(self, keys):
        self._read_only("pull (which creates missing rows)")

    def push(self, keys, grads, counts):
        self._read_only("push")

    def update_weights(self):
        self._read_only("update_weights")

    def set_optimizer(self, category, **cfg):
        self._read_only("set_optimizer")

    def track_changes(self, enable: bool = True) -> None:
        if enable:
            raise NotImplementedError(
                "QuantizedShard does not train, so it has no changes to "
                "track: it receives deltas (import_rows), it cuts none")
