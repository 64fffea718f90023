"""The variable engine: one shard of one embedding variable.

This is the MI355X-native rebuild of the reference's L1/L2 layers
(openembedding/variable/EmbeddingTable.h, EmbeddingOptimizerVariable.h,
server/EmbeddingStorage.h) collapsed into a single per-rank object:

- shard owner of global key k is ``k % shard_num``; local index in array
  mode is ``k // shard_num`` (the reference's layout, EmbeddingShardFile.h:23-25,
  EmbeddingPullOperator.cpp:74-78 — kept for checkpoint compatibility);
- array table (bounded vocabulary) = dense [cap, dim] weights + valid bitmap
  (reference EmbeddingTable.h:171-180 EmbeddingArrayTable);
- hash table (vocabulary >= 2^63, i.e. the full uint64 key space) = open
  addressing key->row-slot over a growable row slab (reference
  EmbeddingHashTable over EmbeddingItemPool);
- rows are created lazily on first pull/update with a deterministic
  initializer (core/rng.py) and optimizer state train_init, matching the
  observable semantics of the reference's ``_new_weights`` side-table +
  commit-time merge (EmbeddingOptimizerVariable.h:242-297);
- gradients pushed for a batch are summed per unique key with occurrence
  counts; ``update_weights`` applies the optimizer once per touched key
  (reference MpscGradientReducer.h:30-53).

The torch backend below runs on CPU (tests, oracle) and on GPU tensors; the
HIP backend (openembedding_amd.ops) replaces the hot paths with fused CDNA4
kernels and is REQUIRED on ROCm devices — on a GPU box a missing extension
raises instead of silently falling back.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import torch

from .initializers import Initializer, make_initializer
from .optimizers import SparseOptimizer, make_optimizer

HASH_VOCAB_THRESHOLD = 1 << 63  # reference Meta.h:44-46 use_hash_table()


@dataclasses.dataclass
class VariableMeta:
    """Wire/JSON metadata (reference openembedding/variable/Meta.h:30-60)."""

    variable_id: int
    embedding_dim: int
    dtype: torch.dtype = torch.float32
    vocabulary_size: int = HASH_VOCAB_THRESHOLD

    @property
    def use_hash_table(self) -> bool:
        return self.vocabulary_size >= HASH_VOCAB_THRESHOLD

    def datatype_str(self) -> str:
        return {torch.float32: "float32", torch.float64: "float64"}[self.dtype]


def hole_fill_plan(dead: torch.Tensor, n: int):
    """The layout rule of a removal from a slab that is dense in [0, n):
    ``dead`` (bool, one per slot) flags the m rows that go. Returns
    (dead_slots, holes, movers), ascending: the holes are the dead slots
    below n' = n - m, the movers the surviving slots in [n', n); there are
    equally many, and the i-th mover's row goes to the i-th hole."""
    dead = dead[:n]
    dead_slots = dead.nonzero(as_tuple=True)[0]
    n2 = n - int(dead_slots.numel())
    holes = dead_slots[dead_slots < n2]
    surv = (~dead).nonzero(as_tuple=True)[0]
    return dead_slots, holes, surv[surv >= n2]


class VariableShard:
    """One rank's shard of one embedding variable (torch backend)."""

    GROW = 2
    # change tracking for delta checkpoints (track_changes); while it is off
    # no row_epoch tensor exists and no stamping runs
    _tracking = False

    def __init__(self, meta: VariableMeta, shard_id: int = 0, shard_num: int = 1,
                 device: str = "cpu", seed: int = 0):
        self.meta = meta
        self.shard_id = shard_id
        self.shard_num = shard_num
        self.device = torch.device(device)
        self.seed = seed ^ (meta.variable_id * 0x9E3779B97F4A7C15 & (1 << 63) - 1)
        self.dim = meta.embedding_dim
        self.dtype = meta.dtype

        self.optimizer: Optional[SparseOptimizer] = None
        self.initializer: Initializer = make_initializer("constant", value=0.0)
        self.state_dim = 0

        if meta.use_hash_table:
            self._index: Dict[int, int] = {}
            self._array_cap = 0
        else:
            # array table: local capacity covers keys k with k % shard_num == shard_id
            vocab = meta.vocabulary_size
            self._array_cap = (vocab - self.shard_id + self.shard_num - 1) // self.shard_num
            self._index = None
            self.valid = torch.zeros(self._array_cap, dtype=torch.bool,
                                     device=self.device)
            self.slot_key = None  # derived: slot s -> key s*shard_num+shard_id

        cap0 = self._array_cap if not meta.use_hash_table else 0
        self.weights = torch.zeros((cap0, self.dim), dtype=self.dtype,
                                   device=self.device)
        self.state = torch.zeros((cap0, 0), dtype=self.dtype, device=self.device)
        self._nrows = cap0 if not meta.use_hash_table else 0
        self._pending: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = []
        self._state_init_row: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ config

    def set_initializer(self, category: str, **cfg) -> None:
        self.initializer = make_initializer(category, **cfg)

    def set_optimizer(self, category: str, **cfg) -> None:
        """Install/replace the optimizer, keeping weights; state is rebuilt
        (reference live-reconfig semantics, EmbeddingVariable.cpp:29-60:
        state is migrated only when the optimizer category is unchanged)."""
        new_opt = make_optimizer(category, **cfg)
        keep_state = (self.optimizer is not None
                      and self.optimizer.category == category
                      and new_opt.state_dim(self.dim) == self.state_dim)
        self.optimizer = new_opt
        if not keep_state:
            self.state_dim = new_opt.state_dim(self.dim)
            self.state = torch.zeros((self.weights.shape[0], self.state_dim),
                                     dtype=self.dtype, device=self.device)
            if self.state_dim:
                # train_init state for every existing row
                if self.meta.use_hash_table:
                    if self._nrows:
                        new_opt.train_init(self.state[:self._nrows], self.dim)
                else:
                    if bool(self.valid.any()):
                        sl = self.valid.nonzero(as_tuple=True)[0]
                        s = self.state[sl]
                        new_opt.train_init(s, self.dim)
                        self.state[sl] = s
            if self._tracking:
                self._stamp_live()  # the state block of every row changed
        self._state_init_row = self._make_state_init_row()

    def _make_state_init_row(self) -> torch.Tensor:
        row = torch.zeros((1, self.state_dim), dtype=self.dtype, device=self.device)
        if self.optimizer is not None and self.state_dim:
            self.optimizer.train_init(row, self.dim)
        return row

    # ------------------------------------------------------------- row storage

    def _ensure_rows(self, need: int) -> None:
        cap = self.weights.shape[0]
        if need <= cap:
            return
        new_cap = max(need, max(1024, cap * self.GROW))
        w = torch.zeros((new_cap, self.dim), dtype=self.dtype, device=self.device)
        w[:cap] = self.weights
        self.weights = w
        s = torch.zeros((new_cap, self.state_dim), dtype=self.dtype,
                        device=self.device)
        s[:cap] = self.state
        self.state = s
        if self._tracking:
            self._grow_row_epoch(new_cap)

    def _lookup_or_insert(self, keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """keys: unique int64 global keys owned by this shard.
        Returns (slots int64 [n], new_mask bool [n]); creates rows for new keys
        (weights via initializer, state via train_init)."""
        if self.meta.use_hash_table:
            slots = torch.empty(keys.numel(), dtype=torch.int64)
            new_mask = torch.zeros(keys.numel(), dtype=torch.bool)
            idx = self._index
            nxt = self._nrows
            for i, k in enumerate(keys.tolist()):
                if k == -1:
                    # reserved: the hash table's empty marker — the
                    # reference reserves the same value (empty_key = -1,
                    # EmbeddingVariable.cpp:21). The GPU backend resolves
                    # it to a zero row; the CPU oracle fails loudly so the
                    # mistake surfaces in development.
                    raise ValueError(
                        "key -1 is reserved in hash mode (table empty "
                        "marker; same reservation as the reference)")
                s = idx.get(k)
                if s is None:
                    s = nxt
                    idx[k] = s
                    nxt += 1
                    new_mask[i] = True
                slots[i] = s
            slots = slots.to(self.device)
            new_mask = new_mask.to(self.device)
            if nxt != self._nrows:
                self._ensure_rows(nxt)
                self._nrows = nxt
        else:
            slots = keys // self.shard_num
            if keys.numel():
                bad = (keys % self.shard_num != self.shard_id)
                if bool(bad.any()):
                    raise ValueError("keys not owned by this shard")
                if bool((slots >= self._array_cap).any()) or bool((slots < 0).any()):
                    raise IndexError("key out of vocabulary range")
            new_mask = ~self.valid[slots]
            self.valid[slots] = True
        if bool(new_mask.any()):
            nk = keys[new_mask]
            ns = slots[new_mask]
            self.weights[ns] = self.initializer(self.seed, nk, self.dim, self.dtype)
            if self.state_dim:
                self.state[ns] = self._state_init_row.expand(ns.numel(), -1)
            if self._tracking:
                self.row_epoch[ns] = self._epoch
        return slots, new_mask

    def _lookup_readonly(self, keys: torch.Tensor) -> torch.Tensor:
        """Slots for existing keys; -1 for missing (read-only/serving path)."""
        if self.meta.use_hash_table:
            idx = self._index
            return torch.tensor([idx.get(k, -1) for k in keys.tolist()],
                                dtype=torch.int64, device=self.device)
        slots = keys // self.shard_num
        slots = torch.where(self.valid[slots.clamp(0, self._array_cap - 1)],
                            slots, torch.full_like(slots, -1))
        return slots

    # --------------------------------------------------------------- admission
    # A count-min filter in front of a hashed row's creation: a key earns its
    # row once it was seen ``min_count`` times. A sighting is one training
    # pull that contains the key and misses the table; keys reach a pull
    # unique, so this counts steps seen, not occurrences, and a layer called
    # twice in a step counts twice. Read-only pulls never count. Until a key
    # is admitted its slot is -1: the pull reads a zero row, its gradient is
    # dropped and nothing is created. The estimate only over-counts, so a key
    # is never admitted late, only sometimes early. With the filter on every
    # commit-time lookup is read-only (a push is no sighting), while
    # import_rows inserts unconditionally (a saved row was admitted once).
    # Removed rows keep their counters: an expired key comes back at its next
    # sighting unless the sketch was aged. Counters are int32 and never
    # saturate on their own; ``age_admission`` is what keeps an endless
    # stream from filling the sketch. This torch form is the CPU path and
    # the oracle of the HIP kernels.

    _admit: Optional[dict] = None  # settings while the filter is on

    def set_admission(self, min_count: Optional[int], width: int = 1 << 22,
                      depth: int = 4, seed: Optional[int] = None) -> None:
        """Turn the admission filter on, with an empty sketch of ``depth``
        rows of ``width`` int32 counters, or off (``min_count`` 0 or None;
        frees the sketch). ``seed`` defaults to the variable's. Setting the
        same width, depth and seed again keeps the counters."""
        if not min_count:
            self._admit = None
            for name in ("admit_sketch", "admit_stats"):
                self.__dict__.pop(name, None)
            return
        if not self.meta.use_hash_table:
            raise ValueError("admission needs a hash table: an array "
                             "table's rows are preallocated")
        min_count, width, depth = int(min_count), int(width), int(depth)
        if min_count < 1 or min_count >= 1 << 31:
            raise ValueError("min_count must be a positive int32")
        if width < 1 or width & (width - 1):
            raise ValueError("width must be a power of two")
        if not 1 <= depth <= 8:
            raise ValueError("depth must be in 1..8")
        seed = self.seed if seed is None else int(seed)
        seed = ((seed + (1 << 63)) % (1 << 64)) - (1 << 63)  # as int64
        old = self._admit
        self._admit = {"min_count": min_count, "width": width,
                       "depth": depth, "seed": seed}
        if old is not None and all(old[k] == self._admit[k]
                                   for k in ("width", "depth", "seed")):
            return
        self.admit_sketch = torch.zeros(depth * width, dtype=torch.int32,
                                        device=self.device)
        self.admit_stats = torch.zeros(2, dtype=torch.int64,
                                       device=self.device)

    def _need_admission(self) -> dict:
        if self._admit is None:
            raise RuntimeError("admission is off: call set_admission() first")
        return self._admit

    def age_admission(self, shift: int = 1) -> None:
        """Every counter ``>> shift``; ``shift >= 31`` empties the sketch."""
        from ..ops import dispatch as ops
        self._need_admission()
        ops.admit_age(self.admit_sketch, shift)

    def admission_stats(self) -> dict:
        """{min_count, width, depth, admitted, turned_away, fill}; fill is
        the share of nonzero counters. All zero while the filter is off."""
        a = self._admit
        if a is None:
            return {"min_count": 0, "width": 0, "depth": 0, "admitted": 0,
                    "turned_away": 0, "fill": 0.0}
        adm, away = self.admit_stats.tolist()
        fill = float((self.admit_sketch != 0).sum()) / self.admit_sketch.numel()
        return {"min_count": a["min_count"], "width": a["width"],
                "depth": a["depth"], "admitted": int(adm),
                "turned_away": int(away), "fill": fill}

    def export_admission(self) -> Optional[torch.Tensor]:
        """A copy of the sketch (int32 [depth * width]); None while off."""
        if self._admit is None:
            return None
        return self.admit_sketch.clone()

    def import_admission(self, sketch: torch.Tensor, add: bool = False
                         ) -> None:
        """Replace the sketch by ``sketch`` or, with ``add``, add to it
        element-wise (the sum of two sketches with equal hashes is the
        sketch of the joined stream)."""
        self._need_admission()
        sketch = sketch.to(self.device, torch.int32).reshape(-1)
        if sketch.numel() != self.admit_sketch.numel():
            raise ValueError("sketch does not hold depth * width counters")
        if add:
            self.admit_sketch += sketch
        else:
            self.admit_sketch.copy_(sketch)

    def _lookup_pull(self, keys: torch.Tensor, *bounded):
        """``_lookup_or_insert`` as a training pull reaches it: through the
        admission filter when that is on."""
        if self._admit is None:
            return self._lookup_or_insert(keys, *bounded)
        return self._lookup_admit(keys, *bounded)

    def _lookup_admit(self, keys: torch.Tensor):
        from ..ops import dispatch as ops
        a = self._admit
        if bool((keys == -1).any()):
            raise ValueError("key -1 is reserved in hash mode (table empty "
                             "marker; same reservation as the reference)")
        slots = self._lookup_readonly(keys)
        new_mask = torch.zeros(keys.numel(), dtype=torch.bool,
                               device=self.device)
        miss = (slots < 0).nonzero(as_tuple=True)[0]
        if miss.numel():
            est = ops.admit_note(self.admit_sketch, keys[miss], a["depth"],
                                 a["seed"])
            ok = miss[est >= a["min_count"]]
            if ok.numel():
                slots[ok], new_mask[ok] = self._lookup_or_insert(keys[ok])
            self.admit_stats[0] += ok.numel()
            self.admit_stats[1] += miss.numel() - ok.numel()
        return slots, new_mask

    # ---------------------------------------------------------------- training

    def pull(self, keys: torch.Tensor) -> torch.Tensor:
        """keys: unique int64 [n] owned by this shard -> weights [n, dim].
        Missing rows are created and initialized (reference
        EmbeddingOptimizerVariable.h:242-266). With an admission filter a
        key that has not earned its row yet reads as a zero row."""
        slots, _ = self._lookup_pull(keys)
        if self._admit is None:
            return self.weights[slots].clone()
        out = torch.zeros((keys.numel(), self.dim), dtype=self.dtype,
                          device=self.device)
        hit = slots >= 0
        out[hit] = self.weights[slots[hit]]
        return out

    def pull_readonly(self, keys: torch.Tensor) -> torch.Tensor:
        """Serving-mode pull: missing rows come back zero, table untouched
        (reference read_only get_weights path, EmbeddingPullOperator.cpp:179-181)."""
        slots = self._lookup_readonly(keys)
        out = torch.zeros((keys.numel(), self.dim), dtype=self.dtype,
                          device=self.device)
        hit = slots >= 0
        out[hit] = self.weights[slots[hit]]
        return out

    def pull_pooled_readonly(self, values: torch.Tensor,
                             offsets: torch.Tensor, mode: str,
                             weights: torch.Tensor = None) -> torch.Tensor:
        """Read-only pooled pull over ragged bags (inference / serving):
        values int64 [nnz_cap] keys (duplicates and the reserved key -1
        allowed), offsets int64 [B+1], mode "sum" | "mean" | "sqrtn",
        optional per-sample weights [nnz_cap] -> [B, dim]. A missing key is
        a zero row that still counts toward its bag's length; the table is
        untouched. This torch form — ``pull_readonly`` then the identity
        pool — is the CPU path and the oracle of the fused GPU kernel."""
        from ..ops import dispatch as ops
        rows = self.pull_readonly(values)
        if weights is None:
            return ops.pool_fwd(rows, None, None, offsets, mode, False)[0]
        return ops.pool_fwd_weighted(rows, None, None, offsets,
                                     weights.to(rows.dtype).contiguous(),
                                     mode)[0]

    def push(self, keys: torch.Tensor, grads: torch.Tensor,
             counts: torch.Tensor) -> None:
        """Queue a pre-aggregated gradient block (keys unique within block,
        grads summed, counts = occurrence counts). Reference
        MpscGradientReducer.h:26-29 push side."""
        self._pending.append((keys, grads, counts))

    def update_weights(self) -> None:
        """Commit the batch: merge pending blocks by key, apply the optimizer
        once per unique key (reference EmbeddingOptimizerVariable.h:273-297)."""
        if not self._pending:
            return
        if self.optimizer is None:
            raise RuntimeError("update_weights called before set_optimizer")
        if len(self._pending) == 1:
            keys, grads, counts = self._pending[0]
        else:
            keys = torch.cat([b[0] for b in self._pending])
            grads = torch.cat([b[1] for b in self._pending])
            counts = torch.cat([b[2] for b in self._pending])
            uk, inv = torch.unique(keys, return_inverse=True)
            g = torch.zeros((uk.numel(), self.dim), dtype=grads.dtype,
                            device=self.device)
            g.index_add_(0, inv, grads)
            c = torch.zeros(uk.numel(), dtype=counts.dtype, device=self.device)
            c.index_add_(0, inv, counts)
            keys, grads, counts = uk, g, c
        self._pending = []
        if self._admit is None:
            slots, _ = self._lookup_or_insert(keys)
        else:
            # a push is no sighting: a key without a row is dropped
            slots = self._lookup_readonly(keys)
            hit = slots >= 0
            keys, grads, counts, slots = (keys[hit], grads[hit], counts[hit],
                                          slots[hit])
        w = self.weights[slots]
        s = self.state[slots]
        self.optimizer.update(w, s, counts, grads)
        self.weights[slots] = w
        self.state[slots] = s
        if self._tracking:
            self.row_epoch[slots] = self._epoch

    # ------------------------------------------------------------- checkpoint

    @property
    def num_rows(self) -> int:
        if self.meta.use_hash_table:
            return self._nrows
        return int(self.valid.sum())

    def export_rows(self, include_state: bool = True
                    ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """All materialized rows: (keys [n], weights [n,dim], state [n,sd] or None).
        Keys come back in stable (slot) order."""
        if self.meta.use_hash_table:
            items = sorted(self._index.items(), key=lambda kv: kv[1])
            keys = torch.tensor([k for k, _ in items], dtype=torch.int64,
                                device=self.device)
            slots = torch.tensor([s for _, s in items], dtype=torch.int64,
                                 device=self.device)
        else:
            slots = self.valid.nonzero(as_tuple=True)[0]
            keys = slots * self.shard_num + self.shard_id
        w = self.weights[slots].clone()
        s = self.state[slots].clone() if (include_state and self.state_dim) else None
        return keys, w, s

    def import_rows(self, keys: torch.Tensor, weights: torch.Tensor,
                    state: Optional[torch.Tensor] = None) -> None:
        """Bulk set rows (load path). State==None leaves state at train_init
        (reference load with include_optimizer=false)."""
        slots, _ = self._lookup_or_insert(keys)
        self.weights[slots] = weights.to(self.device, self.dtype)
        if state is not None and self.state_dim:
            self.state[slots] = state.to(self.device, self.dtype)
        if self._tracking:
            self.row_epoch[slots] = self._epoch

    def get_weights(self, keys: torch.Tensor) -> torch.Tensor:
        return self.pull_readonly(keys)

    def clear(self) -> None:
        """Drop all rows (reference clear_weights, used before load)."""
        if self.meta.use_hash_table:
            self._index = {}
            self._nrows = 0
            self.weights = torch.zeros((0, self.dim), dtype=self.dtype,
                                       device=self.device)
            self.state = torch.zeros((0, self.state_dim), dtype=self.dtype,
                                     device=self.device)
            if self._tracking:
                self.row_epoch = self.row_epoch.new_zeros(0)
        else:
            self.valid.zero_()
            self.weights.zero_()
            self.state.zero_()
            if self._tracking:
                self.row_epoch.zero_()

    # ------------------------------------------------------------- row expiry
    # Removal of rows in place. ``expire_rows`` drops the rows last written
    # before an epoch, ``remove_rows`` the rows of named keys (a delta's
    # tombstones). A hash table fills its holes: with n live rows of which m
    # are dead and n' = n - m, the holes are the dead slots < n' and the
    # movers the surviving slots in [n', n), both ascending; the i-th mover's
    # row (weights, state, key, stamp) moves to the i-th hole, every other
    # survivor keeps its slot and the live count becomes n'. Slots >= n' are
    # dead storage that nothing zeroes. An array table clears the valid bit;
    # nothing moves. A removed key misses afterwards, and a later training
    # pull re-creates it through the ordinary lazy init, which is
    # deterministic in (seed, key). This torch form is the CPU path and the
    # oracle of the HIP kernels.

    def expire_rows(self, before: int) -> torch.Tensor:
        """Remove every live row with ``row_epoch < before`` (tracking only;
        in training every pulled row is written at commit, so the stamp is
        also "last seen"). Stamps zeroed by ``set_epoch(reset=True)`` are
        the oldest: after a base was loaded, every row it brought expires
        under any ``before >= 1`` until it is written again. Returns the
        removed keys, int64 on the shard's device, in ascending old-slot
        order, and logs them for the next delta."""
        self._need_tracking()
        self._check_removable()
        return self._log_removed(self._remove_flagged(
            self._flags_expired(int(before))))

    def remove_rows(self, keys: torch.Tensor) -> torch.Tensor:
        """Remove the rows of ``keys`` (int64; unknown keys, duplicates and
        the reserved key -1 are ignored). Works without tracking. Returns
        the removed keys like ``expire_rows``."""
        self._check_removable()
        keys = keys.to(self.device, torch.int64).reshape(-1).contiguous()
        return self._log_removed(self._remove_flagged(
            self._flags_named(keys)))

    def _check_removable(self) -> None:
        if self._pending or getattr(self, "_pending_bounded", None):
            raise RuntimeError(
                "rows cannot be removed while gradient blocks are queued "
                "(their saved slots would go stale): call update_weights() "
                "first")

    def _owned_slots_readonly(self, keys: torch.Tensor) -> torch.Tensor:
        """``_lookup_readonly`` that also misses, in array mode, on keys
        this shard does not own or that lie outside the vocabulary."""
        if self.meta.use_hash_table:
            return self._lookup_readonly(keys)
        ok = ((keys >= 0) & (keys % self.shard_num == self.shard_id)
              & (keys // self.shard_num < self._array_cap))
        slots = self._lookup_readonly(torch.where(
            ok, keys, torch.full_like(keys, self.shard_id)))
        return torch.where(ok, slots, torch.full_like(slots, -1))

    def _live_mask(self) -> torch.Tensor:
        if not self.meta.use_hash_table:
            return self.valid.clone()
        live = torch.zeros(self.weights.shape[0], dtype=torch.bool,
                           device=self.device)
        live[:self._nrows] = True
        return live

    def _flags_expired(self, before: int) -> torch.Tensor:
        return self._live_mask() & (self.row_epoch < before)

    def _flags_named(self, keys: torch.Tensor) -> torch.Tensor:
        dead = torch.zeros(self.weights.shape[0], dtype=torch.bool,
                           device=self.device)
        slots = self._owned_slots_readonly(keys)
        dead[slots[slots >= 0]] = True
        return dead

    def _remove_flagged(self, dead: torch.Tensor) -> torch.Tensor:
        """Remove the live rows flagged in ``dead`` (bool, one per slot)."""
        if not self.meta.use_hash_table:
            dead_slots = dead.nonzero(as_tuple=True)[0]
            self.valid[dead_slots] = False
            return dead_slots * self.shard_num + self.shard_id
        dead_slots, holes, movers = hole_fill_plan(dead, self._nrows)
        if dead_slots.numel() == 0:
            return dead_slots
        sk = self._slot_key_list()
        removed = sk[dead_slots]
        planes = [self.weights, self.state]
        if self._tracking:
            planes.append(self.row_epoch)
        for p in planes:
            p[holes] = p[movers]
        idx = self._index
        for k in removed.tolist():
            del idx[k]
        for k, h in zip(sk[movers].tolist(), holes.tolist()):
            idx[k] = h
        self._nrows -= int(dead_slots.numel())
        return removed

    # removal log: (epoch, removed keys) entries, kept while tracking is on
    # and written by checkpoint.dump_delta as the delta's tombstones

    def _log_removed(self, keys: torch.Tensor) -> torch.Tensor:
        if self._tracking and keys.numel():
            self.__dict__.setdefault("_removed_log", []).append(
                (self._epoch, keys))
        return keys

    def removed_since(self, since: int) -> torch.Tensor:
        """The logged removed keys of the epochs ``>= since`` (int64; a key
        removed twice occurs twice)."""
        ks = [k for e, k in self.__dict__.get("_removed_log", ())
              if e >= int(since)]
        if not ks:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        return torch.cat(ks)

    def prune_removed(self) -> bool:
        """Forget the removal log; True if that dropped any entry."""
        return bool(self.__dict__.pop("_removed_log", None))

    # -------------------------------------------------------- change tracking
    # Delta checkpoints (checkpoint.dump_delta): ``row_epoch[slot]`` is the
    # epoch of the row's last write and ``epoch`` the current one. A row is
    # stamped when a lookup-or-insert creates it, when update_weights applies
    # the optimizer to it, when import_rows writes it and when set_optimizer
    # rebuilds the state block; reads stamp nothing. A delta is the rows with
    # ``row_epoch >= since`` plus the keys removed since then (the removal
    # log above). This torch form is the CPU path and the oracle of the HIP
    # kernels.

    def track_changes(self, enable: bool = True) -> None:
        """Turn change tracking on (row_epoch zeroed, epoch 1) or off (the
        tensors are dropped). Turning it on twice keeps the stamps."""
        if not enable:
            self._tracking = False
            for name in ("row_epoch", "epoch_dev", "_epoch", "_removed_log"):
                if name in self.__dict__:
                    delattr(self, name)
            return
        if self._tracking:
            return
        self.row_epoch = torch.zeros(self.weights.shape[0],
                                     dtype=torch.int32, device=self.device)
        self._epoch = 1
        self._tracking = True

    @property
    def tracking(self) -> bool:
        return self._tracking

    @property
    def epoch(self) -> int:
        """The epoch that writes are stamped with (tracking only)."""
        self._need_tracking()
        return self._epoch

    def set_epoch(self, epoch: int, reset: bool = False) -> None:
        """Move to ``epoch``; ``reset`` also forgets every stamp (after a
        base was loaded, so that the next delta does not re-emit it)."""
        self._need_tracking()
        if reset:
            self.row_epoch.zero_()
        self._epoch = int(epoch)

    def _need_tracking(self) -> None:
        if not self._tracking:
            raise RuntimeError("change tracking is off: call "
                               "track_changes() first")

    def _grow_row_epoch(self, new_cap: int) -> None:
        old = self.row_epoch
        self.row_epoch = old.new_zeros(new_cap)
        self.row_epoch[:old.numel()] = old

    def _stamp_live(self) -> None:
        if self.meta.use_hash_table:
            self.row_epoch[:self._nrows] = self._epoch
        else:
            self.row_epoch[self.valid] = self._epoch

    def _slot_key_list(self) -> torch.Tensor:
        """slot -> key of the hash table's rows."""
        sk = torch.empty(self._nrows, dtype=torch.int64)
        if self._index:
            ks = torch.tensor(list(self._index.keys()), dtype=torch.int64)
            vs = torch.tensor(list(self._index.values()), dtype=torch.int64)
            sk[vs] = ks
        return sk.to(self.device)

    def select_changed(self, since: int) -> Tuple[torch.Tensor, int]:
        """(slots, n): the live rows with ``row_epoch >= since`` in
        ascending slot order. ``slots`` may be longer than ``n``."""
        self._need_tracking()
        if self.meta.use_hash_table:
            live = torch.zeros(self.row_epoch.numel(), dtype=torch.bool,
                               device=self.device)
            live[:self._nrows] = True
        else:
            live = self.valid
        slots = (live & (self.row_epoch >= int(since))).nonzero(
            as_tuple=True)[0]
        return slots, int(slots.numel())

    def export_changed(self, since: int, include_state: bool = True,
                       selection=None):
        """Yield the rows changed since epoch ``since`` as ``(keys, weights,
        state or None)`` blocks of at most ``checkpoint.BLOCK_ROWS`` rows, in
        ascending slot order. A block is valid until the next one is asked
        for. ``selection`` is a ``select_changed(since)`` result to reuse."""
        from .. import checkpoint
        slots, n = selection if selection is not None \
            else self.select_changed(since)
        want_state = bool(include_state and self.state_dim)
        sk = self._slot_key_list() if self.meta.use_hash_table else None
        step = int(checkpoint.BLOCK_ROWS)
        for start in range(0, n, step):
            sl = slots[start:min(start + step, n)]
            keys = sk[sl] if sk is not None \
                else sl * self.shard_num + self.shard_id
            yield (keys, self.weights[sl].clone(),
                   self.state[sl].clone() if want_state else None)
