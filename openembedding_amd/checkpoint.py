"""Checkpoint dump/load — the reference's portable model format, rebuilt.

Logical layout parity with the reference (SURVEY.md §3.4, §5 Checkpoint):
  <uri>/model_meta                        JSON: sign, variables, version "0.2"
        (reference Model.cpp:89-108, Meta.h:105-145)
  <uri>/<storage_ordinal>/model_<rank>_0  binary shard file: per variable a
        JSON header + blocks of {n, indices[n], weights[n*dim],
        states[n*state_dim]} (reference EmbeddingDumpOperator.cpp:57-96,
        EmbeddingShardFile.h:13-26)

Differences from the reference, by design:
  - keys are stored GLOBAL (the reference stores shard-local indices and
    re-globalizes on load via idx*shard_num+shard_id,
    EmbeddingShardFile.h:23-25); global keys make the file shard-count
    independent by construction — load re-shards by key % world_size exactly
    like the reference's init-push path (EmbeddingLoadOperator.cpp:58-111);
  - serialization is plain little-endian numpy buffers with a JSON header
    (the reference's BinaryArchive lives in the absent pico-core submodule,
    so its byte format is not reproducible, only its structure).

Every rank writes its own shard file (collective dump); load is collective,
each rank reads all files and keeps its own keys.

Delta checkpoints (no reference file format; the reference's incremental
checkpoint was its PMem PersistManager): with change tracking on
(``shard.track_changes``), ``dump_delta`` writes, in the same layout and
section format, only the rows changed since an epoch, and ``apply_delta``
upserts them on top of a loaded base. The meta of a tracked full dump gains
``epoch`` and ``model_uuid``; a delta's meta gains
``"delta": {since, epoch, model_uuid}`` and its section headers
``"delta": true``. Rows removed since that epoch (``expire_rows``, or a
shard's ``remove_rows``) travel as tombstones: per storage and rank that has
any, a file ``removed_<rank>`` of sections {header with ``"removed": true``,
blocks of {n, keys[n]}}. ``apply_delta`` removes first and upserts second,
so a key that expired and came back inside the interval survives.

Admission filters (``shard.set_admission``): every section header records the
variable's ``"admission": {min_count, width, depth, seed}`` (absent while
off), and a full dump writes, per storage and rank that has any, a file
``admission_<rank>`` of sections {header with ``"admission"``, ``shard_id``,
``shard_num`` and ``num_counters``, then the raw little-endian int32 sketch}.
A delta writes no such file. ``load_model`` restores settings and sketch
exactly at the saved shard count; at another one every shard loads the
element-wise sum of the saved sketches, which is the sketch of the joined
stream: it over-counts, so no id is admitted later than it would have been.
"""

from __future__ import annotations

import json
import os
import struct
import warnings
from typing import Optional

import numpy as np
import torch

MAGIC = b"OEAMDSH1"
BLOCK_ROWS = 1 << 16  # rows per block (~ the reference's ~1MiB batching,
                      # EmbeddingVariable.cpp:84-87)


def _var_header(var, include_optimizer: bool) -> dict:
    shard = var.shard
    return {
        "variable_id": shard.meta.variable_id,
        "datatype": shard.meta.datatype_str(),
        "embedding_dim": shard.dim,
        "vocabulary_size": shard.meta.vocabulary_size,
        "state_dim": shard.state_dim if include_optimizer else 0,
        "optimizer": ({"category": shard.optimizer.category,
                       **shard.optimizer.dump_config()}
                      if (include_optimizer and shard.optimizer) else None),
        "initializer": {"category": shard.initializer.category,
                        **shard.initializer.dump_config()},
        "shard_id": shard.shard_id,
        "shard_num": shard.shard_num,
        # "admission" only while a filter is on: without one a header is
        # byte for byte what it was before admission existed
        **({"admission": _admission_cfg(shard)}
           if _admission_cfg(shard) is not None else {}),
    }


def _admission_cfg(shard) -> Optional[dict]:
    a = getattr(shard, "_admit", None)
    return dict(a) if a is not None else None


def _shards(ctx):
    return [var.shard for st in ctx.storages for var in st.variables]


def tracked_epoch(ctx) -> Optional[int]:
    """The change-tracking epoch of a context: None when no variable is
    tracked; otherwise every variable must be, all at the same epoch (they
    advance together, at every dump)."""
    shards = _shards(ctx)
    on = [sh for sh in shards if getattr(sh, "tracking", False)]
    if not on:
        return None
    if len(on) != len(shards):
        raise RuntimeError("change tracking is on for some variables only; "
                           "track all of them or none")
    epochs = {sh.epoch for sh in on}
    if len(epochs) != 1:
        raise RuntimeError(f"tracked variables disagree on the epoch: "
                           f"{sorted(epochs)}")
    return epochs.pop()


def _advance(ctx, epoch: int, reset: bool = False) -> None:
    for sh in _shards(ctx):
        if getattr(sh, "tracking", False):
            sh.set_epoch(epoch, reset=reset)


def dump_model(ctx, uri: str, include_optimizer: bool = True) -> None:
    """Collective: every rank writes its shard of every storage. With
    change tracking on, the meta also records the dump's ``epoch`` and the
    ``model_uuid`` (the base of a delta chain), the epoch advances and the
    removal log is pruned."""
    meta = _model_meta(ctx)
    epoch = tracked_epoch(ctx)
    if epoch is not None:
        meta["epoch"] = epoch
        meta["model_uuid"] = ctx.model_uuid
    _write_dump(ctx, uri, meta, include_optimizer, None)
    _write_admission(ctx, uri)
    if epoch is not None:
        _advance(ctx, epoch + 1)
        # a full dump is a state any consumer can reload: the removals
        # before it need not be kept for later deltas
        _prune_removed(ctx, epoch + 1)


def dump_delta(ctx, uri: str, include_optimizer: bool = True,
               since: Optional[int] = None) -> dict:
    """Collective: write only the rows changed since epoch ``since`` (default:
    since the last dump of either kind, which chains the deltas; an explicit
    earlier ``since`` serves a consumer that is further behind). Same layout
    and shard-file format as ``dump_model``, so ``iter_blocks`` reads it;
    the meta carries ``"delta": {since, epoch, model_uuid}``. The keys
    removed since ``since`` are written as tombstones (``removed_<rank>``
    files, read by ``iter_removed``); a delta without removals has none. An
    explicit ``since`` below the epoch at which a full dump or a load pruned
    logged removals raises ValueError: those removals are gone, so the
    consumer has to reload the base. Returns ``{"since", "epoch", "rows"}``
    (rows of this rank)."""
    epoch = tracked_epoch(ctx)
    if epoch is None:
        raise RuntimeError("dump_delta needs change tracking: call "
                           "track_server_model_changes() (or set "
                           "server.track_changes) before training")
    since = epoch if since is None else int(since)
    if since < 1 or since > epoch:
        raise ValueError(f"since must be in [1, {epoch}], got {since}")
    pruned = getattr(ctx, "removals_pruned_epoch", None)
    if pruned is not None and since < pruned:
        raise ValueError(
            f"since={since} reaches below epoch {pruned}, where a full dump "
            "or a load pruned the log of removed rows: a delta from there "
            "would miss removals. Reload the base (the latest full dump) "
            f"and ask for deltas with since >= {pruned}")
    meta = _model_meta(ctx)
    meta["delta"] = {"since": since, "epoch": epoch,
                     "model_uuid": ctx.model_uuid}
    rows = _write_dump(ctx, uri, meta, include_optimizer, since)
    _write_removed(ctx, uri, since)
    _advance(ctx, epoch + 1)
    return {"since": since, "epoch": epoch, "rows": rows}


def expire_rows(ctx, max_age: Optional[int] = None,
                before: Optional[int] = None) -> dict:
    """Every rank calls it (no communication): remove, from every variable,
    the rows last written before epoch ``before`` (default: the current
    epoch minus ``max_age``; exactly one of the two is given). Needs a
    tracked context. The removed keys are logged and written as tombstones
    by the next ``dump_delta``. Returns ``{"before", "rows"}`` (rows removed
    on this rank)."""
    if (max_age is None) == (before is None):
        raise ValueError("give exactly one of max_age and before")
    epoch = tracked_epoch(ctx)
    if epoch is None:
        raise RuntimeError("expire_rows needs change tracking: call "
                           "track_server_model_changes() (or set "
                           "server.track_changes) before training")
    before = epoch - int(max_age) if before is None else int(before)
    rows = 0
    for sh in _shards(ctx):
        rows += int(sh.expire_rows(before).numel())
    return {"before": before, "rows": rows}


def _prune_removed(ctx, epoch: int, reset: bool = False) -> None:
    """Forget every shard's removal log; if any rank dropped entries,
    remember ``epoch`` as the lowest ``since`` a delta can still serve.
    ``reset`` (a load: the epochs start over) forgets an earlier mark."""
    dropped = False
    for sh in _shards(ctx):
        if getattr(sh, "tracking", False):
            dropped = sh.prune_removed() or dropped
    if ctx.world_size > 1 and torch.distributed.is_initialized():
        box = [None] * ctx.world_size
        torch.distributed.all_gather_object(box, dropped)
        dropped = any(box)
    if dropped:
        ctx.removals_pruned_epoch = int(epoch)
    elif reset:
        ctx.removals_pruned_epoch = None


def _write_removed(ctx, uri: str, since: int) -> None:
    """The tombstones of a delta: ``<storage>/removed_<rank>`` with one
    section per variable that has removals logged at epochs >= since."""
    for st in ctx.storages:
        f = None
        try:
            for var in st.variables:
                sh = var.shard
                if not getattr(sh, "tracking", False):
                    continue
                keys = sh.removed_since(since)
                n = int(keys.numel())
                if not n:
                    continue
                if f is None:
                    f = open(os.path.join(uri, str(st.storage_id),
                                          f"removed_{ctx.rank}"), "wb")
                _write_header(f, {"variable_id": sh.meta.variable_id,
                                  "num_items": n, "removed": True})
                keys = keys.cpu().numpy().astype("<i8")
                for start in range(0, n, BLOCK_ROWS):
                    blk = keys[start:start + BLOCK_ROWS]
                    f.write(struct.pack("<q", int(blk.size)))
                    f.write(blk.tobytes())
                f.write(struct.pack("<q", -1))
        finally:
            if f is not None:
                f.close()
    ctx.barrier()


def _write_admission(ctx, uri: str) -> None:
    """The admission sketches of a full dump: ``<storage>/admission_<rank>``
    with one section per variable whose filter is on."""
    for st in ctx.storages:
        f = None
        try:
            for var in st.variables:
                sh = var.shard
                cfg = _admission_cfg(sh)
                if cfg is None:
                    continue
                sketch = sh.export_admission().cpu().numpy().astype("<i4")
                if f is None:
                    f = open(os.path.join(uri, str(st.storage_id),
                                          f"admission_{ctx.rank}"), "wb")
                _write_header(f, {"variable_id": sh.meta.variable_id,
                                  "admission": cfg, "shard_id": sh.shard_id,
                                  "shard_num": sh.shard_num,
                                  "num_counters": int(sketch.size)})
                f.write(sketch.tobytes())
        finally:
            if f is not None:
                f.close()
    ctx.barrier()


def iter_admission(uri: str, meta: Optional[dict] = None):
    """Stream the admission sketches of a full dump: yields (header_dict,
    sketch <i4 [depth * width]) per section of every ``admission_<rank>``
    file. Nothing for a dump without them."""
    meta = meta or read_meta(uri)
    for st_ord in range(meta["num_storages"]):
        d = os.path.join(uri, str(st_ord))
        for fname in sorted(os.listdir(d)):
            if not fname.startswith("admission_"):
                continue
            with open(os.path.join(d, fname), "rb") as f:
                while True:
                    magic = f.read(8)
                    if not magic:
                        break
                    if magic != MAGIC:
                        raise RuntimeError(f"bad admission file {fname}")
                    (hlen,) = struct.unpack("<q", f.read(8))
                    hdr = json.loads(f.read(hlen))
                    yield hdr, np.frombuffer(
                        f.read(hdr["num_counters"] * 4), dtype="<i4")


def _load_admission(ctx, uri: str, meta: dict, by_id: dict) -> None:
    """Restore the admission filters of a full dump (module docstring). A
    dump without admission files leaves every filter as it is."""
    saved = {}
    for hdr, sketch in iter_admission(uri, meta):
        if hdr["variable_id"] in by_id:
            saved.setdefault(hdr["variable_id"], []).append((hdr, sketch))
    for vid, parts in saved.items():
        shard = by_id[vid].shard
        if getattr(shard, "set_admission", None) is None:
            continue   # a read-only table: a miss is a zero row already
        cfg = parts[0][0]["admission"]
        geometry = {tuple(h["admission"][k] for k in ("width", "depth",
                                                      "seed"))
                    for h, _ in parts}
        try:
            shard.set_admission(**cfg)
        except NotImplementedError as e:
            warnings.warn(f"variable {vid}: admission filter of the dump "
                          f"not restored ({e})")
            continue
        mine = [sk for h, sk in parts
                if h["shard_num"] == shard.shard_num
                and h["shard_id"] == shard.shard_id]
        if len(mine) == 1 and len(parts) == shard.shard_num:
            shard.import_admission(torch.from_numpy(mine[0].copy()))
        elif len(geometry) == 1:
            total = np.zeros(parts[0][1].size, dtype=np.int64)
            for _, sk in parts:
                total += sk
            total = np.minimum(total, np.iinfo(np.int32).max).astype("<i4")
            shard.import_admission(torch.from_numpy(total))
        else:
            warnings.warn(f"variable {vid}: the dump's admission sketches "
                          "differ in width, depth or seed and cannot be "
                          "summed; the filter starts empty")
            shard.age_admission(31)


def _model_meta(ctx) -> dict:
    meta = {
        "model_sign": f"{ctx.model_uuid}-{ctx.model_version}",
        "version": "0.2",
        "num_storages": len(ctx.storages),
        "world_size": ctx.world_size,
        "variables": [],
    }
    for st in ctx.storages:
        for var in st.variables:
            meta["variables"].append({
                "variable_id": var.shard.meta.variable_id,
                "storage_ordinal": st.storage_id,
                # reference ModelVariableMeta field (Meta.h:77-99): with it
                # present, this JSON is a superset of the reference's
                # ModelOfflineMeta schema (model_sign + variables[datatype,
                # embedding_dim, vocabulary_size, storage_name] + version)
                "storage_name": str(st.storage_id),
                "datatype": var.shard.meta.datatype_str(),
                "embedding_dim": var.shard.dim,
                "vocabulary_size": var.shard.meta.vocabulary_size,
            })
    return meta


def _write_dump(ctx, uri: str, meta: dict, include_optimizer: bool,
                since: Optional[int]) -> int:
    """The files of a full dump (``since`` None) or of a delta; returns the
    number of rows this rank wrote."""
    rank = ctx.rank
    rows = 0
    if rank == 0:
        os.makedirs(uri, exist_ok=True)
        for st in ctx.storages:
            os.makedirs(os.path.join(uri, str(st.storage_id)), exist_ok=True)
        with open(os.path.join(uri, "model_meta"), "w") as f:
            json.dump(meta, f, indent=1)
    ctx.barrier()
    # files per rank: the reference's server.server_dump_files knob
    # (EnvConfig.cpp; files named model_{node}_{file_id},
    # EmbeddingDumpOperator.cpp:28). Rows round-robin across files so big
    # shards split for parallel HDFS-style upload.
    n_files = max(1, getattr(ctx.config.server, "server_dump_files", 1)
                  if getattr(ctx, "config", None) else 1)
    for st in ctx.storages:
        files = [open(os.path.join(uri, str(st.storage_id),
                                   f"model_{rank}_{i}"), "wb")
                 for i in range(n_files)]
        try:
            for j, var in enumerate(st.variables):
                if since is None:
                    rows += _dump_variable(files[j % n_files], var,
                                           include_optimizer)
                else:
                    rows += _dump_variable_delta(files[j % n_files], var,
                                                 include_optimizer, since)
        finally:
            for f in files:
                f.close()
    ctx.barrier()
    return rows


def _write_header(f, hdr: dict) -> None:
    hjson = json.dumps(hdr).encode()
    f.write(MAGIC)
    f.write(struct.pack("<q", len(hjson)))
    f.write(hjson)


def _dump_variable_delta(f, var, include_optimizer: bool, since: int) -> int:
    """One variable's section of a delta: the full-dump section format with
    ``"delta": true`` in the header, rows streamed block by block from
    ``export_changed`` (never a copy of the table)."""
    shard = var.shard
    want_state = bool(include_optimizer and shard.state_dim)
    sel = shard.select_changed(since)
    n = int(sel[1])   # the one host read of the changed-row count
    hdr = _var_header(var, want_state)
    hdr["num_items"] = n
    hdr["delta"] = True
    _write_header(f, hdr)
    for keys, w, s in shard.export_changed(since, include_state=want_state,
                                           selection=(sel[0], n)):
        f.write(struct.pack("<q", int(keys.numel())))
        f.write(keys.cpu().numpy().astype("<i8").tobytes())
        f.write(w.cpu().numpy().astype("<f4").tobytes())
        if want_state:
            f.write(s.cpu().numpy().astype("<f4").tobytes())
    if n == 0:
        f.write(struct.pack("<q", 0))
    f.write(struct.pack("<q", -1))  # end of variable section
    return n


def _dump_variable(f, var, include_optimizer: bool) -> int:
    keys, w, s = var.shard.export_rows(include_state=include_optimizer)
    hdr = _var_header(var, include_optimizer and s is not None)
    hdr["num_items"] = int(keys.numel())
    _write_header(f, hdr)
    n = keys.numel()
    sd = hdr["state_dim"]
    for start in range(0, max(n, 1), BLOCK_ROWS):
        if n == 0:
            f.write(struct.pack("<q", 0))
            break
        stop = min(start + BLOCK_ROWS, n)
        blk = stop - start
        f.write(struct.pack("<q", blk))
        f.write(keys[start:stop].cpu().numpy().astype("<i8").tobytes())
        f.write(w[start:stop].cpu().numpy().astype("<f4").tobytes())
        if sd:
            f.write(s[start:stop].cpu().numpy().astype("<f4").tobytes())
    f.write(struct.pack("<q", -1))  # end of variable section
    return int(n)


def _apply_config(var, hdr: dict) -> None:
    """Restore the variable's initializer/optimizer config from the shard
    header (the reference ships init_config with variable creation and
    re-applies it on load, EmbeddingInitOperator.cpp:138-168)."""
    init = hdr.get("initializer")
    if init:
        c = dict(init)
        cat = c.pop("category")
        var.shard.set_initializer(cat, **c)
    opt = hdr.get("optimizer")
    if opt:
        c = dict(opt)
        cat = c.pop("category")
        cur = var.shard.optimizer
        if cur is None or cur.category != cat or cur.dump_config() != c:
            var.shard.set_optimizer(cat, **c)
    adm = hdr.get("admission")
    if adm and getattr(var.shard, "set_admission", None) is not None:
        try:
            var.shard.set_admission(**adm)   # keeps counters of equal shape
        except NotImplementedError as e:
            warnings.warn(f"variable {hdr['variable_id']}: admission filter "
                          f"of the dump not restored ({e})")


def read_meta(uri: str) -> dict:
    with open(os.path.join(uri, "model_meta")) as f:
        return json.load(f)


def iter_blocks(uri: str, meta: Optional[dict] = None):
    """Stream every shard file of a dump: yields (header_dict, keys <i8 [n],
    weights <f4 [n,dim], states <f4 [n,sd] or None) per block. The streaming
    analogue of the reference's EmbeddingLoadOperator generate_push_items
    (EmbeddingLoadOperator.cpp:58-111)."""
    meta = meta or read_meta(uri)
    for st_ord in range(meta["num_storages"]):
        d = os.path.join(uri, str(st_ord))
        for fname in sorted(os.listdir(d)):
            if not fname.startswith("model_"):
                continue
            with open(os.path.join(d, fname), "rb") as f:
                while True:
                    magic = f.read(8)
                    if not magic:
                        break
                    if magic != MAGIC:
                        raise RuntimeError(f"bad shard file {fname}")
                    (hlen,) = struct.unpack("<q", f.read(8))
                    hdr = json.loads(f.read(hlen))
                    dim = hdr["embedding_dim"]
                    sd = hdr["state_dim"]
                    while True:
                        (blk,) = struct.unpack("<q", f.read(8))
                        if blk <= 0:
                            if blk == 0:
                                (end,) = struct.unpack("<q", f.read(8))
                                assert end == -1
                            break
                        keys = np.frombuffer(f.read(blk * 8), dtype="<i8")
                        w = np.frombuffer(f.read(blk * dim * 4),
                                          dtype="<f4").reshape(blk, dim)
                        s = None
                        if sd:
                            s = np.frombuffer(f.read(blk * sd * 4),
                                              dtype="<f4").reshape(blk, sd)
                        yield hdr, keys, w, s


def iter_removed(uri: str, meta: Optional[dict] = None):
    """Stream the tombstones of a delta: yields (header_dict, keys <i8 [n])
    per block of every ``removed_<rank>`` file. Nothing for a directory
    without removals."""
    meta = meta or read_meta(uri)
    for st_ord in range(meta["num_storages"]):
        d = os.path.join(uri, str(st_ord))
        for fname in sorted(os.listdir(d)):
            if not fname.startswith("removed_"):
                continue
            with open(os.path.join(d, fname), "rb") as f:
                while True:
                    magic = f.read(8)
                    if not magic:
                        break
                    if magic != MAGIC:
                        raise RuntimeError(f"bad removal file {fname}")
                    (hlen,) = struct.unpack("<q", f.read(8))
                    hdr = json.loads(f.read(hlen))
                    while True:
                        (blk,) = struct.unpack("<q", f.read(8))
                        if blk < 0:
                            break
                        yield hdr, np.frombuffer(f.read(blk * 8),
                                                 dtype="<i8")


def load_model(ctx, uri: str) -> None:
    """Collective: clears all variables, streams every shard file and keeps
    the keys this rank owns (key % world == rank), re-sharding like the
    reference's load-through-init-push (EmbeddingLoadOperator.cpp:58-111).

    A delta directory is refused (loading clears the tables; use
    ``apply_delta``). The context remembers the dump's ``epoch`` and
    ``model_uuid`` as the base of a delta chain; a tracking context forgets
    its stamps and its removal log and continues at ``epoch + 1`` under the
    dump's uuid, so the base is not re-emitted by its next delta."""
    meta = read_meta(uri)
    if "delta" in meta:
        raise RuntimeError(f"{uri} is a delta checkpoint: load its base "
                           "with load_model, then apply_delta")
    by_id = _match_variables(ctx, meta)
    for mvar in meta["variables"]:
        by_id[mvar["variable_id"]].shard.clear()
    _import_blocks(ctx, uri, meta, by_id)
    _load_admission(ctx, uri, meta, by_id)
    ctx.loaded_epoch = meta.get("epoch")
    ctx.loaded_model_uuid = meta.get("model_uuid")
    if tracked_epoch(ctx) is not None:
        if ctx.loaded_epoch is not None:
            ctx.model_uuid = ctx.loaded_model_uuid
            _advance(ctx, ctx.loaded_epoch + 1, reset=True)
        else:
            _advance(ctx, tracked_epoch(ctx), reset=True)
        _prune_removed(ctx, tracked_epoch(ctx), reset=True)
    ctx.barrier()


def check_delta(meta: dict, loaded_uuid, loaded_epoch) -> dict:
    """The ``delta`` record of a delta's meta if it applies on top of a model
    loaded at ``loaded_epoch`` from ``loaded_uuid``; RuntimeError otherwise
    (not a delta, another model, a gap in the chain, or already applied)."""
    d = meta.get("delta")
    if d is None:
        raise RuntimeError("not a delta checkpoint (its meta has no "
                           "\"delta\" record)")
    if loaded_epoch is None or loaded_uuid is None:
        raise RuntimeError("no delta-capable base is loaded: load a full "
                           "dump written with change tracking on first")
    if d["model_uuid"] != loaded_uuid:
        raise RuntimeError(f"delta belongs to model {d['model_uuid']}, "
                           f"loaded is {loaded_uuid}")
    if d["since"] > loaded_epoch + 1:
        raise RuntimeError(f"delta starts at epoch {d['since']} but the "
                           f"loaded model is at {loaded_epoch}: an earlier "
                           "delta is missing")
    if d["epoch"] <= loaded_epoch:
        raise RuntimeError(f"delta of epoch {d['epoch']} is already "
                           f"contained in the loaded epoch {loaded_epoch}")
    return d


def apply_delta(ctx, uri: str) -> dict:
    """Collective: remove the delta's tombstoned keys, then upsert its rows
    into the loaded tables (nothing is cleared), both re-sharded by
    key % world like ``load_model``. Removals go first: a key that expired
    and was re-created inside the interval is in both lists and must
    survive. Refused with
    RuntimeError, before anything changes, unless ``check_delta`` passes.
    Afterwards ``ctx.loaded_epoch`` is the delta's epoch."""
    meta = read_meta(uri)
    d = check_delta(meta, getattr(ctx, "loaded_model_uuid", None),
                    getattr(ctx, "loaded_epoch", None))
    by_id = _match_variables(ctx, meta)
    _remove_blocks(ctx, uri, meta, by_id)
    _import_blocks(ctx, uri, meta, by_id)
    ctx.loaded_epoch = d["epoch"]
    epoch = tracked_epoch(ctx)
    if epoch is not None and epoch <= d["epoch"]:
        _advance(ctx, d["epoch"] + 1)
    ctx.barrier()
    return d


def _match_variables(ctx, meta: dict) -> dict:
    by_id = {}
    for st in ctx.storages:
        for var in st.variables:
            by_id[var.shard.meta.variable_id] = var
    for mvar in meta["variables"]:
        vid = mvar["variable_id"]
        if vid not in by_id:
            raise RuntimeError(f"checkpoint has variable {vid} missing in model")
        v = by_id[vid]
        if v.shard.dim != mvar["embedding_dim"]:
            raise RuntimeError(f"variable {vid}: dim mismatch "
                               f"{v.shard.dim} != {mvar['embedding_dim']}")
    return by_id


def _remove_blocks(ctx, uri: str, meta: dict, by_id: dict) -> int:
    """Apply a delta's tombstones to this rank's shards; returns how many
    rows went."""
    rank, world = ctx.rank, ctx.world_size
    gone = 0
    for hdr, keys in iter_removed(uri, meta):
        var = by_id.get(hdr["variable_id"])
        if var is None:
            continue
        mine = keys[(keys % world) == rank]
        if mine.size:
            kt = torch.from_numpy(mine.copy()).to(ctx.device)
            gone += int(var.shard.remove_rows(kt).numel())
    return gone


def _import_blocks(ctx, uri: str, meta: dict, by_id: dict) -> None:
    rank, world = ctx.rank, ctx.world_size
    configured = set()
    for hdr, keys, w, s in iter_blocks(uri, meta):
        var = by_id.get(hdr["variable_id"])
        if var is None:
            continue
        if hdr["variable_id"] not in configured:
            configured.add(hdr["variable_id"])
            _apply_config(var, hdr)
        sd = hdr["state_dim"]
        mine = (keys % world) == rank
        if not mine.any():
            continue
        kt = torch.from_numpy(keys[mine].copy()).to(ctx.device)
        wt = torch.from_numpy(w[mine].copy()).to(ctx.device)
        st_t: Optional[torch.Tensor] = None
        if s is not None and sd == var.shard.state_dim:
            st_t = torch.from_numpy(s[mine].copy()).to(ctx.device)
        var.shard.import_rows(kt, wt, st_t)
