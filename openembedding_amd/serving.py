"""Serving: model registry, controller and REST API.

MI355X rebuild of the reference's serving stack:
- ``ModelManager::find_model_variable`` (reference
  client/ModelController.cpp:24-44): sign -> loaded model -> read-only
  variable handle, cached -> :class:`ModelManager.find_model_variable`;
- ``ModelController`` create/delete/show models, show/shutdown nodes with a
  CREATING -> NORMAL status machine and async heavy load (reference
  ModelController.cpp:47-164) -> :class:`ModelController`;
- brpc REST controller ``POST/GET/DELETE /models[/sign]``,
  ``GET/DELETE /nodes[/id]`` (reference entry/controller.cc:100-203) ->
  :func:`make_app` (FastAPI; run with uvicorn).

Architectural difference, by design: the reference serves from live PS
server processes holding training shards with replica HA; here a serving
process loads the dump into its own read-only tables (HBM on a GPU box, host
memory otherwise) — single-node MI355X serving needs no RPC fabric, and HA
across boxes is a deployment concern (run N serving processes behind a load
balancer). Missing keys pull zeros, exactly like the reference read-only
path (EmbeddingPullOperator.cpp:179-181 get_weights).
"""

# NOTE: no `from __future__ import annotations` here — FastAPI must see real
# class objects (not strings) for the locally-defined request models in
# make_app, or it demotes the body params to query params.
import threading
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from .checkpoint import iter_blocks, iter_removed, read_meta
from .core.variable import VariableMeta, VariableShard


class ModelStatus:
    CREATING = "CREATING"
    NORMAL = "NORMAL"
    DELETED = "DELETED"
    ERROR = "ERROR"


STORAGE_KINDS = ("fp32", "int8", "fp16")


def check_quantize(quantize: Optional[str]) -> Optional[str]:
    """``quantize`` of a load: None (fp32 tables) or a packed row format."""
    if quantize is None or quantize in STORAGE_KINDS[1:]:
        return quantize
    raise ValueError(f"quantize must be one of {list(STORAGE_KINDS[1:])} "
                     f"or None, got {quantize!r}")


def _make_shard(mvar: dict, device: str, quantize: Optional[str]):
    """The read-only table of one variable of a dump's meta: an fp32
    (Hip)VariableShard, or a QuantizedShard when ``quantize`` names a packed
    row format (rows are then quantized block by block as they arrive; no
    fp32 table is ever built)."""
    vm = VariableMeta(variable_id=mvar["variable_id"],
                      embedding_dim=mvar["embedding_dim"],
                      vocabulary_size=mvar["vocabulary_size"])
    if quantize is not None:
        if mvar.get("datatype", "float32") != "float32":
            raise ValueError(
                f"variable {vm.variable_id} is {mvar['datatype']}: only "
                "float32 variables can be served quantized")
        from .core.quantized import QuantizedShard
        return QuantizedShard(vm, quantize, device=device)
    if device.startswith("cuda"):
        from .core.variable_gpu import HipVariableShard
        return HipVariableShard(vm, shard_id=0, shard_num=1, device=device)
    return VariableShard(vm, shard_id=0, shard_num=1, device=device)


class ServedVariable:
    """Read-only handle over one loaded variable (reference
    EmbeddingVariableHandle in read-only mode)."""

    def __init__(self, shard: VariableShard):
        self.shard = shard

    @property
    def embedding_dim(self) -> int:
        return self.shard.dim

    @property
    def storage(self) -> str:
        """"fp32", or the packed row format of a quantized table."""
        return getattr(self.shard, "fmt", "fp32")

    @property
    def table_bytes(self) -> int:
        """Bytes the table holds, key map included: a quantized table's
        packed slab, an fp32 table's allocated weight and state rows, plus
        whichever of the probe table, the row -> key list and the valid
        bitmap the shard keeps as tensors (the CPU hash shards index with a
        dict, which is not counted)."""
        sh = self.shard
        if hasattr(sh, "nbytes"):
            return int(sh.nbytes)
        total = 0
        for name in ("weights", "state", "tk", "tv", "slot_keys",
                     "valid_u8", "valid"):
            t = getattr(sh, name, None)
            if torch.is_tensor(t):
                total += t.numel() * t.element_size()
        return int(total)

    def pull_weights(self, indices: torch.Tensor) -> torch.Tensor:
        flat = indices.reshape(-1).to(torch.int64).to(self.shard.device)
        out = self.shard.pull_readonly(flat)
        return out.view(*indices.shape, self.shard.dim)

    def pull_pooled(self, values, offsets, mode: str = "sum",
                    per_sample_weights=None) -> torch.Tensor:
        """Pooled read of ragged bags, the serving side of ``EmbeddingBag``:
        bag b combines the rows of ``values[offsets[b]:offsets[b+1]]`` with
        ``mode`` ("sum" | "mean" | "sqrtn") and, when given, the per-sample
        weights (TF ``embedding_lookup_sparse`` rules) -> [B, dim]. A key
        missing from the table is a zero row that still counts toward its
        bag's length. On a GPU table this is one fused kernel launch.

        Serving input is untrusted, so everything is validated on the host
        before any launch; a violation raises ``ValueError``."""
        from .ops.dispatch import POOL_MODES
        if mode not in POOL_MODES:
            raise ValueError(f"mode must be one of {sorted(POOL_MODES)}, "
                             f"got {mode!r}")
        try:
            vals = torch.as_tensor(values).detach().cpu()
            off = torch.as_tensor(offsets).detach().cpu()
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"values/offsets are not integer lists: {e}")
        if vals.numel() == 0:
            vals = vals.to(torch.int64)
        if vals.dim() != 1 or vals.is_floating_point() \
                or vals.is_complex() or vals.dtype == torch.bool:
            raise ValueError("values must be a 1-D list of integer ids")
        if off.dim() != 1 or off.numel() < 1 or off.is_floating_point() \
                or off.is_complex() or off.dtype == torch.bool:
            raise ValueError("offsets must be a 1-D list of B+1 integer "
                             "row splits")
        vals = vals.to(torch.int64)
        off = off.to(torch.int64)
        if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) \
                or int(off[-1]) > vals.numel():
            raise ValueError("offsets must start at 0, be non-decreasing "
                             f"and end at or below len(values)="
                             f"{vals.numel()}")
        w = None
        if per_sample_weights is not None:
            try:
                w = torch.as_tensor(per_sample_weights).detach().cpu()
                w = w.to(self.shard.dtype)
            except (TypeError, ValueError, RuntimeError) as e:
                raise ValueError(f"per_sample_weights are not numbers: {e}")
            if w.dim() != 1 or w.numel() != vals.numel():
                raise ValueError("per_sample_weights must have len(values)="
                                 f"{vals.numel()} elements, got "
                                 f"{tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()):
                raise ValueError("per_sample_weights must be finite")
            w = w.to(self.shard.device)
        dev = self.shard.device
        return self.shard.pull_pooled_readonly(vals.to(dev), off.to(dev),
                                               mode, w)


class ServedModel:
    """One loaded model: meta + read-only variables keyed by variable_id."""

    def __init__(self, sign: str, uri: str):
        self.sign = sign
        self.uri = uri
        self.status = ModelStatus.CREATING
        self.error: Optional[str] = None
        self.created_at = time.time()
        self.variables: Dict[int, ServedVariable] = {}
        self.meta: Optional[dict] = None
        # base of the delta chain (a dump written with change tracking on)
        self.loaded_epoch: Optional[int] = None
        self.model_uuid: Optional[str] = None
        self._update_lock = threading.Lock()

    def load(self, device: str = "cpu",
             quantize: Optional[str] = None) -> None:
        """Stream the dump into read-only tables. All shards of the dump are
        merged into one local table (shard_num=1 view — serving is per-key
        lookup, the training shard layout is irrelevant).

        On a cuda device the tables are HipVariableShards, so serving pulls
        run the same k_ht_lookup / k_gather_init HIP kernels as training
        (the round-1 CPU-table fallback bypassed every kernel).

        ``quantize`` = "int8" | "fp16" builds QuantizedShards instead: every
        block is quantized into a packed slab as it is read, and the slab is
        reserved from the row counts in the dump's section headers."""
        quantize = check_quantize(quantize)
        meta = read_meta(self.uri)
        if "delta" in meta:
            raise RuntimeError(f"{self.uri} is a delta checkpoint: load its "
                               "base, then apply_delta")
        self.meta = meta
        self.quantize = quantize
        shards: Dict[int, VariableShard] = {}
        for mvar in meta["variables"]:
            shards[mvar["variable_id"]] = _make_shard(mvar, device, quantize)
        self._import(self.uri, meta, shards)
        self.variables = {vid: ServedVariable(sh)
                          for vid, sh in shards.items()}
        self.loaded_epoch = meta.get("epoch")
        self.model_uuid = meta.get("model_uuid")
        self.status = ModelStatus.NORMAL

    def _import(self, uri: str, meta: dict, shards: dict,
                update: bool = False) -> int:
        """Stream the rows of a dump or a delta into ``shards``. A load
        reserves a quantized table exactly, section by section; an
        ``update`` of a live one makes room only when the section could
        outgrow the slab (its keys may all exist already), and then by at
        least half the slab, so that a chain of deltas copies the slab a
        logarithmic number of times."""
        quantize = getattr(self, "quantize", None)
        section = None
        rows = 0
        for hdr, keys, w, _s in iter_blocks(uri, meta):
            sh = shards.get(hdr["variable_id"])
            if sh is None or not len(keys):
                continue
            if quantize is not None and hdr is not section:
                section = hdr       # one header per (file, variable) section
                if "num_items" in hdr and sh.meta.use_hash_table:
                    need = sh.num_rows + int(hdr["num_items"])
                    cap = sh.slab.shape[0]
                    if not update:
                        sh.reserve_rows(need)
                    elif need > cap:
                        sh.reserve_rows(max(need, cap + cap // 2))
            # frombuffer arrays are read-only; copy before wrapping (torch
            # tensors over read-only memory are undefined behavior)
            kt = torch.from_numpy(keys.copy())
            wt = torch.from_numpy(w.copy())
            sh.import_rows(kt.to(sh.device), wt.to(sh.device))
            rows += len(keys)
        return rows

    def _remove(self, uri: str, meta: dict, shards: dict):
        """Apply a delta's tombstones through each shard's ``remove_rows``;
        returns the number of rows that went, None for a delta without
        tombstones."""
        gone = None
        for hdr, keys in iter_removed(uri, meta):
            gone = gone or 0
            sh = shards.get(hdr["variable_id"])
            if sh is None or not len(keys):
                continue
            kt = torch.from_numpy(keys.copy()).to(sh.device)
            gone += int(sh.remove_rows(kt).numel())
        return gone

    def apply_delta(self, uri: str) -> dict:
        """Apply a delta checkpoint to the live tables, whatever their row
        format: first its tombstones (the keys removed by the trainer's
        expiry) through the shard's ``remove_rows``, then its rows through
        ``import_rows``, which overwrites an existing key and, on a
        quantized table, quantizes the row into place. A key that expired
        and came back inside the interval is in both lists and survives.
        Refused with RuntimeError, before anything changes, unless the
        delta continues this model's chain (``checkpoint.check_delta``).
        The result of a delta that carries tombstones has a ``"removed"``
        count beside ``since``, ``epoch`` and ``rows``.

        A block that a quantized table cannot hold (``ValueError`` from its
        ``import_rows``: a non-finite value, an fp16 overflow) stops the
        update there: the blocks before it stay applied and the epoch stays
        where it was, so that the corrected delta can be applied again.

        Readers are not locked out, and nothing orders a read against an
        update: rows are written block by block, each row by one copy or
        one quantizing kernel, and a read that overlaps the update may see
        rows and variables of both epochs, may miss a key that the update
        is creating (a table that grows swaps its buffers), and on a CPU
        table may even catch a row mid-copy. A removal moves the last rows
        of a hash table into the holes and rebuilds its key map: a read
        that overlaps it may miss any key of the table for a moment, or
        briefly resolve a key to a slot whose row has moved. A caller that
        needs a consistent view quiesces reads around the call or updates a
        second replica and switches. Updates of one model are serialized."""
        from .checkpoint import check_delta
        with self._update_lock:
            if self.status != ModelStatus.NORMAL:
                raise RuntimeError(
                    f"model {self.sign!r} status {self.status}")
            meta = read_meta(uri)
            d = check_delta(meta, self.model_uuid, self.loaded_epoch)
            shards = {vid: v.shard for vid, v in self.variables.items()}
            for mvar in meta["variables"]:
                sh = shards.get(mvar["variable_id"])
                if sh is None or sh.dim != mvar["embedding_dim"]:
                    raise RuntimeError(
                        f"delta variable {mvar['variable_id']} does not "
                        "match the loaded model")
            try:
                removed = self._remove(uri, meta, shards)
                rows = self._import(uri, meta, shards, update=True)
            finally:
                self._export_cache = {}  # replica pages must show the update
            self.loaded_epoch = d["epoch"]
            out = {"since": d["since"], "epoch": d["epoch"], "rows": rows}
            if removed is not None:
                out["removed"] = removed
            self.last_update = out
        return out

    def export_block(self, variable_id: int, start: int, count: int):
        """Row block [start, start+count) of a variable in export order —
        the replica-to-replica restore wire (reference
        EmbeddingRestoreOperator.cpp:19-106 pulled shard content from live
        replicas in server_block_num_items batches; here the batches ride
        HTTP). The export snapshot is cached on first use (tables are
        read-only while serving)."""
        if not hasattr(self, "_export_cache"):
            self._export_cache = {}
        blk = self._export_cache.get(variable_id)
        if blk is None:
            sh = self.variables[variable_id].shard
            keys, w, _s = sh.export_rows(include_state=False)
            blk = (keys.cpu(), w.cpu())
            self._export_cache[variable_id] = blk
        keys, w = blk
        end = min(start + count, keys.numel())
        return {"total": int(keys.numel()),
                "keys": keys[start:end].tolist(),
                "weights": w[start:end].tolist()}

    def load_from_replica(self, base_url: str, sign: str,
                          device: str = "cpu",
                          block: int = 65536,
                          quantize: Optional[str] = None) -> None:
        """Coordinated restore: rebuild this model's tables by paging rows
        out of a LIVE replica (no dump needed — the reference's
        restore-from-replica path for a replacement server). With
        ``quantize`` the pages are quantized as they arrive; pages of a
        replica that is itself quantized are dequantized rows, so
        re-quantizing them is lossy once more (docs/serving.md)."""
        import requests

        quantize = check_quantize(quantize)
        self.quantize = quantize

        meta = requests.get(f"{base_url}/models/{sign}", timeout=10).json()
        self.meta = {"model_sign": meta["model_sign"],
                     "variables": meta["variables"], "version": "0.2"}
        shards: Dict[int, VariableShard] = {}
        for mvar in meta["variables"]:
            sh = _make_shard(mvar, device, quantize)
            vid = mvar["variable_id"]
            start = 0
            while True:
                r = requests.get(
                    f"{base_url}/models/{sign}/variables/{vid}/rows",
                    params={"start": start, "count": block},
                    timeout=60).json()
                if quantize is not None and start == 0:
                    sh.reserve_rows(int(r["total"]))
                if r["keys"]:
                    kt = torch.tensor(r["keys"], dtype=torch.int64,
                                      device=sh.device)
                    wt = torch.tensor(r["weights"], dtype=torch.float32,
                                      device=sh.device)
                    sh.import_rows(kt, wt)
                start += block
                if start >= r["total"]:
                    break
            shards[vid] = sh
        self.variables = {vid: ServedVariable(sh)
                          for vid, sh in shards.items()}
        self.status = ModelStatus.NORMAL

    def describe(self) -> dict:
        return {
            "model_sign": self.sign,
            "uri": self.uri,
            "status": self.status,
            "error": self.error,
            # epoch of the dump plus the deltas applied since (None for a
            # dump written without change tracking)
            "epoch": self.loaded_epoch,
            "variables": ([
                {"variable_id": v["variable_id"],
                 "embedding_dim": v["embedding_dim"],
                 "vocabulary_size": v["vocabulary_size"],
                 **self._storage_of(v["variable_id"])}
                for v in self.meta["variables"]] if self.meta else []),
        }

    def _storage_of(self, variable_id: int) -> dict:
        """``storage`` ("fp32" | "int8" | "fp16") and ``table_bytes`` of a
        variable; while the model is still loading, the storage it was
        asked for and 0 bytes."""
        var = self.variables.get(variable_id)
        if var is None:
            return {"storage": getattr(self, "quantize", None) or "fp32",
                    "table_bytes": 0}
        return {"storage": var.storage, "table_bytes": var.table_bytes}


class ModelManager:
    """sign -> ServedModel cache + variable resolution (reference
    ModelManager::find_model_variable, ModelController.cpp:24-44)."""

    def __init__(self, device: str = "cpu"):
        self.device = device
        self._models: Dict[str, ServedModel] = {}
        self._lock = threading.Lock()

    def get(self, sign: str) -> Optional[ServedModel]:
        return self._models.get(sign)

    def find_model_variable(self, sign: str, variable_id: int
                            ) -> ServedVariable:
        m = self._models.get(sign)
        if m is None:
            raise KeyError(f"model {sign!r} not found")
        if m.status != ModelStatus.NORMAL:
            raise RuntimeError(f"model {sign!r} status {m.status}")
        v = m.variables.get(variable_id)
        if v is None:
            raise KeyError(f"model {sign!r} has no variable {variable_id}")
        return v

    def _register(self, model: ServedModel) -> None:
        with self._lock:
            self._models[model.sign] = model

    def _remove(self, sign: str) -> Optional[ServedModel]:
        with self._lock:
            return self._models.pop(sign, None)

    def signs(self) -> List[str]:
        return sorted(self._models)


class ModelController:
    """Create/delete/show models; node surface (reference
    ModelController.cpp:47-164 with the master-lock + async-load machinery
    collapsed to a thread per load — one process owns the registry)."""

    def __init__(self, manager: Optional[ModelManager] = None,
                 device: str = "cpu"):
        self.manager = manager or ModelManager(device=device)
        self.shutdown_requested = False

    def create_model(self, model_uri: str, sign: Optional[str] = None,
                     wait: bool = True,
                     quantize: Optional[str] = None) -> ServedModel:
        """Load a dump for serving. sign defaults to the dump's model_sign.
        wait=False returns immediately with status CREATING (reference async
        heavy load, ModelController.cpp:66-82). ``quantize`` = "int8" |
        "fp16" serves from packed tables (ServedModel.load); an unknown
        value raises ValueError before anything is registered."""
        quantize = check_quantize(quantize)
        meta = read_meta(model_uri)
        sign = sign or meta["model_sign"]
        existing = self.manager.get(sign)
        if existing is not None and existing.status != ModelStatus.ERROR:
            raise ValueError(f"model {sign!r} already exists")
        model = ServedModel(sign, model_uri)
        self.manager._register(model)

        def _load():
            try:
                model.load(device=self.manager.device, quantize=quantize)
            except Exception as e:  # noqa: BLE001
                model.status = ModelStatus.ERROR
                model.error = repr(e)

        if wait:
            _load()
            if model.status == ModelStatus.ERROR:
                self.manager._remove(sign)
                raise RuntimeError(f"load failed: {model.error}")
        else:
            threading.Thread(target=_load, daemon=True).start()
        return model

    def restore_model_from_replica(self, base_url: str, sign: str,
                                   wait: bool = True,
                                   quantize: Optional[str] = None
                                   ) -> ServedModel:
        """Coordinated restore from a live replica (reference
        EmbeddingRestoreOperator replica path / server --restore): page
        the rows out of ``base_url`` instead of a dump URI."""
        quantize = check_quantize(quantize)
        existing = self.manager.get(sign)
        if existing is not None and existing.status != ModelStatus.ERROR:
            raise ValueError(f"model {sign!r} already exists")
        model = ServedModel(sign, f"replica://{base_url}")
        self.manager._register(model)

        def _load():
            try:
                model.load_from_replica(base_url, sign,
                                        device=self.manager.device,
                                        quantize=quantize)
            except Exception as e:  # noqa: BLE001
                model.status = ModelStatus.ERROR
                model.error = repr(e)

        if wait:
            _load()
            if model.status == ModelStatus.ERROR:
                self.manager._remove(sign)
                raise RuntimeError(f"replica restore failed: {model.error}")
        else:
            threading.Thread(target=_load, daemon=True).start()
        return model

    def update_model(self, sign: str, delta_uri: str) -> ServedModel:
        """Apply a delta checkpoint to the live model ``sign`` in place
        (``ServedModel.apply_delta``); the model keeps answering meanwhile.
        KeyError for an unknown sign, RuntimeError for a delta that does
        not continue the model's chain."""
        m = self.manager.get(sign)
        if m is None:
            raise KeyError(f"model {sign!r} not found")
        m.apply_delta(delta_uri)
        return m

    def delete_model(self, sign: str) -> None:
        m = self.manager._remove(sign)
        if m is None:
            raise KeyError(f"model {sign!r} not found")
        m.status = ModelStatus.DELETED
        m.variables = {}

    def show_models(self) -> List[dict]:
        return [self.manager._models[s].describe()
                for s in self.manager.signs()]

    def show_model(self, sign: str) -> dict:
        m = self.manager.get(sign)
        if m is None:
            raise KeyError(f"model {sign!r} not found")
        return m.describe()

    def show_nodes(self) -> List[dict]:
        """Single-process serving: one node = this process (reference
        show_nodes listed PS server processes)."""
        dev = self.manager.device
        info = {"node_id": 0, "device": dev,
                "models": self.manager.signs(),
                "shutdown_requested": self.shutdown_requested}
        if dev.startswith("cuda") and torch.cuda.is_available():
            free, total = torch.cuda.mem_get_info()
            info["hbm_free_bytes"] = free
            info["hbm_total_bytes"] = total
        return [info]

    def shutdown_node(self, node_id: int = 0) -> None:
        self.shutdown_requested = True


class ServingClient:
    """Minimal HTTP pull client with replica failover.

    The documented HA deployment runs N serving processes behind this
    client (or any load balancer); it is the reference's client-side
    replica machinery — pick_one_replica + retry-until-success
    (EmbeddingPullOperator.cpp:50-58, c_api_test.h:117-121) — over HTTP:
    requests rotate round-robin across endpoints and fail over to the next
    replica on connection error or non-200."""

    def __init__(self, endpoints: List[str], timeout: float = 5.0,
                 attempts_per_endpoint: int = 2):
        if not endpoints:
            raise ValueError("need at least one endpoint")
        self.endpoints = [e.rstrip("/") for e in endpoints]
        self.timeout = timeout
        self.attempts = attempts_per_endpoint * len(self.endpoints)
        self._i = 0

    def _request(self, method: str, path: str, json_body=None):
        import requests

        last: Optional[Exception] = None
        for _ in range(self.attempts):
            ep = self.endpoints[self._i % len(self.endpoints)]
            self._i += 1
            try:
                r = requests.request(method, ep + path, json=json_body,
                                     timeout=self.timeout)
                if r.status_code == 200:
                    return r.json()
                last = RuntimeError(f"{ep}{path}: HTTP {r.status_code} "
                                    f"{r.text[:200]}")
            except Exception as e:  # noqa: BLE001 - any replica failure
                last = e
        raise RuntimeError(f"all {len(self.endpoints)} replicas failed: "
                           f"{last!r}")

    def pull(self, sign: str, variable_id: int, indices) -> List:
        if torch.is_tensor(indices):
            indices = indices.tolist()
        r = self._request("POST",
                          f"/models/{sign}/variables/{variable_id}/pull",
                          {"indices": indices})
        return r["weights"]

    def pull_pooled(self, sign: str, variable_id: int, values, offsets,
                    mode: str = "sum", per_sample_weights=None) -> List:
        """Pooled rows [B][dim] of ragged bags (``ServedVariable.
        pull_pooled``), with the replica failover of ``pull``."""
        body = {"values": values, "offsets": offsets, "mode": mode}
        if per_sample_weights is not None:
            body["per_sample_weights"] = per_sample_weights
        for k, v in body.items():
            if torch.is_tensor(v):
                body[k] = v.tolist()
        r = self._request(
            "POST", f"/models/{sign}/variables/{variable_id}/pull_pooled",
            body)
        return r["pooled"]

    def show_models(self) -> List[dict]:
        return self._request("GET", "/models")

    def create_model(self, model_uri: str, sign: Optional[str] = None,
                     quantize: Optional[str] = None) -> dict:
        """``POST /models`` on one replica (the next in rotation)."""
        body = {"model_uri": model_uri}
        if sign is not None:
            body["sign"] = sign
        if quantize is not None:
            body["quantize"] = quantize
        return self._request("POST", "/models", body)


def make_app(controller: Optional[ModelController] = None,
             device: str = "cpu"):
    """REST surface (reference entry/controller.cc routes):
      POST   /models            {"model_uri": ..., "sign"?: ..., "wait"?: bool,
                                 "quantize"?: "int8"|"fp16"}
      GET    /models            list
      GET    /models/{sign}     describe
      DELETE /models/{sign}
      POST   /models/{sign}/deltas   {"model_uri": <delta checkpoint>}
                                apply a delta to the live model in place
      GET    /nodes             list nodes
      DELETE /nodes/{id}        request shutdown
      POST   /models/{sign}/variables/{vid}/pull   {"indices": [[...]]}
      POST   /models/{sign}/variables/{vid}/pull_pooled
             {"values": [...], "offsets": [...], "mode": "sum"|"mean"|"sqrtn",
              "per_sample_weights"?: [...]} -> {"pooled": [[...]]}
    The pull routes are an addition over the reference (whose serving data
    path went through TF-Serving custom ops): they make the server usable
    from any HTTP client without TF. pull_pooled is the read side of
    EmbeddingBag: the combiner runs on the server, so a client fetches
    B x dim floats instead of nnz x dim; 422 on malformed bags."""
    from fastapi import FastAPI, HTTPException
    from pydantic import BaseModel

    controller = controller or ModelController(device=device)
    app = FastAPI(title="openembedding_amd serving controller")
    app.state.controller = controller

    class CreateModelReq(BaseModel):
        model_uri: Optional[str] = None
        sign: Optional[str] = None
        wait: bool = True
        # coordinated restore: rebuild from a live replica instead of a
        # dump (requires sign; reference server --restore semantics)
        from_replica: Optional[str] = None
        # serve from packed tables: "int8" | "fp16" (anything else: 422)
        quantize: Optional[str] = None

    class UpdateModelReq(BaseModel):
        model_uri: str

    class PullReq(BaseModel):
        indices: list

    class PullPooledReq(BaseModel):
        values: list
        offsets: list
        mode: str = "sum"
        per_sample_weights: Optional[list] = None

    @app.post("/models")
    def create_model(req: CreateModelReq):
        try:
            check_quantize(req.quantize)
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        try:
            if req.from_replica:
                if not req.sign:
                    raise HTTPException(status_code=422,
                                        detail="from_replica needs sign")
                m = controller.restore_model_from_replica(
                    req.from_replica, req.sign, wait=req.wait,
                    quantize=req.quantize)
            else:
                if not req.model_uri:
                    raise HTTPException(status_code=422,
                                        detail="model_uri required")
                m = controller.create_model(req.model_uri, sign=req.sign,
                                            wait=req.wait,
                                            quantize=req.quantize)
        except ValueError as e:
            raise HTTPException(status_code=409, detail=str(e))
        except (FileNotFoundError, RuntimeError) as e:
            raise HTTPException(status_code=400, detail=str(e))
        return m.describe()

    @app.post("/models/{sign}/deltas")
    def update_model(sign: str, req: UpdateModelReq):
        """Apply a delta checkpoint to a live model; answers with the
        model's description at the new epoch, with the ``removed`` count of
        a delta that carried tombstones. 404 unknown sign, 409 a delta
        that does not continue the chain, 400 an unreadable URI, 422 rows
        that the table's format cannot hold (the blocks before them stay
        applied, the epoch does not move)."""
        try:
            m = controller.update_model(sign, req.model_uri)
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e))
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        except FileNotFoundError as e:
            raise HTTPException(status_code=400, detail=str(e))
        except RuntimeError as e:
            raise HTTPException(status_code=409, detail=str(e))
        out = m.describe()
        last = getattr(m, "last_update", None) or {}
        if "removed" in last:
            out["removed"] = last["removed"]
        return out

    @app.get("/models/{sign}/variables/{variable_id}/rows")
    def export_rows(sign: str, variable_id: int, start: int = 0,
                    count: int = 65536):
        """Replica-restore wire: row blocks in export order."""
        m = controller.manager.get(sign)
        if m is None or m.status != ModelStatus.NORMAL:
            raise HTTPException(status_code=404, detail=f"model {sign!r}")
        if variable_id not in m.variables:
            raise HTTPException(status_code=404,
                                detail=f"variable {variable_id}")
        return m.export_block(variable_id, start, count)

    @app.get("/models")
    def list_models():
        return controller.show_models()

    @app.get("/models/{sign}")
    def show_model(sign: str):
        try:
            return controller.show_model(sign)
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e))

    @app.delete("/models/{sign}")
    def delete_model(sign: str):
        try:
            controller.delete_model(sign)
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e))
        return {"deleted": sign}

    @app.get("/nodes")
    def list_nodes():
        return controller.show_nodes()

    @app.delete("/nodes/{node_id}")
    def shutdown_node(node_id: int):
        controller.shutdown_node(node_id)
        return {"shutdown_requested": node_id}

    @app.get("/metrics")
    def metrics():
        """Prometheus-style exposition of the process accumulators
        (reference server metrics exposer, entry/server.cc:7-12,35-36)."""
        from starlette.responses import PlainTextResponse

        from .utils.metrics import REGISTRY
        lines = ["# TYPE openembedding_metric gauge"]
        for name in REGISTRY.names():
            a = REGISTRY.accumulator(name)
            safe = name.replace(".", "_").replace("-", "_")
            lines.append(f'openembedding_metric{{name="{safe}",stat="count"}}'
                         f' {a.n}')
            lines.append(f'openembedding_metric{{name="{safe}",stat="sum"}}'
                         f' {a.total}')
        # admission filters of a trainer living in this process (a served
        # table is read-only and has none): sightings that got a row and
        # sightings that were turned away, per variable
        from . import context as _ctxmod
        tctx = _ctxmod._context
        for vid, v in sorted(tctx.variables.items()) if tctx else ():
            if getattr(v.shard, "_admit", None) is None:
                continue
            st = v.shard.admission_stats()
            for stat in ("admitted", "turned_away"):
                lines.append(f'openembedding_admission{{variable="{vid}",'
                             f'stat="{stat}"}} {st[stat]}')
        lines.append(f'openembedding_models {len(controller.manager.signs())}')
        return PlainTextResponse("\n".join(lines) + "\n")

    @app.post("/models/{sign}/variables/{variable_id}/pull")
    def pull(sign: str, variable_id: int, req: PullReq):
        try:
            var = controller.manager.find_model_variable(sign, variable_id)
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e))
        except RuntimeError as e:
            raise HTTPException(status_code=409, detail=str(e))
        idx = torch.tensor(req.indices, dtype=torch.int64)
        out = var.pull_weights(idx)
        return {"weights": out.cpu().tolist()}

    @app.post("/models/{sign}/variables/{variable_id}/pull_pooled")
    def pull_pooled(sign: str, variable_id: int, req: PullPooledReq):
        try:
            var = controller.manager.find_model_variable(sign, variable_id)
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e))
        except RuntimeError as e:
            raise HTTPException(status_code=409, detail=str(e))
        try:
            out = var.pull_pooled(req.values, req.offsets, req.mode,
                                  req.per_sample_weights)
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        return {"pooled": out.cpu().tolist()}

    return app


def main():  # pragma: no cover - thin CLI (reference controller daemon)
    import argparse

    import uvicorn

    p = argparse.ArgumentParser(description="openembedding_amd serving "
                                            "controller (REST)")
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8010)
    p.add_argument("--device", default=(
        "cuda:0" if torch.cuda.is_available() else "cpu"))
    p.add_argument("--model-uri", action="append", default=[],
                   help="dump URI(s) to load at startup")
    p.add_argument("--quantize", choices=list(STORAGE_KINDS[1:]),
                   default=None,
                   help="serve the startup models from packed tables")
    args = p.parse_args()
    controller = ModelController(device=args.device)
    for uri in args.model_uri:
        controller.create_model(uri, quantize=args.quantize)
    uvicorn.run(make_app(controller), host=args.host, port=args.port)


if __name__ == "__main__":  # pragma: no cover
    main()
