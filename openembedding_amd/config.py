"""Typed config tree with per-field defaults and unknown-key warnings.

MI355X rebuild of the reference's EnvConfig (reference
openembedding/client/EnvConfig.{h,cpp}: rpc/master/server sections with
defaults and checkers) plus the unknown-key warning behavior of its
Configurable/CONFIGURE_PROPERTY machinery (reference
openembedding/variable/Factory.h:64-76).

Most rpc/master knobs of the reference configure the TCP/RDMA fabric that
this framework replaced with RCCL over xGMI; they are accepted (so reference
config strings keep working) but unused, and say so in their help. The
``server`` section's knobs that still mean something are mapped:

  server.report_interval  -> periodic metrics report (utils/metrics.Reporter)
  server.cache_size_mb    -> HBM row-cache budget of the host-DRAM tier
  server.update_early_return -> commit on a side stream (overlap analogue)
  server.track_changes    -> new variables record which rows change, for
                             delta checkpoints (checkpoint.dump_delta)
  server.admission_min_count -> new untiered hash variables start with an
                             admission filter of this min_count
                             (VariableShard.set_admission); 0 = off
"""

from __future__ import annotations

import dataclasses
import json
import warnings
from typing import Any, Dict, Optional

import yaml


def _warn_unknown(section: str, cfg: Dict[str, Any], known) -> None:
    for k in cfg:
        if k not in known:
            warnings.warn(
                f"openembedding_amd config: unknown key {section}.{k} ignored "
                f"(known: {sorted(known)})", stacklevel=3)


@dataclasses.dataclass
class RpcConfig:
    """Reference rpc section (EnvConfig.h:14-44). The RPC fabric does not
    exist here (RCCL over xGMI instead); fields accepted for compat."""

    bind_ip: str = ""
    io_thread_num: int = 1
    protocol: str = "rccl"

    @classmethod
    def parse(cls, cfg: Dict[str, Any]) -> "RpcConfig":
        known = {f.name for f in dataclasses.fields(cls)} | {
            "tcp", "rdma"}  # accepted sub-trees, unused on xGMI
        _warn_unknown("rpc", cfg, known)
        return cls(**{k: v for k, v in cfg.items()
                      if k in {f.name for f in dataclasses.fields(cls)}})


@dataclasses.dataclass
class MasterConfig:
    """Reference master section (EnvConfig.h:46-52). Rendezvous is
    torch.distributed's TCPStore (MASTER_ADDR/PORT); endpoint kept so
    reference configs parse."""

    endpoint: str = ""
    type: str = "tcp"
    root_path: str = ""
    recv_timeout: int = 60

    @classmethod
    def parse(cls, cfg: Dict[str, Any]) -> "MasterConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        _warn_unknown("master", cfg, names)
        return cls(**{k: v for k, v in cfg.items() if k in names})


@dataclasses.dataclass
class ServerConfig:
    """Reference server section (EnvConfig.cpp:8-78 defaults)."""

    server_concurrency: int = -1          # engine is in-process; unused
    recv_timeout: int = 60
    report_interval: int = 0              # seconds; 0 = no periodic report
    update_early_return: bool = True      # commit optimizer on side stream
    message_compress: str = ""            # xGMI needs no wire compression
    server_dump_files: int = -1           # files per rank at dump (-1 = 1)
    cache_size_mb: int = 0                # HBM row-cache budget (DRAM tier);
                                          # 0 = everything resident in HBM
    pmem_pool_root_path: str = ""         # host-DRAM tier spill dir analogue
    track_changes: bool = False           # variables start with change
                                          # tracking on (delta checkpoints)
    admission_min_count: int = 0          # new hash variables admit a key
                                          # after this many sightings; 0 = off

    @classmethod
    def parse(cls, cfg: Dict[str, Any]) -> "ServerConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        # reference names kept verbatim where they exist
        alias = {"cache_size": "cache_size_mb"}
        cfg = {alias.get(k, k): v for k, v in cfg.items()}
        _warn_unknown("server", cfg, names)
        return cls(**{k: v for k, v in cfg.items() if k in names})


@dataclasses.dataclass
class EnvConfig:
    rpc: RpcConfig = dataclasses.field(default_factory=RpcConfig)
    master: MasterConfig = dataclasses.field(default_factory=MasterConfig)
    server: ServerConfig = dataclasses.field(default_factory=ServerConfig)

    @classmethod
    def parse(cls, text_or_dict: Optional[object]) -> "EnvConfig":
        """Accepts a YAML or JSON string (the reference's flags.config), a
        dict, or None/empty -> defaults."""
        if not text_or_dict:
            return cls()
        if isinstance(text_or_dict, str):
            try:
                data = json.loads(text_or_dict)
            except json.JSONDecodeError:
                data = yaml.safe_load(text_or_dict)
        else:
            data = text_or_dict
        if data is None:
            return cls()
        if not isinstance(data, dict):
            raise ValueError(f"config must be a mapping, got {type(data)}")
        _warn_unknown("", data, {"rpc", "master", "server"})
        return cls(
            rpc=RpcConfig.parse(data.get("rpc", {}) or {}),
            master=MasterConfig.parse(data.get("master", {}) or {}),
            server=ServerConfig.parse(data.get("server", {}) or {}),
        )
