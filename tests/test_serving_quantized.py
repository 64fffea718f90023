"""Serving from quantized tables on the CPU: POST /models with ``quantize``,
/pull and /pull_pooled against the in-process oracle, describe(), the 422
for an unknown format, a restore from a quantized replica, the CLI flag and
the example."""

import os
import subprocess
import sys

import pytest
import torch
from fastapi.testclient import TestClient

import openembedding_amd.torch as embed
import quantized_ref as qref
from openembedding_amd.checkpoint import iter_blocks, read_meta
from openembedding_amd.core.quantized import QuantizedShard
from openembedding_amd.ops import dispatch as ops
from openembedding_amd.serving import (ModelController, ServedModel,
                                       ServingClient, make_app)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 12
VALUES = [5, 9, 9, 31, 77, 5, 12, 40, 3]    # 77 and 40 were never trained
OFFSETS = [0, 2, 2, 6, 8]                   # an empty bag; values[8] unused
WEIGHTS = [0.5, -1.25, 2.0, 1.0, 3.0, 0.25, 1.5, -0.75, 9.0]


@pytest.fixture()
def dump(tmp_path):
    """Train a small bag 2 steps on the CPU and dump it: (uri, sign, keys,
    fp32 rows of the dump)."""
    torch.manual_seed(3)
    embed.get_context("cpu")
    emb = embed.EmbeddingBag(-1, DIM, mode="mean")
    emb.variable.set_initializer("uniform", minval=-0.5, maxval=0.5)
    emb.variable.set_optimizer("adagrad", learning_rate=0.1)
    vals = torch.tensor([5, 9, 9, 31, 12, 3, 5])
    off = torch.tensor([0, 3, 3, 7])
    for _ in range(2):
        emb(vals, off).sum().backward()
        embed.get_context().update_all_weights()
    uri = str(tmp_path / "dump")
    embed.save_server_model(uri)
    ctx = embed.get_context()
    sign = f"{ctx.model_uuid}-{ctx.model_version}"
    blocks = list(iter_blocks(uri, read_meta(uri)))
    keys = torch.cat([torch.from_numpy(k.copy()) for _, k, _, _ in blocks])
    rows = torch.cat([torch.from_numpy(w.copy()) for _, _, w, _ in blocks])
    assert keys.numel() == 5 and bool((rows != 0).any())
    return uri, sign, keys, rows


def _oracle_rows(keys, rows, fmt, query):
    """Dequantized rows of ``query`` from the dump's rows; zeros for a key
    the dump does not hold."""
    deq = ops.dequantize_rows(ops.quantize_rows(rows, fmt), DIM, fmt)
    table = {int(k): deq[i] for i, k in enumerate(keys.tolist())}
    return torch.stack([table.get(int(q), torch.zeros(DIM)) for q in query])


@pytest.mark.parametrize("fmt", ["int8", "fp16"])
def test_rest_model_with_quantize_answers_like_the_oracle(dump, fmt):
    uri, sign, keys, rows = dump
    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    r = client.post("/models", json={"model_uri": uri, "quantize": fmt})
    assert r.status_code == 200, r.text
    var = r.json()["variables"][0]
    assert var["storage"] == fmt
    stride = ops.row_stride(fmt, DIM)
    assert var["table_bytes"] == 5 * stride + 5 * 8       # reserved exactly
    shard = c.manager.find_model_variable(sign, 0).shard
    assert isinstance(shard, QuantizedShard) and shard.num_rows == 5
    assert client.get(f"/models/{sign}").json()["variables"][0] == var
    assert client.get("/models").json()[0]["variables"][0] == var

    want_rows = _oracle_rows(keys, rows, fmt, VALUES)
    assert bool((want_rows[4] == 0).all()) and bool((want_rows[0] != 0).any())
    r = client.post(f"/models/{sign}/variables/0/pull",
                    json={"indices": VALUES})
    assert r.status_code == 200
    assert torch.equal(torch.tensor(r.json()["weights"]), want_rows)
    off = torch.tensor(OFFSETS)
    for mode in ("sum", "mean", "sqrtn"):
        for weights in (None, WEIGHTS):
            body = {"values": VALUES, "offsets": OFFSETS, "mode": mode}
            if weights is None:
                want = ops.pool_fwd(want_rows, None, None, off, mode,
                                    False)[0]
            else:
                body["per_sample_weights"] = weights
                want = ops.pool_fwd_weighted(want_rows, None, None, off,
                                             torch.tensor(weights), mode)[0]
            r = client.post(f"/models/{sign}/variables/0/pull_pooled",
                            json=body)
            assert r.status_code == 200, r.text
            assert torch.equal(torch.tensor(r.json()["pooled"]), want)
    # host-side validation stays in front of the quantized table
    bad = client.post(f"/models/{sign}/variables/0/pull_pooled",
                      json={"values": [1, 2, 3], "offsets": [0, 2, 1]})
    assert bad.status_code == 422


def test_describe_reports_storage_for_every_model(dump):
    uri, sign, _, _ = dump
    c = ModelController(device="cpu")
    plain = c.create_model(uri, sign="plain")
    packed = c.create_model(uri, sign="packed", quantize="int8")
    a = plain.describe()["variables"][0]
    b = packed.describe()["variables"][0]
    assert a["storage"] == "fp32" and b["storage"] == "int8"
    assert a["table_bytes"] > 0 and 0 < b["table_bytes"] < a["table_bytes"]
    assert a["table_bytes"] == \
        plain.variables[0].shard.weights.numel() * 4
    assert packed.variables[0].storage == "int8"
    assert packed.variables[0].table_bytes == b["table_bytes"]


def test_unknown_quantize_is_422_and_registers_nothing(dump):
    uri, sign, _, _ = dump
    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    for bad in ("int4", "INT8", ""):
        r = client.post("/models", json={"model_uri": uri, "quantize": bad})
        assert r.status_code == 422, (bad, r.text)
    assert c.manager.signs() == []
    with pytest.raises(ValueError):
        c.create_model(uri, quantize="int4")
    with pytest.raises(ValueError):
        ServedModel("m", uri).load(quantize="bf16")
    assert c.manager.signs() == []


def test_float64_variable_is_refused(dump):
    uri, _, _, _ = dump
    m = ServedModel("m", uri)
    meta = read_meta(uri)
    meta["variables"][0]["datatype"] = "float64"
    import json
    with open(os.path.join(uri, "model_meta"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="float64"):
        m.load(quantize="int8")


def test_restore_from_quantized_replica_within_twice_the_bound(dump,
                                                               monkeypatch):
    """A replica restored from a quantized replica re-quantizes dequantized
    rows: not bit-identical to its source, but within twice the int8 bound
    of the original rows."""
    uri, sign, keys, rows = dump
    src = ModelController(device="cpu")
    src.create_model(uri, quantize="int8")
    src_client = TestClient(make_app(src))

    import requests

    class _Resp:
        def __init__(self, r):
            self._r = r

        def json(self):
            return self._r.json()

    def fake_get(url, params=None, timeout=None):
        assert url.startswith("http://replica")
        return _Resp(src_client.get(url[len("http://replica"):],
                                    params=params))

    monkeypatch.setattr(requests, "get", fake_get)
    dst = ModelController(device="cpu")
    m = dst.restore_model_from_replica("http://replica", sign,
                                       quantize="int8")
    assert m.describe()["variables"][0]["storage"] == "int8"
    shard = m.variables[0].shard
    assert isinstance(shard, QuantizedShard) and shard.num_rows == 5
    assert shard.slab.shape[0] == 5                     # reserved from total
    got = m.variables[0].pull_weights(keys)
    bound = qref.int8_bound(rows, ops.quantize_rows(rows, "int8"))
    err = (got.double() - rows.double()).abs().amax(1)
    print(f"worst err / (2 bound) = {float((err / (2 * bound)).max()):.4f}")
    assert bool((err <= 2 * bound).all())
    # restoring without quantize from the same replica gives fp32 tables
    # holding the dequantized rows
    m2 = ModelController(device="cpu").restore_model_from_replica(
        "http://replica", sign)
    assert m2.describe()["variables"][0]["storage"] == "fp32"
    assert torch.equal(m2.variables[0].pull_weights(keys),
                       src.manager.find_model_variable(sign, 0)
                       .pull_weights(keys))


def test_client_create_model_passes_quantize(dump, monkeypatch):
    uri, sign, _, _ = dump
    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    import requests

    def fake_request(method, url, json=None, timeout=None):
        return client.request(method, url[len("http://a"):], json=json)

    monkeypatch.setattr(requests, "request", fake_request)
    info = ServingClient(["http://a"]).create_model(uri, quantize="fp16")
    assert info["variables"][0]["storage"] == "fp16"
    assert c.manager.find_model_variable(sign, 0).storage == "fp16"


def test_cli_has_the_quantize_flag():
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "openembedding_amd.serving",
                        "--help"], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--quantize" in r.stdout and "int8" in r.stdout
    r = subprocess.run([sys.executable, "-m", "openembedding_amd.serving",
                        "--quantize", "int4"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "invalid choice" in r.stderr


def test_serve_quantized_example():
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "serve_quantized.py"),
         "--steps", "3", "--bags", "16"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (
        f"serve_quantized.py failed rc={r.returncode}\n"
        f"stdout:\n{r.stdout[-2000:]}\nstderr:\n{r.stderr[-2000:]}")
    assert "quantized serving: OK" in r.stdout
    assert "storage=int8" in r.stdout and "table bytes: fp32" in r.stdout
