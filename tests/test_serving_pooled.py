"""Serving a trained EmbeddingBag: ``pull_pooled`` through the served
variable, the REST route and ServingClient equals pooling the rows ``/pull``
returns, and malformed bags are refused before any lookup runs."""

import pytest
import torch
from fastapi.testclient import TestClient

import openembedding_amd.torch as embed
from openembedding_amd.ops.dispatch import pool_rows
from openembedding_amd.serving import (ModelController, ServingClient,
                                       make_app)

MODES = ["sum", "mean", "sqrtn"]
DIM = 4
VALUES = [5, 9, 9, 31, 77, 5, 12, 40, 3]    # 77 and 40 were never trained
OFFSETS = [0, 2, 2, 6, 8]                   # an empty bag; values[8] unused
WEIGHTS = [0.5, -1.25, 2.0, 1.0, 3.0, 0.25, 1.5, -0.75, 9.0]


@pytest.fixture()
def served(tmp_path):
    """Train a small bag 2 steps, dump it, load it for serving."""
    torch.manual_seed(3)
    emb = embed.EmbeddingBag(-1, DIM, mode="mean")
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
    c = ModelController()
    c.create_model(uri)
    return c, sign, TestClient(make_app(c))


def _url(sign, vid=0, route="pull_pooled"):
    return f"/models/{sign}/variables/{vid}/{route}"


def _expected(client, sign, mode, weights):
    """Pool the flat rows the /pull route returns."""
    r = client.post(_url(sign, route="pull"), json={"indices": VALUES})
    assert r.status_code == 200
    rows = torch.tensor(r.json()["weights"])
    assert bool((rows[4] == 0).all()) and bool((rows[0] != 0).any())
    w = None if weights is None else torch.tensor(weights)
    return pool_rows(rows, torch.tensor(OFFSETS), mode, weights=w)[0]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_object_rest_and_client_equal_pooling_pulled_rows(served, mode,
                                                          weighted,
                                                          monkeypatch):
    c, sign, client = served
    weights = WEIGHTS if weighted else None
    want = _expected(client, sign, mode, weights)
    assert want.shape == (len(OFFSETS) - 1, DIM)

    var = c.manager.find_model_variable(sign, 0)
    got = var.pull_pooled(VALUES, OFFSETS, mode, weights)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-7)
    got_t = var.pull_pooled(torch.tensor(VALUES), torch.tensor(OFFSETS), mode,
                            None if weights is None
                            else torch.tensor(weights))
    assert torch.equal(got_t, got)

    body = {"values": VALUES, "offsets": OFFSETS, "mode": mode}
    if weighted:
        body["per_sample_weights"] = weights
    r = client.post(_url(sign), json=body)
    assert r.status_code == 200
    torch.testing.assert_close(torch.tensor(r.json()["pooled"]), want,
                               rtol=1e-6, atol=1e-7)

    # ServingClient over the same app: the first replica is down, so the
    # call must fail over to the second
    import requests
    calls = []

    def fake_request(method, url, json=None, timeout=None):
        calls.append(url)
        if url.startswith("http://down"):
            raise requests.ConnectionError("replica down")
        return client.request(method, url[len("http://up"):], json=json)

    monkeypatch.setattr(requests, "request", fake_request)
    sc = ServingClient(["http://down", "http://up"])
    pooled = sc.pull_pooled(sign, 0, torch.tensor(VALUES), OFFSETS, mode,
                            weights)
    assert len(calls) == 2 and calls[1].startswith("http://up")
    torch.testing.assert_close(torch.tensor(pooled), want, rtol=1e-6,
                               atol=1e-7)


def test_default_mode_is_sum(served):
    c, sign, client = served
    r = client.post(_url(sign), json={"values": VALUES, "offsets": OFFSETS})
    assert r.status_code == 200
    torch.testing.assert_close(torch.tensor(r.json()["pooled"]),
                               _expected(client, sign, "sum", None),
                               rtol=1e-6, atol=1e-7)


BAD = {
    "decreasing offsets": dict(values=VALUES, offsets=[0, 4, 2, 6]),
    "offsets past values": dict(values=VALUES, offsets=[0, 4, 10]),
    "offsets not from 0": dict(values=VALUES, offsets=[1, 4]),
    "empty offsets": dict(values=VALUES, offsets=[]),
    "nested offsets": dict(values=VALUES, offsets=[[0, 2]]),
    "float values": dict(values=[1.5, 2.0], offsets=[0, 2]),
    "short weights": dict(values=VALUES, offsets=OFFSETS,
                          per_sample_weights=WEIGHTS[:-1]),
    "unknown mode": dict(values=VALUES, offsets=OFFSETS, mode="max"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_malformed_request_is_422(served, case):
    c, sign, client = served
    r = client.post(_url(sign), json=BAD[case])
    assert r.status_code == 422, r.text
    var = c.manager.find_model_variable(sign, 0)
    kw = dict(BAD[case])
    with pytest.raises(ValueError):
        var.pull_pooled(kw.pop("values"), kw.pop("offsets"), **kw)


@pytest.mark.parametrize("bad", ["NaN", "Infinity"])
def test_non_finite_weight_is_422(served, bad):
    c, sign, client = served
    # a JSON encoder refuses NaN, so the body is written by hand
    body = ('{"values": [5, 9], "offsets": [0, 2], "mode": "mean", '
            '"per_sample_weights": [1.0, %s]}' % bad)
    r = client.post(_url(sign), content=body,
                    headers={"content-type": "application/json"})
    assert r.status_code == 422, r.text
    var = c.manager.find_model_variable(sign, 0)
    with pytest.raises(ValueError):
        var.pull_pooled([5, 9], [0, 2], "mean", [1.0, float(bad)])


def test_unknown_variable_and_model_are_404(served):
    c, sign, client = served
    body = {"values": VALUES, "offsets": OFFSETS}
    assert client.post(_url(sign, vid=9), json=body).status_code == 404
    assert client.post(_url("nope"), json=body).status_code == 404


def test_lookup_inserts_nothing(served):
    c, sign, client = served
    var = c.manager.find_model_variable(sign, 0)
    n0 = var.shard.num_rows
    out = var.pull_pooled([1000, 1001, 1002], [0, 3], "sum")
    assert torch.equal(out, torch.zeros(1, DIM))
    assert var.shard.num_rows == n0
