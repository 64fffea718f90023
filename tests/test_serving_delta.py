"""Live serving updates from delta checkpoints on the CPU: fp32, int8 and
fp16 tables updated in place answer exactly like a fresh load of the final
full dump; the REST route, the replica-restore pages after an update, the
refusals, and the example."""

import os
import subprocess
import sys

import pytest
import torch
from fastapi.testclient import TestClient

import delta_ref as dr
from openembedding_amd.serving import (ModelController, ServedModel,
                                       make_app)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    """One trained chain (A, D1, D2, B) per table kind, shared read-only."""
    out = {}
    for table in ("hash", "array"):
        tmp = tmp_path_factory.mktemp(f"chain_{table}")
        ctx, _st, _var, info = dr.run_chain(tmp, "cpu", table, "adagrad")
        ctx.finalize()
        out[table] = info["uri"]
    return out


@pytest.mark.parametrize("fmt", (None, "int8", "fp16"))
@pytest.mark.parametrize("table", ("hash", "array"))
def test_updated_model_equals_fresh_load(chains, table, fmt):
    m, fresh = dr.check_served_chain(chains[table], "cpu", fmt)
    if fmt is not None:     # the packed rows themselves, by key
        a = m.variables[0].shard
        b = fresh.variables[0].shard
        probe = torch.tensor(dr.PROBE[:-3])
        sa, sb = a._lookup_readonly(probe), b._lookup_readonly(probe)
        assert bool((sa >= 0).all()) and bool((sb >= 0).all())
        assert torch.equal(a.slab[sa], b.slab[sb])


def test_rest_route_and_replica_pages(chains):
    uri = chains["hash"]
    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    r = client.post("/models", json={"model_uri": uri["A"], "sign": "m"})
    assert r.status_code == 200 and r.json()["epoch"] == 1
    # warm the replica-restore cache, then update
    page = client.get("/models/m/variables/0/rows",
                      params={"start": 0, "count": 100000}).json()
    assert page["total"] == 1000
    r = client.post("/models/m/deltas", json={"model_uri": uri["D1"]})
    assert r.status_code == 200, r.text
    assert r.json()["epoch"] == 2 and r.json()["status"] == "NORMAL"
    assert client.get("/models/m").json()["epoch"] == 2
    r = client.post("/models/m/deltas", json={"model_uri": uri["D2"]})
    assert r.status_code == 200 and r.json()["epoch"] == 3

    fresh = ServedModel("fresh", uri["B"])
    fresh.load(device="cpu")
    want = fresh.variables[0].pull_weights(torch.tensor(dr.PROBE))
    r = client.post("/models/m/variables/0/pull",
                    json={"indices": dr.PROBE})
    assert torch.equal(torch.tensor(r.json()["weights"]), want)
    # the pages show the new rows: the export cache was invalidated
    page = client.get("/models/m/variables/0/rows",
                      params={"start": 0, "count": 100000}).json()
    assert page["total"] == 1060
    rows = dict(zip(page["keys"], page["weights"]))
    got = torch.tensor([rows[k] for k in dr.PROBE[:-3]])
    assert torch.equal(got, want[:-3])

    # refusals over REST: twice, unknown sign, a full dump, a missing path
    assert client.post("/models/m/deltas",
                       json={"model_uri": uri["D2"]}).status_code == 409
    assert client.post("/models/nope/deltas",
                       json={"model_uri": uri["D2"]}).status_code == 404
    assert client.post("/models/m/deltas",
                       json={"model_uri": uri["B"]}).status_code == 409
    assert client.post("/models/m/deltas",
                       json={"model_uri": uri["B"] + "x"}).status_code == 400
    assert client.get("/models/m").json()["epoch"] == 3


def test_refusals_leave_the_served_table_unchanged(chains):
    uri = chains["hash"]
    c = ModelController(device="cpu")
    m = c.create_model(uri["A"], sign="m")
    probe = torch.tensor(dr.PROBE)
    before = m.variables[0].pull_weights(probe)
    other = chains["array"]
    for bad in (uri["D2"], other["D1"], uri["A"]):
        with pytest.raises(RuntimeError):
            c.update_model("m", bad)
        assert torch.equal(m.variables[0].pull_weights(probe), before)
        assert m.loaded_epoch == 1
    with pytest.raises(KeyError):
        c.update_model("other", uri["D1"])
    # a delta is no base
    with pytest.raises(RuntimeError):
        c.create_model(uri["D1"], sign="d")
    assert c.manager.get("d") is None
    c.update_model("m", uri["D1"])
    with pytest.raises(RuntimeError):
        c.update_model("m", uri["D1"])
    assert m.loaded_epoch == 2


@pytest.mark.parametrize("fmt", ("int8", "fp16"))
def test_quantized_update_copies_the_slab_only_to_grow(chains, fmt):
    """An update makes room only when the delta could outgrow the slab, and
    then by half: D1 (50 new keys on a slab reserved for exactly 1000)
    regrows it to 1500 rows, D2 (10 new keys) fits and must leave the slab
    where it is."""
    uri = chains["hash"]
    m = ServedModel("m", uri["A"])
    m.load(device="cpu", quantize=fmt)
    sh = m.variables[0].shard
    assert sh.slab.shape[0] == sh.num_rows == 1000
    m.apply_delta(uri["D1"])
    assert sh.slab.shape[0] == 1500 and sh.num_rows == 1050
    ptr = sh.slab.data_ptr()
    m.apply_delta(uri["D2"])
    assert sh.slab.data_ptr() == ptr and sh.slab.shape[0] == 1500
    assert sh.num_rows == 1060


def test_rows_a_packed_format_cannot_hold_are_422(tmp_path):
    """fp16 overflow in the delta's second block: the route answers 422, the
    first block stays applied, the epoch does not move, and the corrected
    delta still applies."""
    from openembedding_amd import checkpoint
    ctx, st, var = dr.make_trainer()
    dr.train(st, var, list(range(100)), 1)
    base, bad, good = (str(tmp_path / n) for n in ("base", "bad", "good"))
    checkpoint.dump_model(ctx, base)
    sh = var.shard
    first = torch.arange(0, 10)
    sh.import_rows(first, torch.full((10, dr.DIM), 2.0))
    sh.import_rows(torch.tensor([50]), torch.full((1, dr.DIM), 1e6))
    old = checkpoint.BLOCK_ROWS
    checkpoint.BLOCK_ROWS = 10          # key 50 lands in the second block
    try:
        checkpoint.dump_delta(ctx, bad)
    finally:
        checkpoint.BLOCK_ROWS = old
    sh.import_rows(torch.tensor([50]), torch.full((1, dr.DIM), 3.0))
    checkpoint.dump_delta(ctx, good, since=2)
    ctx.finalize()

    c = ModelController(device="cpu")
    client = TestClient(make_app(c))
    r = client.post("/models", json={"model_uri": base, "sign": "m",
                                     "quantize": "fp16"})
    assert r.status_code == 200, r.text
    r = client.post("/models/m/deltas", json={"model_uri": bad})
    assert r.status_code == 422, r.text
    assert client.get("/models/m").json()["epoch"] == 1
    v = c.manager.find_model_variable("m", 0)
    assert bool((v.pull_weights(first) == 2.0).all())       # block 1 applied
    r = client.post("/models/m/deltas", json={"model_uri": good})
    assert r.status_code == 200 and r.json()["epoch"] == 3
    assert bool((v.pull_weights(torch.tensor([50])) == 3.0).all())


def test_online_update_example():
    env = dict(os.environ, OMP_NUM_THREADS="2", OEAMD_DEVICE="cpu")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "online_update.py")],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "updated model equals a fresh load: OK" in r.stdout
