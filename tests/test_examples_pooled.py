"""Smoke-run examples/serve_multihot.py on CPU (tiny sizes), in the style of
tests/test_examples.py: train a bag, dump it, serve it, query pull_pooled."""

import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_serve_multihot():
    pytest.importorskip("fastapi")
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "serve_multihot.py"),
         "--steps", "3", "--bags", "16"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (
        f"serve_multihot.py failed rc={r.returncode}\n"
        f"stdout:\n{r.stdout[-2000:]}\nstderr:\n{r.stderr[-2000:]}")
    assert "pooled serving matches evaluation: OK" in r.stdout
