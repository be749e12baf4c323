"""A plain bench.py run does only what its headline figure needs, --full adds the rest, and --dump-outputs writes the
last timed step's answers: the same arrays from run to run with the same arguments, plain or --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--workload", "small", "--steps", "6", "--warmup", "2", "--settle-ms", "0"]


def _run(tmp_path, dump, extra=()):
    env = dict(os.environ)
    for k_ in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k_, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(tmp_path / dump)] +
                       list(extra), capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {n: np.load(tmp_path / dump / (n + ".npy")) for n in ("distances", "tids")}


def test_plain_runs_dump_the_same_answers_and_full_adds_recall(tmp_path):
    plain, a = _run(tmp_path, "a")
    assert plain["value"] > 0 and plain["steps"] == 6 and plain["ms_per_step"] > 0
    assert "recall_at_10" not in plain and "value_unsettled" not in plain and "parity" not in plain
    assert a["distances"].dtype == np.float32 and a["tids"].dtype == np.float64
    assert a["distances"].shape == a["tids"].shape == (1024, 10)
    assert (np.diff(a["distances"], axis=1) >= 0).all()
    assert (a["tids"] >= 0).all() and (a["tids"] < 100_000).all() and (a["tids"] == np.round(a["tids"])).all()
    _, b = _run(tmp_path, "b")
    full, c = _run(tmp_path, "c", ["--full", "--no-sweeps", "--no-traffic", "--no-cpu-baseline"])
    assert full["recall_at_10"] >= 0.99 and full["value_unsettled"] > 0
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])
        np.testing.assert_array_equal(a[n], c[n])
