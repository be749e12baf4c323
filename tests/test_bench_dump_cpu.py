"""bench.py --dump-outputs: the arrays a run writes so that two builds can be compared output for output (no GPU needed
for this part; tests/test_bench_plain_gpu.py runs the benchmark itself)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def _arrays(rows, k=10):
    # every row carries its own index, so a sample shows which rows it kept
    idx = np.arange(rows, dtype=np.float64)[:, None]
    return {"distances": np.repeat(idx, k, axis=1).astype(np.float32), "tids": np.repeat(idx, k, axis=1) + 0.5}


def test_a_dump_under_the_cap_is_every_array_whole_in_its_dtype(tmp_path):
    bench = _bench()
    arrays = _arrays(1024)
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["distances.npy", "tids.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == a.dtype and got.shape == a.shape
        np.testing.assert_array_equal(got, a)


def test_a_dump_over_the_cap_is_the_same_seeded_sample_of_rows_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 10)
    rows = 4096
    arrays = _arrays(rows)
    total = sum(a.nbytes for a in arrays.values())
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {d: {n: np.load(tmp_path / d / (n + ".npy")) for n in arrays} for d in ("a", "b")}
    for n, a in arrays.items():
        np.testing.assert_array_equal(got["a"][n], got["b"][n])
        assert got["a"][n].dtype == a.dtype
    assert sum(x.nbytes for x in got["a"].values()) <= bench.DUMP_CAP_BYTES
    kept = got["a"]["distances"][:, 0].astype(np.int64)
    assert len(kept) == rows * bench.DUMP_CAP_BYTES // total
    # the same rows of every array, in their original order, each row whole
    assert (np.diff(kept) > 0).all() and kept[0] >= 0 and kept[-1] < rows
    np.testing.assert_array_equal(got["a"]["tids"][:, 0], kept + 0.5)
    np.testing.assert_array_equal(got["a"]["distances"], arrays["distances"][kept])
