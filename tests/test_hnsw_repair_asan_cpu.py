"""pgv_host_hnsw_repair's host logic under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
(tests/c/hnsw_repair_asan_driver.c against tests/c/mock_hip.c; the three device entries the mock lacks are stood in for
by the driver itself).  Its buffers are sized batch by batch and grow at different rates -- the selections, the back links,
the scoring requests, the patch -- so the runs vary the batch size: max_batch 1 walks the patch's totals across the first
powers of two, the large batches grow everything at once."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# batch sizes whose patches put the two patch arrays on different sides of a power of two: with one capacity shared by
# both (an earlier form of the driver) this very run writes past the tuples' buffer
RUNS = ["1", "2", "3", "5", "7", "11", "64", "1024"]


def test_repair_driver_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "hnsw_repair_asan")
    srcs = [os.path.join(ROOT, "tests", "c", "hnsw_repair_asan_driver.c"), os.path.join(ROOT, "tests", "c", "mock_hip.c")]
    srcs += sorted(glob.glob(os.path.join(ROOT, "pgvector_amd", "host", "*.c")))
    cc = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-rdynamic",
                         "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "c", "omp_stub"),
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pgvector_amd", "host")] + srcs +
                        ["-o", exe, "-lm", "-lpthread", "-lrt"], capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in cc.stderr.lower():
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    assert cc.returncode == 0, cc.stderr[-2000:]
    r = subprocess.run([exe, "700"] + RUNS, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count("rc 0 ") == len(RUNS) and "BROKEN" not in out, out[-2000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    # every run went through the overflow redo and the reselections: the paths whose buffers grow
    for line in [ln for ln in out.splitlines() if ln.startswith("rc 0 ")]:
        assert " redos 0 " not in line and " reselections 0 " not in line, line
