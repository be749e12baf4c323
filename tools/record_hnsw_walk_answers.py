#!/usr/bin/env python3
"""Records tests/golden/hnsw_walk_parent_answers.json: what the loaded library answers to the cases of
tests/hnsw_walk_steps_cases.py.  tests/test_gpu_hnsw_walk_steps.py holds every later hnsw_search_kernel to these answers,
so record them from the commit whose walk is the yardstick: build that commit's library somewhere else and name it in
PGV_HIP_LIB.

    PGV_HIP_LIB=/path/to/that/libpgv_hip.so python tools/record_hnsw_walk_answers.py [OUT.json]

Needs a GPU.  The file holds the cases' names and outputs only; the inputs are seeds in the cases module."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hnsw_walk_steps_cases as cases  # noqa: E402
from pgvector_amd import _lib, api  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "hnsw_walk_parent_answers.json")
    ctx = api.Context(0, stream=0)
    got = cases.answers(ctx)
    ctx.close()
    with open(out, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in got.items()) + "\n}\n")
    print("%d cases from %s -> %s (%d bytes)" % (len(got), _lib.LIB_PATH, out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
