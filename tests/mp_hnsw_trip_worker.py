"""Run by tests/test_gpu_hnsw_ties.py in a process of its own under the PGV_HNSW_ROWS_PER_TRIP the parent chose (the library
reads it once per process): the tie-heavy random set of tests/hnsw_tie_cases.py over fp32 and fp16 rows, every metric and
every (ef, k), plus one walk over non-integer normal data (dim 136, fp16 rows).  Saves every output in the .npz named on
the command line; the parent compares the files of the three row-scoring forms byte for byte."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hnsw_tie_cases as tc  # noqa: E402
from helpers import gen  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from pgvector_amd import api  # noqa: E402

METRIC = {"l2": api.PGV_L2SQ, "negip": api.PGV_NEG_IP, "l1": api.PGV_L1}


def main():
    oracle = po.Oracle()
    ctx = api.Context(0)
    out = {}
    for form in tc.METRICS:
        elements, queries, ex, _ = tc.random_graph(oracle, form)
        for name, dtype in (("f32", api.PGV_F32), ("f16", api.PGV_F16)):
            h = api.Hnsw(ctx, METRIC[form], dtype, tc.RDIM, elements)
            h.set_graph(8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
            for ef, k in tc.ef_k():
                elem, dist, scored = h.search(queries, ef, k)
                key = "%s_%s_%d_%d" % (form, name, ef, k)
                out[key + "_elem"], out[key + "_dist"], out[key + "_scored"] = elem, dist, scored
            h.close()
    data = gen(1500, 136, seed=51, dist="normal").astype(np.float16)
    g = po.HnswGraph(oracle, po.OPS_L2, po.ORA_F32, data.astype(np.float32), m=8, ef_construction=32, seed=7)
    ex = g.export_tuples()
    g.close()
    h = api.Hnsw(ctx, api.PGV_L2SQ, api.PGV_F16, 136, data[ex["rows"]])
    h.set_graph(8, ex["entry"], ex["levels"], ex["nbr_start"], ex["nbr"])
    out["normal_elem"], out["normal_dist"], out["normal_scored"] = h.search(gen(48, 136, seed=52, dist="normal"), 64, 10)
    h.close()
    ctx.close()
    np.savez(sys.argv[1], **out)
    print("TRIP-OK %s %d" % (os.environ.get("PGV_HNSW_ROWS_PER_TRIP"), len(out)))


if __name__ == "__main__":
    main()
