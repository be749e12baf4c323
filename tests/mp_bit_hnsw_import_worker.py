"""child process of test_bit_mirror_across_processes: imports a bit HNSW mirror by handle, searches and scores it.
argv: <npz with handle, queries, ef, k, words> <npz to write>"""
import sys

import numpy as np

from pgvector_amd import api


def main():
    job = np.load(sys.argv[1])
    ctx = api.Context(0)
    h = api.BitHnsw.from_handle(ctx, job["handle"].tobytes())
    elem, dist, scored = h.search(job["queries"], int(job["ef"]), int(job["k"]))
    nq = job["queries"].shape[0]
    score = h.score(job["queries"], np.arange(nq, dtype=np.int32), np.arange(nq, dtype=np.int32))
    pay = h.get_payload(np.asarray(elem), words=int(job["words"]))
    np.savez(sys.argv[2], elem=np.asarray(elem), dist=np.asarray(dist), scored=np.asarray(scored), score=score, payload=pay)
    h.close()
    ctx.close()


if __name__ == "__main__":
    main()
