"""child process of test_imported_mirror_refuses_by_name: imports a dense HNSW mirror by handle and asks it for the
vacuum-side entries.  argv: <npz with handle, n, m> <npz to write>"""
import sys

import numpy as np

from pgvector_amd import api


def main():
    job = np.load(sys.argv[1])
    ctx = api.Context(0)
    h = api.Hnsw.from_handle(ctx, job["handle"].tobytes(), api.PGV_F32)
    codes, texts = [], []
    for call in (lambda: h.set_live(np.ones(int(job["n"]), dtype=bool)),
                 lambda: h.repair_neighbors(np.arange(2, dtype=np.int32), int(job["m"]), 8, 1, 4)):
        try:
            call()
            codes.append(0)
            texts.append("")
        except api.PgvError as e:
            codes.append(e.code)
            texts.append(e.message)
    np.savez(sys.argv[2], codes=np.asarray(codes), texts=np.asarray(texts))
    h.close()
    ctx.close()


if __name__ == "__main__":
    main()
