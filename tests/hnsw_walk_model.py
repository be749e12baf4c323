"""Plain-Python model of the device's HNSW walk (hnsw_search_kernel, pgvector_amd/csrc/kernels_hnsw.hip), for
tests/test_hnsw_walk_model_cpu.py and tests/test_gpu_hnsw_ties.py: no GPU, no ctypes, distances from a callable.  On
integer-valued data fp32 arithmetic is exact, so Python integers are the device's distances.

It restates what the kernel documents, tie order and all:
  * layers run from levels[entry] down to 0, with ef_l = ef on layers <= qlevel and 1 above;
  * a layer starts with a fresh visited set holding the previous layer's W, every entry unexpanded again;
  * the next candidate is the first unexpanded entry of W; when W has none, the next unread entry of the tie list T;
  * its neighbours are its tuple's slots of this layer in tuple order, minus the visited ones (negative slots skipped);
  * on layers > 0 an element below the layer is scored, stays visited and is never admitted;
  * the scored batch is merged stably into W (old entries before batch entries of the same distance, batch entries in
    batch order) and W is truncated to ef_l;
  * T takes the unexpanded entries pushed out of a full W at exactly W's new furthest distance K: old entries first, in
    W's order, then the batch entries that had been admitted when their turn came and were pushed out by a later one.
    T and its read position stay while K stays, T is emptied when K moves, and it is read only when W has no unexpanded
    entry left;
  * scored counts layer 0's entry points and layer 0's batches.

"Admitted when its turn came" is decided here by replaying the reference's loop over the batch one element at a time
(`eDistance < f->distance || wlen < ef`, src/hnswutils.c:936), which also checks the kernel's claim that the stable
merge truncated to ef_l is what that loop leaves: the two are asserted equal on every batch.

tie_cap bounds T the way the kernel's array does (an append past it is lost); None is unbounded, and then |T| < ef_l is
asserted after every batch: once an entry leaves W at K while K is W's furthest distance, W is full of distances <= K, so
nothing at K is admitted any more -- everything that ever enters T at K was in W or admitted from the batch at that moment,
and one entry at K stays in W for K to remain its furthest."""
from collections import namedtuple

Walk = namedtuple("Walk", "ids dist scored layers counters")


def _neighbours(levels, nbr_start, nbr, m, c, lc):
    lm = 2 * m if lc == 0 else m
    o = int(nbr_start[c]) + (int(levels[c]) - lc) * m
    return [int(e) for e in nbr[o:o + lm] if e >= 0]


def walk(dist, levels, nbr_start, nbr, m, entry, ef, qlevel=0, tie_cap=None):
    """dist(e) -> the query's distance to element e.  Returns Walk(ids, dist: the final W nearest first; scored;
    layers: {lc: (ids, dist)} W of every layer <= qlevel; counters: old_appends, batch_appends, lost (to tie_cap), resets
    (of a non-empty T), reads, max_t)."""
    cnt = {"old_appends": 0, "batch_appends": 0, "lost": 0, "resets": 0, "reads": 0, "max_t": 0}
    if entry < 0:
        return Walk([], [], 0, {}, cnt)
    W = [[dist(entry), int(entry), False]]  # [distance, element, expanded], ascending
    scored, layers = 0, {}
    for lc in range(int(levels[entry]), -1, -1):
        ef_l = ef if lc <= qlevel else 1
        visited = {w[1] for w in W}
        for w in W:
            w[2] = False
        T, t_read, t_key = [], 0, None
        if lc == 0:
            scored += len(W)
        while True:
            cand = next((w for w in W if not w[2]), None)
            if cand is not None:
                cand[2] = True
                c = cand[1]
            elif t_read < len(T):
                c = T[t_read]
                t_read += 1
                cnt["reads"] += 1
            else:
                break
            batch = []
            for e in _neighbours(levels, nbr_start, nbr, m, c, lc):
                if e not in visited:
                    visited.add(e)
                    batch.append(e)
            if not batch:
                continue
            if lc == 0:
                scored += len(batch)
            batch = [(dist(e), e) for e in batch]
            if lc > 0:
                batch = [b for b in batch if levels[b[1]] >= lc]
            # the stable merge, truncated
            tagged = [(w[0], 0, j) for j, w in enumerate(W)] + [(b[0], 1, i) for i, b in enumerate(batch)]
            kept = sorted(tagged)[:ef_l]
            # the reference's loop over the same batch: who is admitted in their turn, and what it leaves
            sim, admitted = [(w[0], 0, j) for j, w in enumerate(W)], set()
            for i, b in enumerate(batch):
                if len(sim) < ef_l or b[0] < sim[-1][0]:
                    admitted.add(i)
                    at = len(sim)
                    while at > 0 and sim[at - 1][0] > b[0]:
                        at -= 1
                    sim.insert(at, (b[0], 1, i))
                    del sim[ef_l:]
            assert sim == kept, "the truncated stable merge is not what one-by-one admission leaves"
            if len(W) + len(batch) > ef_l:
                K = kept[-1][0]
                if T and t_key != K:
                    T, t_read = [], 0
                    cnt["resets"] += 1
                inside = set(kept)
                old = [W[j][1] for j in range(len(W)) if W[j][0] == K and not W[j][2] and (W[j][0], 0, j) not in inside]
                new = [b[1] for i, b in enumerate(batch) if b[0] == K and i in admitted and (b[0], 1, i) not in inside]
                for e, kind in [(e, "old_appends") for e in old] + [(e, "batch_appends") for e in new]:
                    if tie_cap is None or len(T) < tie_cap:
                        T.append(e)
                        cnt[kind] += 1
                    else:
                        cnt["lost"] += 1
                t_key = K
                cnt["max_t"] = max(cnt["max_t"], len(T))
                if tie_cap is None:
                    assert len(T) < ef_l, ("the tie list outgrew ef - 1", len(T), ef_l)
            W = [[k, W[i][1], W[i][2]] if o == 0 else [k, batch[i][1], False] for k, o, i in kept]
        if lc <= qlevel:
            layers[lc] = ([w[1] for w in W], [w[0] for w in W])
    return Walk([w[1] for w in W], [w[0] for w in W], scored, layers, cnt)


def tuples(m, levels, lists):
    """hand-written graphs: lists = {(element, layer): [neighbours]} -> (levels, nbr_start, nbr) in the neighbour-tuple
    layout ((level + 2) * m slots per element, layer lc at (level - lc) * m, -1 = empty)"""
    import numpy as np
    levels = np.asarray(levels, dtype=np.int32)
    start = np.concatenate([[0], np.cumsum((levels.astype(np.int64) + 2) * m)]).astype(np.int64)
    nbr = np.full(int(start[-1]), -1, dtype=np.int32)
    for (e, lc), ids in lists.items():
        assert lc <= levels[e] and len(ids) <= (2 * m if lc == 0 else m), (e, lc)
        o = int(start[e]) + (int(levels[e]) - lc) * m
        nbr[o:o + len(ids)] = ids
    return levels, start, nbr
