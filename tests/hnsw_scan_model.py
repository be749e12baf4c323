"""Plain-Python models of an HNSW iterative scan, for tests/test_hnsw_scan_model_cpu.py and tests/test_gpu_hnsw_scan.py: no
GPU, no ctypes, distances from a callable, graphs in the neighbour-tuple layout (hnsw_walk_model.tuples).

ref_scan is the reference transliterated: GetScanItems / ResumeScanItems (src/hnswscan.c:25-87) over HnswSearchLayer
(src/hnswutils.c:824-987) with real heaps (heapq; equal distances leave a heap in insertion order, one of the orders the
reference's pairing heaps may produce).

model_scan is the device's array form (pgv_hnsw_scan_*, hnsw_search_kernel's SCAN form): hnsw_walk_model.walk's layer
loop -- W ascending with expanded flags, the tie list T, the stable merge -- plus a POOL per query:
  * during a layer-0 batch everything the truncated stable merge leaves past position ef is appended: the old entries of
    W that were pushed out, in W's order, then the batch entries that did not fit, in batch order (an entry that also
    enters T still goes to the pool); upper layers discard nothing;
  * a resumed batch takes the ef pool entries smallest by (distance, pool position) out of the pool (the rest keep their
    order); they become W in that order, all unexpanded, T empty; the visited set carries over and the entry points are
    not counted again;
  * drain(count) takes the count smallest the same way and walks nothing.
Without ties the two give the same batches; with ties they may differ in the order among equal distances only."""
import heapq
import itertools

from hnsw_walk_model import _neighbours


def ref_scan(dist, levels, nbr_start, nbr, m, entry, ef, max_batches=10 ** 9):
    """-> [(ids, dist, tuples)] per batch, nearest first, until `discarded` is empty (or max_batches)"""
    if entry < 0:
        return []
    tick = itertools.count()
    state = {"visited": set(), "discarded": [], "tuples": 0}

    def search_layer(ep, ef_l, lc, visited, discarded, init_visited, count):
        C, W = [], []
        for d, e in ep:
            if init_visited:
                visited.add(e)
                if count:
                    state["tuples"] += 1
            heapq.heappush(C, (d, next(tick), e))
            heapq.heappush(W, (-d, next(tick), e))
        wlen = len(ep)
        while C:
            d, _, c = heapq.heappop(C)
            if d > -W[0][0]:
                break
            unvisited = []
            for e in _neighbours(levels, nbr_start, nbr, m, c, lc):
                if e not in visited:
                    visited.add(e)
                    unvisited.append(e)
            if count:
                state["tuples"] += len(unvisited)
            for e in unvisited:
                always = wlen < ef_l
                ed, f = dist(e), -W[0][0]
                if not (ed < f or always):
                    if discarded is not None:
                        heapq.heappush(discarded, (ed, next(tick), e))
                    continue
                if levels[e] < lc:
                    continue
                heapq.heappush(C, (ed, next(tick), e))
                heapq.heappush(W, (-ed, next(tick), e))
                wlen += 1
                if wlen > ef_l:
                    nd, _, x = heapq.heappop(W)
                    if discarded is not None:
                        heapq.heappush(discarded, (-nd, next(tick), x))
        return sorted(((-nd, t, e) for nd, t, e in W))

    def batch(w):
        return [e for _, _, e in w], [d for d, _, _ in w], state["tuples"]

    ep = [(dist(entry), int(entry))]
    for lc in range(int(levels[entry]), 0, -1):
        ep = [(d, e) for d, _, e in search_layer(ep, 1, lc, set(), None, True, False)]
    out = [batch(search_layer(ep, ef, 0, state["visited"], state["discarded"], True, True))]
    while state["discarded"] and len(out) < max_batches:
        ep = []
        for _ in range(ef):
            if not state["discarded"]:
                break
            d, _, e = heapq.heappop(state["discarded"])
            ep.append((d, e))
        out.append(batch(search_layer(ep, ef, 0, state["visited"], state["discarded"], False, True)))
    return out


class model_scan:
    """model_scan(dist, levels, nbr_start, nbr, m, entry, ef): one query's scan in the device's array form.
    next() -> (ids, dist, tuples) of the next batch, ids == [] once exhausted; drain(count) -> (ids, dist);
    run() -> every remaining batch; set_graph(...) swaps the graph between batches (pgv_hnsw_update_graph);
    pool: the live discarded candidates [(distance, element)]; max_pool: the most there ever were"""

    def __init__(self, dist, levels, nbr_start, nbr, m, entry, ef):
        self.dist, self.ef = dist, ef
        self.set_graph(levels, nbr_start, nbr, m, entry)
        self.visited, self.pool, self.tuples, self.started, self.max_pool = set(), [], 0, False, 0

    def set_graph(self, levels, nbr_start, nbr, m, entry):
        self.graph = (levels, nbr_start, nbr, m)
        self.entry = int(entry)

    def _layer(self, W, ef_l, lc, visited, pool):
        """hnsw_walk_model.walk's loop over one layer, W's entries unexpanded; pool: where a layer-0 batch's discards go"""
        levels, nbr_start, nbr, m = self.graph
        dist = self.dist
        T, t_read, t_key = [], 0, None
        while True:
            cand = next((w for w in W if not w[2]), None)
            if cand is not None:
                cand[2] = True
                c = cand[1]
            elif t_read < len(T):
                c = T[t_read]
                t_read += 1
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
                self.tuples += len(batch)
            batch = [(dist(e), e) for e in batch]
            if lc > 0:
                batch = [b for b in batch if levels[b[1]] >= lc]
            tagged = [(w[0], 0, j) for j, w in enumerate(W)] + [(b[0], 1, i) for i, b in enumerate(batch)]
            merged = sorted(tagged)
            kept, out = merged[:ef_l], merged[ef_l:]
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
            if out:
                K = kept[-1][0]
                if T and t_key != K:
                    T, t_read = [], 0
                inside = set(kept)
                T += [W[j][1] for j in range(len(W)) if W[j][0] == K and not W[j][2] and (W[j][0], 0, j) not in inside]
                T += [b[1] for i, b in enumerate(batch) if b[0] == K and i in admitted and (b[0], 1, i) not in inside]
                t_key = K
                assert len(T) < ef_l, ("the tie list outgrew ef - 1", len(T), ef_l)
                if pool is not None:
                    outs = set(out)
                    pool.extend((W[j][0], W[j][1]) for j in range(len(W)) if (W[j][0], 0, j) in outs)
                    pool.extend(b for i, b in enumerate(batch) if (b[0], 1, i) in outs)
                    self.max_pool = max(self.max_pool, len(pool))
            W = [[k, W[i][1], W[i][2]] if o == 0 else [k, batch[i][1], False] for k, o, i in kept]
        return W

    def _take(self, count):
        order = sorted(range(len(self.pool)), key=lambda p: (self.pool[p][0], p))[:count]
        taken, gone = [self.pool[p] for p in order], set(order)
        self.pool[:] = [x for p, x in enumerate(self.pool) if p not in gone]
        return taken

    def next(self):
        levels = self.graph[0]
        if not self.started:
            self.started = True
            if self.entry < 0:
                return [], [], 0
            W = [[self.dist(self.entry), self.entry, False]]
            for lc in range(int(levels[self.entry]), 0, -1):
                W = self._layer(W, 1, lc, {w[1] for w in W}, None)
                for w in W:
                    w[2] = False
            self.visited = {w[1] for w in W}
            self.tuples += len(W)
        else:
            W = [[d, e, False] for d, e in self._take(self.ef)]
            if not W:
                return [], [], self.tuples
        W = self._layer(W, self.ef, 0, self.visited, self.pool)
        return [w[1] for w in W], [w[0] for w in W], self.tuples

    def drain(self, count):
        taken = self._take(count)
        return [e for _, e in taken], [d for d, _ in taken]

    def run(self, max_batches=10 ** 9):
        out = []
        while len(out) < max_batches:
            b = self.next()
            if not b[0]:
                break
            out.append(b)
        return out

    def iterative_search(self, k, keep, max_scan_tuples=20000, strict=False):
        """hnswgettuple's loop (src/hnswscan.c:242-327) over this scan: batches nearest first through the filter `keep`
        (indexable by element), `strict` dropping an element nearer than the last one emitted (:313-319), k results at the
        most; once tuples >= max_scan_tuples the remaining pool entries come out nearest first instead of another walk
        (:259-266).  -> (ids, dist, tuples)"""
        ids, ds, prev = [], [], float("-inf")
        while len(ids) < k:
            if self.started and self.tuples >= max_scan_tuples:
                e, d = self.drain(self.ef)
            else:
                e, d, _ = self.next()
            if not e:
                break
            for x, dx in zip(e, d):
                if len(ids) >= k:
                    break
                if strict:
                    if dx < prev:
                        continue
                    prev = dx
                if keep[x]:
                    ids.append(x)
                    ds.append(dx)
        return ids, ds, self.tuples
