"""The in-memory HNSW build's graph updates as the reference states them, on the host: the model that the device's
pgv_hnsw_link_* (csrc/kernels_hnsw_link.hip, csrc/hnsw_link_core.h) is held to in tests/test_gpu_hnsw_link_edges.py, and
that tests/test_hnsw_link_model_cpu.py pins to the oracle (oracle/oracle_hnsw.c: ora_hnsw_update_connections /
ora_hnsw_set_neighbors).

Written from the reference's src/hnswutils.c:992-1231 (CompareCandidateDistances, CheckElementCloser, SelectNeighbors,
HnswUpdateConnection) and src/hnswbuild.c:376-431 (HnswUpdateNeighborsInMemory, the order requests are applied in) -- not
from csrc/hnsw_link_core.h.

  select_recompute   Algorithm 4 with every `closer` flag recomputed: the authority for results
  select_cached      the reference's cached form (:1098-1140) stated literally; an instrument: which pair distances it
                     looks up, and whether a list's replay on the device has to wait for its member triangle
  update_connection  HnswUpdateConnection
  link_batch         one batch of (new element, chosen neighbor, layer) requests in the reference's order
  host_select        the plain sweep of SelectNeighbors for a new element's own list (no cached flags)
  scenarios          hand-made batches on integer grids that cross the device code's edges

Coordinates are small integers (|x| <= 16, dim <= 8): every squared L2 distance and inner product is an integer below
2^24, exact in fp32 (and the rows exact in fp16 storage) in any summation order, so the device, numpy and the oracle agree
bit for bit and ties are plentiful."""
import numpy as np

L2, IP = "l2", "ip"              # squared L2 / negative inner product: FUNCTION 1 of the two opclasses


# ------------------------------------------------------------------------------------------------------------ distances
_SCRATCH = {}


def pair_matrix(rows, metric, idx, reuse=False):
    """the distances between rows[idx], fp32 (exact: integers).  reuse: into a buffer kept per size, valid until the next
    such call (update_connection's: a fresh 160 KB array per update costs more than the arithmetic)"""
    x = (rows if reuse else np.asarray(rows, dtype=np.float32))[np.asarray(idx, dtype=np.int64)]
    n = len(x)
    if reuse:
        if n not in _SCRATCH:
            _SCRATCH[n] = (np.empty((n, n), np.float32), np.empty((n, n), np.float32))
        g, out = _SCRATCH[n]
        np.matmul(x, x.T, out=g)
    else:
        g, out = x @ x.T, np.empty((n, n), np.float32)
    if metric == IP:
        return np.negative(g, out=out)
    n2 = g.diagonal().copy()
    np.add(n2[:, None], n2[None, :], out=out)
    np.subtract(out, g, out=out)
    return np.subtract(out, g, out=out)


def distances_to(rows, metric, e, idx):
    x = np.asarray(rows, dtype=np.float32)
    y = x[np.asarray(idx, dtype=np.int64)]
    if metric == IP:
        return -(y @ x[e])
    d = y - x[e]
    return np.einsum("ij,ij->i", d, d)


# ------------------------------------------------------------------------------------------------------ SelectNeighbors
def _order(elem, dist):
    """list_sort(w, CompareCandidateDistances) (:992-1010) is descending by (distance, element) and the loop takes
    candidates from its end: the order they are looked at is ascending by (distance, element id).  -0.0 == 0.0."""
    return np.lexsort((np.asarray(elem), np.asarray(dist, dtype=np.float32) + np.float32(0.0)))


def select_recompute(elem, dist, D, lm, order=None):
    """Algorithm 4 (:1064-1165) over candidates 0 .. nc - 1 (nc > lm), every flag recomputed.
    CheckElementCloser(e, r) is `no x in r with D[e, x] <= dist[e]`; it is kept as a mask that every accepted x extends.
    -> (r: the selection in r's order, closer: flag per candidate or -1 where the loop never looked, pruned)"""
    dist = np.asarray(dist, dtype=np.float32)
    nc = len(elem)
    order = _order(elem, dist) if order is None else order
    not_closer = np.zeros(nc, dtype=bool)
    closer = np.full(nc, -1, dtype=np.int8)
    r, wd, p = [], [], 0
    while p < nc and len(r) < lm:
        # a rejection changes nothing the loop depends on: the candidates up to the next one that is still closer are
        # rejected one after the other, then that one is accepted
        rest = not_closer[order[p:]]
        k = len(rest) if rest.all() else int(np.argmin(rest))
        if k:
            closer[order[p:p + k]] = 0
            wd += order[p:p + k].tolist()
        p += k
        if p < nc:
            e = int(order[p])
            closer[e] = 1
            r.append(e)
            not_closer |= D[e] <= dist
            p += 1
    wdoff = 0
    while wdoff < len(wd) and len(r) < lm:          # keep pruned connections (:1146-1148)
        r.append(wd[wdoff])
        wdoff += 1
    pruned = wd[wdoff] if wdoff < len(wd) else int(order[-1])      # :1150-1157 (else: the furthest)
    return r, closer, pruned


def select_cached(elem, dist, D, lm, cf, closer_set, loc=None, frm=1, order=None):
    """The reference's cached form (:1098-1140): candidate nc - 1 is the newcomer, cf the `closer` flags the list's last
    selection left, closer_set the list's closerSet.  loc / frm: each candidate's local in the batch's record and the
    first local whose pairs the first round fetches -- a pair of two locals below frm is member-member and unfetched.
    -> dict(r, closer (the flags after this call, per candidate), pruned, lookups, removed_any, readded,
            wait_in_order: looking the pairs up in order, an unfetched one comes before a deciding one (what
                           pgv_link_check_closer meets), wait_any: some check's set holds an unfetched pair (what the
                           wavefront kernel's ballot meets))"""
    dist = np.asarray(dist, dtype=np.float32)
    nc = len(elem)
    new = nc - 1
    if loc is None:
        loc = list(range(nc))
    order = (_order(elem, dist) if order is None else order).tolist()
    must_calculate = not closer_set
    out = dict(lookups=0, removed_any=False, readded=False, wait_in_order=False, wait_any=False)
    flags = [int(f) for f in cf]

    def check(e, against):           # CheckElementCloser(e, against) (:1040-1059)
        de, le = dist[e], loc[e]
        verdict, stopped = 1, False
        for x in against:
            unfetched = le < frm and loc[x] < frm
            if unfetched:
                out["wait_any"] = True
            if not stopped:
                out["lookups"] += 1
                if unfetched:
                    out["wait_in_order"] = True
                if D[e, x] <= de:
                    verdict, stopped = 0, True
        return verdict

    r, wd, added = [], [], []
    for e in order:
        if len(r) >= lm:
            break
        closer = flags[e]
        if must_calculate:
            closer = check(e, r)
        elif added:
            if closer:
                closer = check(e, added)
                if not closer:
                    out["removed_any"] = True
            elif out["removed_any"]:
                closer = check(e, r)
                if closer:
                    added.append(e)
                    out["readded"] = True
        elif e == new:
            closer = check(e, r)
            if closer:
                added.append(e)
        flags[e] = closer
        (r if closer else wd).append(e)
    wdoff = 0
    while wdoff < len(wd) and len(r) < lm:
        r.append(wd[wdoff])
        wdoff += 1
    out.update(r=r, closer=flags, pruned=wd[wdoff] if wdoff < len(wd) else int(order[-1]))
    return out


def host_select(ids, dist, tri, lm):
    """src/hnswutils.c:1064-1165 for a list without cached flags, candidates nearest first, pair distances in the
    (u, v < u) triangle: (neighbors, distances, closer flags) in r's order"""
    nw = len(ids)
    if nw <= lm:
        return ids[::-1].tolist(), dist[::-1].tolist(), [0] * nw
    chosen, looked = [], 0
    for j in range(nw):
        if len(chosen) >= lm:
            break
        looked = j + 1
        if all(tri[j * (j - 1) // 2 + r] > dist[j] for r in chosen):
            chosen.append(j)
    order = list(chosen)
    for x in range(looked):
        if len(order) >= lm:
            break
        if x not in chosen:
            order.append(x)
    return [int(ids[x]) for x in order], [float(dist[x]) for x in order], [1 if i < len(chosen) else 0 for i in range(len(order))]


# ---------------------------------------------------------------------------------------------------- the graph's lists
class NeighborList:
    __slots__ = ("elem", "dist", "cf", "closer_set", "loc", "nstart", "frm", "nnew", "wait_in_order", "wait_any", "batch")

    def __init__(self):
        self.elem, self.dist, self.cf, self.closer_set = [], [], [], False
        self.batch = -1


def group_pairs(n, frm):
    """pairs (u, v < u) with u >= frm among n locals"""
    frm = max(frm, 1)
    return (n * (n - 1) - frm * (frm - 1)) // 2 if n > frm else 0


class Graph:
    """lists[(element, layer)] -> NeighborList; every list starts empty"""

    def __init__(self, rows, metric, m, levels):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.metric, self.m = metric, int(m)
        self.levels = np.ascontiguousarray(levels, dtype=np.int32)
        self.lists = {}
        self.nbatch = 0
        self.events = []         # one dict per overflowing update (see update_connection)

    def lm(self, lc):
        return 2 * self.m if lc == 0 else self.m       # HnswGetLayerM

    def list_of(self, e, lc):
        key = (int(e), int(lc))
        lst = self.lists.get(key)
        if lst is None:
            lst = self.lists[key] = NeighborList()
        return lst

    def tuples(self):
        """the neighbor tuples as the index stores them: (level + 2) * m slots per element, layer lc at (level - lc) * m"""
        m = self.m
        start = np.zeros(len(self.levels) + 1, np.int64)
        start[1:] = np.cumsum((self.levels.astype(np.int64) + 2) * m)
        nbr = np.full(int(start[-1]), -1, np.int32)
        for (e, lc), lst in self.lists.items():
            o = int(start[e]) + (int(self.levels[e]) - lc) * m
            nbr[o:o + len(lst.elem)] = lst.elem
        return start, nbr


def _record(g, lst):
    """the list's record of the current batch: its members' locals, what the first round fetches"""
    if lst.batch != g.nbatch:
        lst.batch = g.nbatch
        lst.nstart = len(lst.elem)
        lst.frm = max(lst.nstart, 1) if lst.closer_set else 1
        lst.loc = list(range(lst.nstart))
        lst.nnew = 0
        lst.wait_in_order = lst.wait_any = False


def update_connection(g, owner, lc, new_element, distance, literal_below=66):
    """HnswUpdateConnection (:1183-1231): append while the list has room; otherwise SelectNeighbors over the list plus the
    newcomer and the pruned item replaced in its place -- nothing changes when the newcomer itself is pruned.
    Both forms of the selection run and are compared (select_cached literally wherever the list has cached flags or is
    short; with closerSet clear its loop IS Algorithm 4's, which is what the long lists then run alone)."""
    lst = g.list_of(owner, lc)
    lm = g.lm(lc)
    _record(g, lst)
    local = lst.nstart + lst.nnew
    lst.nnew += 1
    if len(lst.elem) < lm:
        lst.elem.append(int(new_element))
        lst.dist.append(float(distance))
        lst.cf.append(0)
        lst.loc.append(local)
        return
    elem = lst.elem + [int(new_element)]
    dist = np.asarray(lst.dist + [float(distance)], dtype=np.float32)
    loc = lst.loc + [local]
    D = pair_matrix(g.rows, g.metric, elem, reuse=True)
    order = _order(elem, dist)
    r, closer, pruned = select_recompute(elem, dist, D, lm, order)
    ev = dict(owner=int(owner), lc=int(lc), m=g.m, batch=g.nbatch, pruned=pruned, new_pruned=pruned == lm,
              closer_set=lst.closer_set, mismatch=False, removed_readded=False,
              mixed_signs=bool((dist < 0).any() and (dist > 0).any()))
    if lst.closer_set or len(elem) < literal_below:
        c = select_cached(elem, dist, D, lm, lst.cf + [0], lst.closer_set, loc, lst.frm, order)
        looked = closer >= 0
        ev["mismatch"] = not (c["r"] == r and c["pruned"] == pruned and
                              [c["closer"][i] for i in np.flatnonzero(looked)] == closer[looked].tolist())
        ev["removed_readded"] = bool(lst.closer_set and c["removed_any"] and c["readded"])
        lst.wait_in_order |= c["wait_in_order"]
        lst.wait_any |= c["wait_any"]
        flags = c["closer"]
    else:
        flags = np.maximum(closer, 0).tolist()
    ev["tie_split"] = ev["equal_pair"] = False
    if len(elem) < literal_below:
        # ties: the pruned candidate and a kept neighbor of it in the order are at the same distance
        at = int(np.flatnonzero(order == pruned)[0])
        ev["tie_split"] = any(0 <= j < len(order) and dist[order[j]] == dist[pruned] for j in (at - 1, at + 1))
        # a CheckElementCloser pair that decides by equality: of the neighbors accepted before e, in r's order, the first
        # with D <= d has D == d
        rank = {int(e): i for i, e in enumerate(order)}
        for e in np.flatnonzero(closer == 0):
            for x in r:
                if closer[x] != 1 or rank[x] > rank[int(e)]:
                    break
                if D[e, x] <= dist[e]:
                    ev["equal_pair"] |= bool(D[e, x] == dist[e])
                    break
    g.events.append(ev)
    lst.cf = flags[:lm]
    lst.closer_set = True                            # :1143-1144
    if pruned != lm:
        lst.elem[pruned], lst.dist[pruned], lst.cf[pruned], lst.loc[pruned] = elem[lm], float(dist[lm]), flags[lm], loc[lm]


def requests_of(batch, levels):
    """a batch's requests in the reference's order (src/hnswbuild.c:376-431): the new elements in ascending slot order --
    the order they were inserted in --, each one's layers from its level down to 0, its neighbors in list order;
    elements that were not linked (duplicates) make none.  -> arrays (owner, layer, new element, distance)"""
    el = np.asarray(batch["elements"])
    qs = np.argsort(el, kind="stable")
    qs = qs[np.asarray(batch["linked"])[qs] != 0]
    lcs = np.arange(batch["lcap"] - 1, -1, -1)                     # layers downwards
    cnt = np.where(lcs[None, :] <= np.asarray(levels)[el[qs]][:, None], batch["sel_cnt"][qs][:, lcs], 0)
    mask = np.arange(batch["sel_ids"].shape[2])[None, None, :] < cnt[:, :, None]
    q, l, _ = np.nonzero(mask)                                     # row-major: element, layer, neighbor
    return batch["sel_ids"][qs][:, lcs][mask], lcs[l].astype(np.int32), el[qs][q].astype(np.int32), batch["sel_dist"][qs][:, lcs][mask]


def link_batch(g, batch):
    """one batch applied to g: every request through HnswUpdateConnection, then the batch's own lists put in place (their
    flags are the sweep's, closerSet stays clear: :1143-1144 applies to sorted lists only).  An update reads and writes
    its own list only, so the requests are taken list by list, each list's in the reference's order; a list that the
    batch cannot fill beyond lm takes its newcomers in one step (appends, :1192-1193).
    -> dict(nrec, pairs: the first round's pair count, deferred_in_order / deferred_any: lists whose replay waits)"""
    g.nbatch += 1
    touched = {}
    owner, lc, new, dist = requests_of(batch, g.levels)
    o = np.argsort(owner.astype(np.int64) * batch["lcap"] + lc, kind="stable")
    owner, lc, new, dist = owner[o].tolist(), lc[o].tolist(), new[o].tolist(), dist[o].tolist()
    a, n = 0, len(owner)
    while a < n:
        b = a + 1
        while b < n and owner[b] == owner[a] and lc[b] == lc[a]:
            b += 1
        lst = g.list_of(owner[a], lc[a])
        touched[(owner[a], lc[a])] = True
        if len(lst.elem) + (b - a) <= g.lm(lc[a]):
            _record(g, lst)
            lst.elem += new[a:b]
            lst.dist += dist[a:b]
            lst.cf += [0] * (b - a)
            lst.loc += range(lst.nstart, lst.nstart + b - a)
            lst.nnew = b - a
        else:
            for i in range(a, b):
                update_connection(g, owner[i], lc[i], new[i], dist[i])
        a = b
    st = dict(nrec=len(touched), pairs=0, deferred_in_order=0, deferred_any=0)
    for owner, lc in touched:
        lst = g.lists[(owner, lc)]
        if lst.nstart + lst.nnew > g.lm(lc):
            st["pairs"] += group_pairs(lst.nstart + lst.nnew, lst.frm)
        st["deferred_in_order"] += bool(lst.wait_in_order)
        st["deferred_any"] += bool(lst.wait_any)
    el = batch["elements"]
    for q in range(len(el)):
        if not batch["linked"][q]:
            continue
        e = int(el[q])
        for lc in range(min(int(g.levels[e]), batch["lcap"] - 1) + 1):
            n = int(batch["sel_cnt"][q, lc])
            lst = g.list_of(e, lc)
            lst.elem = batch["sel_ids"][q, lc, :n].tolist()
            lst.dist = batch["sel_dist"][q, lc, :n].tolist()
            lst.cf = [int(x) & 1 for x in batch["sel_closer"][q, lc, :n]]
            lst.closer_set = False
    return st


PREFIX_ROWS = 500         # scenarios up to this size are also checked after every batch (the device runs each prefix)


def run_model(sc, prefixes=None):
    """a scenario through the model -> (graph, [per-batch stats]); prefixes: a list that receives the tuples after
    every batch"""
    g = Graph(sc["rows"], sc["metric"], sc["m"], sc["levels"])
    st = []
    for b in sc["batches"]:
        st.append(link_batch(g, b))
        if prefixes is not None:
            prefixes.append(g.tuples()[1])
    return g, st


# ------------------------------------------------------------------------------------------------------------ scenarios
def make_batch(rows, metric, m, levels, elements, linked, lcap, candidates):
    """the arrays pgv_hnsw_link_prepare takes.  candidates(e, lc) -> the element ids the new element's search "found" on
    that layer (already linked, level >= lc); nearest first (ties by id) they go through the plain sweep."""
    nq, stride = len(elements), 2 * m
    b = dict(elements=np.asarray(elements, np.int32), linked=np.asarray(linked, np.uint8), lcap=int(lcap),
             sel_ids=np.full((nq, lcap, stride), -1, np.int32), sel_dist=np.zeros((nq, lcap, stride), np.float32),
             sel_closer=np.zeros((nq, lcap, stride), np.uint8), sel_cnt=np.zeros((nq, lcap), np.int32))
    for q, e in enumerate(elements):
        if not linked[q]:
            continue
        for lc in range(min(int(levels[e]), lcap - 1) + 1):
            ids = np.asarray(candidates(int(e), lc), dtype=np.int32)
            if ids.size == 0:
                continue
            assert (levels[ids] >= lc).all()
            d = distances_to(rows, metric, int(e), ids).astype(np.float32)
            o = np.lexsort((ids, d + np.float32(0.0)))
            ids, d = ids[o], d[o]
            lm = 2 * m if lc == 0 else m
            tri = None
            if len(ids) > lm:
                D = pair_matrix(rows, metric, ids)
                tri = np.concatenate([D[u, :u] for u in range(1, len(ids))])
            wi, wd, wc = host_select(ids, d, tri, lm)
            n = len(wi)
            b["sel_ids"][q, lc, :n], b["sel_dist"][q, lc, :n], b["sel_closer"][q, lc, :n], b["sel_cnt"][q, lc] = wi, wd, wc, n
    return b


def scenario(name, rows, metric, m, levels, batches, f16=False):
    return dict(name=name, rows=np.ascontiguousarray(rows, np.float32), metric=metric, m=m,
                levels=np.ascontiguousarray(levels, np.int32), batches=batches, f16=f16)


def _grid(rng, n, dim, amp):
    return rng.integers(-amp, amp + 1, (n, dim)).astype(np.float32)


def random_scenario(name, seed, n, dim, amp, m, metric, levels, batch_sizes, ncand, lcap=None, unlinked=0, f16=False,
                    dup=0, shuffle=True):
    """batches of consecutive elements; each new element's candidates are a seeded subset (up to ncand) of the elements
    linked in EARLIER batches with level >= lc.  dup: that many rows are copies of earlier rows; unlinked: that many of
    the copies are handed over with linked = 0, as a duplicate that found its twin is."""
    rng = np.random.default_rng(seed)
    rows = _grid(rng, n, dim, amp)
    levels = np.asarray(levels, np.int32)
    first = batch_sizes[0]
    dups = rng.choice(np.arange(first, n), dup, replace=False) if dup else np.zeros(0, np.int64)
    for e in dups:
        rows[e] = rows[rng.integers(0, e)]
    skip = set(int(e) for e in dups[:unlinked])
    lcap = int(levels.max()) + 1 if lcap is None else lcap
    linked_so_far, batches, at = [], [], 0
    for bs in batch_sizes:
        el = np.arange(at, at + bs)
        at += bs
        if shuffle:
            rng.shuffle(el)
        pool = np.asarray(linked_so_far, np.int64)

        def cands(e, lc, pool=pool):
            p = pool[levels[pool] >= lc] if pool.size else pool
            k = min(len(p), int(rng.integers(1, ncand + 1)))
            return rng.choice(p, k, replace=False) if k else p
        linked = [0 if int(e) in skip else 1 for e in el]
        batches.append(make_batch(rows, metric, m, levels, el, linked, lcap, cands))
        linked_so_far += [int(e) for e, f in zip(el, linked) if f]
    return scenario(name, rows, metric, m, levels, batches, f16)


def hub_scenario(metric=L2, f16=False, name="hub"):
    """m = 4: every new element chooses element 0 on layer 0; batches of 1, 3, 40 and 200 newcomers, handed over shuffled"""
    rng = np.random.default_rng(41)
    n, m = 300, 4
    rows = _grid(rng, n, 3, 4)
    levels = np.zeros(n, np.int32)
    batches, at = [], 0
    for bs in (1, 1, 3, 40, 200, 55):
        el = np.arange(at, at + bs)
        at += bs
        rng.shuffle(el)
        batches.append(make_batch(rows, metric, m, levels, el, [1] * bs, 1, lambda e, lc: [0] if e else []))
    return scenario(name, rows, metric, m, levels, batches, f16)


def ties_scenario(m):
    return random_scenario("ties_m%d" % m, 50 + m, 420, 2, 4, m, L2, np.zeros(420, np.int32), (40, 60, 80, 120, 120),
                           ncand=3 * m, dup=60, unlinked=20)


def cache_scenario(metric=L2, f16=False, name="cache"):
    return random_scenario(name, 77, 340, 3, 5, 4, metric, np.zeros(340, np.int32), (40, 100, 100, 100), ncand=12, f16=f16)


def layers_scenario():
    rng = np.random.default_rng(5)
    n = 400
    levels = np.minimum(rng.geometric(0.5, n) - 1, 3).astype(np.int32)
    levels[:4] = (3, 2, 1, 0)
    return random_scenario("layers", 6, n, 4, 6, 5, L2, levels, (60, 120, 120, 100), ncand=16, lcap=4)


def fill_scenario(name, seed, m, dim, amp, groups, later):
    """layer-0 lists filled to exactly lm = 2m by one batch, then overflowing: `groups` = owner counts; batch 1 = lm new
    elements that each choose every owner (lists short -> exactly full, inside one batch); then one batch per entry of
    `later`: a list of newcomers, each given as the number of leading owner groups it chooses"""
    lm = 2 * m
    nown = sum(groups)
    n = nown + lm + sum(len(x) for x in later)
    rng = np.random.default_rng(seed)
    rows = _grid(rng, n, dim, amp)
    levels = np.zeros(n, np.int32)
    owners = np.arange(nown)
    batches = [make_batch(rows, L2, m, levels, owners, [1] * nown, 1, lambda e, lc: [])]
    el = np.arange(nown, nown + lm)
    batches.append(make_batch(rows, L2, m, levels, el, [1] * lm, 1, lambda e, lc: owners))
    at = nown + lm
    for newcomers in later:
        el = np.arange(at, at + len(newcomers))
        take = {int(e): int(np.sum(groups[:k])) for e, k in zip(el, newcomers)}
        at += len(newcomers)
        batches.append(make_batch(rows, L2, m, levels, el, [1] * len(el), 1, lambda e, lc: owners[:take[e]]))
    return scenario(name, rows, L2, m, levels, batches)


def lanes_scenario(m):
    """m = 31: lists of 62, the newcomer in lane 62 of the wavefront form; m = 32: lists of 64, hnsw_link_kernel<64>;
    m = 16: lists of 32, the last shape of hnsw_link_kernel<32> (PGV_HNSW_LINK_SERIAL=1).
    20 owners; one batch fills their lists, one of 10 newcomers overflows them without cached flags, one of 5 with"""
    return fill_scenario("lanes_m%d" % m, 310 + m, m, 8, 16, [20], [[1] * 10, [1] * 5])


def tri_cap_scenario(m):
    """full lists without cached flags receiving 2 newcomers (the first 6 owners) and 1 (the other 6): records of
    lm + 2 and lm + 1 ids, i.e. 1035 and 990 pairs at m = 22, 1128 and 1081 at m = 23, round the 1024 the wavefront
    kernel keeps in LDS; a further batch meets the cached flags"""
    return fill_scenario("tri_cap_m%d" % m, 220 + m, m, 6, 12, [6, 6], [[2, 1], [2, 2, 2]])


WIDE_SPECIAL = [3600 + 200 * i for i in range(6)]      # owners of wide_scenario's crafted lists


def wide_scenario():
    """m = 100 (lists of 200, uint8 candidate indexes up to 200): 7 200 owners in two halves; the second half's elements
    each choose 200 of the first half, so that all 7 200 lists are exactly full (the first half's by 200 appends each, the
    second's as their own selections); then two batches of 36 new elements that each choose 200 distinct owners: 7 200
    records of 201 ids each -- 7 200 x 19 900 member pairs x 4 bytes is above the 512 MB that pgv_hnsw_link_apply
    enqueues without asking, so its second round runs the synchronous way, and in the second batch lists wait.

    On random 4-d rows a selection over 201 candidates accepts some 25 and fills up with the rejected ones, so the pruned
    item is the furthest reject whatever the second round decides.  Six lists (WIDE_SPECIAL) are therefore crafted so that
    the pruned item IS the second round's decision.  The owner sits at the origin; its 200 members are
      B = (-1, 0): the nearest; every point with x <= -1 is rejected because of it (|p - B|^2 = |p|^2 + 2x + 1 <= |p|^2)
      X = (4, 0), F = (8, -8): F, at 128 the furthest member but G, is rejected because of X only (|F - X|^2 = 80 <= 128)
      G = (-12, 0) at 144, and 196 fillers with x <= -1 below 128.
    The first wide batch's newcomer is one more filler: G is pruned and the list has its flags (B, X closer).  The second's
    is N = (2, 3) at 13: closer than X and within 13 of it, so X loses its flag, the former rejects are checked against
    r = {B, N} -- member-member pairs: the list waits -- and F, 145 from B and 157 from N, is re-added: the pruned item is
    the furthest filler.  With any member-member distance of F read as 128 or less it is F instead."""
    m, half, lm = 100, 3600, 200
    n = 2 * half + 72
    rng = np.random.default_rng(100)
    rows = _grid(rng, n, 4, 16)
    pool = np.asarray([(x, y, z, 0) for x in range(-11, 0) for y in range(-11, 12) for z in (-1, 0, 1)
                       if 2 <= x * x + y * y + z * z <= 127], np.float32)
    for owner in WIDE_SPECIAL:
        j0 = owner - half
        f = pool[rng.choice(len(pool), 197, replace=False)]
        rows[owner] = 0
        rows[j0:j0 + lm] = np.concatenate([[(-1, 0, 0, 0), (4, 0, 0, 0), (8, -8, 0, 0), (-12, 0, 0, 0)], f[:196]])
        rows[2 * half + owner // lm] = f[196]                    # the first wide batch's newcomer into this list
        rows[2 * half + 36 + owner // lm] = (2, 3, 0, 0)         # the second's
    levels = np.zeros(n, np.int32)
    a = np.arange(half)
    batches = [make_batch(rows, L2, m, levels, a, [1] * half, 1, lambda e, lc: [])]
    batches.append(make_batch(rows, L2, m, levels, a + half, [1] * half, 1, lambda e, lc: (e - half + np.arange(lm)) % half))
    for k in range(2):
        el = np.arange(2 * half + 36 * k, 2 * half + 36 * (k + 1))
        batches.append(make_batch(rows, L2, m, levels, el, [1] * 36, 1,
                                  lambda e, lc: ((e - 2 * half) % 36) * lm + np.arange(lm)))
    return scenario("wide", rows, L2, m, levels, batches)


def scan_scenario(nlists):
    """m = 4: one batch whose requests touch exactly `nlists` distinct lists (the scan takes 4 096 values a trip), one
    more after it that touches them again and overflows eight of them"""
    m = 4
    per = (nlists + 7) // 8
    n = nlists + 2 * per + 8
    rng = np.random.default_rng(nlists)
    rows = _grid(rng, n, 4, 16)
    levels = np.zeros(n, np.int32)
    owners = np.arange(nlists)
    batches = [make_batch(rows, L2, m, levels, owners, [1] * nlists, 1, lambda e, lc: [])]
    for k in range(2):
        base = nlists + k * per
        el = np.arange(base, base + per + (8 if k else 0))
        batches.append(make_batch(rows, L2, m, levels, el, [1] * len(el), 1,
                                  lambda e, lc, base=base: owners[8 * (e - base):8 * (e - base) + 8] if e - base < per else owners[:8]))
    return scenario("scan_%d" % nlists, rows, L2, m, levels, batches)


def all_scenarios():
    """name -> builder (built on demand: the large ones take a moment)"""
    return {
        "hub": hub_scenario,
        "ties_m4": lambda: ties_scenario(4),
        "ties_m8": lambda: ties_scenario(8),
        "cache": cache_scenario,
        "layers": layers_scenario,
        "lanes_m16": lambda: lanes_scenario(16),
        "lanes_m31": lambda: lanes_scenario(31),
        "lanes_m32": lambda: lanes_scenario(32),
        "tri_cap_m22": lambda: tri_cap_scenario(22),
        "tri_cap_m23": lambda: tri_cap_scenario(23),
        "wide": wide_scenario,
        "scan_4095": lambda: scan_scenario(4095),
        "scan_4096": lambda: scan_scenario(4096),
        "scan_4097": lambda: scan_scenario(4097),
        "hub_ip": lambda: hub_scenario(IP, name="hub_ip"),
        "cache_ip": lambda: cache_scenario(IP, name="cache_ip"),
        "hub_f16": lambda: hub_scenario(L2, True, "hub_f16"),
        "cache_f16": lambda: cache_scenario(L2, True, "cache_f16"),
        "hub_ip_f16": lambda: hub_scenario(IP, True, "hub_ip_f16"),
        "cache_ip_f16": lambda: cache_scenario(IP, True, "cache_ip_f16"),
    }
