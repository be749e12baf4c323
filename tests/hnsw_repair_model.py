"""Plain-Python restatement of hnswvacuum's graph repair, for tests/test_hnsw_repair_model_cpu.py and
tests/test_gpu_hnsw_repair.py: no GPU, no ctypes.  On integer-valued data fp32 arithmetic is exact, so Python integers
are the device's distances.

What is restated, from the reference's sources:
  * search_layer: HnswSearchLayer with skipElement set (src/hnswutils.c:824-987), with real heaps: C nearest first, W
    furthest first; only live elements count towards ef (CountElement, :715-728, at :884 and :962); alwaysAdd = wlen < ef;
    a live admission raises wlen and, once wlen > ef, evicts W's furthest whatever it is; a dead one evicts nothing;
  * find_neighbors: HnswFindElementNeighbors(existing = true) (:1280-1357): ef = 1 above the element's level,
    ef_construction + 1 from min(level, entry level) down, RemoveElements (:1236-1259), SelectNeighbors (:1064-1165) as
    the plain sweep a list without cached closer flags gets, the next layer entered from the unstripped W;
  * update_index / back_link: GetUpdateIndex, ConnectionExists and UpdateNeighborOnDisk (src/hnswinsert.c:409-540);
  * repair_graph: RemoveHeapTids' highest and fallback point, RepairGraphEntryPoint, NeedsUpdated, RepairGraphElement
    and RepairGraph's order (src/hnswvacuum.c:36-502), with max_batch as a parameter: a batch is the next max_batch
    elements that need repair on the graph as it stands, their searches read that graph, and their tuples and back links
    are then applied one element after the other.  max_batch = 1 is the reference's loop.

The order among EQUAL distances is unspecified in the reference (pairing-heap internals, pointer order).  Every place
where an equality could decide something counts into TIES; the tests assert it stays 0 on the data they use."""
import heapq

TIES = [0]


def layer_m(m, lc):
    return 2 * m if lc == 0 else m


def neighbours(levels, nbr_start, nbr, m, c, lc):
    o = int(nbr_start[c]) + (int(levels[c]) - lc) * m
    return [int(e) for e in nbr[o:o + layer_m(m, lc)] if e >= 0]


def search_layer(qd, levels, nbr_start, nbr, m, ep, ef, lc, live, stats=None):
    """ep: [(distance, element)].  Returns W nearest first as [(distance, element)]."""
    visited = set()
    C, W = [], []
    wlen, seq = 0, 0
    for d, e in ep:
        visited.add(e)
        heapq.heappush(C, (d, seq, e))
        heapq.heappush(W, (-d, seq, e))
        seq += 1
        if live[e]:
            wlen += 1
    while C:
        d, _, c = heapq.heappop(C)
        if d > -W[0][0]:
            break
        unvisited = []
        for e in neighbours(levels, nbr_start, nbr, m, c, lc):
            if e not in visited:
                visited.add(e)
                unvisited.append(e)
        for e in unvisited:
            always = wlen < ef
            f = -W[0][0]
            ed = qd(e)
            if not always and ed == f:
                TIES[0] += 1
            if not (ed < f or always):
                continue
            if levels[e] < lc:
                continue
            if any(-w[0] == ed for w in W):
                TIES[0] += 1
            heapq.heappush(C, (ed, seq, e))
            heapq.heappush(W, (-ed, seq, e))
            seq += 1
            if live[e]:
                wlen += 1
                if wlen > ef:
                    heapq.heappop(W)
            if stats is not None:
                stats["max_w"] = max(stats["max_w"], len(W))
                stats["max_over"] = max(stats["max_over"], len(W) - ef)
    return sorted((-nd, e) for nd, _, e in W)


def select_neighbors(cands, lm, d):
    """cands: [(distance, element)] nearest first -> [(element, distance, closer)] in the order of the reference's r"""
    if len(cands) <= lm:
        return [(e, dist, 0) for dist, e in reversed(cands)]  # taken whole, W's furthest-first order
    r, wd = [], []
    for dist, e in cands:
        if len(r) >= lm:
            break
        closer = True
        for x, _, _ in r:
            dx = d(e, x)
            if dx == dist:
                TIES[0] += 1
            if dx <= dist:
                closer = False
                break
        (r if closer else wd).append((e, dist, 1 if closer else 0))
    for x in wd:
        if len(r) >= lm:
            break
        r.append(x)
    return r


def find_neighbors(d, levels, nbr_start, nbr, m, element, entry, ef_construction, live, stats=None):
    """-> {lc: [(element, distance, closer)]} for every layer from min(level, entry level) down"""
    out = {}
    if entry < 0:
        return out

    def qd(e):
        return d(element, e)
    ep = [(qd(entry), int(entry))]
    level, entry_level = int(levels[element]), int(levels[entry])
    for lc in range(entry_level, level, -1):
        ep = search_layer(qd, levels, nbr_start, nbr, m, ep, 1, lc, live, None)
    ef = ef_construction + 1
    for lc in range(min(level, entry_level), -1, -1):
        w = search_layer(qd, levels, nbr_start, nbr, m, ep, ef, lc, live, stats)
        lw = [(dist, e) for dist, e in w if e != element and live[e]]
        out[lc] = select_neighbors(lw, layer_m(m, lc), d)
        ep = w
    return out


def new_stats():
    return {"max_w": 0, "max_over": 0}


def dead_cap_needed(d, levels, nbr_start, nbr, m, element, entry, ef_construction, live):
    """the smallest dead_cap with which the device's W (ef_construction + 1 + dead_cap entries) holds this search"""
    st = new_stats()
    find_neighbors(d, levels, nbr_start, nbr, m, element, entry, ef_construction, live, st)
    return max(0, st["max_over"])


def update_index(d, owner, members, lm, newcomer, new_dist, live):
    """GetUpdateIndex: -2 a free slot, i the member to replace, -1 the newcomer is not selected"""
    if len(members) < lm:
        return -2
    for i, x in enumerate(members):
        if not live[x]:
            return i  # LoadElementsForInsert: the first member being deleted
    # HnswUpdateConnection: SelectNeighbors from scratch over the sorted candidates, no cached flags
    cands = [(d(owner, x), x) for x in members] + [(new_dist, newcomer)]
    if len({c[0] for c in cands}) != len(cands):
        TIES[0] += 1
    w = sorted(cands, key=lambda c: (-c[0], -c[1]))  # CompareCandidateDistances: furthest first
    r, wd = [], []
    while w and len(r) < lm:
        dist, e = w.pop()
        closer = True
        for _, x in r:
            dx = d(e, x)
            if dx == dist:
                TIES[0] += 1
            if dx <= dist:
                closer = False
                break
        (r if closer else wd).append((dist, e))
    wdoff = 0
    while wdoff < len(wd) and len(r) < lm:
        r.append(wd[wdoff])
        wdoff += 1
    pruned = wd[wdoff] if wdoff < len(wd) else w[0]
    if pruned[1] == newcomer:
        return -1
    return members.index(pruned[1])


def back_link(d, levels, nbr_start, nbr, m, owner, lc, newcomer, new_dist, live, counters=None):
    """HnswUpdateNeighborsOnDisk's step for one chosen neighbor; returns True when owner's tuple changed"""
    lm = layer_m(m, lc)
    o = int(nbr_start[owner]) + (int(levels[owner]) - lc) * m
    members = []
    for x in nbr[o:o + lm]:
        if x < 0:
            break
        members.append(int(x))
    # ConnectionExists wins over whatever GetUpdateIndex finds (the reference asks it afterwards; the outcome is the same,
    # and asking first keeps the selection's tie counter off a candidate list that holds the newcomer twice)
    if newcomer in members:
        return False
    idx = update_index(d, owner, members, lm, newcomer, new_dist, live)
    if counters is not None and len(members) == lm and all(live[x] for x in members):
        counters["reselections"] += 1
    if idx == -1:
        return False
    if idx == -2:
        idx = len(members)
    nbr[o + idx] = newcomer
    return True


def needs_updated(nbr_start, nbr, live, e):
    tup = nbr[int(nbr_start[e]):int(nbr_start[e + 1])]
    if any(x >= 0 and not live[x] for x in tup):
        return True
    return len(tup) > 0 and tup[-1] < 0


def highest_points(levels, live):
    highest, fallback, hl, fl = -1, -1, -1, -1
    for e in range(len(levels)):
        if not live[e]:
            continue
        if levels[e] > hl:
            if highest >= 0:
                fallback, fl = highest, hl
            highest, hl = e, int(levels[e])
        elif levels[e] > fl:
            fallback, fl = e, int(levels[e])
    return highest, fallback


def repair_graph(d, levels, nbr_start, nbr, entry, live, m, ef_construction, max_batch=1, stats=None):
    """-> (nbr, entry, counters); nbr is a repaired copy"""
    nbr = nbr.copy()
    n = len(levels)
    cnt = {"examined": 0, "repaired": 0, "batches": 0, "reselections": 0}

    def repair_elements(elems, search_entry):
        snapshot = nbr.copy()
        found = [find_neighbors(d, levels, nbr_start, snapshot, m, e, search_entry, ef_construction, live, stats)
                 for e in elems]
        for e, layers in zip(elems, found):
            level = int(levels[e])
            for lc in range(level, -1, -1):
                o = int(nbr_start[e]) + (level - lc) * m
                chosen = layers.get(lc, [])
                nbr[o:o + layer_m(m, lc)] = -1
                nbr[o:o + len(chosen)] = [x for x, _, _ in chosen]
            for lc in range(level, -1, -1):
                for x, dist, _ in layers.get(lc, []):
                    back_link(d, levels, nbr_start, nbr, m, x, lc, e, dist, live, cnt)
            cnt["repaired"] += 1
        cnt["batches"] += 1

    highest, fallback = highest_points(levels, live)
    if highest >= 0:
        if entry == highest:
            highest = fallback
        if highest >= 0 and needs_updated(nbr_start, nbr, live, highest):
            repair_elements([highest], entry)
    if entry >= 0:
        if not live[entry]:
            entry = highest
        elif needs_updated(nbr_start, nbr, live, entry):
            repair_elements([entry], highest)
    cursor = 0
    while cursor < n:
        batch, tall = [], False
        while cursor < n and len(batch) < max_batch:
            e = cursor
            if live[e]:
                is_tall = entry < 0 or levels[e] > levels[entry]
                if e != entry and needs_updated(nbr_start, nbr, live, e):
                    if is_tall and batch:
                        break
                    batch.append(e)
                    tall = is_tall
                cnt["examined"] += 1
            cursor += 1
            if tall:
                break
        if not batch:
            continue
        if tall:
            old = entry
            entry = batch[0]
            repair_elements(batch, old)
        else:
            repair_elements(batch, entry)
    return nbr, entry, cnt


def check_invariants(levels, nbr_start, nbr, entry, live, m):
    """what every repaired graph satisfies: no live element's tuple names a dead slot, a repaired list holds no duplicate
    and not the element itself, the entry point is live while any element is"""
    for e in range(len(levels)):
        if not live[e]:
            continue
        tup = nbr[int(nbr_start[e]):int(nbr_start[e + 1])]
        assert len(tup) == (int(levels[e]) + 2) * m
        assert all(x < 0 or live[x] for x in tup), "a live element's tuple names a dead slot"
        for lc in range(int(levels[e]) + 1):
            o = (int(levels[e]) - lc) * m
            ids = [x for x in tup[o:o + layer_m(m, lc)] if x >= 0]
            assert len(set(ids)) == len(ids) and e not in ids
    assert entry < 0 or live[entry]
    assert (entry >= 0) == bool(live.any())


# ---------------------------------------------------------------------------------------------- the tests' graphs

def sqdist(pts):
    """d(a, b) over integer rows: the squared L2 distance as a Python integer (from the full matrix: the rows are few)"""
    p = pts.astype("int64")
    sq = (p * p).sum(axis=1)
    mat = sq[:, None] + sq[None, :] - 2 * (p @ p.T)

    def d(a, b):
        return int(mat[a, b])
    return d


def knn_graph(pts, m, seed, top=2):
    """A layered graph for the tests, built without any search: levels drawn geometrically (at least one element on layer
    `top`), every element linked on each of its layers to its nearest layer_m elements of that layer, the tuple in a
    shuffled order (the admission order inside a tuple is what the repair search has to replay).  -> (levels, nbr_start,
    nbr, entry): entry the first element of the greatest level."""
    import numpy as np
    rng = np.random.RandomState(seed)
    n = len(pts)
    levels = np.minimum(rng.geometric(1.0 - 1.0 / m, size=n) - 1, top).astype(np.int32)
    levels[rng.randint(n)] = top
    start = np.concatenate([[0], np.cumsum((levels.astype(np.int64) + 2) * m)]).astype(np.int64)
    nbr = np.full(int(start[-1]), -1, dtype=np.int32)
    p = pts.astype(np.int64)
    for lc in range(top, -1, -1):
        on = np.nonzero(levels >= lc)[0]
        lm = layer_m(m, lc)
        sub = p[on]
        for e in on:
            dd = ((sub - p[e]) ** 2).sum(axis=1)
            order = on[np.argsort(dd, kind="stable")]
            near = [int(x) for x in order if x != e][:lm]
            rng.shuffle(near)
            o = int(start[e]) + (int(levels[e]) - lc) * m
            nbr[o:o + len(near)] = near
    entry = int(np.nonzero(levels == levels.max())[0][0])
    return levels, start, nbr, entry


def int_points(n, dim, seed, span):
    import numpy as np
    return np.random.RandomState(seed).randint(-span, span + 1, size=(n, dim)).astype(np.int64)


def line_graph(m, spec, extra=None):
    """Hand-built one-layer traps on a line: spec = [(position, live)] per element; element 0 is the one being repaired
    (position 0), element 1 the entry point; extra = {element: [neighbours]}.  Elements without an entry in extra link to
    the entry point alone.  -> (pts [n x 8] with the position in the first coordinate, live, levels, nbr_start, nbr)"""
    import numpy as np
    from hnsw_walk_model import tuples
    n = len(spec)
    pts = np.zeros((n, 8), dtype=np.int64)
    pts[:, 0] = [s[0] for s in spec]
    live = np.array([bool(s[1]) for s in spec])
    lists = {(e, 0): [1] for e in range(n) if e != 1}
    for e, ids in (extra or {}).items():
        lists[(e, 0)] = list(ids)
    levels, start, nbr = tuples(m, [0] * n, lists)
    return pts, live, levels, start, nbr


# The three traps where truncating W to ef after a batch gives another W than the reference's rule (ef_construction 4, so
# ef = 5; m = 4: 8 slots on layer 0).  Element 0 at position 0 is repaired from entry point 1; names in the comments.
def trap_dead_before_ef_live():
    """S A D B C E F: the dead D (far) is admitted while wlen < ef and stays past ef; it is expanded and leads to F, whose
    live admission evicts D.  Truncation drops D with the batch and never finds F."""
    spec = [(0, 1), (1, 1), (10, 0), (2, 1), (3, 1), (4, 1), (5, 1)]
    return line_graph(4, spec, {1: [0, 2, 3, 4, 5], 2: [6]}), [1, 3, 4, 5, 6]


def trap_dead_late_then_evicted():
    """S A B C G D H I: W is full of live ones when the dead D is admitted below the furthest; H evicts the live G, I
    evicts D: six live entries in a W of ef = 5.  Truncation rejects I."""
    spec = [(0, 1), (1, 1), (2, 1), (3, 1), (9, 1), (8, 0), (4, 1), (5, 1)]
    return line_graph(4, spec, {1: [0, 2, 3, 4, 5, 6, 7]}), [1, 2, 3, 6, 7]


def trap_dead_furthest_evicted_first():
    """S A D B C E G: the dead D is W's furthest when ef live ones are in; the live G, farther than every live entry,
    is still nearer than D and takes its place.  Truncation has dropped D and rejects G."""
    spec = [(0, 1), (1, 1), (10, 0), (2, 1), (3, 1), (4, 1), (6, 1)]
    return line_graph(4, spec, {1: [0, 2, 3, 4, 5, 6]}), [1, 3, 4, 5, 6]


TRAPS = (trap_dead_before_ef_live, trap_dead_late_then_evicted, trap_dead_furthest_evicted_first)


def truncating_search(qd, levels, nbr_start, nbr, m, entry, ef, live):
    """what an implementation that reuses the walk kernel's merge gives on one layer: W truncated to ef after each batch"""
    from hnsw_walk_model import walk
    return walk(qd, levels, nbr_start, nbr, m, entry, ef, qlevel=0)


# The shapes and plantings the GPU tests use; the CPU test asserts their preconditions on the same seeds.
N = 600
CASES = (
    # name, dim, span, m, ef_construction, seed, dead share
    ("d8_m4_ef8_25", 8, 700, 4, 8, 11, 0.25),
    ("d20_m8_ef40_60", 20, 400, 8, 40, 12, 0.60),
    ("d20_m4_ef40_25", 20, 400, 4, 40, 13, 0.25),
    ("d8_m8_ef8_60", 8, 700, 8, 8, 14, 0.60),
)
# the whole-graph repairs of the driver tests: seeds on which every search, selection and reselection of the run is
# tie-free at max_batch 1, 7 and 64.  (dim 20 with ef_construction 40 has no such seed among those tried: with W past a
# hundred entries some equal pair of distances decides something in one of the ~300 searches; the second case therefore
# has ef_construction 16 -- layer 0 holds 16 links, the search cases above cover ef_construction 40)
DRIVER_CASES = (("driver_d8_m4_ef8_25", 8, 700, 4, 8, 21, 0.25), ("driver_d20_m8_ef16_25", 20, 400, 8, 16, 43, 0.25))
DRIVER_CASE = DRIVER_CASES[0]
CLUSTER = 40   # the dead cluster: this many nearest elements of its centre
NQUERIES = 24  # random live query elements per case, besides the planted ones


def make_case(case):
    """-> dict: pts, graph, live, the query elements (planted first) and which is which"""
    import numpy as np
    name, dim, span, m, efc, seed, share = case
    pts = int_points(N, dim, seed, span)
    levels, start, nbr, entry = knn_graph(pts, m, seed)
    rng = np.random.RandomState(seed + 1000)
    live = rng.random_sample(N) >= share
    # an element all of whose neighbours are dead
    lonely = int(rng.randint(N))
    while lonely == entry:
        lonely = int(rng.randint(N))
    for x in nbr[int(start[lonely]):int(start[lonely + 1])]:
        if x >= 0:
            live[x] = False
    # a dead cluster around a live centre
    centre = int(rng.randint(N))
    while centre in (entry, lonely) or not live[centre]:
        centre = int(rng.randint(N))
    dd = ((pts - pts[centre]) ** 2).sum(axis=1)
    for x in np.argsort(dd, kind="stable")[1:CLUSTER + 1]:
        live[x] = False
    live[lonely] = live[centre] = True
    # a query element on the top layer (not the entry point), alive
    tops = [int(e) for e in np.nonzero(levels == levels.max())[0] if e != entry]
    assert tops, "no second element on the top layer: take another seed"
    top = tops[0]
    live[top] = True
    live[entry] = True
    others = [int(e) for e in rng.permutation(N) if live[e] and e not in (lonely, centre, top)][:NQUERIES]
    return {"name": name, "dim": dim, "m": m, "efc": efc, "pts": pts, "levels": levels, "nbr_start": start, "nbr": nbr,
            "entry": entry, "live": live, "lonely": lonely, "centre": centre, "top": top,
            "queries": [lonely, centre, top] + others}


def make_overflow_case():
    """The planted overflow: the first case's graph with ONLY the cluster dead.  The centre's search holds the whole
    cluster in W; the other queries are the live elements farthest from the centre.  dead_cap = 2 is what the test gives."""
    import numpy as np
    c = make_case(CASES[0])
    live = np.ones(N, dtype=bool)
    dd = ((c["pts"] - c["pts"][c["centre"]]) ** 2).sum(axis=1)
    order = np.argsort(dd, kind="stable")
    live[order[1:CLUSTER + 1]] = False
    far = [int(e) for e in order[::-1] if e != c["entry"]][:12]
    c.update(live=live, queries=[c["centre"]] + far, dead_cap=2)
    return c
