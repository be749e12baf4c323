"""Inputs of the tie tests of the HNSW walk (tests/test_hnsw_walk_model_cpu.py, tests/test_gpu_hnsw_ties.py,
tests/mp_hnsw_trip_worker.py): hand-written graphs whose answer holds in every tie order, and small-integer random data
on which most distances are shared.  Data only; the walk's model is tests/hnsw_walk_model.py.

A planted element at distance d is the row of d ones and DIM - d zeros.  With the query below, d is its squared L2
distance, its L1 distance, its negative inner product and -- packed -- its Hamming distance, all exact in fp32 and fp16."""
import numpy as np

from hnsw_walk_model import tuples

DIM = 16  # also the planted bit strings' length


def planted_rows(dists):
    return np.array([[1.0] * d + [0.0] * (DIM - d) for d in dists], dtype=np.float32)


def planted_query(metric_name):
    """zeros for L2 / L1 / Hamming; minus ones for the negative inner product: -(q . x) = the number of ones"""
    return np.full((1, DIM), -1.0 if metric_name == "negip" else 0.0, dtype=np.float32)


def _case(m, ef, dists, lists, levels=None, **want):
    levels, nbr_start, nbr = tuples(m, levels if levels is not None else [0] * len(dists), lists)
    return dict(m=m, ef=ef, dists=list(dists), levels=levels, nbr_start=nbr_start, nbr=nbr, entry=0, **want)


def planted():
    """name -> case.  `head`: the runs of the answer, nearest first, as (distance, candidates, how many of them); `scored`;
    `unscored`: elements no walk may reach (they would be in the head if one did).  Element 0 is the entry point e0 at
    distance 9 throughout; links are one-directional; ef is as small as the case allows."""
    cases = {}
    # A. an old entry pushed out of W at W's new furthest distance leads on.  e0(9) -> x(5), y(5); x -> z(3); y -> t(1).
    # ef 2: W = {x, y}.  Whichever of x / y is expanded first brings its neighbour in and pushes one 5 out; the other 5 is
    # W's furthest, so both 5s are still candidates (the stop test is strict) and both get expanded: z and t are scored,
    # W ends {t, z}; every element is scored once: 5.  Without T the kernel stops at {z, x}.
    e0, x, y, z, t = range(5)
    cases["A"] = _case(2, 2, [9, 5, 5, 3, 1], {(e0, 0): [x, y], (x, 0): [z], (y, 0): [t]},
                       head=[(1, [t], 1), (3, [z], 1)], scored=5, unscored=[])
    # B. T is dropped when W's furthest gets nearer.  e0(9) -> a(1), x(5), y(5); a -> z(3); z -> w(2); x, y -> t(0).
    # ef 3: W = {a, x, y}; a brings z: {a, z, one 5}, the other 5 still a candidate; z brings w: {a, w, z}, furthest 3.
    # Now both 5s are strictly farther than the furthest: the search stops, t is never scored.  Scored: e0, a, x, y, z, w.
    e0, a, x, y, z, w, t = range(7)
    cases["B"] = _case(2, 3, [9, 1, 5, 5, 3, 2, 0], {(e0, 0): [a, x, y], (a, 0): [z], (z, 0): [w], (x, 0): [t], (y, 0): [t]},
                       head=[(1, [a], 1), (2, [w], 1), (3, [z], 1)], scored=6, unscored=[t])
    # C. more ties than 64.  m 40: e0(9) -> a(1), c1 .. c79(5); a -> b1 .. b70(2); c79 -> t(0).  ef 80: W = {a, c1 .. c79};
    # a's 70 neighbours at 2 push 70 of the c's out, 9 stay, so W's furthest stays 5 and all 79 c's remain candidates:
    # c79 is expanded whatever the order, t is scored, and W ends t, a, the 70 b's and 8 c's.  Every element is scored: 152.
    a, c, b, t = 1, list(range(2, 81)), list(range(81, 151)), 151
    cases["C"] = _case(40, 80, [9, 1] + [5] * 79 + [2] * 70 + [0], {(0, 0): [a] + c, (a, 0): b, (c[-1], 0): [t]},
                       head=[(0, [t], 1), (1, [a], 1), (2, b, 70), (5, c, 8)], scored=152, unscored=[])
    # D. a batch entry admitted in its turn and pushed out later in the same batch.  e0(9) -> y(5), x(5), z(3) in this
    # order; x -> t(1).  ef 2: y and x are admitted (W not full, then 5 < 9), z pushes one of them out at 5 = the new
    # furthest, so both stay candidates; x is expanded, t is scored: {t, z}, 5 scored.
    e0, y, x, z, t = range(5)
    cases["D"] = _case(2, 2, [9, 5, 5, 3, 1], {(e0, 0): [y, x, z], (x, 0): [t]},
                       head=[(1, [t], 1), (3, [z], 1)], scored=5, unscored=[])
    # E. a rejected batch entry is no candidate.  e0(9) -> z(3), y(5), x(5), v(5); v -> t(0).  ef 2: z and y are admitted
    # ({z, y}, e0 leaves at 9); x and v fail `5 < 5` against a full W and are never candidates; nothing ever leaves W at
    # its furthest distance.  {z, y}, t unscored, 5 scored.  (The tuple order differs from E2's so that T stays empty.)
    e0, z, y, x, v, t = range(6)
    cases["E"] = _case(2, 2, [9, 3, 5, 5, 5, 0], {(e0, 0): [z, y, x, v], (v, 0): [t]},
                       head=[(3, [z], 1), (5, [y], 1)], scored=5, unscored=[t])
    # E2. the same with a tie beside the rejected entry.  e0(9) -> y(5), x(5), v(5), z(3); v -> t(0).  ef 2: y and x are
    # admitted, v fails `5 < 5`, z pushes one of y / x out at the furthest distance: y and x are candidates, v is not.
    e0, y, x, v, z, t = range(6)
    cases["E2"] = _case(2, 2, [9, 5, 5, 5, 3, 0], {(e0, 0): [y, x, v, z], (v, 0): [t]},
                        head=[(3, [z], 1), (5, [y, x], 1)], scored=5, unscored=[t])
    # F. an element below the layer.  e0 (level 1) lists u (level 1) and d (level 0, distance 1) on layer 1; on layer 0,
    # e0 -> d, u and u -> d, e0.  Layer 1 scores d but never admits it and ends on the nearer of e0 / u; layer 0 starts
    # there and scores the other two: {d, nearer of e0 / u}, 3 scored.  A kernel admitting d on layer 1 starts layer 0 at
    # d, whose tuple is empty: {d}, 1 scored.  F1: u(5) nearer than e0.  F2: u(12) farther.
    e0, u, d = range(3)
    lists = {(e0, 1): [u, d], (e0, 0): [d, u], (u, 0): [d, e0]}
    cases["F1"] = _case(2, 2, [9, 5, 1], lists, levels=[1, 1, 0], head=[(1, [d], 1), (5, [u], 1)], scored=3, unscored=[])
    cases["F2"] = _case(2, 2, [9, 12, 1], lists, levels=[1, 1, 0], head=[(1, [d], 1), (9, [e0], 1)], scored=3, unscored=[])
    return cases


def check_head(case, ids, dist, what=""):
    """ids / dist: a walk's whole W (k = ef), nearest first, against the case's answer up to the order inside a run"""
    ids, dist = [int(i) for i in ids if i >= 0], [float(x) for x in dist]
    want = [float(d) for d, _, c in case["head"] for _ in range(c)]
    assert dist[:len(ids)] == want and len(ids) == len(want), (what, ids, dist, want)
    assert len(set(ids)) == len(ids), (what, "an element twice", ids)
    at = 0
    for d, members, c in case["head"]:
        assert set(ids[at:at + c]) <= set(members), (what, "distance %g" % d, ids[at:at + c])
        at += c


# ------------------------------------------------------------------------------------------------- tie-heavy random data
EFS = (1, 2, 10, 40, 64, 65, 200)
N, NQ, RDIM, NBITS = 1500, 48, 6, 12
METRICS = ("l2", "negip", "l1")


def ef_k():
    """(ef, k): k = min(ef, 10) for every ef, and k = ef once"""
    return [(ef, min(ef, 10)) for ef in EFS] + [(40, 40)]


def random_ints(seed=31):
    """rows [N x RDIM] and queries [NQ x RDIM] in {0, 1, 2}: 729 distinct points, every distance a small integer"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, (N, RDIM)).astype(np.float32), rng.integers(0, 3, (NQ, RDIM)).astype(np.float32)


def random_bits(seed=37):
    """the 0/1 form: rows [N x NBITS] and queries [NQ x NBITS] in {0, 1} as float32 (np.packbits packs them)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2, (N, NBITS)).astype(np.float32), rng.integers(0, 2, (NQ, NBITS)).astype(np.float32)


def distances(metric_name, queries, rows):
    """[nq x n] Python-int-valued distances (int64): exactly what fp32 and fp16 arithmetic give on these inputs"""
    q, r = queries.astype(np.int64)[:, None, :], rows.astype(np.int64)[None, :, :]
    if metric_name == "l2":
        return ((q - r) ** 2).sum(-1)
    if metric_name == "l1":
        return np.abs(q - r).sum(-1)
    return -(q * r).sum(-1)


def insert_levels(count, top, seed=41):
    """random insert levels for build-side searches, every layer of the graph drawn at least once"""
    rng = np.random.default_rng(seed)
    lv = rng.integers(0, top + 1, count).astype(np.int32)
    lv[:top + 1] = np.arange(top + 1)
    return lv


def random_graph(oracle, form):
    """form: one of METRICS, or "bits".  The oracle's build (m 8, ef_construction 32) over the form's rows ->
    (elements [n' x dim] float32 in the graph's element order -- equal rows share an element, so n' < N --, queries,
    the graph as export_tuples() gives it, distances [NQ x n'] of every query to every element)"""
    from oracle import pyoracle as po
    rows, queries = random_bits() if form == "bits" else random_ints()
    metric = "l2" if form == "bits" else form
    g = po.HnswGraph(oracle, {"l2": po.OPS_L2, "negip": po.OPS_IP, "l1": po.OPS_L1}[metric], po.ORA_F32, rows, m=8,
                     ef_construction=32, seed=7)
    ex = g.export_tuples()
    g.close()
    elements = np.ascontiguousarray(rows[ex["rows"]])
    return elements, queries, ex, distances(metric, queries, elements)
