"""pgv_search_filtered -- the IVFFlat iterative scan under a keep bitmap -- against a numpy restatement of its loop
(include/pgv_hip.h), on one hand-made index of 9 lists whose starts fall on and off the bitmap's word boundaries.

Integer data (-8..8) makes every fp32 distance exact, so the float64 model decides by equality: slots, distance bits,
tids, counts and probes_used, with the score tasks cut at 64 rows (the 300-row list spans five, the 65-row one two).  On
float data the model is fed the device's own pgv_scan_lists values, which the emitted values must equal bit for bit."""

import numpy as np
import pytest

from pgvector_amd import _lib, api

pytestmark = pytest.mark.gpu

LENS = [0, 1, 31, 32, 33, 64, 65, 2, 300]
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N, NL, NQ = int(OFF[-1]), len(LENS), 5
WORDS = (N + 31) // 32
METRIC = {"l2": api.PGV_L2SQ, "negip": api.PGV_NEG_IP}
DTYPE = {"f32": (api.PGV_F32, np.float32), "f16": (api.PGV_F16, np.float16)}
SHAPES = [("f32", d) for d in (1, 3, 8, 130)] + [("f16", d) for d in (9, 136)]
# (probes, max_probes, k): one batch | every list | a short last batch | k above the kept rows
PMK = [(1, 0, 5), (2, 9, 5), (2, 5, 5), (3, 9, 400)]
_cases = {}


def case(ctx, dtype, metric, dim, integer=True):
    """the index, its rows / queries / tids on the host, and every query's ranked lists"""
    key = (dtype, metric, dim, integer)
    if key not in _cases:
        rng = np.random.default_rng([dim, integer] + list(map(ord, dtype + metric)))
        draw = (lambda *s: rng.integers(-8, 9, s)) if integer else (lambda *s: rng.standard_normal(s))
        rows, centers, queries = (draw(m, dim).astype(DTYPE[dtype][1]) for m in (N, NL, NQ))
        # duplicate rows inside a list and across lists: the tie rule
        rows[OFF[8] + 7] = rows[OFF[8] + 3]
        rows[OFF[2]] = rows[OFF[8] + 3]
        rows[OFF[5] + 1] = rows[OFF[6] + 2]
        tids = np.arange(N, dtype=np.uint64) * 3 + 1
        ix = api.IvfIndex(ctx, METRIC[metric], DTYPE[dtype][0], dim, centers, OFF, rows, tids)
        _cases[key] = (ix, rows, queries, tids, ix.rank_lists(queries, NL, want_dist=False)[0])
    return _cases[key]


def exact_values(rows, queries, metric):
    r, q = rows.astype(np.float64), queries.astype(np.float64)
    if metric == "l2":
        return ((q[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    return -(q @ r.T)


def model(vals, ranked, keep, probes, max_probes, k):
    """the loop for one query: vals [N] what its rows sort by, keep [N] booleans -> (emitted slots, probes used)"""
    probes = min(probes, NL)
    P = min(max(max_probes, probes), NL)
    out, used = [], 0
    while len(out) < k and used < P:
        batch, used = ranked[used:min(used + probes, P)], min(used + probes, P)
        slots = np.concatenate([np.arange(OFF[l], OFF[l + 1]) for l in batch]).astype(np.int64)
        order = np.argsort(vals[slots], kind="stable")  # float8 order (NaN last, -0 = +0), ties in input order
        out += [int(s) for s in slots[order] if keep[s]][:k - len(out)]
    return out, used


def filters(seed):
    """name -> (what search_filtered takes, booleans [NQ x N]); the last two are one bitmap per query, stride > WORDS"""
    rng = np.random.default_rng(seed)
    one = lambda s: np.arange(N) == s  # noqa: E731
    shared = {"null": None, "ones": np.ones(N, bool), "zeros": np.zeros(N, bool), "first": one(OFF[8]), "last": one(OFF[6] - 1),
              "half": rng.random(N) < 0.5, "few": rng.random(N) < 0.03}
    out = {name: (f, np.broadcast_to(np.ones(N, bool) if f is None else f, (NQ, N))) for name, f in shared.items()}
    for name, share in (("half_each", 0.5), ("few_each", 0.03)):
        f = rng.random((NQ, N)) < share
        words = np.full((NQ, WORDS + 3), 0xffffffff, dtype=np.uint32)
        words[:, :WORDS] = api.pack_keep(f)
        out[name] = (words, f)
    return out


def check_against_model(got, vals, want_bits_of, ranked, tids, keep, probes, max_probes, k, what):
    dist, slot, tid, count, used = got
    for q in range(NQ):
        want, want_used = model(vals[q], ranked[q], keep[q], probes, max_probes, k)
        m, at = len(want), np.asarray(want, dtype=np.int64)
        assert (int(count[q]), int(used[q])) == (m, want_used), (what, q)
        assert slot[q].tolist() == want + [-1] * (k - m), (what, q)
        assert tid[q].tolist() == tids[at].tolist() + [2 ** 64 - 1] * (k - m), (what, q)
        assert dist[q].view(np.uint32).tolist() == want_bits_of(q, at) + [0x7f800000] * (k - m), (what, q)


@pytest.mark.parametrize("probes,max_probes,k", PMK)
@pytest.mark.parametrize("metric", ["l2", "negip"])
@pytest.mark.parametrize("dtype,dim", SHAPES)
def test_integer_data_matches_the_model(ctx, monkeypatch, dtype, dim, metric, probes, max_probes, k):
    monkeypatch.setenv("PGV_IVF_FILTER_TASK_ROWS", "64")
    ix, rows, queries, tids, ranked = case(ctx, dtype, metric, dim)
    vals = exact_values(rows, queries, metric)
    bits_of = lambda q, s: vals[q][s].astype(np.float32).view(np.uint32).tolist()  # noqa: E731
    for name, (keep, booleans) in filters(dim).items():
        got = ix.search_filtered(queries, probes, k, keep=keep, max_probes=max_probes, want_tid=True)
        check_against_model(got, vals, bits_of, ranked, tids, booleans, probes, max_probes, k, name)


@pytest.mark.parametrize("dtype,dim", [("f32", 130), ("f16", 136)])
def test_a_batch_that_ends_at_exactly_k_stops_the_scan(ctx, dtype, dim):
    ix, rows, queries, tids, ranked = case(ctx, dtype, "l2", dim)
    keep = filters(dim)["half"][1][0]
    # k = what query 0's first batches of 2 lists keep, taking batches until that is not nothing
    kept = np.cumsum([keep[OFF[l]:OFF[l + 1]].sum() for l in ranked[0]])
    end = next(e for e in range(2, NL + 1, 2) if kept[e - 1] > 0)
    dist, slot, count, used = ix.search_filtered(queries[:1], 2, int(kept[end - 1]), keep=keep, max_probes=NL)
    assert (int(count[0]), int(used[0])) == (int(kept[end - 1]), end)
    assert sorted(slot[0].tolist()) == sorted(s for l in ranked[0][:end] for s in range(OFF[l], OFF[l + 1]) if keep[s])


@pytest.mark.parametrize("dtype,dim", [("f32", 130), ("f16", 136)])
@pytest.mark.parametrize("metric", ["l2", "negip"])
def test_float_data_emits_the_list_scan_values(ctx, dtype, dim, metric):
    ix, rows, queries, tids, ranked = case(ctx, dtype, metric, dim, integer=False)
    vals = np.stack([ix.scan_lists(q, np.arange(NL))[0] for q in queries])  # slot order: every list in turn
    bits_of = lambda q, s: vals[q][s].view(np.uint32).tolist()  # noqa: E731
    for name in ("null", "half", "few_each"):
        keep, booleans = filters(dim)[name]
        got = ix.search_filtered(queries, 2, 40, keep=keep, max_probes=NL, want_tid=True)
        check_against_model(got, vals, bits_of, ranked, tids, booleans, 2, NL, 40, name)


ARG_ERRORS = {"index": dict(index=None), "queries": dict(queries=None), "out_dist": dict(dist=None), "out_slot": dict(slot=None),
              "out_count": dict(count=None), "k = 0": dict(k=0), "k = 4097": dict(k=4097), "probes = 0": dict(probes=0),
              "keep_stride": dict(stride=WORDS - 1), "out_tid without tids": dict(no_tids=True)}


@pytest.mark.parametrize("name", list(ARG_ERRORS))
def test_argument_errors(ctx, name):
    ix, rows, queries, tids, ranked = case(ctx, "f32", "l2", 8)
    a = dict(index=ix.h, queries=queries, probes=2, k=4, stride=0, dist=np.empty((NQ, 4), np.float32),
             slot=np.empty((NQ, 4), np.int64), tid=None, count=np.empty(NQ, np.int32), no_tids=False)
    a.update(ARG_ERRORS[name])
    keep = np.zeros((NQ, WORDS), np.uint32)
    if a["no_tids"]:
        bare = api.IvfIndex(ctx, api.PGV_L2SQ, api.PGV_F32, 8, rows[:NL], OFF, rows)
        a.update(index=bare.h, tid=np.empty((NQ, 4), np.uint64))
    rc = _lib.lib.pgv_search_filtered(a["index"], api.ptr(a["queries"]), NQ, a["probes"], 9, a["k"], api.ptr(keep), a["stride"],
                                      api.ptr(a["dist"]), api.ptr(a["slot"]), api.ptr(a["tid"]), api.ptr(a["count"]), None)
    assert rc == _lib.PGV_ERR_ARG, _lib.lib.pgv_last_error()
    if a["no_tids"]:
        bare.close()


def test_a_bit_index_is_refused_by_name(ctx):
    bits = np.zeros((4, 2), np.uint8)
    ix = api.BitIvfIndex(ctx, 16, bits[:2], np.array([0, 2, 4], np.int64), bits)
    with pytest.raises(api.PgvError, match="bit index") as e:
        ix.search_filtered(bits[:1], 1, 3)
    assert e.value.code == _lib.PGV_ERR_ARG
    ix.close()
