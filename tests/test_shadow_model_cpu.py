"""The adversarial data of tests/test_gpu_shadow_edges.py, checked on the host with the float64 model of the shadow
(tests/shadow_model.py): if these hold, the GPU cases really do sit at the edge of the rounding band -- a band too
narrow by half, or without its row or query representation term, answers the decoys."""
import numpy as np
import pytest

import shadow_model as sm

SETS = {"rows": sm.row_inversion_set, "query": sm.query_inversion_set}
K = (10, 16)


def _values(st):
    s, sh, E, P, t = st.model()
    return s, sh, t, sm.exact_values(st.rows, st.query), sm.shadow_values(st.rows, st.centers, st.list_offsets, st.query)


@pytest.mark.parametrize("name", sorted(SETS))
def test_scale_puts_the_largest_residual_in_the_top_binade(name):
    st = SETS[name]()
    s, sh, _, _, _ = _values(st)
    m = np.max(np.abs(st.rows - st.centers[0]))
    assert 2.0 ** 13 <= np.ldexp(float(m), -s) < 2.0 ** 14
    assert np.isfinite(sh.astype(np.float64)).all()
    # the fillers (and the query set's rows) lie on the fp16 grid: their shadow is exact
    for g in (["filler"] if name == "rows" else ["true", "decoy", "filler"]):
        rows = st.rows[st.groups[g]]
        assert np.array_equal(np.ldexp(sh[st.groups[g]].astype(np.float64), s), rows.astype(np.float64)), g


@pytest.mark.parametrize("name", sorted(SETS))
def test_only_one_representation_term_carries_the_error(name):
    st = SETS[name]()
    _, _, t, _, _ = _values(st)
    if name == "rows":
        assert t["dq"] == 0.0 and t["rep_rows"] > 0.0          # q = 1 is exact in fp16
    else:
        assert t["rep_rows"] == 0.0 and t["rep_query"] > 0.0    # rows on the grid: E = 0
    assert -125 <= t["exponent"] <= 125


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("k", K)
def test_shadow_order_inverts_the_true_neighbours(name, k):
    st = SETS[name]()
    _, _, t, ex, sv = _values(st)
    g = st.groups
    rep = t["rep_rows"] + t["rep_query"]
    true_topk = set(np.argsort(ex, kind="stable")[:k].tolist())
    shadow_topk = set(np.argsort(sv, kind="stable")[:k].tolist())
    assert set(g["true"].tolist()) <= true_topk and true_topk != shadow_topk
    # the decoys are exactly farther, clearly beyond the tie tolerance of the checks (4e-5 relative to the distance)
    dist = ex + float(np.sum(st.query.astype(np.float64) ** 2))
    gap = ex[g["decoy"]].min() - ex[g["true"]].max()
    assert gap > 2 * 4e-5 * dist[g["decoy"]].max()
    # ... yet ahead of them in shadow order by almost the whole representation term
    inversion = sv[g["true"]].min() - sv[g["decoy"]].max()
    assert 1.2 * rep < inversion < 2.0 * rep, (inversion / rep)
    # more than k' rows come before the first true neighbour
    ahead = int(np.sum(sv < sv[g["true"]].min()))
    assert ahead > sm.approx_candidates(k), (ahead, sm.approx_candidates(k))


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("k", K)
def test_half_the_band_proves_the_wrong_candidates_complete(name, k):
    """with k' candidates by shadow value (decoys and the nearest fillers), the k-th exact value among them is a decoy's;
    the smallest shadow value left out is a filler's.  The full band cannot prove the set complete (the query is
    flagged: widening or the exact pass finds the true rows); half of it, or the band without its representation
    term, can -- and would answer the decoys."""
    st = SETS[name]()
    _, _, t, ex, sv = _values(st)
    kp = sm.approx_candidates(k)
    order = np.argsort(sv, kind="stable")
    cand, rest = order[:kp], order[kp:]
    assert not set(st.groups["true"].tolist()) & set(cand.tolist())
    kth = np.sort(ex[cand])[k - 1]
    lowest_out = sv[rest].min()
    eps = t["eps"]
    assert lowest_out - eps < kth                                   # flagged
    assert lowest_out - 0.5 * eps > kth                             # eps / 2: "complete"
    assert lowest_out - (eps - t["rep_rows"] - t["rep_query"]) > kth  # no representation term: "complete"
