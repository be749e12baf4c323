"""The band of the batch ranking over the fp16 center shadow (pgv_internal.h) and the pair-term chain of
the ranking's recheck, on the host model of tests/rank_shadow_model.py: the value the fp16 path computes never leaves the
band round the true |c|^2 - 2 q.c, on benign data, on data of a huge dynamic range and on subnormals; and t = -2 q.c as
the recheck accumulates it stays inside g_pair 2 |q||c|.  Where the bound comes from: the representation terms are
Cauchy-Schwarz on measured E_c / P_c, the chains are Higham's gamma_n with n the roundings counted in the kernels."""
import numpy as np
import pytest

import rank_shadow_model as rm
import shadow_model as sm


def _data(kind, dim, nc, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        c = rng.random((nc, dim), dtype=np.float32)
        q = c[rng.integers(0, nc, nq)] + np.float32(0.1) * rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "range":  # element magnitudes over 2^-40 .. 2^20 inside one vector
        c = (rng.standard_normal((nc, dim)) * np.exp2(rng.integers(-40, 21, (nc, dim)))).astype(np.float32)
        q = (rng.standard_normal((nq, dim)) * np.exp2(rng.integers(-40, 21, (nq, dim)))).astype(np.float32)
    elif kind == "huge coordinate":
        c = rng.random((nc, dim), dtype=np.float32)
        c[:, 3] += np.float32(4096.0)
        q = c[rng.integers(0, nc, nq)] + np.float32(0.1) * rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "subnormal":  # fp32 subnormals and values whose fp16 casts are subnormal or zero
        c = (rng.standard_normal((nc, dim)) * 2.0 ** -140).astype(np.float32)
        c[::3] = (rng.standard_normal((len(c[::3]), dim)) * 2.0 ** -20).astype(np.float32)
        q = (rng.standard_normal((nq, dim)) * 2.0 ** -130).astype(np.float32)
        q[::2, 0] = 1.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(c), np.ascontiguousarray(q.astype(np.float32))


@pytest.mark.parametrize("kind", ["random", "range", "huge coordinate", "subnormal"])
@pytest.mark.parametrize("dim", [40, 256, 1536])
def test_the_fp16_ranking_value_stays_in_its_band(kind, dim):
    c, q = _data(kind, dim, 96, 24, seed=dim)
    s_c, ch, E, P = rm.cast_centers(c)
    assert np.isfinite(E) and np.isfinite(P)
    cn_max = float(rm.center_norms_f32(c).max())
    got, exps = rm.ranking_values_f32(c, q)
    want = rm.true_values(c, q)
    worst = 0.0
    for i in range(len(q)):
        band, e = rm.rank_band(q[i], s_c, E, P, cn_max, dim)
        assert e == exps[i]
        if not np.isfinite(band):
            continue  # the kernel puts everything in the band: batch_fix_kernel scores the query exactly
        err = np.abs(got[i].astype(np.float64) - want[i])
        assert (err <= band).all(), (kind, dim, i, err.max(), band)
        worst = max(worst, float((err / band).max()) if band > 0 else 0.0)
    print("%s dim %d: largest error / band = %.3g" % (kind, dim, worst))
    assert worst <= 1.0


def test_the_band_is_not_vacuous_on_the_headline_shape():
    """|q| ~ |c| ~ 22.6 at 1536-d: the representation term is a few tenths (the issue's estimate: ~0.3), so the band holds
    a candidate or two more than the fp32 ranking's, not all 26"""
    c, q = _data("random", 1536, 64, 8, seed=1)
    s_c, _, E, P = rm.cast_centers(c)
    band, _ = rm.rank_band(q[0], s_c, E, P, float((c.astype(np.float64) ** 2).sum(1).max()), 1536)
    assert 0.01 < band < 1.0, band


@pytest.mark.parametrize("kind", ["random", "range", "subnormal"])
@pytest.mark.parametrize("dim", [1, 3, 16, 40, 100, 256, 777, 1536, 2000])
def test_the_rechecks_pair_term_stays_inside_g_pair(kind, dim):
    c, q = _data(kind, dim, 12, 6, seed=1000 + dim)
    n, by_pair_kernel, by_recheck = rm.pair_chain_length(dim)
    g_pair = rm.gamma(n)
    for qi in q:
        for cj in c:
            t = float(rm.recheck_dot_f32(qi, cj))
            true = -2.0 * float(qi.astype(np.float64) @ cj.astype(np.float64))
            # Higham 3.5 on sum |q_i c_i| <= |q||c|; products that underflow in fp32 lose at most FLT_MIN each
            slack = 2.0 * dim * rm.FLT_MIN
            bound = g_pair * 2.0 * float(np.abs(qi.astype(np.float64)) @ np.abs(cj.astype(np.float64))) + slack
            assert abs(t - true) <= bound, (kind, dim, t, true, bound)


def test_pair_chain_length_covers_both_routes():
    """the term is the longer route's; at 1536-d the recheck's chain (19) is shorter than shadow_pair_kernel's (30).
    row_geom keeps at most 64 vectors on a lane, so the recheck's chain never passes 4 * 32 + 1 + 6 = 135 roundings;
    it is long where few lanes share a row (249-d: 63 vectors on one lane, 129 against 10)"""
    assert rm.pair_chain_length(1536) == (30, 30, 19)
    assert rm.pair_chain_length(249) == (129, 10, 129)
    for dim in range(1, 16001):
        n, a, b = rm.pair_chain_length(dim)
        assert n == max(a, b) and b <= 135
