"""tests/chain_model.py without a GPU: the exact fp32 evaluator against rational arithmetic, the chain length the host
charges against the chains of real products, what the swamping builders attain, and the margins of every adversarial
set -- adversarial for the kernels' band and FATAL for a band of half the width.

The evaluator's addition is a float64 two-sum with a half-way correction (chain_model.fmaf), not inputs chosen to make
it exact: the random cases below include sums whose float64 rounding lands on an fp32 half-way point."""
import numpy as np
import pytest

import chain_model as cm

DIMS = (64, 100, 256, 1536, 1600, 2000)
SETS = [("scan32", 256), ("scan32", 1536), ("scan32", 100), ("scan64", 256), ("scan64", 1600), ("dense", 1536),
        ("dense", 2000)]


def _chain_for(form, dtype, dim):
    return cm.dense_chain_length(dim, dtype) if form in ("scan64", "dense") else cm.scan_chain_length(dim, dtype, False)


def test_fmaf_matches_rational_arithmetic():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(np.float32)
    # double-rounding traps: c + a b exactly half an fp32 ulp of c away, plus or minus a term below float64's reach
    a[:8] = np.float32(2.0 ** -12)
    b[:8] = np.float32(2.0 ** -12) * np.float32(1.0 + 2.0 ** -23)
    c[:8] = 1.0
    a[8:16] = np.float32(2.0 ** -12) * np.float32(1.0 - 2.0 ** -24)
    b[8:16] = np.float32(2.0 ** -12)
    c[8:16] = np.float32(1.0 + 2.0 ** -23)
    got = cm.fmaf(a, b, c)
    want = np.array([cm.fmaf_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == np.float32(1.0 + 2.0 ** -23) and got[8] == np.float32(1.0 + 2.0 ** -23)   # past / short of the tie


@pytest.mark.parametrize("form", cm.FORMS)
@pytest.mark.parametrize("dim", (37, 100, 260))
def test_evaluator_matches_rational_arithmetic(form, dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((3, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    for d in (-1, 1):
        x, qs = cm.swamp(form, cm.F32, dim, d)
        got = cm.chain_dot(form, x, qs)[0]
        assert got.view(np.uint32) == cm.chain_dot_exact(form, x[0], qs).view(np.uint32)
    got = cm.chain_dot(form, rows, q)
    for r in range(3):
        assert got[r].view(np.uint32) == cm.chain_dot_exact(form, rows[r], q).view(np.uint32), (form, dim, r)


def test_chain_maps_partition_the_row():
    for dtype in (cm.F32, cm.F16):
        for form in cm.FORMS:
            for dim in (1, 7, 64, 72, 100, 1600):
                chains, _ = cm.chain_map(form, dtype, dim)
                assert sorted(i for ch in chains for i in ch) == list(range(dim)), (dtype, form, dim)
                assert len(chains) <= 4 and (form != "argmin" or len(chains) == 1)


def test_charged_chain_length_covers_the_real_chains():
    """dims 1 .. 4000, both types, every path: the chain length g_dot is computed from is at least the longest chain of
    real products of every form that may take a task.  The formula used before scan_chain_length (ld / 4 for the
    32-query kernel) fails this for fp16: 64-d puts 32 products on a chain of the 16-wide form, 72-d 24 on one of the
    32-query form."""
    short = {}
    for dtype in (cm.F32, cm.F16):
        for dim in range(1, 4001):
            real = {f: cm.longest_chain(f, dtype, dim) for f in ("scan32", "scan16", "scan64", "dense")}
            for path in ("scan", "scan_wide", "rank", "topk32", "topk128"):
                need = max(real[f] for f in cm.forms_of(path))
                assert cm.charged_chain(path, dtype, dim) >= need, (dtype, dim, path)
                old = cm.dense_chain_length(dim, dtype) if path in ("scan_wide", "topk128") else cm.padded(dim, dtype) / 4.0
                if old < need:
                    short.setdefault((dtype, path), []).append(dim)
    assert not any(d == cm.F32 for d, _ in short), short.keys()           # fp32 never had a ragged case
    assert 64 in short[(cm.F16, "scan")] and 72 in short[(cm.F16, "scan")] and 1600 in short[(cm.F16, "rank")]
    assert cm.longest_chain("scan16", cm.F16, 64) == 32 and cm.longest_chain("scan16", cm.F16, 1600) == 416
    assert cm.longest_chain("scan32", cm.F16, 72) == 24
    # fp32 and every whole-slice fp16 shape keep the value they had
    for dim in (256, 1536, 3072):
        assert cm.scan_chain_length(dim, cm.F32, False) == dim // 4 and cm.scan_chain_length(dim, cm.F16, False) == dim // 4


@pytest.mark.parametrize("form", ("scan32", "scan16", "scan64", "dense"))
@pytest.mark.parametrize("dim", DIMS)
def test_swamping_attains_what_it_claims(form, dim):
    chain = _chain_for(form, cm.F32, dim)
    claim = cm.claimed_fraction(form, cm.F32, dim, chain)
    for d in (-1, 1):
        x, q = cm.swamp(form, cm.F32, dim, d, n=2)
        v = cm.chain_dot(form, x, q)
        true = x.astype(np.float64) @ q.astype(np.float64)
        assert (np.sign(v.astype(np.float64) - true) == d).all()
        frac = cm.attained_fraction(v, x, q, chain)
        print("%s dim %d dir %+d: attained %.4f of g_dot |q||x| (claimed %.4f)" % (form, dim, d, frac[0], claim))
        assert (frac >= claim).all() and (frac <= 1.0).all(), (frac, claim)
    if form == "scan32" and dim in (256, 1536):
        assert claim > (0.91 if dim == 256 else 0.97)


@pytest.mark.parametrize("form,dim", SETS)
def test_adversarial_set_margins(form, dim):
    chain = _chain_for(form, cm.F32, dim)
    s = cm.band_set(form, cm.F32, dim, k=10, chain=chain)
    m = s.margins()
    print("%s dim %d: T %.3f eps over a_k (rank %d, k' %d), last candidate %.3f eps over a_k" %
          (form, dim, m["T_over_ak"], m["rank_T"], m["kprime"], m["last_candidate"]))
    t = int(s.groups["true"][0])
    assert m["rank_T"] >= m["kprime"]                        # T is not among the candidates by value
    want, d64 = s.want()
    assert want[0] == t                                      # ... and is the true nearest in float64
    d32 = cm.exact_form_f32(s.rows, s.query)
    order32 = np.lexsort((np.arange(d32.size), d32))[:s.k]
    np.testing.assert_array_equal(order32, want)             # the fp32 exact form agrees, id for id
    dk = np.sort(d64)[:s.k + 1]
    assert (np.diff(dk) > 4.0 * cm.scan_bound(dim, cm.F32, chain)[2] * dk[1:]).all()    # apart by >> g_ref d: no ties
    assert (d64[s.groups["filler"]] > d64[s.groups["decoy"]].max()).all()
    assert m["flag_full"] and m["T_in_full_band"]            # the kernels' band: flagged, and T inside the wider band
    assert not m["flag_half"] and m["last_candidate"] > 1.0  # half the width: a candidate outside, T is lost
    assert 1.0 < m["T_over_ak"] <= 2.0


def test_fp16_sets_are_representable_and_ordered():
    for form, dim in (("scan32", 256), ("scan16", 1600), ("scan64", 320)):
        s = cm.band_set(form, cm.F16, dim, k=10, chain=cm.scan_chain_length(dim, cm.F16, form == "scan64"))
        want, d64 = s.want()
        assert want[0] == s.groups["true"][0] and set(want[1:]) <= set(s.groups["decoy"])
        assert (np.diff(np.sort(d64)[:11]) > 0).all()


def test_the_librarys_chain_length_is_the_models():
    """pgv_scan_chain_length (what scan_bound_chain is fed on each path) against the chain maps themselves and the
    model's copy of the formula: a wrong constant in the library fails here, whatever the Python copy says"""
    from pgvector_amd import _lib
    for dtype, code in ((cm.F32, _lib.PGV_F32), (cm.F16, _lib.PGV_F16)):
        for dim in list(range(1, 300)) + [1000, 1536, 1600, 2000, 3072, 4000]:
            real = {f: cm.longest_chain(f, dtype, dim) for f in ("scan32", "scan16", "scan64", "dense")}
            for path, name in ((0, "scan"), (1, "scan_wide"), (2, "topk128")):
                got = _lib.lib.pgv_scan_chain_length(dim, code, path)
                assert got == cm.charged_chain(name, dtype, dim), (dtype, dim, name, got)
                assert got >= max(real[f] for f in cm.forms_of(name)), (dtype, dim, name, got)
    assert _lib.lib.pgv_scan_chain_length(64, _lib.PGV_F16, 0) == 32
    assert _lib.lib.pgv_scan_chain_length(64, 7, 0) == -1 and _lib.lib.pgv_scan_chain_length(64, _lib.PGV_F32, 3) == -1


def test_a_ragged_chain_length_is_out_of_the_sets_reach():
    """scan_bound_chain ignoring its chain at 1600-d (quarter forms: 416 charged, ld / 4 = 400): the band computed from
    400 parts from the right one at 2 eps(404) / eps(420) = 1.92 eps above the k-th value.  A set defeats the narrow
    band only if a candidate lies beyond that, and every candidate lies below the true neighbour -- which the swamping
    puts at 1.77 eps.  So no set of this construction tells the two bands apart; the library's figure is checked
    directly instead (test_the_librarys_chain_length_is_the_models)."""
    dim = 1600
    for form in ("dense", "scan64"):
        chain = cm.dense_chain_length(dim, cm.F32)
        s = cm.band_set(form, cm.F32, dim, chain=chain)
        m = s.margins()
        qn, rn = cm.row_norms(s.query[None, :])[0], cm.row_norms(s.rows).max()
        narrow = float(cm.band_eps(cm.scan_bound(dim, cm.F32, dim / 4.0), qn, rn))
        parts_at = 2.0 * narrow / m["eps"]
        print("%s: the bands part at %.3f eps, T sits at %.3f eps" % (form, parts_at, m["T_over_ak"]))
        assert chain == 416 and 1.9 < parts_at < 1.95
        assert m["last_candidate"] < m["T_over_ak"] < parts_at


def test_the_assignments_band_at_half_width_is_out_of_reach():
    """argmin_reach over |a| / |c| in (0, 8] and every angle: what two swamped values can be inverted by stays below the
    band with gamma halved, and below the band with gamma AND gamma_exact halved -- so no input makes those mutations
    return a wrong center, and the assign test asserts answers and the recheck, not a half-width failure"""
    worst = 0.0
    for t in np.linspace(0.01, 8.0, 400):
        for rho in np.linspace(-1.0, 1.0, 201):
            inv, band = cm.argmin_reach(t, rho, 0.5, 1.0)
            assert inv < band, (t, rho, inv, band)
            inv2, band2 = cm.argmin_reach(t, rho, 0.5, 0.5)
            assert inv2 <= band2 * (1.0 + 1e-12), (t, rho, inv2, band2)
            worst = max(worst, inv / band)
    print("largest inversion / band with gamma halved: %.3f" % worst)
    rows, centers, t = cm.assign_set(256, cm.F32)
    d = np.sum((centers.astype(np.float64) - rows[0].astype(np.float64)) ** 2, axis=1)
    order = np.argsort(d)
    assert order[0] == t and d[order[1]] - d[t] > 1e-6 and d[order[4]] > 1.0
    assert centers.shape[0] >= 64 and np.allclose(np.sum(centers.astype(np.float64) ** 2, axis=1)[order[:4]], 4.0, atol=0.05)
