"""hnsw_search_kernel against answers recorded once from the commit before its steps were named
(tests/golden/hnsw_walk_parent_answers.json, tools/record_hnsw_walk_answers.py): element ids, the distances' bit patterns,
scored, per-batch counts and pool sizes, equal -- the order among equal keys included, which the host models leave open.
The cases and why they are the smallest that can go wrong: tests/hnsw_walk_steps_cases.py."""
import json
import os

import pytest

import hnsw_walk_steps_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_walk_parent_answers.json")
with open(GOLDEN) as f:
    WANT = json.load(f)

_got = {}


def got(ctx):
    if not _got:
        _got.update(cases.answers(ctx))
    return _got


def test_every_recorded_case_is_replayed(ctx):
    names = ["search %s ef %d" % (f, ef) for f in ("f32_l2", "f16_ip", "hamming", "jaccard", "sparse_l1") for ef in cases.EFS]
    names += ["scan %s ef %d" % (f, ef) for f in ("f32_l2", "jaccard") for ef in cases.EFS]
    names += ["build %s ef %d" % (f, ef) for f in ("f32_l2", "hamming", "jaccard") for ef in cases.BUILD_EFS]
    assert sorted(got(ctx)) == sorted(WANT) == sorted(names)


@pytest.mark.parametrize("name", sorted(WANT))
def test_walk_answers_as_recorded(ctx, name):
    assert got(ctx)[name] == WANT[name], name


def test_the_cases_reach_the_edges(ctx):
    """what the shapes are for, read off the answers: a W that is not full and one that is, pools that grow, a drain that
    returns entries, upper layers searched, and ties in every form's results"""
    g = got(ctx)
    for name, a in g.items():
        if name.startswith("search"):
            ef = int(name.split()[-1])
            assert len(a["elem"]) == cases.NQ * ef and all(e >= 0 for e in a["elem"]) and min(a["scored"]) >= ef
            if ef == 65:
                assert len(a["dist"]) < cases.NQ * ef // 4, name  # runs of equal distances
        elif name.startswith("scan"):
            ef = int(name.split()[-1])
            assert all(c == ef for b in a["batches"] for c in b["count"]), name
            assert max(a["batches"][-1]["left"]) > 0 and a["batches"][-1]["scored"] > a["batches"][0]["scored"]
            assert max(a["drain"]["count"]) > 0, name
        else:
            cnt = a["count"]
            assert len(cnt) == cases.NQ * cases.LAYER_CAP and max(cnt[1::cases.LAYER_CAP]) > 0 and max(cnt[2::cases.LAYER_CAP]) > 0
            for q, lv in enumerate(cases.BUILD_LEVELS):
                assert all((cnt[q * cases.LAYER_CAP + lc] > 0) == (lc <= lv) for lc in range(cases.LAYER_CAP)), (name, q)
