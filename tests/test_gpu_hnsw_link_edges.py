"""The device's graph updates of the in-memory HNSW build (pgv_hnsw_link_begin / _prepare / _apply / _end:
csrc/kernels_hnsw_link.hip, csrc/hnsw_link_core.h, the link section of csrc/pgv_abi_hnsw.hip) driven directly, with
hand-made requests on an empty graph and no searches, against the reference's update rule as tests/hnsw_link_model.py
restates it (pinned to the oracle in tests/test_hnsw_link_model_cpu.py).  Per scenario and knob setting:
  - the tuples pgv_hnsw_link_end returns equal the model's, tuple for tuple;
  - every batch's out_pairs of pgv_hnsw_link_prepare equals the model's first-round pair count;
  - out_deferred equals the model's count of lists that wait for their member triangle, under the verdict of the form
    that ran (any unfetched pair in a checked set: the wavefront form; the first unfetched pair before a deciding one:
    the serial forms);
  - pgv_hnsw_link_end returns OK: no update was left waiting;
  - for the scenarios of up to 500 rows the same after EVERY batch: pgv_hnsw_link_end is the one search-free way to read
    the tuples and the counts back, and it ends the build, so the child runs every prefix of the batches on its own.

The knobs are read once per process, so each setting runs every scenario in one child (tests/mp_hnsw_link_worker.py).
Which replay launch a scenario reaches (launch_hnsw_link_replay):

  m                        default                    PGV_HNSW_LINK_SERIAL=1
  4, 5, 8, 16 (2m <= 32)   hnsw_link_wave_kernel      hnsw_link_kernel<32>
  22, 23, 31 (2m+1 <= 64)  hnsw_link_wave_kernel      hnsw_link_kernel<64>
  32                       hnsw_link_kernel<64>       hnsw_link_kernel<64>
  100                      hnsw_link_kernel<200>      hnsw_link_kernel<200>

PGV_HNSW_PAIRS_GATHER=1 changes how the pair distances are produced (hnsw_link_pairs_kernel writes the slot pairs,
score_gather_kernel scores them) and makes the second round synchronous; it does not change the replay launch.

The scenarios (tests/hnsw_link_model.py builds them; the CPU test asserts the condition on each):
  hub       m 4: every new element chooses element 0; batches of 1, 3, 40, 200, shuffled: short -> full -> overflowing
            inside one batch, up to 200 newcomers into one list, handed over out of heap order
  ties      m 4 / 8 on a 2-d grid in [-4, 4] with identical rows, some not linked: equal distances next to each other in
            the order, CheckElementCloser pairs equal to the candidate's distance
  cache     m 4, three batches into the same lists: cached flags reused, removals, re-added rejects, deferred lists, lists
            where the two verdicts differ
  layers    m 5, levels 0..3: lists of m and of 2m overflow, layer_cap above some elements' levels
  lanes     m 31 (lists of 62, the newcomer in lane 62), m 32 (lists of 64), m 16 (lists of 32: the last shape of <32>)
  tri_cap   m 22 / 23: records of 990, 1035, 1081, 1128 pairs round the 1024 the wavefront form keeps in LDS
  wide      m 100: 7 200 records of 201 ids, twice: the synchronous second round, candidate indexes above 127; six
            crafted lists whose pruned item is what the second round decides from member-member distances
  scan      m 4: 4 095, 4 096, 4 097 records round the scan's 4 096 values a trip
  types     hub and cache with PGV_NEG_IP (distances of both signs) and with PGV_F16 rows

Also here: pgv_hnsw_build_neighbors at the ef <= 64 switch of launch_hnsw_select (select_cases in the worker)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hnsw_link_model as hm
import mp_hnsw_link_worker as w

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {
    "default": {},
    "serial": {"PGV_HNSW_LINK_SERIAL": "1"},
    "gather": {"PGV_HNSW_PAIRS_GATHER": "1"},
    "serial_gather": {"PGV_HNSW_LINK_SERIAL": "1", "PGV_HNSW_PAIRS_GATHER": "1"},
}
NAMES = list(hm.all_scenarios())
_MODEL, _RUNS = {}, {}


def model(name):
    """the model's answer for a scenario, computed once for all settings"""
    if name not in _MODEL:
        sc = hm.all_scenarios()[name]()
        prefixes = [] if len(sc["rows"]) <= hm.PREFIX_ROWS else None
        g, st = hm.run_model(sc, prefixes)
        _MODEL[name] = dict(m=sc["m"], nbr=g.tuples()[1], pairs=[s["pairs"] for s in st], prefixes=prefixes,
                            in_order=np.cumsum([s["deferred_in_order"] for s in st]).tolist(),
                            any=np.cumsum([s["deferred_any"] for s in st]).tolist())
    return _MODEL[name]


CHILD_SECONDS = 60       # on an MI355X a link child takes 2.5 - 4 s, the select child 2.3 s, start-up included


def device(setting, tmp_path_factory):
    """every scenario under one knob setting, in one fresh child.  The child is started ONCE per setting: if it fails,
    faults or runs into its time limit, the failure is kept and every later test of the setting fails from it without
    starting anything on the GPU again."""
    if setting not in _RUNS:
        path = str(tmp_path_factory.mktemp("hnsw_link") / (setting + ".npz"))
        env = {k: v for k, v in os.environ.items() if k not in ("PGV_HNSW_LINK_SERIAL", "PGV_HNSW_PAIRS_GATHER")}
        env.update(SETTINGS[setting])
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_hnsw_link_worker.py"), "link", path],
                               capture_output=True, text=True, timeout=CHILD_SECONDS, env=env)
            print(r.stdout)
            if r.returncode == 0 and "LINK-OK %d" % len(NAMES) in r.stdout:
                _RUNS[setting] = dict(np.load(path))
            else:
                _RUNS[setting] = "child under %s: exit %d\n%s\n%s" % (setting, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        except subprocess.TimeoutExpired as e:
            _RUNS[setting] = "child under %s: no end after %d s\n%s" % (setting, CHILD_SECONDS, str(e.stdout)[-3000:])
    if isinstance(_RUNS[setting], str):
        pytest.fail(_RUNS[setting], pytrace=False)
    return _RUNS[setting]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_device_links_are_the_reference_rule(setting, name, tmp_path_factory):
    got, want = device(setting, tmp_path_factory), model(name)
    wave = 2 * want["m"] + 1 <= 64 and "serial" not in setting
    deferred = want["any"] if wave else want["in_order"]
    print(name, setting, "pairs", got[name + "/pairs"].tolist(), want["pairs"], "deferred", int(got[name + "/deferred"]),
          "model in-order %s any %s" % (want["in_order"], want["any"]), "pairs2", int(got[name + "/pairs2"]))
    np.testing.assert_array_equal(got[name + "/nbr"], want["nbr"])
    assert got[name + "/pairs"].tolist() == want["pairs"]
    assert int(got[name + "/deferred"]) == deferred[-1]
    assert (int(got[name + "/pairs2"]) > 0) == (int(got[name + "/deferred"]) > 0)
    if want["prefixes"] is not None:                     # the state after every batch
        for k in range(1, len(want["pairs"])):
            np.testing.assert_array_equal(got["%s/nbr@%d" % (name, k)], want["prefixes"][k - 1], err_msg="after batch %d" % k)
            assert int(got["%s/deferred@%d" % (name, k)]) == deferred[k - 1], k
            assert (int(got["%s/pairs2@%d" % (name, k)]) > 0) == (deferred[k - 1] > 0), k


@pytest.mark.parametrize("name", NAMES)
def test_the_wavefront_and_the_serial_form_build_the_same_lists(name, tmp_path_factory):
    a, b = device("default", tmp_path_factory), device("serial", tmp_path_factory)
    np.testing.assert_array_equal(a[name + "/nbr"], b[name + "/nbr"])
    np.testing.assert_array_equal(a[name + "/pairs"], b[name + "/pairs"])


def test_select_neighbors_at_the_ef_64_switch(ctx):
    """ef_construction 64 / 65 x m 4 / 31 / 32 on a 600-row integer grid, in this process (the wavefront form up to
    ef 64)"""
    thinned = w.select_cases(ctx)
    print(thinned)
    assert set(thinned) == set(w.SELECT_CASES) and min(thinned.values()) >= 100, thinned


def test_select_neighbors_at_the_ef_64_switch_serial_form():
    """the same in a child with PGV_HNSW_SELECT_SERIAL=1"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_hnsw_link_worker.py"), "select"], capture_output=True,
                       text=True, timeout=CHILD_SECONDS, env=dict(os.environ, PGV_HNSW_SELECT_SERIAL="1"))
    print(r.stdout)
    assert r.returncode == 0 and "SELECT-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_select_neighbors_at_the_ef_64_switch_gathered_pairs():
    """the same in a child with PGV_HNSW_PAIRS_GATHER=1: the lists' pair triangles by expand_groups_kernel (the candidate
    lists described as g * ef ids, cnt[g] of them) and score_gather_kernel"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp_hnsw_link_worker.py"), "select"], capture_output=True,
                       text=True, timeout=CHILD_SECONDS, env=dict(os.environ, PGV_HNSW_PAIRS_GATHER="1"))
    print(r.stdout)
    assert r.returncode == 0 and "SELECT-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
