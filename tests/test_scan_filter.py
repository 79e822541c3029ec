"""The one-core twin of the laser pretreatment with its voxel filters (include/visfs_scan_filter.h, h == NULL) against the
plain-Python checker tests/scan_filter_oracle.py, byte for byte in the records, the range data, the match clouds and the hook data,
on the cases of tests/scan_filter_cases.py; the checker itself is first held to answers known without any code.
tests/test_gpu_scan_filter.py holds the device to the twin on the same cases."""
import numpy as np
import pytest

import scan_filter_cases as fc
import scan_filter_oracle as fo
from visfs_amd import abi
from visfs_amd import scan_filter as sf
from visfs_amd import scan_match as scm

CASES = fc.cases()
KNOWN = fc.known_answers()
_ORACLE = {}


def oracle(case):
    """The checker's result of every scan of a case, computed once."""
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = [fo.process(p, T, o, case["params"]) for p, T, o in case["scans"]]
    return _ORACLE[case["name"]]


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def results(f, case):
    """What a filter object gives for a case: per scan dict(record, range_data, match, cls, sub, kept, trace)."""
    rc, recs = f.process(case["scans"], sf.default_params(**case["params"]))
    assert rc == abi.OK, f.last_error()
    assert f.num_scans() == len(case["scans"])
    out = []
    for i, (pts, _, _) in enumerate(case["scans"]):
        assert f.record(i) == (abi.OK, recs[i])
        out.append(dict(f.download(i, len(pts)), record=recs[i], range_data=f.range_data(i), match=f.match_cloud(i)))
    return out


def assert_same_result(a, b, what=""):
    assert a["record"] == b["record"], what
    assert len(a["range_data"]) == len(b["range_data"]) == a["record"]["n_range_data"], what
    for (o1, r1, m1), (o2, r2, m2) in zip(a["range_data"], b["range_data"]):
        same(o1, o2, what); same(r1, r2, what); same(m1, m2, what)
    same(a["match"], b["match"], what)
    for k in ("cls", "sub", "kept"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["trace"] == b["trace"], what


@pytest.mark.parametrize("name,points,length,kept", KNOWN, ids=[k[0] for k in KNOWN])
def test_the_checker_meets_the_known_answers(name, points, length, kept):
    assert fo.voxel_filter(points, length) == kept
    r = fo.process(points, fc.IDENTITY, fc.ZERO, dict(fc.ALL_RETURNS, voxel_size=length, adaptive_max_length=0.0))
    assert list(np.flatnonzero(r["kept"])) == kept and r["record"]["n_returns"] == len(kept)
    same(r["range_data"][0][1], points[kept]); same(r["match"], points[kept])


@pytest.mark.parametrize("name,points,length,kept", KNOWN, ids=[k[0] for k in KNOWN])
def test_the_twin_meets_the_known_answers(name, points, length, kept):
    f = sf.ScanFilter()
    rc, recs = f.process([points], sf.default_params(**dict(fc.ALL_RETURNS, voxel_size=length, adaptive_max_length=0.0)))
    assert rc == abi.OK and recs[0]["n_returns"] == len(kept)
    assert list(np.flatnonzero(f.download(0, len(points))["kept"])) == kept
    same(f.match_cloud(0), points[kept])
    f.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_checker(case):
    f = sf.ScanFilter()
    got, want = results(f, case), oracle(case)
    for i, (a, b) in enumerate(zip(got, want)):
        assert_same_result(a, b, (case["name"], i))
    assert f.last_counts() == (0, 0, 0)
    bad = [i for i, r in enumerate(got) if r["record"]["status"] != abi.OK]
    assert bad == case.get("bad", [])
    for i in bad:
        assert got[i]["record"] == dict(status=abi.ERR_UNSUPPORTED, n_range_data=0, n_returns=0, n_misses=0, n_in_range=0, n_match=0, passes=0,
                                        match_length=0.0)
        assert got[i]["range_data"] == [] and len(got[i]["match"]) == 0 and not got[i]["kept"].any()
    f.close()


ADAPTIVE = [c for c in CASES if "branch" in c]


@pytest.mark.parametrize("case", ADAPTIVE, ids=[c["name"] for c in ADAPTIVE])
def test_the_adaptive_case_takes_its_branch(case):
    f = sf.ScanFilter()
    r = results(f, case)[0]
    prm = dict(fo.DEFAULTS, **case["params"])
    got, want = fc.branch_of(r["record"], r["trace"], prm), case["branch"]
    assert got[:2] == want[:2], got
    if len(want) > 2:
        assert want[2] in got[2], got
        assert r["record"]["passes"] == 1 + want[1] + len(got[2]) <= 12
    o = oracle(case)[0]
    assert fc.branch_of(o["record"], o["trace"], prm) == got
    f.close()


def test_the_shapes_are_what_they_claim():
    by = {c["name"]: c for c in CASES}
    f = sf.ScanFilter()
    one = results(f, by["n_16384_one_voxel"])[0]
    assert one["record"]["n_returns"] == 1 and one["kept"][0] == 1
    full = results(f, by["n_16384_all_distinct"])[0]
    assert full["record"]["n_returns"] == 16384 and full["record"]["passes"] == 1
    two = results(f, by["n_2_one_voxel"])[0]
    assert list(two["kept"]) == [1, 0]
    for n in (1023, 1024, 1025):
        r = results(f, by[f"n_{n}"])[0]
        assert n // 8 < r["record"]["n_returns"] < n                        # the filter has work to do
    assert results(f, by["all_below_min_range"])[0]["record"]["n_returns"] == 0
    r = results(f, by["all_below_min_range"])[0]
    assert (r["record"]["n_range_data"], r["record"]["n_misses"]) == (2, 0) and not r["cls"].any()
    r = results(f, by["all_misses"])[0]
    assert r["record"]["n_returns"] == 0 and r["record"]["n_misses"] > 0 and (r["cls"] == sf.MISS).all()
    r = results(f, by["more_subdivisions_than_points"])[0]
    assert r["record"]["n_range_data"] == 5 and len(r["cls"]) == 5
    r = results(f, by["adaptive_range_cut_first"])[0]
    assert (r["record"]["n_returns"], r["record"]["n_in_range"], r["record"]["n_match"]) == (300, 150, 150)
    f.close()


def test_the_collision_case_collides_in_the_library_table():
    case = next(c for c in CASES if c["name"] == "colliding_keys")
    pts = case["scans"][0][0]
    vox = np.round(pts / 0.25).astype(np.int32)
    assert len(pts) == 128 and len({tuple(v) for v in vox}) == 64
    for v in vox:
        assert sf.hook_slot(v, len(pts)) == (abi.OK, 256, 5)
        assert fc.hash_slot(v, 0, 256) == 5
    rng = np.random.default_rng(5)
    for v, lst, cnt in zip(rng.integers(-sf.MAX_VOXEL, sf.MAX_VOXEL + 1, (200, 3)), rng.integers(0, 32, 200), rng.integers(0, 16385, 200)):
        rc, slots, slot = sf.hook_slot(v, int(cnt), int(lst))               # the restated hash is the library's
        assert (rc, slots, slot) == (abi.OK, fc.table_slots(int(cnt)), fc.hash_slot(v, int(lst), fc.table_slots(int(cnt))))
    assert sf.hook_slot((sf.MAX_VOXEL + 1, 0, 0), 4)[0] == abi.ERR_UNSUPPORTED


PRETREAT = [c for c in CASES if c.get("pretreat_only")]


@pytest.mark.parametrize("case", PRETREAT, ids=[c["name"] for c in PRETREAT])
def test_filters_off_reproduces_scan_pretreat(case):
    f = sf.ScanFilter()
    prm = sf.default_params(**case["params"])
    pts, T, o = case["scans"][0]
    rc, recs = f.process(case["scans"], prm)
    assert rc == abi.OK
    want, got = scm.pretreat(pts, T, o, prm.pretreat), f.range_data(0)
    assert len(want) == len(got) == prm.pretreat.num_subdivisions
    assert sum(len(r) for _, r, _ in want) > 0 and sum(len(m) for _, _, m in want) > 0
    for (o1, r1, m1), (o2, r2, m2) in zip(want, got):
        same(o1, o2); same(r1, r2); same(m1, m2)
    assert recs[0]["passes"] == 0 and recs[0]["match_length"] == 0.0 and recs[0]["n_match"] == recs[0]["n_in_range"]
    f.close()


def test_each_scan_of_the_batch_equals_a_call_with_that_scan_alone():
    case = next(c for c in CASES if c["name"] == "batch_64")
    f, g = sf.ScanFilter(), sf.ScanFilter()
    batch = results(f, case)
    assert sorted({len(p) for p, _, _ in case["scans"]})[0] == 0 and len(case["scans"]) == 64
    for i in range(0, 64, 3):
        alone = results(g, dict(case, scans=[case["scans"][i]]))[0]
        assert_same_result(batch[i], alone, i)
    without = results(g, dict(case, scans=[s for i, s in enumerate(case["scans"]) if i not in case["bad"]]))
    kept = [r for i, r in enumerate(batch) if i not in case["bad"]]
    for i, (a, b) in enumerate(zip(kept, without)):
        assert_same_result(a, b, i)                                         # unchanged by the refused scan's presence
    f.close(); g.close()


def test_every_refusal_leaves_the_previous_results_readable():
    case = next(c for c in CASES if c["name"] == "filtered_room_4_subdivisions")
    f = sf.ScanFilter()
    before = results(f, case)[0]
    pts = case["scans"][0][0]
    nan, inf = float("nan"), float("inf")
    bad_pts = pts.copy(); bad_pts[7, 1] = nan
    big = np.zeros((sf.MAX_POINTS + 1, 3))
    refusals = [
        ([bad_pts], {}, abi.ERR_BAD_ARGUMENT),
        ([(pts, (inf,) + fc.IDENTITY[1:], fc.ZERO)], {}, abi.ERR_BAD_ARGUMENT),
        ([(pts, fc.IDENTITY, (0.0, nan, 0.0))], {}, abi.ERR_BAD_ARGUMENT),
        ([pts], dict(voxel_size=-0.1), abi.ERR_BAD_ARGUMENT),
        ([pts], dict(adaptive_max_length=-0.5), abi.ERR_BAD_ARGUMENT),
        ([pts], dict(adaptive_max_range=-1.0), abi.ERR_BAD_ARGUMENT),
        ([pts], dict(voxel_size=nan), abi.ERR_BAD_ARGUMENT),
        ([pts], dict(adaptive_min_num_points=-1), abi.ERR_BAD_ARGUMENT),
        ([pts], dict(num_subdivisions=0), abi.ERR_BAD_ARGUMENT),
        ([pts] * (sf.MAX_SCANS + 1), {}, abi.ERR_UNSUPPORTED),
        ([pts, big], {}, abi.ERR_UNSUPPORTED),
        ([pts], dict(num_subdivisions=sf.MAX_SUBDIVISIONS + 1), abi.ERR_UNSUPPORTED),
    ]
    for scans, kw, want in refusals:
        rc, recs = f.process(scans, sf.default_params(**kw))
        assert rc == want and recs == [] and f.last_error(), (kw, rc)
        assert f.num_scans() == 1 and f.last_counts() == (0, 0, 0)
        after = dict(f.download(0, len(pts)), record=f.record(0)[1], range_data=f.range_data(0), match=f.match_cloud(0))
        assert_same_result(before, after, kw)
    assert f.record(1)[0] == abi.ERR_BAD_ARGUMENT and f.record(-1)[0] == abi.ERR_BAD_ARGUMENT
    rc, recs = f.process([], sf.default_params())                          # m == 0: fine, and nothing left to read
    assert (rc, recs, f.num_scans()) == (abi.OK, [], 0) and f.record(0)[0] == abi.ERR_BAD_ARGUMENT
    rc, recs = f.process([np.zeros((0, 3))], sf.default_params(num_subdivisions=3))
    assert rc == abi.OK and recs[0] == dict(status=abi.OK, n_range_data=0, n_returns=0, n_misses=0, n_in_range=0, n_match=0, passes=0, match_length=0.0)
    assert f.range_data(0) == [] and len(f.match_cloud(0)) == 0
    f.close()


def test_abi_and_defaults():
    assert sf.load().visfs_scan_filter_abi_version() == sf.ABI_VERSION == 1
    p = sf.default_params()
    assert (p.voxel_size, p.adaptive_max_length, p.adaptive_min_num_points, p.adaptive_max_range) == (0.025, 0.5, 200, 50.0)
    q = scm.default_pretreat_params()
    assert (p.pretreat.num_subdivisions, p.pretreat.min_range, p.pretreat.max_range, p.pretreat.missing_ray_length) == \
        (q.num_subdivisions, q.min_range, q.max_range, q.missing_ray_length)
