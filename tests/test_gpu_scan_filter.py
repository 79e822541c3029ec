"""The laser pretreatment with its voxel filters on the GPU (include/visfs_scan_filter.h on a visfs_ba handle: k_scan_filter, one
workgroup per scan) against the one-core host twin, byte for byte in the records, the range data, the match clouds and the hook
data, on the cases of tests/scan_filter_cases.py; tests/test_scan_filter.py holds the twin to the plain-Python checker on the
same cases."""
import numpy as np
import pytest

import scan_filter_cases as fc
import scan_match_cases as smc
from test_scan_filter import assert_same_result, results, same
from visfs_amd import abi, backend
from visfs_amd import scan_filter as sf
from visfs_amd import scan_match as scm
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu

CASES = fc.cases()
COUNTS = (1, 2, 1)          # launches, copies (one upload, one download), waits of a call, whatever it holds


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture(scope="module")
def twin_results():
    """The twin's result of every case, computed once."""
    f = sf.ScanFilter()
    out = {c["name"]: results(f, c) for c in CASES}
    f.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin(solver, twin_results, case):
    dev = sf.ScanFilter(solver)
    got, want = results(dev, case), twin_results[case["name"]]
    for i, (a, b) in enumerate(zip(got, want)):
        assert_same_result(a, b, (case["name"], i))
    assert [i for i, r in enumerate(got) if r["record"]["status"] != abi.OK] == case.get("bad", [])
    assert dev.last_counts() == COUNTS
    dev.close()


def test_the_largest_call_64_scans_of_16384_points(solver):
    case = fc.big_batch()
    dev, host = sf.ScanFilter(solver), sf.ScanFilter()
    prm = sf.default_params(**case["params"])
    rc, a = dev.process(case["scans"], prm)
    assert rc == abi.OK, dev.last_error()
    rc, b = host.process(case["scans"], prm)
    assert rc == abi.OK and a == b and dev.last_counts() == COUNTS
    assert all(r["n_returns"] > 1000 and r["n_misses"] > 0 and 200 <= r["n_match"] < r["n_in_range"] for r in a)
    for i in range(64):
        ra, rb = dev.range_data_struct(i), host.range_data_struct(i)
        assert ra[2] == rb[2] == 2
        for k in range(2):
            x, y = ra[1][k], rb[1][k]
            assert (x.n_returns, x.n_misses, list(x.origin)) == (y.n_returns, y.n_misses, list(y.origin))
            same(np.ctypeslib.as_array(x.returns, shape=(x.n_returns, 3)), np.ctypeslib.as_array(y.returns, shape=(y.n_returns, 3)), i)
            same(np.ctypeslib.as_array(x.misses, shape=(x.n_misses, 3)), np.ctypeslib.as_array(y.misses, shape=(y.n_misses, 3)), i)
        same(dev.match_cloud(i), host.match_cloud(i), i)
    for i in (0, 63):
        x, y = dev.download(i, 16384), host.download(i, 16384)
        assert x["trace"] == y["trace"] and all(np.array_equal(x[k], y[k]) for k in ("cls", "sub", "kept"))
    dev.close(); host.close()


def test_the_counts_do_not_depend_on_the_number_of_scans(solver):
    rng = np.random.default_rng(51)
    scans = [fc.bare(fc.room_scan(rng, 300 + 17 * b, far=0.1)) for b in range(64)]
    dev = sf.ScanFilter(solver)
    assert dev.last_counts() == (0, 0, 0)
    counts = []
    for m in (1, 64, 2):
        rc, recs = dev.process(scans[:m], sf.default_params(num_subdivisions=3))
        assert rc == abi.OK and len(recs) == m
        counts.append(dev.last_counts())
    assert counts == [COUNTS] * 3
    rc, recs = dev.process([], sf.default_params())                        # m == 0 launches nothing
    assert rc == abi.OK and dev.last_counts() == (0, 0, 0)
    dev.close()


def test_one_object_through_growing_and_shrinking_calls(solver):
    rng = np.random.default_rng(52)
    dev, host = sf.ScanFilter(solver), sf.ScanFilter()
    for sizes in ((40,), (3000, 5, 0, 700), (9,), (16384, 1), (2, 2, 2), (1500,) * 9, (0,), (64,)):
        case = dict(name="sizes", scans=[fc.bare(fc.room_scan(rng, n, far=0.1, near=0.05)) for n in sizes], params=dict(num_subdivisions=2, voxel_size=0.05))
        got, want = results(dev, case), results(host, case)
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same_result(a, b, (sizes, i))
    # a refusal leaves the last call's results and counts
    before = results(dev, case)[0]
    rc, _ = dev.process([np.full((3, 3), np.nan)], sf.default_params())
    assert rc == abi.ERR_BAD_ARGUMENT and dev.last_counts() == COUNTS and dev.num_scans() == 1
    after = dict(dev.download(0, 64), record=dev.record(0)[1], range_data=dev.range_data(0), match=dev.match_cloud(0))
    assert_same_result(before, after)
    dev.close(); host.close()


def test_a_scan_match_fed_the_device_cloud_equals_one_fed_the_twin_cloud(solver):
    case = smc.base_cases()[0]
    sub = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]), solver=solver)
    smc.fill(sub, case)
    raw = smc.cast(case["truth"], 6000, np.random.default_rng(53))          # a dense scan from the truth pose, robot frame
    dev, host = sf.ScanFilter(solver), sf.ScanFilter()
    prm = sf.default_params(num_subdivisions=2, adaptive_min_num_points=150)
    assert dev.process([raw], prm)[0] == abi.OK and host.process([raw], prm)[0] == abi.OK
    a, b = dev.match_cloud(0), host.match_cloud(0)
    assert 150 <= len(a) < 6000 // 4
    same(a, b)
    w = case["prm"]
    mp = scm.default_params(linear_search_window=w[0], angular_search_window=w[1], translation_delta_cost_weight=w[2], rotation_delta_cost_weight=w[3])
    ra = sub.match(case["guess"], a, mp)
    da = sub.match_download()
    rb = sub.match(case["guess"], b, mp)
    db = sub.match_download()
    assert ra[0] == abi.OK and ra == rb and ra[1]["matched"] == 1
    for x, y in zip(da, db):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert abs(ra[1]["x"] - case["truth"][0]) < 0.05 and abs(ra[1]["y"] - case["truth"][1]) < 0.05 and abs(ra[1]["yaw"] - case["truth"][2]) < 0.03
    # the device's filtered range data go into the sub-maps as visfs_submaps_insert takes them
    assert sub.insert(smc.pose_T(*case["truth"]), dev.range_data(0)) == abi.OK, sub.last_error()
    dev.close(); host.close(); sub.close()
