"""The verified place query on the GPU (include/visfs_place_verify.h): the device path against the host twin in every byte of both
result blocks and every hook on the inputs of place_verify_cases.py, what a call issues (one upload, seven launches, one download, one
wait for zero, one and eight candidates alike), the plain query and the plain PnP solve unchanged beside it, and the chain scene end
to end on resident images.  tests/test_place_verify_host.py holds the twin to the checker and to the staged calls on the same inputs."""
import numpy as np
import pytest

import place_cases as pc
import place_verify_cases as vc
from visfs_amd import abi, backend, flow, place, pnp
from visfs_amd import place_verify as pv

pytestmark = pytest.mark.gpu

HOOK_KEYS = ("m", "n_hypotheses", "n_passes", "winner") + vc.HOOK_KEYS


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _same_hooks(dv, hv, n_candidates):
    for c in range(8):
        for stage in (1, 2):
            got, want = dv.download_pnp(c, stage), hv.download_pnp(c, stage)
            for key in HOOK_KEYS:
                assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (c, stage, key)
        for got, want in zip(dv.download_guided(c), hv.download_guided(c)):
            assert got.tobytes() == want.tobytes(), c


def _same_call(dv, ds, hv, hs, params, query_xyz, **place_params):
    rc, r, w = dv.query_verify_raw(ds, params, query_xyz, **place_params)
    assert rc == abi.OK, dv.last_error()
    assert dv.last_counts() == (1, pv.LAUNCHES, 1, 1) == (1, 7, 1, 1)
    rc, hr, hw = hv.query_verify_raw(hs, params, query_xyz, **place_params)
    assert rc == abi.OK, hv.last_error()
    assert bytes(memoryview(r)) == bytes(memoryview(hr)), "place block"
    for c in range(8):
        for stage in ("stage1", "stage2"):
            assert bytes(memoryview(getattr(w.candidate[c], stage))) == bytes(memoryview(getattr(hw.candidate[c], stage))), (c, stage)
    assert bytes(memoryview(w)) == bytes(memoryview(hw)), "verify block"
    _same_hooks(dv, hv, r.n_candidates)
    return place.unpack(r), pv.unpack(w, r.n_candidates)


@pytest.mark.parametrize("name", list(vc.CASES))
def test_device_equals_the_host_twin(solver, name):
    case = vc.case(name)
    dev, hst = flow.Flow(flow.default_params(**pc.FLOW), 160, 120, solver=solver), flow.Flow(flow.default_params(**pc.FLOW), 160, 120)
    ds, ddb = vc.load(case, dev, solver)
    hs, hdb = vc.load(case, hst)
    dv, hv = pv.Verifier(ddb), pv.Verifier(hdb)
    seen = set()
    for variant in case["variants"]:
        p, w = _same_call(dv, ds, hv, hs, vc.params(variant), case["query_xyz"] if variant["xyz"] else None, **variant["place"])
        seen.add(len(p["candidates"]))
        rc, plain = ddb.query_raw(ds, **variant["place"])             # the plain query beside it: its own launches, the same block
        assert rc == abi.OK and ddb.last_counts() == (1, 2, 1, 1) and bytes(memoryview(plain)) == p["raw"]
    if name == "ten_equal":
        assert seen == {0, 1, 8}
    for o in (dv, hv, ddb, hdb, ds, hs, dev, hst):
        o.close()


def test_the_plain_calls_are_what_they_were_on_the_device(solver):
    """visfs_place_query and the device visfs_pnp_solve on the same inputs before and after a verify call: same bytes, same counts;
    a shorter call after a longer one leaves nothing of the longer one behind."""
    case = vc.case("geometry")
    dev, hst = flow.Flow(flow.default_params(**pc.FLOW), 160, 120, solver=solver), flow.Flow(flow.default_params(**pc.FLOW), 160, 120)
    ds, ddb = vc.load(case, dev, solver)
    hs, hdb = vc.load(case, hst)
    psolver, cam = pnp.Pnp(512, solver=solver), pnp.camera(*vc.K, Tir=vc.TIR)
    rc, before = ddb.query_raw(ds, min_matches=1)
    assert rc == abi.OK and ddb.last_counts() == (1, 2, 1, 1)
    rows = place.unpack(before)["candidates"][0]["rows"]
    a = psolver.solve(pnp.default_params(), cam, rows["from_xyz"], rows["to_xy"])
    dv, hv = pv.Verifier(ddb), pv.Verifier(hdb)
    first = _same_call(dv, ds, hv, hs, vc.params(case["variants"][0]), None, min_matches=1)
    assert ddb.last_counts() == (1, 2, 1, 1)
    rc, after = ddb.query_raw(ds, min_matches=1)
    assert bytes(memoryview(after)) == bytes(memoryview(before))
    b = psolver.solve(pnp.default_params(), cam, rows["from_xyz"], rows["to_xy"])
    for key in ("T", "cov", "matches", "inliers"):
        assert a[key].tobytes() == b[key].tobytes()
    assert first[1]["candidates"][0]["stage1"]["T"].tobytes() == a["T"].tobytes()
    none = _same_call(dv, ds, hv, hs, vc.params(case["variants"][0]), None, min_matches=500)      # no candidate after one
    assert none[1]["best"] == -1 and len(none[0]["candidates"]) == 0
    again = _same_call(dv, ds, hv, hs, vc.params(case["variants"][0]), None, min_matches=1)
    assert again[1]["raw"] == first[1]["raw"]
    for o in (dv, hv, psolver, ddb, hdb, ds, hs, dev, hst):
        o.close()


@pytest.mark.parametrize("seed", [1, 3])
def test_the_chain_scene_on_the_device(solver, seed):
    """Describe, add, query, verify and the guided stage on resident images (tests/test_place_verify_host.py states the counts)."""
    df, ds, ddb, moved, xyz = vc.chain_scene(seed, solver)
    hf, hs, hdb, _, hxyz = vc.chain_scene(seed)
    assert xyz.tobytes() == hxyz.tobytes()
    dv, hv = pv.Verifier(ddb), pv.Verifier(hdb)
    p, w = _same_call(dv, ds, hv, hs, pv.default_params(camera=vc.chain_camera()), xyz)
    assert w["best"] == 0
    c = w["candidates"][0]
    assert len(c["stage2"]["inliers"]) >= len(c["stage1"]["inliers"]) >= 160
    for o in (dv, hv, ddb, hdb, ds, hs, df, hf):
        o.close()
