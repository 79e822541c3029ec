"""One GPU object through its growth paths and its life (visfs_amd/csrc/ba_host.hpp: DeviceBuf, PinnedBuf, Staged): the smallest
shape, a shape that crosses the capacity of a buffer pair, the smallest shape again, each call held to the host twin with the
comparison of the object's own GPU test; then the object is destroyed and made again three times.  Only the growth paths that no
other GPU test crosses in both directions stand here; DESIGN.md section 1a lists the test of every path."""
import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo
import global_map_cases as gc
import scan_refine_cases as rc
from visfs_amd import abi, backend, corners, flow
from visfs_amd import global_map as gm

pytestmark = pytest.mark.gpu

LIVES = 3


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


# ---------------------------------------------------------------- corner extraction: the discs and their half-widths (h_disc, d_disc)
def grid_discs(n, w):
    """n discs of radius 1 that do not touch, so every one is drawn and takes 16 bytes of the block."""
    per_row = (w - 4) // 4
    return [(float(2 + 4 * (k % per_row)), float(2 + 4 * (k // per_row)), 1) for k in range(n)]


def same_corners(dev, host, discs):
    got, want = corners.corners(dev, discs=discs, max_corners=150, min_distance=10.0), corners.corners(host, discs=discs, max_corners=150, min_distance=10.0)
    a, b = corners.download(dev, len(discs)), corners.download(host, len(discs))
    for key in ("eig", "mask", "disc_drawn", "max_val"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_candidates"] == b["n_candidates"] and a["disc_drawn"].all()
    assert got.tobytes() == want.tobytes() and len(got) > 0


def test_corner_discs_grow_past_the_first_block_and_back(solver):
    """The first block holds 16384 bytes: one disc, then 1100 (17600 bytes of discs alone), then one."""
    w, h = 320, 240
    img = fc.base_image(w, h)
    host = flow.Flow(flow.default_params(), w, h)
    host.push_frame(img, img)
    for _ in range(LIVES):
        dev = flow.Flow(flow.default_params(), w, h, solver=solver)
        dev.push_frame(img, img)
        for n in (1, 1100, 1):
            same_corners(dev, host, grid_discs(n, w))
        dev.close()
    host.close()


# ---------------------------------------------------------------- global map: the table of tiles (h_tab, d_tab), 16 records at first
def test_map_table_grows_past_sixteen_tiles_and_back(solver):
    rng = np.random.default_rng(31)
    one = [gc.tile(rng, 1, 1, unknown=0.0)]
    many = [gc.tile(rng, 3, 2, pose=(0.1 * k, -0.05 * k, 0.2 * k)) for k in range(17)]
    host = gm.GlobalMap()
    for _ in range(LIVES):
        dev = gm.GlobalMap(solver)
        for tiles in (one, many, one):
            for m in (dev, host):
                assert m.clear() == abi.OK
                for k, t in enumerate(tiles):
                    assert m.add_grid(t["cells"], t["limits"], t["pose"]) == (abi.OK, k), m.last_error()
            for mode in (gm.ODDS, gm.LATEST, gm.OCCUPIED):
                out = []
                for m in (dev, host):
                    rc_, info = m.compose(mode, 0.05, None)
                    assert rc_ == abi.OK, m.last_error()
                    out.append((info,) + tuple(m.download()))
                (ia, ra, ca, na), (ib, rb, cb, nb) = out
                assert ia == ib and ra == rb == abi.OK
                assert ca.shape == cb.shape and ca.tobytes() == cb.tobytes() and na.tobytes() == nb.tobytes()
                assert dev.last_counts() == (1, 1, 1) and host.last_counts() == (0, 0, 0)
        dev.close()
    host.close()


# ---------------------------------------------------------------- scan refinement: the job and its points (h_up, d_up)
def test_refine_upload_grows_with_the_points_and_back(solver):
    """A stack's single calls with 1 point, 1025 points, 1 point: the upload is the job and 16 bytes per point, half as much again."""
    case = next(c for c in rc.cases() if c["name"] == "n1025")
    pts = np.asarray(case["points"])
    host = rc.Opened(case)
    for _ in range(LIVES):
        dev = rc.Opened(case, solver)
        for n in (1, len(pts), 1):
            (sd, rd), (sh, rh) = dev.refine(points=pts[:n]), host.refine(points=pts[:n])
            assert sd == sh == abi.OK, (dev.last_error(), host.last_error())
            rc.same_refinement(rd, rh, dev.trace(), host.trace())
            assert rd["refined"] == 1
        dev.close()
    host.close()


# ---------------------------------------------------------------- window covariances: the factor and the band of Sigma (d_cov)
def test_covariance_scratch_grows_with_the_window_and_back(olib):
    """This object has no host twin: one handle through a small window, a larger one and the small one again returns the bytes
    that a fresh handle returns for each, as test_gpu_phase_edges.py holds the uploads of two sizes on one handle."""
    from helpers import graph_of
    from visfs_amd import synth
    prm = abi.default_params(iterations=10, solver=0)
    graphs = {cfg: graph_of(olib.oracle_pack_window, prm, synth.make_window(cfg))[1] for cfg in ("C1", "C2")}

    def covariances(s, gb):
        s.upload(gb)
        assert s.optimize()[0] == abi.OK
        pose, cross, pt = s.covariance(points=True, cross=True)
        return pose.tobytes(), cross.tobytes(), pt.tobytes()

    fresh = {}
    for cfg, gb in graphs.items():
        s = backend.Solver(prm)
        fresh[cfg] = covariances(s, gb)
        s.close()
    assert len(fresh["C1"][0]) < len(fresh["C2"][0])
    for _ in range(LIVES):
        s = backend.Solver(prm)
        for cfg in ("C1", "C2", "C1"):
            assert covariances(s, graphs[cfg]) == fresh[cfg], cfg
        s.close()


# ---------------------------------------------------------------- flow: a call's points in and results out (h_io, d_io)
def test_flow_points_grow_past_the_initial_capacity_and_back(solver):
    w, h = 320, 240
    frames = fc.sequence(2)
    host = flow.Flow(flow.default_params(), w, h)
    for pair in frames:
        host.push_frame(*pair)
    pts = fo.random_points(1500, w, h, 5, seed=9)
    want = {n: host.track(pts[:n]) for n in (1, 1500)}
    for _ in range(LIVES):
        dev = flow.Flow(flow.default_params(), w, h, solver=solver)
        for pair in frames:
            dev.push_frame(*pair)
        for n in (1, 1500, 1):
            got = dev.track(pts[:n])
            assert len(got) == len(want[n]) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want[n])), n
        dev.close()
    host.close()


# ---------------------------------------------------------------- batches: the graphs and the gathered LM states (d_graphs, d_lm, h_lm, d_all)
def test_batch_scratch_grows_with_the_batch_and_back(olib):
    """No host twin here either: one handle through batches of 1, 5 and 1, as solve_batch of windows and as batch_upload, batch_reset
    and batch_optimize of resident graphs, returns the bytes that a fresh handle returns for a batch of that size."""
    from helpers import graph_of
    from visfs_amd import synth
    prm = abi.default_params(iterations=10, solver=2)
    ws = [synth.make_window("C1", window_index=i) for i in range(5)]
    gbs = [graph_of(olib.oracle_pack_window, prm, w)[1] for w in ws]

    def windows(s, n):
        out = []
        for rb in s.solve_batch([abi.WindowBuffers(w) for w in ws[:n]]):
            assert rb.struct.status == abi.OK
            out.append((rb.pose_Twr_out.tobytes(), tuple(rb.outliers()), tuple(rb.struct.iterations_run), rb.struct.chi2_final))
        return out

    def resident(s, n):
        s.batch_upload(gbs[:n])
        s.batch_reset()
        rc_, stats = s.batch_optimize()
        assert rc_ == abi.OK and all(st.status == abi.OK for st in stats)
        return [tuple(a.tobytes() for a in s.batch_download(i)) for i in range(n)]

    fresh = {}
    for n in (1, 5):
        for run in (windows, resident):
            s = backend.Solver(prm)
            fresh[run, n] = run(s, n)
            s.close()
    for _ in range(LIVES):
        s = backend.Solver(prm)
        for n in (1, 5, 1):
            assert windows(s, n) == fresh[windows, n], n
            assert resident(s, n) == fresh[resident, n], n
        s.close()
