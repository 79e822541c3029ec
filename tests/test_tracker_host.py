"""The resident front end (include/visfs_tracker.h) on the CPU: the host twin of visfs_tracker_process against the checker of
tracker_oracle.py, frame by frame, byte for byte in every output array, flag and intermediate list.  No tolerances."""
import numpy as np
import pytest

import tracker_cases as tc
import tracker_oracle as to
from visfs_amd import abi, backend, flow, tracker


def _run(scn, what=""):
    ref, sub = tc.checker(scn), tc.Subject(scn)
    try:
        return tc.lockstep(scn, ref, [sub], what), ref.stats
    finally:
        ref.close(); sub.close()


@pytest.mark.parametrize("name", sorted(tc.BASE))
def test_base_sequence_equals_the_checker(name):
    log, stats = _run(tc.BASE[name](), name)
    print(name, stats)
    # the sequence exercised what it is for
    assert stats["left_border"] >= 1                  # words left through the image border (Tracker.cpp:286)
    assert stats["topups_after_first"] >= 1           # a top-up happened after frame 1
    assert stats["undrawn"] >= 1                      # a disc was not drawn because its centre was covered
    assert stats["unequal_counts"] >= 1               # track counts in one frame were not all equal
    assert log[0][0]["flags"] == to.NO_PREVIOUS and log[1][0]["flags"] == to.BOOTSTRAPPED
    assert all(r["flags"] == 0 for r, _ in log[2:])


def test_full_size_equals_the_checker():
    log, _ = _run(tc.full_size(), "full size")
    assert len(log[2][0]["word_id"]) > 150


@pytest.mark.parametrize("name", sorted(tc.WAVE))
def test_wave_boundary_counts_equal_the_checker(name):
    scn = tc.WAVE[name]()
    log, _ = _run(scn, name)
    assert max(len(r["covisible_id"]) for r, _ in log) >= scn["trk"]["max_features"] - 8      # the rows do reach the boundary


@pytest.mark.parametrize("name", list(tc.WINDOW))
def test_window_sizes_equal_the_checker(name):
    """Window sizes other than 21 through the whole front end.  Every scenario bootstraps on frame 1 and then tracks: frames 2-4
    carry no LOST flag and at least 40 words on the checker, so the comparison is not one of empty lists."""
    log, _ = _run(tc.WINDOW[name](), name)
    words = [len(r["word_id"]) for r, _ in log]
    print(f"{name}: flags {[int(r['flags']) for r, _ in log]}, words per frame {words}, covisible {[len(r['covisible_id']) for r, _ in log]}")
    assert log[1][0]["flags"] == to.BOOTSTRAPPED
    assert all(not (r["flags"] & to.LOST) for r, _ in log[2:]) and min(words[2:]) >= 40


def test_bootstrap_and_its_quirk():
    scn = tc.scenario(tc.sequence(4), 60, 12)
    ref, sub = tc.checker(scn), tc.Subject(scn)
    log = tc.lockstep(scn, ref, [sub], "bootstrap")
    (r1, i1), (r2, i2), (r3, i3) = log[0], log[1], log[2]
    assert r1["flags"] == to.NO_PREVIOUS and i1 is None and len(r1["word_id"]) == 0
    assert r2["flags"] == to.BOOTSTRAPPED
    assert len(i2["discs"]) == 0                      # bootstrapped rows have no count and nothing is blocked: no disc at all
    assert len(r2["new_id"]) > 0 and r2["new_id"].min() > r2["covisible_id"].max()
    assert ref.stats["duplicate_pixels"] >= 1         # a new id sits on a bootstrapped word
    assert (r2["word_count"] == 1).all()
    assert (i3["disc_drawn"] == 0).any()              # the duplicate's second disc is not drawn
    ref.close(); sub.close()


def test_bootstrap_discs_come_only_from_blocked_words():
    scn = tc.blocked_bootstrap()
    ref, sub = tc.checker(scn), tc.Subject(scn)
    log = tc.lockstep(scn, ref, [sub], "blocked bootstrap")
    r, i = log[2]
    n_before = len(log[1][0]["word_id"])
    assert r["flags"] == to.BOOTSTRAPPED and len(r["blocked_id"]) == n_before
    assert len(i["discs"]) == n_before and (i["discs"]["radius"] == 6).all()      # 13 / 2, integer division
    assert r["covisible_id"].min() > log[1][0]["word_id"].max()
    ref.close(); sub.close()


def test_nan_points_of_the_ungated_bootstrap_reach_the_covisible_rows():
    scn = tc.bootstrap_nan()
    ref, sub = tc.checker(scn), tc.Subject(scn)
    log = tc.lockstep(scn, ref, [sub], "bootstrap nan")
    xyz = log[1][0]["covisible_from_xyz"]
    assert np.isnan(xyz).any() and np.isfinite(xyz).any() and ref.stats["nan_covisible"] >= 1
    assert np.isfinite(log[1][0]["word_xyz"]).all()
    ref.close(); sub.close()


@pytest.mark.parametrize("name", sorted(tc.guess_cases()))
def test_guess_equals_the_checker(name):
    scn = tc.guess_cases()[name]
    log, _ = _run(scn, name)
    plain, _ = _run(tc.scenario(scn["frames"], 60, 12), "no guess")
    if name == "translation":                         # the guess is close to the motion: it loses nothing
        assert all(len(a["covisible_id"]) >= len(b["covisible_id"]) - 2 for (a, _), (b, _) in zip(log[1:], plain[1:]))
        i = log[2][1]
        assert np.abs(i["guess_xy"] - i["to_xy"])[i["lk_status"] == 1].max() < 4.0
    if name == "thrown_out":
        i = log[2][1]
        w, h = scn["width"], scn["height"]
        outside = ~(to.in_bounds(i["guess_xy"][:, 0], w) & to.in_bounds(i["guess_xy"][:, 1], h))
        assert outside.any() and not outside.all()
        assert len(log[2][0]["covisible_id"]) < len(plain[2][0]["covisible_id"])


@pytest.mark.parametrize("name", sorted(tc.pretreatment_cases()))
def test_pretreatment_equals_the_checker(name):
    scn = tc.pretreatment_cases()[name]
    log, _ = _run(scn, name)
    if name == "first_middle_last":
        prev, (r, i) = log[1][0], log[2]
        ids = prev["word_id"]
        assert r["blocked_id"].tolist() == [int(ids[0]), int(ids[len(ids) // 2]), int(ids[-1])]
        assert not set(r["blocked_id"].tolist()) & set(r["covisible_id"].tolist())
        assert (i["discs"]["radius"][-3:] == 6).all() and (i["discs"]["radius"][:-3] == 13).all()
    if name == "every_id":
        assert log[3][0]["flags"] == to.BOOTSTRAPPED and len(log[3][0]["blocked_id"]) == len(log[2][0]["word_id"])
        assert log[4][0]["flags"] == 0
    if name == "empty":
        assert all(len(r["blocked_id"]) == 0 for r, _ in log)


def test_full_length_outlier_list_equals_the_checker():
    log, _ = _run(tc.full_outliers(), "4096 outliers")
    assert len(tc.full_outlier_list(log[1][0])) == tracker.MAX_OUTLIERS
    assert log[2][0]["flags"] == 0 and log[2][0]["blocked_id"].tolist() == tc.every_third(log[1][0])


def test_lost_tracking_and_the_bootstrap_behind_it():
    scn = tc.lost_case()
    log, _ = _run(scn, "lost")
    r, i = log[3]
    assert r["flags"] == to.LOST and len(r["word_id"]) == 0 and len(r["covisible_id"]) == 0 and i is not None
    assert log[4][0]["flags"] == to.BOOTSTRAPPED and log[5][0]["flags"] == 0
    assert log[4][0]["covisible_id"].min() >= log[3][0]["next_id"]


def test_min_inliers_at_and_just_above_the_kept_count():
    seq = tc.sequence(4)
    log, _ = _run(tc.scenario(seq, 60, 12, min_inliers=0), "kept count")
    kept = len(log[2][0]["covisible_id"])
    at, _ = _run(tc.scenario(seq, 60, 12, min_inliers=kept), "at")
    above, _ = _run(tc.scenario(seq, 60, 12, min_inliers=kept + 1), "above")
    assert at[2][0]["flags"] == 0 and len(at[2][0]["covisible_id"]) == kept
    assert above[2][0]["flags"] == to.LOST and above[3][0]["flags"] == to.BOOTSTRAPPED


def test_no_top_up_when_every_feature_is_kept():
    scn = tc.no_top_up()
    log, _ = _run(scn, "no top-up")
    full = [k for k, (r, _) in enumerate(log) if len(r["covisible_id"]) == 8]
    assert full, [len(r["covisible_id"]) for r, _ in log]
    for k in full:
        assert len(log[k][0]["new_id"]) == 0 and len(log[k][1]["discs"]) == 0


def test_top_up_that_finds_nothing():
    scn = tc.empty_top_up()
    log, _ = _run(scn, "empty top-up")
    r, i = log[3]
    assert 0 < len(r["covisible_id"]) < 60 and len(r["new_id"]) == 0 and len(i["discs"]) > 0


def test_reset_empties_the_table_and_keeps_the_counter():
    scn = tc.scenario(tc.sequence(4), 60, 12)
    ref, sub = tc.checker(scn), tc.Subject(scn)
    frames = scn["frames"]
    for k in range(3):
        want, _ = ref.process(*frames[k])
        got, _ = sub.process(*frames[k])
        to.assert_same(got, want, f"frame {k}")
    ref.reset(); sub.trk.reset()
    want, _ = ref.process(*frames[3])
    got, _ = sub.process(*frames[3])
    to.assert_same(got, want, "after reset")
    assert got["flags"] == to.BOOTSTRAPPED and got["covisible_id"].min() >= 60
    ref.close(); sub.close()


def test_foreign_push_is_refused():
    scn = tc.scenario(tc.sequence(3), 60, 12)
    sub = tc.Subject(scn)
    sub.process(*scn["frames"][0])
    sub.process(*scn["frames"][1])
    sub.flow.push_frame(*scn["frames"][2])
    rc, _ = sub.trk.process_status(*scn["frames"][2])
    assert rc == abi.ERR_NOT_LOADED and "pushed" in sub.trk.last_error()
    sub.close()


def test_argument_checks():
    f = flow.Flow(flow.default_params(), 320, 240)
    cam = flow.camera()
    assert tracker.create_status(f, cam, tracker.default_params(max_features=0))[0] == abi.ERR_BAD_ARGUMENT
    assert tracker.create_status(f, cam, tracker.default_params(max_features=4097))[0] == abi.ERR_UNSUPPORTED
    assert tracker.create_status(f, cam, tracker.default_params(min_distance=-1))[0] == abi.ERR_BAD_ARGUMENT
    assert tracker.create_status(f, cam, tracker.default_params(quality_level=0.0))[0] == abi.ERR_BAD_ARGUMENT
    assert tracker.create_status(f, None, tracker.default_params())[0] == abi.ERR_BAD_ARGUMENT
    t = tracker.Tracker(f, cam, max_features=4096)
    img = np.zeros((240, 320), dtype=np.uint8)
    assert t.process_status(img, img, outliers=[1], n_outliers=4097)[0] == abi.ERR_BAD_ARGUMENT
    assert t.process_status(img, img, n_outliers=-1)[0] == abi.ERR_BAD_ARGUMENT
    assert t.process_status(None, img)[0] == abi.ERR_BAD_ARGUMENT
    assert t.process_status(img, None)[0] == abi.ERR_BAD_ARGUMENT
    assert t.process_status(img, img, delta_guess=np.full((3, 4), np.nan))[0] == abi.ERR_BAD_ARGUMENT
    with pytest.raises(backend.BackendError):
        t.download()
    rc, out = t.process_status(img, img)
    assert rc == abi.OK and out["flags"] == tracker.NO_PREVIOUS
    rc, out = t.process_status(img, img)                              # a flat image: nothing to extract, so tracking is lost
    assert rc == abi.OK and out["flags"] == tracker.LOST and len(out["word_id"]) == 0
    f.close()                                                         # the flow object goes first: the tracker refuses from then on
    assert t.process_status(img, img)[0] == abi.ERR_NOT_LOADED
    t.close()
