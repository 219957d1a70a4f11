"""The numpy restatement of the IoU tracker kernel (tests/track_iou_ref.py) against the reference-run fixture
tests/golden/iou_tracking.npz (make_golden_tracking.py: the reference's own match_tracks / convert_det_to_list), and its own properties.

What is asked:
  ids, membership   exact.  The fixture's generator asserts that no compared quantity is closer than 1e-9 (`margin`) to what it is
                    compared against, so no rounding difference between the reference's BLAS product for t_wo and the fixed-order sum here
                    can change a decision.
  deciding IoUs     |restatement - reference| <= 4 x the largest such difference the generator observed (`iou_err_observed`, written into
                    iou_tracking.md; the factor covers other BLAS builds), and that bound itself is below 1e-12.
  resumable         a frame loop split at every frame boundary equals the unsplit loop, bit for bit.
  ties              equal scores by descending index: np.argsort(kind="stable") reversed."""
import numpy as np
import pytest

import track_iou_ref as R


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("iou_tracking.npz")
    scenes = R.fixture_scenes(z)
    thr = R.fixture_thresholds(z)
    runs = [R.run(s["blk"], s["cnt"], s["frame_ids"], s["T_wcs"], float(z["img_w"]), float(z["img_h"]), **thr) for s in scenes]
    return z, scenes, thr, runs


def test_fixture_covers_what_it_must(fx):
    z, scenes, thr, _ = fx
    by = {s["name"]: s for s in scenes}
    many, long_, ordered = by["many"], by["long"], by["ordered"]
    assert 64 < many["n_tracks"] < 128 and (many["cnt"] == 30).any() and (many["cnt"] == 0).any() and len(many["cnt"]) <= 150
    gaps = np.diff(many["frame_ids"])
    assert (gaps > thr["max_gap"]).any() and ((gaps > 1) & (gaps <= thr["max_gap"])).any()
    assert np.bincount(long_["members"][:, 0]).max() >= 200
    # the constructed frame: the scan took track 0, the arg-max of the 2D IoU is track 1 and that of the 3D IoU track 2
    assert ordered["ids"][1, 0] == 0 and int(np.argmax(z["ordered_iou2d"])) == 1 and int(np.argmax(z["ordered_iou3d"])) == 2
    assert float(z["margin"]) >= 1e-9
    for s in scenes:      # no score ties
        for f in range(len(s["cnt"])):
            sc = s["blk"][f, :s["cnt"][f], 14]
            assert len(np.unique(sc)) == len(sc)
    # same-place objects of different classes: two tracks started in one frame by detections within 10 cm whose classes differ
    blk, ids = many["blk"], many["ids"]
    found = False
    for f in range(len(many["cnt"])):
        n = many["cnt"][f]
        T = many["T_wcs"][f]
        c = blk[f, :n, 9:12].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        for a in range(n):
            for b in range(a + 1, n):
                if np.abs(c[a] - c[b]).max() < 0.1 and blk[f, a, 1] != blk[f, b, 1] and ids[f, a] >= 0 and ids[f, b] >= 0:
                    found = found or ids[f, a] != ids[f, b]
    assert found


def test_restatement_equals_the_reference_run(fx):
    z, scenes, thr, runs = fx
    bound = 4 * float(z["iou_err_observed"])
    assert 0 < bound <= 1e-12, bound
    for s, (ids, o2, o3, S) in zip(scenes, runs):
        assert np.array_equal(ids, s["ids"]), s["name"]
        assert S.n == s["n_tracks"]
        assert np.array_equal(R.member_rows(ids, s["cnt"]), s["members"]), s["name"]
        assert np.array_equal(o2 == -1, s["iou2d"] == -1) and np.array_equal(o3 == -1, s["iou3d"] == -1)
        e2, e3 = np.abs(o2 - s["iou2d"]).max(), np.abs(o3 - s["iou3d"]).max()
        print("%s: largest |restatement - reference| iou2d %.3g iou3d %.3g (bound %.3g)" % (s["name"], e2, e3, bound))
        assert e2 <= bound and e3 <= bound, (s["name"], e2, e3)
        # the running sums are the track means: np.mean over the members' rows, bit for bit
        for t in (0, S.n // 2, S.n - 1):
            rows = s["members"][s["members"][:, 0] == t]
            vals = [R.detection_values(s["blk"][f, d:d + 1], s["T_wcs"][f], float(z["img_w"]), float(z["img_h"])) for _, f, d in rows]
            dims = np.concatenate([v[1] for v in vals]); tw = np.concatenate([v[2] for v in vals])
            assert np.array_equal(S.sum[:3, t] / len(rows), np.mean(dims, axis=0)) and np.array_equal(S.sum[3:, t] / len(rows), np.mean(tw, axis=0))


def test_split_at_every_frame_boundary(fx):
    z, scenes, thr, runs = fx
    w, h = float(z["img_w"]), float(z["img_h"])
    for name, n in (("many", 24), ("ordered", 4)):
        s = [x for x in scenes if x["name"] == name][0]
        a = [s[k][:n] for k in ("blk", "cnt", "frame_ids", "T_wcs")]
        whole = R.run(*a, w, h, **thr)
        assert whole[3].n > 20 or name == "ordered"
        for cut in range(0, n + 1):
            S = R.State()
            p = R.step(S, a[0][:cut], a[1][:cut], a[2][:cut], a[3][:cut], w, h, **thr)
            q = R.step(S, a[0][cut:], a[1][cut:], a[2][cut:], a[3][cut:], w, h, **thr)
            for k in range(3):
                got = np.concatenate([p[k], q[k]])
                assert got.tobytes() == whole[k].tobytes(), (name, cut, k)
            assert S.n == whole[3].n and S.sum.tobytes() == whole[3].sum.tobytes() and S.lo.tobytes() == whole[3].lo.tobytes()


def test_tie_rule():
    rs = np.random.RandomState(3)
    for trial in range(200):
        n = rs.randint(0, 31)
        sc = rs.choice(np.r_[rs.uniform(0, 1, 6), 0.0, -0.0], n).astype(np.float32).astype(np.float64)
        assert np.array_equal(R.score_order(sc), np.argsort(sc, kind="stable")[::-1]), sc
    sc = np.array([0.5, np.nan, 0.7, np.nan, 0.5])      # a NaN sorts as the largest, as numpy sorts it
    assert R.score_order(sc).tolist() == np.argsort(sc, kind="stable")[::-1].tolist() == [3, 1, 2, 4, 0]


def test_ties_decide_who_scans_first():
    """two detections of one score over one track: the one with the larger index scans first and takes it"""
    T = np.eye(4)[None]
    row = lambda score: np.r_[0, 1, 0.4, 0.4, 0.6, 0.6, 1, 1, 1, 0, 0, 3, 0, 1, score].astype(np.float32)
    S = R.State()
    blk = np.full((1, 30, 15), -1, np.float32); blk[0, 0] = row(0.9)
    ids, _, _ = R.step(S, blk, [1], [0], T, 100, 100)
    assert ids[0, 0] == 0
    blk[0, 0] = row(0.7); blk[0, 1] = row(0.7)
    ids, o2, _ = R.step(S, blk, [2], [1], T, 100, 100)
    assert ids[0, :2].tolist() == [-1, 0] and o2[0, 1] == 1.0 and o2[0, 0] == -1.0


def test_overflow_stops_before_the_frame(fx):
    z, scenes, thr, runs = fx
    s = [x for x in scenes if x["name"] == "many"][0]
    w, h = float(z["img_w"]), float(z["img_h"])
    S = R.State(64)
    with pytest.raises(R.Overflow) as e:
        R.step(S, s["blk"], s["cnt"], s["frame_ids"], s["T_wcs"], w, h, **thr)
    f = e.value.frame
    ids = e.value.partial[0]
    assert 0 < f < len(s["cnt"]) and S.n <= 64
    assert np.array_equal(ids[:f], s["ids"][:f]) and (ids[f:] == -1).all()
    assert s["ids"][:f].max() < 64 <= s["ids"][f].max()
    # the state is as after frame f - 1: the same frames on an unlimited state
    U = R.State()
    R.step(U, s["blk"][:f], s["cnt"][:f], s["frame_ids"][:f], s["T_wcs"][:f], w, h, **thr)
    assert S.n == U.n and S.sum[:, :S.n].tobytes() == U.sum[:, :U.n].tobytes()


def test_nan_iou_never_matches():
    """a degenerate track box (zero volume, zero area) gives 0 / 0: the reference asserts, here it compares false"""
    T = np.eye(4)[None]
    S = R.State()
    blk = np.full((1, 30, 15), -1, np.float32)
    blk[0, 0] = np.r_[0, 1, 0.5, 0.5, 0.5, 0.5, 0, 0, 0, 0, 0, 3, 0, 1, 0.9]
    R.step(S, blk, [1], [0], T, 100, 100)
    ids, o2, o3 = R.step(S, blk, [1], [1], T, 100, 100)
    assert S.n == 2 and ids[0, 0] == 1 and o2[0, 0] == -1 and o3[0, 0] == -1
