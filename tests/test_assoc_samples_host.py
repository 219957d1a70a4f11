"""The validation samples without a GPU: tests/assoc_samples_ref.py (the row-by-row restatement) and odam_amd.assoc_samples (plan +
cut_host, the planned and vectorised path the device store follows) against the reference's own ScanNetTrack.get_by_sequence / collater
run (tests/golden/assoc_samples.npz, made by tests/golden/make_golden_assoc_samples.py); the three planted mistakes against that fixture;
plan() and batches() on hand-made tables; and the argument contract of odam_samples_create / _load / _cut -- every refusal happens before
the library touches a device (dummy non-null pointers are never dereferenced, odam_samples_create is host bookkeeping only)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import assoc_samples_ref as ref  # noqa: E402

FIX, FRAMES, USE_GT, IMG_SIZE, UNMATCHED = ref.load_fixture()
I_LONG, I_BORN, I_CAP = 5, 1, 4      # samples: a track past 100 rows; an object born in the frame; past the cap
ulps = ref.ulps


def fixture_unmatched():
    return UNMATCHED


def check_tensors(tracks, dets, i, what):
    return ref.check_against_fixture(FIX, tracks, dets, i, what)


@pytest.fixture(scope="module")
def restated():
    """tests/assoc_samples_ref.py on the six samples of the fixture, computed once (read only)"""
    un = fixture_unmatched()
    return [ref.sample(FIX["table"], un, f, FIX["T_wcs"][f], IMG_SIZE, use_gt_det=g) for f, g in zip(FRAMES, USE_GT)]


@pytest.fixture(scope="module")
def scene():
    from odam_amd import assoc_samples
    return assoc_samples.SceneTable(FIX["table"], fixture_unmatched(), FIX["T_wcs"], IMG_SIZE, device=None)


def test_fixture_holds_the_cases_it_was_made_for():
    assert (FIX[f"s{I_LONG}_tracks"][0, 0] != -1).all() and (FIX["table"][0, :FRAMES[I_LONG], 0] != -1).sum() > 100
    m = FIX[f"s{I_BORN}_match"]
    n_frame_objs = int((FIX["table"][:, FRAMES[I_BORN], 0] != -1).sum())
    assert ((m[:, 0] == -1) & (m[:, 1] < n_frame_objs)).any()                       # an object first seen in the sampled frame
    assert any(str(f) in fixture_unmatched() for f in FRAMES)
    assert FIX[f"s{I_CAP}_detections"].shape[1] == 30 and len(FIX[f"s{I_CAP}_match"]) == 30
    assert (FIX["table"][:, FRAMES[I_CAP], 0] != -1).sum() + len(fixture_unmatched()[str(FRAMES[I_CAP])]) > 30
    assert sum(USE_GT) == 1 and FIX["table"].shape == (8, 140, 83)


@pytest.mark.parametrize("i", range(6))
def test_restatement_equals_the_reference_discrete(restated, i):
    r = restated[i]
    assert np.array_equal(r["match"], FIX[f"s{i}_match"]) and np.array_equal(r["scores"], FIX[f"s{i}_scores"])
    assert r["global_track_ids"] == FIX[f"s{i}_gids"].tolist()
    assert (r["tracks"].shape[0], r["detections"].shape[1]) == tuple(FIX["collate_valid_list"][i])
    assert r["tracks"].shape == FIX[f"s{i}_tracks"].shape and r["detections"].shape == FIX[f"s{i}_detections"].shape


@pytest.mark.parametrize("i", range(6))
def test_restatement_equals_the_reference_tensors(restated, i):
    check_tensors(restated[i]["tracks"], restated[i]["detections"], i, "restatement")


def test_restated_collate_equals_the_reference_collater(restated):
    col = ref.collate(restated)
    assert [tuple(v) for v in col["valid_list"]] == [tuple(v) for v in FIX["collate_valid_list"]]
    assert ulps(col["detections"], FIX["collate_detections"]).max() <= 1
    assert np.array_equal(col["detections"] == -1, FIX["collate_detections"] == -1)


@pytest.mark.parametrize("mutate,i", [("window_from_start", I_LONG), ("own_box", 0), ("cap_detections_only", I_CAP)])
def test_fixture_sees_the_planted_mistakes(mutate, i):
    f = FRAMES[i]
    m = ref.sample(FIX["table"], fixture_unmatched(), f, FIX["T_wcs"][f], IMG_SIZE, use_gt_det=USE_GT[i], mutate=mutate)
    if mutate == "cap_detections_only":
        assert len(m["match"]) > 30 and not np.array_equal(m["match"], FIX[f"s{i}_match"])
    else:
        assert m["tracks"].shape == FIX[f"s{i}_tracks"].shape and ulps(m["tracks"], FIX[f"s{i}_tracks"]).max() > 1


def test_plan_and_cut_host_equal_the_reference(scene):
    """the library's own host path, sample by sample and as one batch per use_gt_det setting: same discrete outputs, same bounds"""
    from odam_amd import assoc_samples
    plans = [assoc_samples.plan(FIX["table"], fixture_unmatched(), [f], use_gt_det=g)[0] for f, g in zip(FRAMES, USE_GT)]
    for i, p in enumerate(plans):
        assert np.array_equal(p["match"], FIX[f"s{i}_match"]) and np.array_equal(p["scores"], FIX[f"s{i}_scores"])
        assert p["global_track_ids"] == FIX[f"s{i}_gids"].tolist() and p["valid"] == tuple(FIX["collate_valid_list"][i])
    idx = [i for i in range(6) if not USE_GT[i]]
    out = scene.cut_host([FRAMES[i] for i in idx])
    assert sorted(set(out) - {"gt_scores", "scores", "global_track_ids", "frames"}) == sorted(
        ["tracks", "detections", "gt_matches", "gt_masks", "img_names", "track_batch_split", "detection_batch_split", "poses", "valid_list"])
    t0 = 0
    for b, i in enumerate(idx):
        T, n = out["valid_list"][b]
        check_tensors(out["tracks"][t0:t0 + T].numpy(), out["detections"][b, :, :n].numpy(), i, "cut_host")
        assert (out["detections"][b, :, n:] == -1).all()
        t0 += T
    i = USE_GT.index(True)
    one = scene.cut_host([FRAMES[i]], use_gt_det=True)
    check_tensors(one["tracks"].numpy(), one["detections"][0, :, :one["valid_list"][0][1]].numpy(), i, "cut_host")
    # gt_scores: the collater's block matrix (the fixture's is over all six samples in the fixture's order)
    both = [scene.cut_host([f], use_gt_det=g) for f, g in zip(FRAMES, USE_GT)]
    want = FIX["collate_gt_scores"]
    t0 = d0 = 0
    for o in both:
        T, n = o["valid_list"][0]
        assert np.array_equal(o["gt_scores"].numpy(), want[t0:t0 + T, d0:d0 + n])
        t0, d0 = t0 + T, d0 + n
    assert (t0, d0) == want.shape


def test_cut_host_raises_the_reference_assertion(scene):
    from odam_amd import assoc_samples
    table = FIX["table"].copy()
    table[0, FRAMES[2], 79:83] = -1
    bad = assoc_samples.SceneTable(table, fixture_unmatched(), FIX["T_wcs"], IMG_SIZE, device=None)
    with pytest.raises(AssertionError, match="wrong projected bbox"):
        bad.cut_host([FRAMES[2]])
    with pytest.raises(AssertionError, match="wrong projected bbox"):
        ref.sample(table, fixture_unmatched(), FRAMES[2], FIX["T_wcs"][FRAMES[2]], IMG_SIZE)


# ---- plan on hand-made tables ---------------------------------------------------------------------------------------------------
POSE = ref.make_poses(np.random.RandomState(0), 1)[0]


def hand_table(n_obj, n_frames, seen):
    """a table whose valid entries are `seen` [(object, frame), ...]; the values do not matter to plan() beyond columns 0 and 14"""
    t = -np.ones((n_obj, n_frames, 83))
    for o, f in seen:
        t[o, f, :79] = 0.5
        t[o, f, 0], t[o, f, 14] = f, 40 + o
    t[:, :, 79:83] = 10.0
    return t


def test_plan_no_track_before_the_frame_is_not_usable():
    from odam_amd import assoc_samples
    t = hand_table(2, 6, [(0, 2), (1, 2), (0, 4)])
    p = assoc_samples.plan(t, {}, [2])[0]
    assert p["valid"] == (0, 2) and p["match"].tolist() == [[-1, 0], [-1, 1]] and p["scores"].shape == (0, 2)
    s = assoc_samples.SceneTable(t, {"3": [np.zeros(79)]}, np.tile(POSE, (6, 1, 1)), (100, 50), device=None)
    assert s.usable_frames() == [3, 4]               # 0-2: no track; 3: the unmatched row; 4: object 0; 5: no detection
    assert s.usable_frames(use_gt_det=True) == [4]
    p = s.plan([4])[0]
    assert p["track_objs"].tolist() == [0, 1] and p["match"].tolist() == [[0, 0], [1, -1]] and p["global_track_ids"] == [40, 41]
    assert p["row0"].tolist() == [0, 2] and p["k"].tolist() == [1, 1] and p["det_src"].tolist() == [1]


@pytest.mark.parametrize("earlier", [100, 101])
def test_plan_window_at_100_and_101_rows(earlier):
    from odam_amd import assoc_samples
    t = hand_table(2, 130, [(0, f) for f in range(3, 3 + earlier)] + [(1, 0), (1, 120)])
    p = assoc_samples.plan(t, {}, [120])[0]
    assert p["track_objs"].tolist() == [0, 1] and p["k"].tolist() == [100, 1]
    assert p["row0"].tolist() == [earlier - 100, earlier] and p["det_src"].tolist() == [earlier + 1]
    assert assoc_samples.plan(t, {}, [120], n_times=7)[0]["row0"].tolist() == [earlier - 7, earlier]
    r = ref.sample(t, {}, 120, POSE, (100, 50))
    assert (r["tracks"][0, 0] == np.arange(3 + earlier - 100, 3 + earlier)).all()      # image ids of the kept rows: the LAST 100


@pytest.mark.parametrize("n_unm,pairs", [(28, 32), (29, 30)])
def test_plan_cap_at_30_and_31_detections(n_unm, pairs):
    """2 frame objects + 28 unmatched = 30 detections: nothing is cut, 4 tracks + 28 = 32 pairs; + 29 = 31: both lists are cut to 30"""
    from odam_amd import assoc_samples
    t = hand_table(4, 5, [(0, 0), (1, 0), (2, 1), (3, 1), (0, 3), (3, 3)])
    un = {"3": [np.full(79, 0.25)] * n_unm}
    p = assoc_samples.plan(t, un, [3])[0]
    assert p["valid"] == (4, 30) and len(p["match"]) == pairs
    assert p["match"][:4].tolist() == [[0, 0], [1, -1], [2, -1], [3, 1]] and p["match"][4:].tolist() == [[-1, 2 + u] for u in range(pairs - 4)]
    assert p["det_src"][:2].tolist() == [1, 5] and p["det_src"][2:].tolist() == [-(u + 1) for u in range(28)]
    r = ref.sample(t, un, 3, POSE, (100, 50))
    assert np.array_equal(r["match"], p["match"]) and np.array_equal(r["scores"], p["scores"])
    g = assoc_samples.plan(t, un, [3], use_gt_det=True)[0]
    assert g["valid"] == (4, 2) and len(g["match"]) == 4


def test_batches_respect_both_limits():
    from odam_amd import assoc_samples
    rs = np.random.RandomState(3)
    t, un = ref.make_table(rs, 70, 60, p_obs=0.1, last_birth=10)
    s = assoc_samples.SceneTable(t, un, ref.make_poses(rs, 60), (1296, 968), device=None)
    frames = s.usable_frames() * 3
    n_t = dict(zip(frames, s.ix.n_tracks(frames).tolist()))
    for size in (1, 16, 64, 500):
        got = s.batches(frames, size)
        assert [f for b in got for f in b] == frames
        assert all(1 <= len(b) <= min(size, 64) and sum(n_t[f] for f in b) <= 1024 for b in got)
    assert any(sum(n_t[f] for f in b) > 1024 - 70 and len(b) < 64 for b in s.batches(frames, 64))      # the track limit did split


# ---- the argument contract -------------------------------------------------------------------------------------------------------
P = ctypes.c_void_p(16)      # a pointer that only has to be non-null
N = None


@pytest.fixture(scope="module")
def L():
    from odam_amd import _lib
    return _lib.lib()


@pytest.fixture()
def bare_store(L):
    """odam_samples_create alone: a store that was never loaded owns nothing on a device"""
    made = []

    def make(n_obj=3, n_frames=10, n_obs=12, n_unm=4):
        h = ctypes.c_void_p()
        assert L.odam_samples_create(n_obj, n_frames, n_obs, n_unm, ctypes.byref(h)) == 0
        made.append(h)
        return h
    yield make
    for h in made:
        L.odam_samples_destroy(h)


@pytest.mark.parametrize("args,code,fragment", [((0, 10, 5, 0), 3, "n_obj >= 1"), ((3, 0, 5, 0), 3, "n_frames >= 1"), ((3, 10, 0, 0), 3, "n_obs >= 1"),
                                                ((3, 10, 5, -1), 3, "n_unm >= 0"), ((3, 10, 31, 0), 3, "more observations than"),
                                                ((50000, 50000, 2 ** 31, 0), 3, "31 bits")])
def test_create_refuses(L, args, code, fragment):
    h = ctypes.c_void_p()
    assert L.odam_samples_create(*args, ctypes.byref(h)) == code and not h
    err = L.odam_last_error().decode()
    assert err.startswith("odam_samples_create:") and fragment in err, err
    assert L.odam_samples_create(3, 10, 5, 0, N) == 1


def _i64(v):
    return np.ascontiguousarray(v, np.int64)


LOAD_CASES = [
    (dict(obs_off=[1, 4, 8, 12]), "must start at 0"), (dict(unm_off=[1] + [4] * 10), "must start at 0"),
    (dict(obs_off=[0, 5, 4, 12]), "obs_off must not decrease"), (dict(obs_off=[0, 11, 12, 12]), "more rows than the scene has frames"),
    (dict(unm_off=[0, 2, 1] + [4] * 8), "unm_off must not decrease"), (dict(obs_off=[0, 4, 8, 11]), "do not end at the row counts"),
    (dict(unm_off=[0] * 10 + [3]), "do not end at the row counts"), (dict(w=0.0), "image size must be positive"),
    (dict(h=float("nan")), "image size must be positive")]


@pytest.mark.parametrize("change,fragment", LOAD_CASES, ids=[str(i) for i in range(len(LOAD_CASES))])
def test_load_refuses(L, bare_store, change, fragment):
    a = dict(obs_off=[0, 4, 8, 12], unm_off=[0] * 5 + [4] * 6, w=640.0, h=480.0)
    a.update(change)
    oo, uo = _i64(a["obs_off"]), _i64(a["unm_off"])
    assert L.odam_samples_load(bare_store(), P, oo.ctypes.data, P, P, P, uo.ctypes.data, a["w"], a["h"], N) == 1
    err = L.odam_last_error().decode()
    assert err.startswith("odam_samples_load:") and fragment in err, err


def test_load_null_pointers(L, bare_store):
    oo, uo = _i64([0, 4, 8, 12]), _i64([0] * 5 + [4] * 6)
    good = [bare_store(), P, oo.ctypes.data, P, P, P, uo.ctypes.data, 640.0, 480.0, N]
    for i in (0, 1, 2, 3, 4, 5, 6):      # 5: the unmatched rows may be null only when the store has none
        args = list(good)
        args[i] = N
        assert L.odam_samples_load(*args) == 1 and "null pointer" in L.odam_last_error().decode(), i


def cut_args(h, **change):
    a = dict(B=2, frames=[3, 9], n_det=[2, 30], det_src=np.zeros((2, 30), np.int32), sum_t=3, slot_sample=[0, 0, 1], slot_obj=[0, 1, 2],
             slot_row0=[0, 4, 8], slot_k=[2, 1, 4], n_times=100)
    a.update(change)
    arrs = {k: np.ascontiguousarray(a[k], np.int32) for k in ("frames", "n_det", "det_src", "slot_sample", "slot_obj", "slot_row0", "slot_k")}
    args = [h, a["B"], arrs["frames"].ctypes.data, arrs["n_det"].ctypes.data, arrs["det_src"].ctypes.data, a["sum_t"], arrs["slot_sample"].ctypes.data,
            arrs["slot_obj"].ctypes.data, arrs["slot_row0"].ctypes.data, arrs["slot_k"].ctypes.data, a["n_times"], P, P, P, N]
    return args, arrs


def _src(j, v):
    d = np.zeros((2, 30), np.int32)
    d[0, j] = v
    return d


CUT_CASES = [
    (dict(B=0), 3, ["1 <= B <= 64"]), (dict(B=65), 3, ["1 <= B <= 64"]),
    (dict(sum_t=0), 3, ["1 <= sum_t <= 1024"]), (dict(sum_t=1025), 3, ["1 <= sum_t <= 1024"]),
    (dict(n_times=0), 3, ["1 <= n_times <= 128"]), (dict(n_times=129), 3, ["1 <= n_times <= 128"]),
    (dict(n_det=[0, 30]), 3, ["sample 0", "n_det = 0"]), (dict(n_det=[2, 31]), 3, ["sample 1", "n_det = 31", "after the cap"]),
    (dict(slot_k=[2, 0, 4]), 3, ["slot 1 keeps 0 rows"]), (dict(slot_k=[2, 1, 8], n_times=7), 3, ["slot 2 keeps 8 rows", "n_times = 7"]),
    (dict(frames=[3, 10]), 1, ["sample 1 names frame 10", "the scene has 10"]), (dict(frames=[-1, 9]), 1, ["sample 0 names frame -1"]),
    (dict(det_src=_src(1, 12)), 1, ["detection 1 of sample 0", "source 12", "outside the store"]),
    (dict(det_src=_src(0, -5)), 1, ["detection 0 of sample 0", "source -5"]),
    (dict(slot_sample=[0, 2, 1]), 1, ["slot 1 names sample 2"]), (dict(slot_sample=[1, 0, 1]), 1, ["slot 1 names sample 0", "not decreasing"]),
    (dict(slot_row0=[0, 4, 9]), 1, ["slot 2 reads rows 9 .. 13", "outside the store's 12"]), (dict(slot_row0=[-1, 4, 8]), 1, ["slot 0 reads rows -1"]),
    (dict(slot_obj=[0, 3, 2]), 1, ["slot 1 names object 3", "the scene has 3"]), (dict(slot_obj=[-1, 1, 2]), 1, ["slot 0 names object -1"]),
    # everything in order (sources 11 and -4 are the last rows of the store): refused only because nothing was loaded
    (dict(det_src=_src(0, 11) + _src(1, -4)), 1, ["call odam_samples_load first"]),
]


@pytest.mark.parametrize("change,code,fragments", CUT_CASES, ids=[str(i) for i in range(len(CUT_CASES))])
def test_cut_refuses(L, bare_store, change, code, fragments):
    args, keep = cut_args(bare_store(), **change)
    rc = L.odam_samples_cut(*args)
    err = L.odam_last_error().decode()
    assert rc == code, err
    assert err.startswith("odam_samples_cut:"), err
    for f in fragments:
        assert f in err, err


def test_cut_null_pointers(L, bare_store):
    good, keep = cut_args(bare_store())
    for i in (0, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13):
        args = list(good)
        args[i] = N
        assert L.odam_samples_cut(*args) == 1 and "null pointer" in L.odam_last_error().decode(), i
