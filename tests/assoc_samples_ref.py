"""Numpy restatement of the association network's validation samples (likojack/ODAM src/datasets/scan_net_track.py:142-341:
get_by_sequence, _get_match_list, _concat_unmatched, _preprocess_tracks, _preprocess; :34-97 collater) from the DENSE table, object by object
and row by row -- written independently of odam_amd/assoc_samples.py's planned, vectorised path, which the tests hold against it -- with the
arithmetic in the order odam_amd/csrc/assoc_samples.hip uses: t_co = ((x c0 + y c1) + z c2) + c3, float64, rounded to float32 once.
make_table() draws synthetic scene tables.  mutate= plants one of three mistakes (tests/test_assoc_samples_host.py shows that the fixture
sees each):
    "window_from_start"    a track keeps its FIRST n_times rows
    "own_box"              every kept row keeps its own detected box (normalised and clipped) instead of the projected box of the frame
    "cap_detections_only"  past 30 detections only the detections are cut, the pair list stays whole"""
import os

import numpy as np

MAX_DETS = 30
COPIES = [0, 1, 6, 7, 8, 14] + list(range(15, 79))      # channels whose values are copies of table entries


def ulps(a, b):
    """element-wise distance of two float32 arrays in units in the last place (0 for equal bits, and for +0 / -0)"""
    def order(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(order(a) - order(b))


def load_fixture():
    """tests/golden/assoc_samples.npz (the reference's own run) -> (npz, frames, use_gt_det flags, img_size, the unmatched dict)"""
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assoc_samples.npz"))
    unmatched = {}
    for f, row in zip(fix["unm_frames"], fix["unm_rows"]):
        unmatched.setdefault(str(int(f)), []).append(row)
    return fix, [int(f) for f in fix["frames"]], [bool(g) for g in fix["use_gt_det"]], tuple(int(x) for x in fix["img_size"]), unmatched


def check_against_fixture(fix, tracks, dets, i, what):
    """The bound of every test against the fixture's sample i: 1 float32 ulp everywhere, equal bits on the copied channels and on all
    padding.  Derived, not measured: both sides round ONE float64 value to float32; the float64 values differ only by the summation order of
    a three-term dot product and by the last bits of sin / cos, so the float32 results are equal or neighbours.  Returns how many elements
    of the tracks and of the detections differ at all."""
    want_t, want_d = fix[f"s{i}_tracks"], fix[f"s{i}_detections"]
    assert tracks.shape == want_t.shape and dets.shape == want_d.shape and tracks.dtype == dets.dtype == np.float32
    ut, ud = ulps(tracks, want_t), ulps(dets, want_d)
    print(f"{what} sample {i}: tracks differ in {int((ut > 0).sum())} of {ut.size} elements (max {int(ut.max())} ulp), "
          f"detections in {int((ud > 0).sum())} of {ud.size} (max {int(ud.max()) if ud.size else 0} ulp)")
    assert ut.max() <= 1 and (ud.size == 0 or ud.max() <= 1)
    assert np.array_equal(tracks[:, COPIES], want_t[:, COPIES]) and np.array_equal(dets[COPIES], want_d[COPIES])
    pad = np.broadcast_to((want_t[:, 0] == -1)[:, None, :], tracks.shape)      # image id -1 = a padded time step
    assert (tracks[pad] == -1).all()
    return int((ut > 0).sum()), int((ud > 0).sum())


def cam_azi(T_wc):  # scannet_utils.py:213-222
    o = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])
    o = (o @ T_wc.T)[:, :3]
    o = o[0] - o[1]
    o[2] = 0
    o = o / np.linalg.norm(o)
    return np.arctan2(o[1], o[0])


def _row79(row78, box, T_cw, azi):
    """one 78-column row (ground-truth id removed) -> the 79 network channels, float64"""
    out = np.empty(79)
    out[0:2] = row78[0:2]
    out[2:6] = box
    out[6:9] = row78[6:9]
    x, y, z = row78[9:12]
    for i in range(3):
        out[9 + i] = ((x * T_cw[i, 0] + y * T_cw[i, 1]) + z * T_cw[i, 2]) + T_cw[i, 3]
    rel = row78[12] - azi
    out[12], out[13] = np.sin(rel), np.cos(rel)
    out[14] = row78[13]
    out[15:79] = row78[14:78]
    return out


def sample(tracks, unmatched, f, T_wc, img_size, img_name=None, use_gt_det=False, n_times=100, mutate=None):
    """the sample of frame f: {"tracks" [T, 79, n_times] float32, "detections" [79, n] float32, "match" [pairs, 2], "scores" [T, n] float32,
    "global_track_ids"}"""
    tracks = np.asarray(tracks, np.float64)
    n_obj = tracks.shape[0]
    w, h = img_size
    wh = np.array([w, h, w, h], np.float64)
    T_cw = np.linalg.inv(T_wc)
    azi = cam_azi(T_wc)
    drop14 = [c for c in range(79) if c != 14]
    name = str(f if img_name is None else img_name)
    extra = [] if use_gt_det else [np.asarray(r, np.float64)[drop14] for r in unmatched.get(name, [])]
    # tracks: objects with a valid row before f; detections: objects valid in f, then the unmatched rows
    track_ids = [o for o in range(n_obj) if (tracks[o, :f, 0] != -1).any()]
    frame_ids = [o for o in range(n_obj) if tracks[o, f, 0] != -1]
    match = [[i, frame_ids.index(o) if o in frame_ids else -1] for i, o in enumerate(track_ids)]
    match += [[-1, j] for j, o in enumerate(frame_ids) if o not in track_ids]
    match += [[-1, len(frame_ids) + u] for u in range(len(extra))]
    det_rows = [tracks[o, f][drop14] for o in frame_ids] + extra
    if not use_gt_det and len(det_rows) > MAX_DETS:
        det_rows = det_rows[:MAX_DETS]
        if mutate != "cap_detections_only":
            match = match[:MAX_DETS]
    out_tracks = -np.ones((len(track_ids), 79, n_times), np.float32)
    gids = []
    for i, o in enumerate(track_ids):
        rows = tracks[o, :f][tracks[o, :f, 0] != -1]
        gids.append(int(rows[0, 14]))
        pb = tracks[o, f, 79:83]
        assert not (pb == -1).all(), "wrong projected bbox"
        box = np.clip(pb / wh, -1, 2)
        kept = rows[:n_times] if mutate == "window_from_start" else rows[-n_times:]
        for t, r in enumerate(kept):
            b = np.clip(r[2:6] / wh, -1, 2) if mutate == "own_box" else box
            out_tracks[i, :, t] = _row79(r[drop14], b, T_cw, azi).astype(np.float32)
    dets = np.empty((79, len(det_rows)), np.float32)
    for j, r in enumerate(det_rows):
        dets[:, j] = _row79(r, r[2:6] / wh, T_cw, azi).astype(np.float32)
    match = np.asarray(match, np.int64).reshape(-1, 2)
    scores = np.zeros((len(track_ids), len(det_rows)), np.float32)
    for i, j in match:
        if i != -1 and j != -1 and j < len(det_rows):
            scores[i, j] = 1
    return {"tracks": out_tracks, "detections": dets, "match": match, "scores": scores, "global_track_ids": gids}


def collate(samples):
    """the collater's tensors: tracks [sum T, 79, n_times], detections [B, 79, 30] padded with -1, valid_list"""
    det = -np.ones((len(samples), 79, MAX_DETS), np.float32)
    for b, s in enumerate(samples):
        det[b, :, :s["detections"].shape[1]] = s["detections"]
    return {"tracks": np.concatenate([s["tracks"] for s in samples]), "detections": det,
            "valid_list": [(s["tracks"].shape[0], s["detections"].shape[1]) for s in samples]}


def make_poses(rs, n_frames):
    """[n_frames, 4, 4] rigid T_wc: a camera that turns about the upright axis, tilts a little and walks"""
    out = np.zeros((n_frames, 4, 4))
    for f in range(n_frames):
        a, b = 0.05 * f + rs.uniform(-0.1, 0.1), rs.uniform(-0.4, 0.4)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        out[f, :3, :3] = Rz @ Rx @ np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]])
        out[f, :3, 3] = rs.uniform(-3, 3, 3)
        out[f, 3, 3] = 1
    return out


def make_table(rs, n_obj, n_frames, p_obs=0.08, dense=(0,), quiet=4, last_birth=None, unmatched_max=3, forced_unmatched=None,
               img_size=(1296, 968)):
    """A synthetic scene: (tracks [n_obj, n_frames, 83], unmatched {str(frame): [79-vectors]}).  The objects in `dense` are observed in every
    frame from frame 0; every other object is born in a frame of quiet + 1 .. last_birth (birth frames not decreasing with the object index;
    default last_birth: 2/3 of the scene), observed there and afterwards with probability p_obs per frame.  Frames 1 .. quiet hold the dense
    objects alone and no unmatched detection.  Unmatched rows: 0 .. unmatched_max per frame, or forced_unmatched[frame] of them.  A projected
    box is drawn for every (object, frame) from the object's birth on, partly outside the image (the clip at -1 and 2 is reached)."""
    w, h = img_size
    last_birth = (2 * n_frames) // 3 if last_birth is None else last_birth
    births = np.sort(rs.randint(quiet + 1, max(quiet + 2, last_birth + 1), n_obj))
    births[list(dense)] = 0
    t = -np.ones((n_obj, n_frames, 83))
    for o in range(n_obj):
        for f in range(births[o], n_frames):
            t[o, f, 79:81] = rs.uniform(-1.5, 1.5, 2) * (w, h)
            t[o, f, 81:83] = t[o, f, 79:81] + rs.uniform(0.01, 1.2, 2) * (w, h)
            seen = o in dense or f == births[o] or (f > quiet and rs.rand() < p_obs)
            if not seen:
                continue
            x0, y0 = rs.uniform(0, 0.8 * w), rs.uniform(0, 0.8 * h)
            t[o, f, 0] = f
            t[o, f, 1] = o % 8
            t[o, f, 2:6] = (x0, y0, x0 + rs.uniform(5, 0.2 * w), y0 + rs.uniform(5, 0.2 * h))
            t[o, f, 6:9] = rs.uniform(0.2, 2.0, 3)
            t[o, f, 9:12] = rs.uniform(-4, 4, 3)
            t[o, f, 12] = rs.uniform(-np.pi, np.pi)
            t[o, f, 13] = rs.uniform(0.3, 1.0)
            t[o, f, 14] = 100 + o
            t[o, f, 15:79] = rs.randn(64)
    unmatched = {}
    forced = forced_unmatched or {}
    for f in range(n_frames):
        n = forced.get(f, 0 if f <= quiet else int(rs.randint(0, unmatched_max + 1)))
        rows = []
        for _ in range(n):
            r = np.empty(79)
            x0, y0 = rs.uniform(0, 0.8 * w), rs.uniform(0, 0.8 * h)
            r[0], r[1] = f, rs.randint(0, 8)
            r[2:6] = (x0, y0, x0 + rs.uniform(5, 0.2 * w), y0 + rs.uniform(5, 0.2 * h))
            r[6:9] = rs.uniform(0.2, 2.0, 3)
            r[9:12] = rs.uniform(-4, 4, 3)
            r[12], r[13], r[14] = rs.uniform(-np.pi, np.pi), rs.uniform(0.3, 1.0), -1
            r[15:79] = rs.randn(64)
            rows.append(r)
        if rows:
            unmatched[str(f)] = rows
    return t, unmatched
