"""Golden for the IoU tracker: the reference's own match_tracks and convert_det_to_list (src/scripts/run_tracking.py:106-170, :37-52,
imported here) with init_tracks' rule without its ORB / depth side data (:65-75, :100-103) over synthetic posed scenes.  Writes
iou_tracking.npz + iou_tracking.md.

Detections are generated as float32 rows in this project's layout (parallel.pack_detections: frame id, class, normalised box, dims,
camera-frame centre, sin, cos, score); the `bboxes` handed to the reference are the float64 pixel values OdamProcess._track_rows forms
from them, everything else the float32 values widened -- both sides start from the same numbers.

Scenes:
  many      150 frames, non-contiguous frame ids (gaps 1 .. 12), up to 30 detections per frame (some frames exactly 30, some none),
            ~100 objects of which some share place and size with an object of another class; ends with 65 < tracks < 128
  long      210 frames, three objects, one of them seen in every frame: a track of >= 200 observations (the running mean)
  ordered   constructed: a detection whose ordered both-maxima scan picks track 0 while the arg-max of the 2D IoU is track 1 and the
            arg-max of the 3D IoU is track 2; then the same detection after a gap > 5, decided by the 3D-only branch

What is recorded per scene: inputs, per detection slot the track id and the deciding (max_iou_2d, max_iou_3d) as the reference's scan
left them (its box_utils.iou_2d / iou_3d calls are logged and the scan's decisions replayed from the logged values; the replay is
asserted to make the attachments match_tracks made), and the final track membership.

The margin: the smallest distance of any compared quantity from what it is compared against, over every comparison that could change
an outcome -- asserted >= 1e-9 and written to the .md.  t_wo comes from a BLAS product there and from a fixed-order sum in this
project; with this margin no such rounding difference can change a decision, so ids are demanded exactly.

Run: python tests/golden/make_golden_tracking.py"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

IMG_W, IMG_H = 1296, 968
MATCH_T, TRACK_T, IOU3_T, GAP = 0.5, 0.8, 0.2, 5
MIN_MARGIN = 1e-9


def rot(yaw, tilt):
    cz, sz, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])


def poses(rs, n):
    T = np.tile(np.eye(4), (n, 1, 1))
    t = np.cumsum(rs.normal(0, 0.05, (n, 3)), axis=0) + [3.0, 3.0, 1.5]
    yaw = np.cumsum(rs.normal(0, 0.04, n)) + 0.3
    for f in range(n):
        T[f, :3, :3] = rot(yaw[f], -1.2 + 0.1 * np.sin(f / 9.0))
        T[f, :3, 3] = t[f]
    return T


def det_row(rs, fid, cls, box, dims, centre_w, T_wc, score):
    t_co = T_wc[:3, :3].T @ (np.asarray(centre_w) - T_wc[:3, 3])
    a = rs.uniform(-np.pi, np.pi)
    return np.r_[fid, cls, box, dims, t_co, np.sin(a), np.cos(a), score].astype(np.float32)


def pack(frames):
    """list (per frame) of lists of float32 rows -> blk [N, 30, 15], cnt [N]"""
    blk = np.full((len(frames), 30, 15), -1.0, np.float32)
    cnt = np.zeros(len(frames), np.int32)
    for f, rows in enumerate(frames):
        assert len(rows) <= 30
        cnt[f] = len(rows)
        if rows:
            blk[f, :len(rows)] = np.asarray(rows, np.float32)
    return blk, cnt


def distinct_scores(rs, n):
    while True:
        s = rs.uniform(0.55, 1.0, n).astype(np.float32)
        if len(np.unique(s)) == n and np.abs(s.astype(np.float64) - TRACK_T).min(initial=1.0) > 1e-6:
            return s


def scene_many(rs):
    n_base, n_twin, N = 88, 10, 150
    gx, gy = np.meshgrid(np.arange(11), np.arange(8))
    centre = np.stack([gx.reshape(-1) * 1.5, gy.reshape(-1) * 1.5, np.zeros(88)], axis=1) + rs.uniform(-0.2, 0.2, (88, 3)) * [1, 1, 2]
    dims = rs.uniform(0.45, 1.1, (n_base, 3))
    cls = rs.randint(0, 8, n_base)
    bc = rs.uniform(0.15, 0.85, (n_base, 2)); bh = rs.uniform(0.05, 0.15, (n_base, 2))
    edge = rs.choice(n_base, 12, replace=False)          # boxes that reach over the image border: the clip
    bc[edge[:6]] = rs.uniform(0.0, 0.04, (6, 2)); bc[edge[6:]] = rs.uniform(0.96, 1.0, (6, 2)); bh[edge] = rs.uniform(0.1, 0.15, (12, 2))
    twins = rs.choice(n_base, n_twin, replace=False)     # same place, same size, same box, another class
    centre = np.concatenate([centre, centre[twins]]); dims = np.concatenate([dims, dims[twins]])
    cls = np.concatenate([cls, (cls[twins] + 1 + rs.randint(0, 6, n_twin)) % 8])
    bc = np.concatenate([bc, bc[twins]]); bh = np.concatenate([bh, bh[twins]])
    n_obj = n_base + n_twin
    phase = rs.uniform(0, 6.28, n_obj)
    start = rs.randint(0, 115, n_obj)
    frame_ids = np.cumsum(rs.choice([1, 1, 1, 1, 2, 3, 4, 5, 6, 8, 12], N)).astype(np.int64)
    T = poses(rs, N)
    frames = []
    for f in range(N):
        inside = (f >= start) & (f < start + 55)
        vis = np.flatnonzero((inside & (rs.uniform(size=n_obj) < 0.5)) | (~inside & (f >= start) & (rs.uniform(size=n_obj) < 0.04)))
        if f in (10, 50, 90, 120):       # exactly 30
            rest = np.setdiff1d(np.arange(n_obj), vis)
            vis = np.concatenate([vis, rs.choice(rest, max(0, 30 - len(vis)), replace=False)])
        if f in (5, 6, 77):
            vis = vis[:0]
        vis = rs.permutation(vis)[:30]
        sc = distinct_scores(rs, len(vis))
        rows = []
        for k, o in enumerate(vis):
            c2 = bc[o] + 0.05 * np.sin(f / 15.0 + phase[o]) + rs.normal(0, 0.006, 2)
            h2 = bh[o] * (1 + rs.normal(0, 0.03, 2))
            rows.append(det_row(rs, frame_ids[f], cls[o], np.r_[c2 - h2, c2 + h2], dims[o] * (1 + rs.normal(0, 0.02, 3)),
                                centre[o] + rs.normal(0, 0.02, 3), T[f], sc[k]))
        frames.append(rows)
    blk, cnt = pack(frames)
    assert (cnt == 30).sum() >= 3 and (cnt == 0).sum() >= 3
    return blk, cnt, frame_ids, T


def scene_long(rs):
    N = 210
    centre = np.array([[0.0, 0, 0], [2.5, 0.3, 0], [0.4, 2.6, 0.2]]); dims = rs.uniform(0.5, 1.0, (3, 3)); cls = [3, 3, 5]
    bc = np.array([[0.3, 0.4], [0.7, 0.5], [0.5, 0.8]]); bh = rs.uniform(0.08, 0.12, (3, 2))
    frame_ids = np.arange(N).astype(np.int64) + 100
    T = poses(rs, N)
    frames = []
    for f in range(N):
        vis = [0] + [o for o in (1, 2) if rs.uniform() < 0.4]
        sc = distinct_scores(rs, len(vis))
        if f == 0:
            sc[0] = np.float32(0.93)
        rows = [det_row(rs, frame_ids[f], cls[o], np.r_[bc[o] - bh[o], bc[o] + bh[o]] + rs.normal(0, 0.004, 4),
                        dims[o] * (1 + rs.normal(0, 0.02, 3)), centre[o] + rs.normal(0, 0.02, 3), T[f], sc[k]) for k, o in enumerate(vis)]
        frames.append([rows[i] for i in rs.permutation(len(rows))])
    blk, cnt = pack(frames)
    return blk, cnt, frame_ids, T


def scene_ordered(rs):
    """frame 0 starts tracks 0, 1, 2 (one class); frame 1 has one detection D with
         track 0: iou_2d 0.60, iou_3d 0.30      track 1: iou_2d 0.70, iou_3d 0.25      track 2: iou_2d 0.55, iou_3d 0.50
    (unit cubes and 0.2 x 0.2 boxes shifted along one axis by s: IoU = (1 - s) / (1 + s)).  The scan takes track 0, refuses track 1
    (3D IoU not above 0.30) and track 2 (2D IoU not above 0.60).  Frame id 20 repeats D: every track is stale, the 3D-only branch decides."""
    sh = lambda iou: (1 - iou) / (1 + iou)
    T = poses(rs, 4)
    frame_ids = np.array([0, 1, 2, 20], np.int64)
    one = np.ones(3)
    box = lambda dx: np.r_[0.4 + dx, 0.4, 0.6 + dx, 0.6]
    f0 = [det_row(rs, 0, 2, box(0.2 * sh(0.60)), one, [sh(0.30), 0, 0], T[0], 0.95),
          det_row(rs, 0, 2, box(-0.2 * sh(0.70)), one, [-sh(0.25), 0, 0], T[0], 0.90),
          det_row(rs, 0, 2, box(0.2 * sh(0.55)), one, [0, sh(0.50), 0], T[0], 0.85)]
    D = lambda f: det_row(rs, frame_ids[f], 2, box(0.0), one, [0, 0, 0], T[f], 0.7)
    blk, cnt = pack([f0, [D(1)], [], [D(3)]])
    return blk, cnt, frame_ids, T


def run_reference(rt, bu, blk, cnt, frame_ids, T_wcs):
    """the reference's frame loop (run_tracking.py:279-321 with match_tracks in place of match_tracks_feature and the ORB-free
    init rule) -> ids, deciding IoUs, membership, margins, per-detection IoU rows of the replay"""
    log = []
    orig2, orig3 = bu.iou_2d, bu.iou_3d

    def gap_margin(a, b):
        """how far two disjoint boxes are from touching: the largest separation over the axes (0 when they overlap)"""
        ext = np.minimum(a[1], b[1]) - np.maximum(a[0], b[0])
        return float(np.max(-ext))

    def rec2(a, b):
        v = orig2(a, b); log.append(("2", float(v), gap_margin(a, b))); return v

    def rec3(a, b):
        v = orig3(a, b); log.append(("3", float(v), gap_margin(a, b))); return v
    rt.box_utils = types.SimpleNamespace(iou_2d=rec2, iou_3d=rec3)
    N = len(cnt)
    ids = np.full((N, 30), -1, np.int32); o2 = np.full((N, 30), -1.0); o3 = np.full((N, 30), -1.0)
    tracks, members = [], []
    margin = {"iou_vs_threshold": np.inf, "iou_vs_running_max": np.inf, "disjoint_boxes_vs_touching": np.inf, "score_vs_track_threshold": np.inf,
              "gap_vs_5": np.inf}
    decided = {"recent": 0, "stale": 0}
    scans = {}
    try:
        for f in range(N):
            n = int(cnt[f])
            if n == 0:
                continue            # `if not out_objects: continue`
            rows = blk[f, :n]
            fid = int(frame_ids[f])
            r64 = rows.astype(np.float64)
            px = r64[:, 2:6] * np.array([[IMG_W, IMG_H, IMG_W, IMG_H]])          # OdamProcess._track_rows
            det = {"classes": rows[:, 1].astype(np.int64), "bboxes": px.reshape(n, 2, 2).copy(), "dimensions": r64[:, 6:9].copy(),
                   "translates": r64[:, 9:12].copy(), "angles": np.degrees(np.arctan2(r64[:, 12], r64[:, 13])), "scores": r64[:, 14].copy()}
            assert len(np.unique(det["scores"])) == n, "score tie"
            n_before = len(tracks)
            last_fid = [tr[-1][0] for tr in tracks]; tcls = [tr[-1][1] for tr in tracks]; length = [len(tr) for tr in tracks]
            used = []
            del log[:]
            rt.match_tracks(tracks, det, fid, used, [], IMG_H, IMG_W, T_wcs[f], MATCH_T)
            # ---- replay of the scan's decisions from the logged IoUs
            calls = list(log)
            used_tracks = []
            for d in np.argsort(det["scores"])[::-1]:
                m2, m3, best, last_branch = -1, -1, -1, None
                row2, row3 = np.full(n_before, np.nan), np.full(n_before, np.nan)
                for t in range(n_before):
                    if t in used_tracks:
                        continue
                    k, v3, g3 = calls.pop(0); assert k == "3"
                    row3[t] = v3
                    gap = fid - last_fid[t]
                    margin["gap_vs_5"] = min(margin["gap_vs_5"], abs(gap - (GAP + 0.5)))
                    same = tcls[t] == det["classes"][d]
                    if v3 == 0:
                        margin["disjoint_boxes_vs_touching"] = min(margin["disjoint_boxes_vs_touching"], g3)
                    if not gap > GAP:
                        k, v2, g2 = calls.pop(0); assert k == "2"
                        row2[t] = v2
                        if v2 == 0:
                            margin["disjoint_boxes_vs_touching"] = min(margin["disjoint_boxes_vs_touching"], g2)
                        a, b = v2 > m2, v3 > m3
                        if same:
                            e2 = np.inf if (v2 == 0 and m2 == 0) else abs(v2 - m2)      # two exact zeros: disjoint on both sides, see above
                            e3 = np.inf if (v3 == 0 and m3 == 0) else abs(v3 - m3)
                            m = min(e2, e3) if (a and b) else (e3 if a else (e2 if b else max(e2, e3)))
                            margin["iou_vs_running_max"] = min(margin["iou_vs_running_max"], m)
                        if a and b and same:
                            m2, m3, best, last_branch = v2, v3, t, "recent"
                    else:
                        if same:
                            e3 = np.inf if (v3 == 0 and m3 == 0) else abs(v3 - m3)
                            margin["iou_vs_running_max"] = min(margin["iou_vs_running_max"], e3)
                        if v3 > m3 and same:
                            m3, best, last_branch = v3, t, "stale"
                a, b = m2 > MATCH_T, m3 > IOU3_T
                e2, e3 = abs(m2 - MATCH_T), abs(m3 - IOU3_T)
                margin["iou_vs_threshold"] = min(margin["iou_vs_threshold"], max(e2, e3) if (a and b) else (e2 if a else (e3 if b else min(e2, e3))))
                o2[f, d], o3[f, d] = m2, m3
                scans[(f, int(d))] = (row2, row3)
                if a or b:
                    assert best != -1
                    ids[f, d] = best
                    used_tracks.append(best)
                    decided[last_branch] += 1
            assert not calls, "the replay did not consume every logged IoU"
            assert sorted(used) == sorted(int(d) for d in np.flatnonzero(ids[f] >= 0)), "the replay attached other detections than match_tracks"
            for d in used:           # ... and to the tracks match_tracks chose
                t = ids[f, d]
                assert len(tracks[t]) == length[t] + 1 and tracks[t][-1][-1] == t and tracks[t][-1][13] == det["scores"][d]
                members.append((t, f, d))
            # ---- init_tracks without the ORB / depth side data (run_tracking.py:65-75, :100-103)
            current_track_id = len(tracks)
            for det_id in range(n):
                if det_id in used:
                    continue
                margin["score_vs_track_threshold"] = min(margin["score_vs_track_threshold"], abs(det["scores"][det_id] - TRACK_T))
                if det["scores"][det_id] < TRACK_T:
                    continue
                obj = rt.convert_det_to_list(det, det_id, fid, IMG_H, IMG_W, T_wcs[f])
                obj[-1] = current_track_id
                tracks.append([obj])
                ids[f, det_id] = current_track_id
                members.append((current_track_id, f, det_id))
                current_track_id += 1
    finally:
        rt.box_utils = bu
    members = np.asarray(sorted(members), np.int32).reshape(-1, 3)
    assert [len(t) for t in tracks] == np.bincount(members[:, 0], minlength=len(tracks)).tolist()
    return {"ids": ids, "iou2d": o2, "iou3d": o3, "members": members, "n_tracks": len(tracks), "margin": margin, "decided": decided,
            "scans": scans, "longest": max(len(t) for t in tracks)}


def main():
    import refenv
    refenv._install_stubs()
    sys.path.insert(0, refenv.REF)
    os.chdir(refenv.REF)
    import src.scripts.run_tracking as rt
    import src.utils.box_utils as bu
    import track_iou_ref as R
    rs = np.random.RandomState(20)
    names = ["many", "long", "ordered"]
    scenes = [scene_many(rs), scene_long(rs), scene_ordered(rs)]
    out = {"names": np.array(names), "img_w": IMG_W, "img_h": IMG_H, "match_threshold": MATCH_T, "track_threshold": TRACK_T,
           "iou3d_threshold": IOU3_T, "max_gap": GAP}
    margin, worst, lines = {}, 0.0, []
    for k, (name, (blk, cnt, frame_ids, T)) in enumerate(zip(names, scenes)):
        ref = run_reference(rt, bu, blk, cnt, frame_ids, T)
        ids, r2, r3, _ = R.run(blk, cnt, frame_ids, T, IMG_W, IMG_H)
        assert np.array_equal(ids, ref["ids"]), name
        upd = (ref["iou2d"] != -1) | (ref["iou3d"] != -1)
        assert np.array_equal(r2 == -1, ref["iou2d"] == -1) and np.array_equal(r3 == -1, ref["iou3d"] == -1)
        err = max(np.abs(r2 - ref["iou2d"]).max(), np.abs(r3 - ref["iou3d"]).max())
        worst = max(worst, float(err))
        for key, v in ref["margin"].items():
            margin[key] = min(margin.get(key, np.inf), v)
        gaps = np.diff(frame_ids)
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %d / %d | %.3g |" % (
            name, len(cnt), int(cnt.sum()), int(cnt.max()), int((cnt == 0).sum()), ref["n_tracks"], ref["longest"], ref["decided"]["recent"],
            ref["decided"]["stale"], err))
        if name == "many":
            assert 64 < ref["n_tracks"] < 128, ref["n_tracks"]
            assert (gaps > GAP).any() and ((gaps > 1) & (gaps <= GAP)).any() and ref["decided"]["recent"] > 0 and ref["decided"]["stale"] > 0
            assert (ref["members"][:, 0] >= 64).sum() > 20      # tracks of the second lane chunk take detections
        if name == "long":
            assert ref["longest"] >= 200, ref["longest"]
        if name == "ordered":
            row2, row3 = ref["scans"][(1, 0)]
            assert ref["ids"][1, 0] == 0 and int(np.argmax(row2)) == 1 and int(np.argmax(row3)) == 2, (row2, row3)
            assert ref["ids"][3, 0] == 0 and ref["iou2d"][3, 0] == -1 and ref["iou3d"][3, 0] > IOU3_T
            out["ordered_iou2d"], out["ordered_iou3d"] = row2, row3
        p = "s%d_" % k
        out.update({p + "blk": blk, p + "cnt": cnt, p + "frame_ids": frame_ids.astype(np.int32), p + "T_wcs": T, p + "ids": ref["ids"],
                    p + "iou2d": ref["iou2d"], p + "iou3d": ref["iou3d"], p + "members": ref["members"], p + "n_tracks": ref["n_tracks"],
                    p + "compared": upd})
    smallest = min(margin.values())
    assert smallest >= MIN_MARGIN, margin
    out["margin"] = smallest
    out["iou_err_observed"] = worst
    np.savez_compressed(os.path.join(HERE, "iou_tracking.npz"), **out)
    with open(os.path.join(HERE, "iou_tracking.md"), "w") as f:
        f.write("# iou_tracking.npz\n\nWritten by make_golden_tracking.py: the reference's match_tracks / convert_det_to_list (run_tracking.py) with the\n"
                "ORB-free init rule over three synthetic posed scenes; thresholds %.1f / %.1f / %.1f, gap %d, image %d x %d.\n\n"
                % (MATCH_T, TRACK_T, IOU3_T, GAP, IMG_W, IMG_H))
        f.write("| scene | frames | detections | most per frame | empty frames | tracks | longest track | attached by the recent / the 3D-only branch | "
                "largest abs(restatement - reference) of a deciding IoU |\n|---|---|---|---|---|---|---|---|---|\n" + "\n".join(lines) + "\n\n")
        f.write("Ids and track membership of tests/track_iou_ref.py equal the reference's on every scene.\n\n")
        f.write("Largest |restatement - reference| of a deciding IoU over all scenes: %.3g (`iou_err_observed`; the host test allows 4 x this).\n\n" % worst)
        f.write("Smallest distance of a compared quantity from what it is compared against, over every comparison that could change an\noutcome "
                "(`margin`): %.3g.  By kind:\n\n" % smallest)
        for key, v in margin.items():
            f.write("* %s: %.3g\n" % (key.replace("_", " "), v))
        f.write("\nTwo IoUs that are both exactly 0 (boxes disjoint on both sides) are an exact tie everywhere and are not counted under the running\n"
                "maximum; how far such boxes are from touching is counted instead.  A frame-id gap is an integer: its distance is taken from 5.5.\n"
                "No two detections of a frame have the same score.\n")
    print("iou tracking golden: margin %.3g, restatement vs reference %.3g" % (smallest, worst))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
