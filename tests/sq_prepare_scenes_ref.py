"""numpy restatement of odam_sq_prepare_scenes (include/odam_sq.h): sq_prepare_ref.prepare_ref per scene, written at the scene's offsets
-- the contract itself, "every word is the word the single-scene entry writes for that scene alone" -- and the scenes the tests of
the many-scene prelude share (tests/test_map_scenes_host.py, tests/test_map_scenes_gpu.py)."""
import numpy as np

import sq_prepare_ref as P

PER_TRACK = ("cls", "n_obs", "n_valid", "status", "init", "half_dims", "pose", "bboxes_dl")
PER_VIEW = ("view_img", "view_row", "valid", "tgt", "mask", "P")


def cap_of(max_rows):
    """rows the launch odam_sq_prepare_batch(max_rows) holds per track: the next power of two, at most 16384"""
    cap = 1
    while cap < max_rows and cap < P.MAX_ROWS:
        cap <<= 1
    return cap


def prepare_scenes_ref(rows, row_off, trk_off, img_names_list, P_cws_list, img_hs, img_ws, representation="super_quadric", thr=20, max_rows=None):
    """max_rows: None = every scene sized from its own longest track (what SqFitter.prepare does with host offsets), or one value for
    all scenes"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    row_off, trk_off = np.asarray(row_off, np.int64), np.asarray(trk_off, np.int64)
    n, R = len(row_off) - 1, len(rows)
    dual = representation == "dual_quadric"
    out = {"cls": np.full(n, -1, np.int32), "n_obs": np.zeros(n, np.int32), "n_valid": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
           "init": np.full((n, 5 if dual else 9), P.FILL_F, np.float32), "half_dims": np.full((n, 3), P.FILL_F, np.float32) if dual else None,
           "pose": np.full((n, 7), P.FILL_F), "bboxes_dl": np.full((n, 8, 3), P.FILL_F),
           "view_img": np.full(R, P.FILL_I, np.int32), "view_row": np.full(R, P.FILL_I, np.int32), "valid": np.full(R, P.FILL_I, np.int32),
           "tgt": np.full((R, 4), P.FILL_F, np.float32), "mask": np.full((R, 4), P.FILL_F, np.float32), "P": np.full((R, 12), P.FILL_F, np.float32)}
    for s in range(len(trk_off) - 1):
        t0, t1 = int(trk_off[s]), int(trk_off[s + 1])
        if t1 == t0:
            continue
        r0, r1 = int(row_off[t0]), int(row_off[t1])
        most = int(np.diff(row_off[t0:t1 + 1]).max()) if max_rows is None else int(max_rows)
        one = P.prepare_ref(rows[r0:r1], row_off[t0:t1 + 1] - r0, img_names_list[s], P_cws_list[s], img_hs[s], img_ws[s], representation, thr,
                            cap=cap_of(max(most, 1)))
        for k in PER_TRACK:
            if one[k] is not None:
                out[k][t0:t1] = one[k]
        for k in PER_VIEW:
            out[k][r0:r1] = one[k]
    return out


def _track(rs, n, ids, w, h, cls, dup=False):
    """n rows on frame ids drawn from `ids`; a quarter of the boxes sit where an edge is a constraint in a 640 x 480 image and none in a
    320 x 256 one"""
    tr = np.zeros((n, 14))
    tr[:, 0] = rs.choice(ids, n, replace=dup or n > len(ids))
    tr[:, 1] = cls
    x0, y0 = rs.uniform(-5, w * 0.5, n), rs.uniform(-5, h * 0.5, n)
    box = np.stack([x0, y0, x0 + rs.uniform(5, w * 0.5, n), y0 + rs.uniform(5, h * 0.5, n)], 1)
    edge = rs.uniform(size=n) < 0.25
    box[edge] = [30.0, 30.0, 310.0, 246.0]      # 310 < 640 - 20 but not < 320 - 20; 246 < 480 - 20 but not < 256 - 20
    tr[:, 2:6] = box
    tr[:, 6:9] = rs.uniform(0.2, 2.0, 3) * rs.uniform(0.8, 1.2, (n, 3))
    tr[:, 9:12] = rs.uniform(-3, 3, 3) + rs.standard_normal((n, 3)) * 0.2
    tr[:, 12] = rs.uniform(-np.pi, np.pi) + rs.uniform(-1, 1, n) * 0.9
    tr[:, 13] = rs.uniform(size=n)
    return tr


def scenes(seed=5):
    """Four scenes, the smallest in which a scene mix-up shows: image counts 7, (5), 40 and 120; image sizes 640 x 480 and 320 x 256; frame
    ids that overlap between the scenes under different projections; an empty scene in the middle; tracks of 1, 33, 100, 300 and 520
    rows; a row whose frame id only another scene's table holds; one track each without a view (all its ids are another scene's), with
    a class that is no integer, and -- under max_rows = 512 -- with too many rows.
    Returns a dict: tracks (list per scene), img_names, P_cws, img_h, img_w (lists per scene), and which track is which."""
    rs = np.random.RandomState(seed)
    names = [list(range(1000, 1007)), list(range(1003, 1008)), rs.permutation(np.arange(1000, 1120, 3)).tolist(),
             rs.permutation(np.arange(1000, 1120)).tolist()]
    sizes = [(480, 640), (480, 640), (256, 320), (480, 640)]      # (img_h, img_w)
    P_cws = [rs.standard_normal((len(n), 3, 4)) for n in names]
    only_3 = [i for i in names[3] if i not in names[0]]          # ids scene 0 does not have
    t0 = [_track(rs, 1, names[0], 640, 480, 3), _track(rs, 33, names[0], 640, 480, 2, dup=True), _track(rs, 6, names[0], 640, 480, 4),
          _track(rs, 4, only_3, 640, 480, 1), _track(rs, 9, names[0], 640, 480, 5, dup=True)]
    t0[2][3, 0] = only_3[0]          # one row of an ordinary track: no view in scene 0, a view in scene 3
    t0[4][2, 1] = 2.5                # a class that is no integer
    t2 = [_track(rs, 100, names[2], 320, 256, 1, dup=True), _track(rs, 70, names[2], 320, 256, 6, dup=True), _track(rs, 5, names[2], 320, 256, 0)]
    t3 = [_track(rs, 300, names[3], 640, 480, 7, dup=True), _track(rs, 33, names[3], 640, 480, 2), _track(rs, 520, names[3], 640, 480, 3, dup=True),
          _track(rs, 64, names[3], 640, 480, 4)]
    return {"tracks": [t0, [], t2, t3], "img_names": names, "P_cws": P_cws, "img_h": [s[0] for s in sizes], "img_w": [s[1] for s in sizes],
            "no_view": 3, "bad_class": 4, "too_many_under_512": 5 + 3 + 2, "foreign_row": (2, 3)}


def pack(sc):
    """-> rows [R, 14], row_off [n + 1], trk_off [S + 1] of the scenes' tracks, scene after scene"""
    flat = [t for ts in sc["tracks"] for t in ts]
    rows, off = P.pack(flat)
    trk = np.zeros(len(sc["tracks"]) + 1, np.int64)
    trk[1:] = np.cumsum([len(ts) for ts in sc["tracks"]])
    return rows, off, trk
