"""numpy restatement of odam_sq_prepare_batch (include/odam_sq.h): the prelude of a fit pass per track, with the closed-form yaw
(DESIGN 6l).  tests/test_sq_prepare_host.py holds it against the host path of multi_view.optim_process, tests/test_sq_prepare_gpu.py
holds the kernel against it.

Per-view outputs are [R]-row arrays; words no view owns keep FILL_I / FILL_F, so a test that fills its device buffers with the same
values compares whole buffers and checks "untouched beyond a track's views" with the same assertion.  The same goes for the
per-track rows a non-zero status leaves unwritten."""
import math

import numpy as np

from odam_amd import multi_view, sq

MAX_ROWS = 16384
NO_VIEW, BAD_CLASS, TOO_MANY_ROWS = 1, 2, 3
FILL_I = -7
FILL_F = float("nan")
# the largest gap between this restatement and the scipy path (Rotation.mean's eigenvector, as_euler, get_3d_box of its matrix) over the
# 420 tracks of tests/test_sq_prepare_host.py, which measures it again on every run, prints it and fails if it has grown: 8.882e-16
# rad for the yaw (two units in the last place of pi) and 8.882e-16 for a corner of bboxes_dl.  The GPU test allows 16 times as much.
YAW_GAP = 2.0 ** -50
BOX_GAP = 2.0 ** -50


def seq_sum(x):
    """sum over axis 0, one row after the other, starting with the first (cumsum is sequential by definition)"""
    return np.cumsum(np.asarray(x, np.float64), axis=0)[-1]


def frame_tables(img_names):
    names = np.asarray([int(f) for f in img_names], np.int64)
    order = np.argsort(names, kind="stable")
    return names[order], order.astype(np.int32)


def track_views(track, ids, order):
    """(image index, row) of the views of one track: rows whose truncated frame id is in ids, lowest row of an id, image order"""
    f = np.asarray(track[:, 0], np.float64)
    ok = (f > -2147483649.0) & (f < 2147483648.0)
    i = np.flatnonzero(ok)
    fid = np.trunc(f[i]).astype(np.int64)
    pos = np.minimum(np.searchsorted(ids, fid), len(ids) - 1)
    hit = ids[pos] == fid
    img = order[pos[hit]].astype(np.int64)
    i = i[hit]
    inside = (img >= 0) & (img < len(ids))
    keys = np.sort((img[inside] << 32) | i[inside])
    img, i = keys >> 32, keys & 0xffffffff
    first = np.ones(len(keys), bool)
    first[1:] = img[1:] != img[:-1]
    return img[first], i[first]


def prepare_ref(rows, row_off, img_names, P_cws, img_h, img_w, representation="super_quadric", thr=20, cap=MAX_ROWS):
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    row_off = np.asarray(row_off, np.int64)
    n, R = len(row_off) - 1, len(rows)
    P_cws = np.asarray(P_cws, np.float64).reshape(-1, 12)
    ids, order = frame_tables(img_names)
    dual = representation == "dual_quadric"
    out = {"cls": np.full(n, -1, np.int32), "n_obs": np.zeros(n, np.int32), "n_valid": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
           "init": np.full((n, 5 if dual else 9), FILL_F, np.float32), "half_dims": np.full((n, 3), FILL_F, np.float32) if dual else None,
           "pose": np.full((n, 7), FILL_F), "bboxes_dl": np.full((n, 8, 3), FILL_F),
           "view_img": np.full(R, FILL_I, np.int32), "view_row": np.full(R, FILL_I, np.int32), "valid": np.full(R, FILL_I, np.int32),
           "tgt": np.full((R, 4), FILL_F, np.float32), "mask": np.full((R, 4), FILL_F, np.float32), "P": np.full((R, 12), FILL_F, np.float32)}
    lims = np.array([img_w, img_w, img_h, img_h], np.float64)
    for o in range(n):
        r0, r1 = int(row_off[o]), int(row_off[o + 1])
        if r1 - r0 > cap:      # from the offsets alone
            out["status"][o] = TOO_MANY_ROWS
            continue
        if r1 - r0 <= 0:
            out["status"][o] = NO_VIEW
            continue
        tr = rows[r0:r1]
        c = tr[:, 1]
        bad = not bool(np.all((c >= 0) & (c <= 63) & (c == np.floor(c))))
        if not bad:
            out["cls"][o] = int(np.median(c))
        img, i = track_views(tr, ids, order)
        k = len(img)
        if k == 0:
            out["status"][o] = NO_VIEW
            continue
        out["status"][o] = BAD_CLASS if bad else 0
        sub = tr[i]
        vals = sub[:, [2, 4, 3, 5]]
        m = (vals > thr) & (vals < lims - thr)
        g = slice(r0, r0 + k)
        out["n_obs"][o] = k
        out["n_valid"][o] = int(m.any(axis=1).sum())
        out["view_img"][g], out["view_row"][g], out["valid"][g] = img, i, m.any(axis=1)
        out["mask"][g] = m
        out["tgt"][g] = np.where(m, vals.astype(np.float32), np.float32(0))
        out["P"][g] = P_cws[img].astype(np.float32)
        t_wo = seq_sum(tr[:, 9:12]) / (r1 - r0)
        trans = seq_sum(np.repeat(t_wo[None], k, axis=0)) / k
        scales = seq_sum(sub[:, 6:9]) / k
        yaw = math.atan2(np.sum(np.sin(sub[:, 12])), np.sum(np.cos(sub[:, 12])))
        out["pose"][o] = np.concatenate([trans, [yaw], scales])
        if dual:
            out["init"][o], out["half_dims"][o] = sq.init_dual(trans, yaw, scales)
        else:
            out["init"][o] = sq.init_params(trans, yaw, scales, representation)
        out["bboxes_dl"][o] = multi_view.get_3d_box(scales, multi_view.rotz(yaw), trans)
    return out


def random_tracks(seed, n_tracks, n_img=120, max_rows=300, img_h=480, img_w=640, thr=20, sizes=None):
    """synthetic tracks with everything the prelude branches on: duplicate and absent frame ids, rows out of image order, edges near,
    on and beyond the border band, unsorted image ids.  The yaws of a track lie within +-w of a centre, w <= 1.2 rad, so the
    resultant length of any of its views is at least cos(1.2) = 0.36 (the host test asserts >= 0.1)."""
    rs = np.random.RandomState(seed)
    img_names = rs.permutation(np.arange(1000, 1000 + 3 * n_img, 3))[:n_img].tolist()
    P_cws = rs.standard_normal((n_img, 3, 4))
    tracks = []
    for t in range(n_tracks):
        n = int(rs.randint(1, max_rows + 1)) if t % 7 else int(rs.randint(1, 4))
        if sizes is not None:
            n = int(sizes[t])
        tr = np.zeros((n, 14))
        pool = np.asarray(img_names)
        f = rs.choice(pool, n, replace=n > len(pool) or bool(t % 3 == 0))      # duplicates in a third of the tracks
        gone = rs.uniform(size=n) < 0.1
        gone[rs.randint(n)] = False                                            # at least one row is a view
        f = np.where(gone, f + 1, f)                                           # ids between the images' ids: absent
        if t % 2:
            f = np.sort(f)
        tr[:, 0] = f + (rs.uniform(0, 0.9, n) if t % 5 == 0 else 0)            # the id is the truncated value
        tr[:, 1] = rs.choice([rs.randint(0, 8), rs.randint(0, 8)], n)
        x0, y0 = rs.uniform(-5, img_w * 0.6, n), rs.uniform(-5, img_h * 0.6, n)
        x1, y1 = x0 + rs.uniform(5, img_w * 0.5, n), y0 + rs.uniform(5, img_h * 0.5, n)
        box = np.stack([x0, y0, x1, y1], 1)
        snap = rs.uniform(size=box.shape) < 0.08                               # exactly on the band: masked out
        band = np.array([thr, thr, img_w - thr, img_h - thr], np.float64)
        box = np.where(snap, band, box)
        whole = rs.uniform(size=n) < 0.05                                      # a box that fills the frame: no edge is a constraint
        box[whole] = [5, thr, img_w - 1, img_h - thr]
        tr[:, 2:6] = box
        tr[:, 6:9] = rs.uniform(0.2, 2.0, 3) * rs.uniform(0.8, 1.2, (n, 3))
        tr[:, 9:12] = rs.uniform(-3, 3, 3) + rs.standard_normal((n, 3)) * 0.2
        tr[:, 12] = rs.uniform(-np.pi, np.pi) + rs.uniform(-1, 1, n) * rs.uniform(0, 1.2)
        tr[:, 13] = rs.uniform(size=n)
        tracks.append(tr)
    return tracks, img_names, P_cws, img_h, img_w


def pack(tracks):
    offs = np.zeros(len(tracks) + 1, np.int64)
    offs[1:] = np.cumsum([len(t) for t in tracks])
    rows = np.concatenate([np.asarray(t, np.float64)[:, :14] for t in tracks]) if tracks else np.zeros((0, 14))
    return rows, offs


def ulps32(a, b):
    """distance of two float32 arrays in units in the last place (same sign assumed where they differ)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
