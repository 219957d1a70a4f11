"""numpy restatement of odam_rows_emit_tracked and odam_rows_marks (include/odam_rows.h, csrc/track_emit.hip): which detection slots
become track rows, where in the log they go, the rows' arithmetic in the kernel's fixed order, and the per-track outputs.

Everything here is the kernel's bit for bit -- single IEEE operations in binary64, evaluated one after the other, nothing fused --
except column 12, where np.arctan2 (the C library's atan2) stands for the device library's: see ATAN_ULPS in test_track_emit_gpu.py."""
import numpy as np

DETS = 30
BAD_ID, OVERFLOW = 1, 2


def cam_azi(T_wc):
    """processor.get_cam_azi, restated so that this file needs nothing of the package"""
    T = np.asarray(T_wc, np.float64)
    o = np.array([[0.0, 0, 1, 1], [0, 0, 0, 1]]) @ T.T
    o = o[0, :3] - o[1, :3]
    o[2] = 0
    o = o / np.linalg.norm(o)
    return np.arctan2(o[1], o[0])


def flags(cnt, ids, n_tracks):
    """[N, 30] bool: the emitted slots; and whether a live slot holds an id that is not below n_tracks"""
    cnt = np.asarray(cnt, np.int64)
    ids = np.asarray(ids, np.int64).reshape(len(cnt), DETS)
    live = np.arange(DETS)[None, :] < np.clip(cnt, 0, DETS)[:, None]
    return live & (ids >= 0) & (ids < n_tracks), bool((live & (ids >= n_tracks)).any())


def rows_of(blk, T_wcs, azi, img_w, img_h):
    """[N, 30, 14] float64: the row every slot WOULD give"""
    r = np.asarray(blk, np.float32).astype(np.float64)
    T = np.asarray(T_wcs, np.float64).reshape(-1, 4, 4)
    out = np.empty(r.shape[:2] + (14,))
    out[..., 0:2] = r[..., 0:2]
    out[..., 2] = r[..., 2] * float(img_w)
    out[..., 3] = r[..., 3] * float(img_h)
    out[..., 4] = r[..., 4] * float(img_w)
    out[..., 5] = r[..., 5] * float(img_h)
    out[..., 6:9] = r[..., 6:9]
    x, y, z = r[..., 9], r[..., 10], r[..., 11]
    for q in range(3):
        a = x * T[:, q, 0][:, None]
        b = y * T[:, q, 1][:, None]
        c = z * T[:, q, 2][:, None]
        out[..., 9 + q] = ((a + b) + c) + T[:, q, 3][:, None]
    out[..., 12] = np.arctan2(r[..., 12], r[..., 13]) + np.asarray(azi, np.float64)[:, None]
    out[..., 13] = r[..., 14]
    return out


def centre_bound(blk, T_wcs):
    """[N, 30, 3]: 8 * 2^-53 * (|x T[q][0]| + |y T[q][1]| + |z T[q][2]| + |T[q][3]|), what two evaluations of the 4-term sum of columns
    9-11 may differ by, in whatever order and with or without fused multiply-add: each lies within gamma_4 of the exact sum"""
    r = np.asarray(blk, np.float32).astype(np.float64)
    T = np.asarray(T_wcs, np.float64).reshape(-1, 4, 4)
    s = np.stack([np.abs(r[..., 9] * T[:, q, 0][:, None]) + np.abs(r[..., 10] * T[:, q, 1][:, None]) + np.abs(r[..., 11] * T[:, q, 2][:, None])
                  + np.abs(T[:, q, 3])[:, None] for q in range(3)], axis=-1)
    return 8.0 * 2.0 ** -53 * s


def emit(blk, cnt, ids, T_wcs, azi, img_w, img_h, n_tracks, log, tid, base):
    """odam_rows_emit_tracked on host arrays: writes log [cap, 14] float64 and tid [cap] int32 in place and returns
    {"n_emitted", "counts", "first_pos", "last_pos" [n_tracks] int32, "status"}"""
    N = len(cnt)
    cap = len(log)
    counts = np.zeros(n_tracks, np.int32)
    first = np.full(n_tracks, -1, np.int32)
    last = np.full(n_tracks, -1, np.int32)
    if N == 0:
        return {"n_emitted": 0, "counts": counts, "first_pos": first, "last_pos": last, "status": 0}
    on, bad = flags(cnt, ids, n_tracks)
    n = int(on.sum())
    status = (BAD_ID if bad else 0) | (OVERFLOW if base + n > cap else 0)
    if not status & OVERFLOW and n:
        k, d = np.nonzero(on)                    # (k, d) lexicographic: the arrival order
        pos = base + np.arange(n)
        t = np.asarray(ids, np.int32).reshape(N, DETS)[k, d]
        log[pos] = rows_of(blk, T_wcs, azi, img_w, img_h)[k, d]
        tid[pos] = t
        counts += np.bincount(t, minlength=n_tracks).astype(np.int32)
        first_of = np.full(n_tracks, np.iinfo(np.int32).max, np.int64)
        np.minimum.at(first_of, t, pos)
        np.maximum.at(last, t, pos.astype(np.int32))
        first[counts > 0] = first_of[counts > 0]
    return {"n_emitted": n, "counts": counts, "first_pos": first, "last_pos": last, "status": status}


def marks(log, res, n_log=None):
    """odam_rows_marks: [n_tracks + 1, 4] float64"""
    n_log = len(log) if n_log is None else n_log
    T = len(res["counts"])
    out = np.zeros((T + 1, 4))
    out[:T, 0] = res["counts"]
    out[:T, 1:] = -1.0
    f, l = res["first_pos"].astype(np.int64), res["last_pos"].astype(np.int64)
    hf, hl = (f >= 0) & (f < n_log), (l >= 0) & (l < n_log)
    out[:T, 1][hf] = log[f[hf], 0]
    out[:T, 2][hl] = log[l[hl], 0]
    out[:T, 3][hl] = log[l[hl], 9]
    out[T, 0], out[T, 1] = res["n_emitted"], res["status"]
    return out


def host_tracks(log, tid, n_rows, n_tracks):
    """TrackRows.host_tracks of a log: [n, 82] per track in arrival order"""
    out = []
    for t in range(n_tracks):
        r = log[:n_rows][tid[:n_rows] == t]
        full = np.full((len(r), 82), -1.0)
        full[:, :14] = r
        full[:, 78:82] = r[:, 2:6]
        out.append(full)
    return out


def tracker_ids(cnt, n_tracks, seed, grow=1):
    """ids as a tracker gives them -> ([N, 30] int32, tracks in all): -1 beyond the count and in a fifth of the live slots, tracks
    numbered in order of first appearance (so none is empty), at most one row per track and frame, up to `grow` new tracks a frame"""
    rs = np.random.RandomState(seed)
    ids = np.full((len(cnt), DETS), -1, np.int32)
    seen = 0
    for k, c in enumerate(np.clip(cnt, 0, DETS)):
        n_new = min(int(rs.randint(0, grow + 1)), int(c), n_tracks - seen)
        old = rs.permutation(seen)[:c - n_new]
        old = np.where(rs.uniform(size=len(old)) < 0.2, -1, old)
        pick = rs.permutation(np.concatenate([old, np.arange(seen, seen + n_new)]))
        ids[k, :len(pick)] = pick
        seen += n_new
    return ids, seen


def scene(N, n_tracks, seed, live=0.5, empty_chunks=()):
    """a synthetic call: N frames of random detections with counts in -2 .. 33, ids in -1 .. n_tracks - 1 (about `live` of the live
    slots emitted; ids are also set in slots BEYOND the count, where they must be ignored), poses that are rotations about a tilted
    axis plus a translation.  empty_chunks: chunks of 4096 slots whose frames get count 0.  sin / cos columns are a real angle's."""
    rs = np.random.RandomState(seed)
    blk = rs.uniform(-1, 1, (N, DETS, 15)).astype(np.float32)
    blk[..., 0] = np.arange(N, dtype=np.float32)[:, None] * 3 + 1
    blk[..., 1] = rs.randint(0, 9, (N, DETS))
    blk[..., 2:6] = rs.uniform(-0.2, 1.2, (N, DETS, 4))
    ang = rs.uniform(-np.pi, np.pi, (N, DETS)).astype(np.float32)
    blk[..., 12], blk[..., 13] = np.sin(ang), np.cos(ang)
    blk[..., 9:12] = rs.normal(0, 2.5, (N, DETS, 3))
    cnt = rs.randint(-2, 34, N).astype(np.int32)
    for c in empty_chunks:
        cnt[(c * 4096) // DETS:-(-((c + 1) * 4096) // DETS)] = 0      # every frame with a slot in the chunk
    ids = np.where(rs.uniform(size=(N, DETS)) < live, rs.randint(0, max(n_tracks, 1), (N, DETS)), -1).astype(np.int32)
    if n_tracks == 0:
        ids[:] = -1
    T = np.tile(np.eye(4), (N, 1, 1))
    for k in range(N):
        a, b = 0.07 * k + 0.3, 0.4
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        T[k, :3, :3] = Rz @ Rx
        T[k, :3, 3] = rs.normal(0, 2, 3)
    azi = np.array([cam_azi(T[k]) for k in range(N)])
    return blk, cnt, ids, T, azi
