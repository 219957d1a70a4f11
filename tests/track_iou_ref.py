"""The IoU tracker kernel (odam_amd/csrc/track_iou.hip, include/odam_track.h) restated in numpy float64: the same operations in the
same order, so that the kernel can be held to it bit for bit.  The rule is the reference's (likojack/ODAM
src/scripts/run_tracking.py:106-170 match_tracks over :37-52 convert_det_to_list, :55-103 init_tracks without ORB / depth data,
src/utils/box_utils.py:123-144 iou_2d, :424-447 iou_3d); what is spelled out here and left to numpy / BLAS there:
  * t_wo[r] = ((x T[r][0] + y T[r][1]) + z T[r][2]) + T[r][3] (the reference: a 1 x 4 by 4 x 4 matrix product);
  * a track's mean is its running sum, extended row by row, divided by the count (np.mean over axis 0 of an [n, 3] block adds the rows
    one after the other: the same bits);
  * Python's max / min, max(0, .), left-to-right products, one division in the IoUs;
  * the order of equal scores: descending index (np.argsort(kind="stable")[::-1]); a NaN score is the largest, as numpy sorts it;
  * a NaN IoU compares false and never matches (the reference asserts).
The scan over the tracks is the plain sequential loop of the reference, track by track -- not the kernel's ballot form.

`State` is one sequence; `step` takes any number of that sequence's frames and can be called again with the following ones."""
import numpy as np

MAX_DETS = 30
DEFAULTS = dict(match_threshold=0.5, track_threshold=0.8, iou3d_threshold=0.2, max_gap=5)


class Overflow(Exception):
    """a frame would take the sequence past max_tracks; .frame is its index in the step's frame arrays.  The state is as after the
    frame before it and the outputs from that frame on are as step() found them (-1)."""

    def __init__(self, frame, partial):
        super().__init__("frame %d would exceed max_tracks" % frame)
        self.frame, self.partial = frame, partial


class State:
    def __init__(self, max_tracks=1024):
        self.max_tracks = int(max_tracks)
        self.n = 0
        M = self.max_tracks
        self.sum = np.zeros((6, M))         # dims 0-2, t_wo 3-5
        self.lo = np.zeros((3, M)); self.hi = np.zeros((3, M))
        self.box = np.zeros((4, M))         # clipped pixel box of the last observation
        self.cls = np.zeros(M, np.float32)
        self.nobs = np.zeros(M, np.int64)
        self.last = np.zeros(M, np.int64)

    def copy(self):
        o = State.__new__(State)
        o.max_tracks, o.n = self.max_tracks, self.n
        for k in ("sum", "lo", "hi", "box", "cls", "nobs", "last"):
            setattr(o, k, getattr(self, k).copy())
        return o


def score_order(scores):
    """detection indices by rank: descending score, equal scores by descending index, a NaN first -- counted, as the kernel counts"""
    sc = np.asarray(scores, np.float64)
    n = len(sc)
    order = np.zeros(n, np.int64)
    for p in range(n):
        o = sc
        gt = (o > sc[p]) | (np.isnan(o) & ~np.isnan(sc[p]))
        eq = (o == sc[p]) | (np.isnan(o) & np.isnan(sc[p]))
        order[int(np.sum(gt | (eq & (np.arange(n) > p))))] = p
    return order


def _py_max(a, b):
    return np.where(b > a, b, a)


def _py_min(a, b):
    return np.where(b < a, b, a)


def _py_pos(v):
    return np.where(v > 0.0, v, 0.0)


def _clip(x, hi):
    v = np.where(x < 0.0, 0.0, x)
    return np.where(v > hi, hi, v)


def detection_values(rows, T_wc, img_w, img_h):
    """rows [n, 15] float32 of one frame -> clipped pixel boxes [n, 4], dims [n, 3], t_wo [n, 3], lo [n, 3], hi [n, 3], class, score"""
    r = np.asarray(rows, np.float32).astype(np.float64)
    T = np.asarray(T_wc, np.float64)
    wh = np.array([img_w, img_h, img_w, img_h], np.float64)
    box = _clip(r[:, 2:6] * wh, wh)
    dims = r[:, 6:9]
    x, y, z = r[:, 9], r[:, 10], r[:, 11]
    tw = np.stack([((x * T[k, 0] + y * T[k, 1]) + z * T[k, 2]) + T[k, 3] for k in range(3)], axis=1)
    lo = (-dims) / 2.0 + tw
    hi = dims / 2.0 + tw
    return box, dims, tw, lo, hi, np.asarray(rows, np.float32)[:, 1], r[:, 14]


def pair_ious(S, box, lo, hi):
    """both IoUs of one detection with the first S.n tracks: iou_2d(track, detection), iou_3d(detection, track)"""
    n = S.n
    a = S.box[:, :n]
    with np.errstate(all="ignore"):
        x_min, y_min = _py_max(a[0], box[0]), _py_max(a[1], box[1])
        x_max, y_max = _py_min(a[2], box[2]), _py_min(a[3], box[3])
        inter = _py_pos(x_max - x_min) * _py_pos(y_max - y_min)
        area_a = (a[2] - a[0]) * (a[3] - a[1]); area_b = (box[2] - box[0]) * (box[3] - box[1])
        i2 = inter / (area_a + area_b - inter)
        tl, th = S.lo[:, :n], S.hi[:, :n]
        mn = [_py_max(lo[k], tl[k]) for k in range(3)]
        mx = [_py_min(hi[k], th[k]) for k in range(3)]
        inter = _py_pos(mx[0] - mn[0]) * _py_pos(mx[1] - mn[1]) * _py_pos(mx[2] - mn[2])
        vol_a = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
        vol_b = (th[0] - tl[0]) * (th[1] - tl[1]) * (th[2] - tl[2])
        i3 = inter / (vol_a + vol_b - inter)
    return i2, i3


def step(S, blk, cnt, frame_ids, T_wcs, img_w, img_h, match_threshold=0.5, track_threshold=0.8, iou3d_threshold=0.2, max_gap=5):
    """the frames of blk [N, 30, 15] float32 / cnt [N] in order on the sequence state S (changed in place).
    Returns ids [N, 30] int32, iou2d [N, 30], iou3d [N, 30] float64 (-1 in unused slots); raises Overflow before the frame that does
    not fit."""
    blk = np.asarray(blk, np.float32); cnt = np.asarray(cnt)
    N = len(cnt)
    ids = np.full((N, MAX_DETS), -1, np.int32)
    o2 = np.full((N, MAX_DETS), -1.0); o3 = np.full((N, MAX_DETS), -1.0)
    for f in range(N):
        n = int(min(max(int(cnt[f]), 0), MAX_DETS))
        if n == 0:
            continue
        fid = int(frame_ids[f])
        box, dims, tw, lo, hi, cls, score = detection_values(blk[f, :n], T_wcs[f], img_w, img_h)
        my_id = np.full(n, -1, np.int64); my2 = np.full(n, -1.0); my3 = np.full(n, -1.0)
        used = np.zeros(S.n, bool)
        recent = ~((fid - S.last[:S.n]) > max_gap)
        for d in score_order(score):
            i2, i3 = pair_ious(S, box[d], lo[d], hi[d])
            ceq = S.cls[:S.n] == cls[d]
            m2, m3, best = -1.0, -1.0, -1
            for t in range(S.n):
                if used[t] or not ceq[t]:
                    continue
                if recent[t]:
                    if i2[t] > m2 and i3[t] > m3:
                        m2, m3, best = float(i2[t]), float(i3[t]), t
                elif i3[t] > m3:
                    m3, best = float(i3[t]), t
            my2[d], my3[d] = m2, m3
            if best >= 0 and (m2 > match_threshold or m3 > iou3d_threshold):
                my_id[d] = best
                used[best] = True
        fresh = (my_id < 0) & ~(score < track_threshold)
        if S.n + int(fresh.sum()) > S.max_tracks:
            raise Overflow(f, (ids, o2, o3))
        my_id[fresh] = S.n + np.arange(int(fresh.sum()))
        for d in range(n):
            t = int(my_id[d])
            if t < 0:
                continue
            new = np.concatenate([dims[d], tw[d]])
            if fresh[d]:
                S.sum[:, t] = new; S.nobs[t] = 1; S.cls[t] = cls[d]
            else:
                S.sum[:, t] = S.sum[:, t] + new; S.nobs[t] += 1
            nn = float(S.nobs[t])
            md, mt = S.sum[:3, t] / nn, S.sum[3:, t] / nn
            S.lo[:, t] = (-md) / 2.0 + mt
            S.hi[:, t] = md / 2.0 + mt
            S.box[:, t] = box[d]
            S.last[t] = fid
        S.n += int(fresh.sum())
        ids[f, :n] = my_id; o2[f, :n] = my2; o3[f, :n] = my3
    return ids, o2, o3


def run(blk, cnt, frame_ids, T_wcs, img_w, img_h, max_tracks=1024, **thresholds):
    """one whole sequence from an empty state -> ids, iou2d, iou3d, final State"""
    S = State(max_tracks)
    ids, o2, o3 = step(S, blk, cnt, frame_ids, T_wcs, img_w, img_h, **thresholds)
    return ids, o2, o3, S


def membership(ids, cnt):
    """tracks as lists of (frame index, detection index), in the order the observations were attached within the sequence (frame
    order; a track takes at most one detection per frame)"""
    tracks = {}
    for f in range(len(cnt)):
        for d in range(int(min(cnt[f], MAX_DETS))):
            if ids[f, d] >= 0:
                tracks.setdefault(int(ids[f, d]), []).append((f, d))
    return [tracks[t] for t in range(len(tracks))]


def fixture_scenes(z):
    """the scenes of tests/golden/iou_tracking.npz as dicts (inputs, the reference's ids / deciding IoUs / membership rows)"""
    out = []
    for k, name in enumerate(z["names"]):
        p = "s%d_" % k
        out.append({"name": str(name), **{key: z[p + key] for key in ("blk", "cnt", "frame_ids", "T_wcs", "ids", "iou2d", "iou3d", "members")},
                    "n_tracks": int(z[p + "n_tracks"])})
    return out


def fixture_thresholds(z):
    return dict(match_threshold=float(z["match_threshold"]), track_threshold=float(z["track_threshold"]),
                iou3d_threshold=float(z["iou3d_threshold"]), max_gap=int(z["max_gap"]))


def member_rows(ids, cnt):
    """membership as the fixture stores it: rows (track, frame index, detection index), sorted"""
    rows = [(t, f, d) for t, obs in enumerate(membership(ids, cnt)) for f, d in obs]
    return np.asarray(sorted(rows), np.int32).reshape(-1, 3)
