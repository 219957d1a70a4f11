"""Multi-view super-quadric fitting of object tracks -- host driver over the gfx950 kernel.

Drop-in for the reference's `optim_process` (likojack/ODAM src/scripts/run_multi_view.py:22-76):
same arguments, same output dict {"tracks", "bboxes_qc", "bboxes_dl", "quadrics"}.  What changes
is the schedule: the reference fits one object at a time on the CPU (autograd, 200 steps); here
the host prelude is vectorised per object and ALL objects with enough views go to the GPU in one
`odam_sq_fit_batch` launch (one workgroup per object).

Reference pieces restated here (host, float64 numpy, same library calls where a library defines
the result):
  src/utils/tracking_gt_utils.py:145-211  load_pred_object   -> _object_constraints
  src/utils/tracking_gt_utils.py:59-66    averaging_T_wos    -> scipy Rotation.mean (same call)
  src/super_quadric/quadric_helper.py:69-109  bbox_to_lines  -> _edge_lines
  src/utils/box_utils.py:286-308          get_3d_box
  src/utils/box_utils.py:319-410          compute_oriented_bbox (qhull hull + rotating calipers)
With prelude="device" the part before the launch is one launch too (_device_prelude -> SqFitter.prepare, include/odam_sq.h
odam_sq_prepare_batch); the host prelude above is the default and the fallback.
"""
import logging
import math

import numpy as np
from scipy.spatial import ConvexHull
from scipy.spatial.transform import Rotation

from . import sq as _sq

EDGE_THRESHOLD = _sq.EDGE_THRESHOLD  # tracking_gt_utils.py:199
_log = logging.getLogger(__name__)


def rotz(t):  # box_utils.py:311-316
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def get_3d_box(box_size, rot_mat, center):
    """8 corners of an oriented box (box_utils.py:286-308)."""
    l, w, h = box_size
    x = [l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2]
    y = [w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2]
    z = [h / 2, h / 2, h / 2, h / 2, -h / 2, -h / 2, -h / 2, -h / 2]
    c = np.dot(rot_mat, np.vstack([x, y, z]))
    c[0, :] += center[0]
    c[1, :] += center[1]
    c[2, :] += center[2]
    return np.transpose(c)


def compute_oriented_bbox(pts):
    """Minimum-area upright box of a point set (box_utils.py:319-410).

    Quirks kept: the hull polygon is NOT closed (the edge from the last vertex back to the first is
    never tested), angles are folded into [0, pi/2) and de-duplicated, the first smallest area wins.
    """
    z_min = np.min(pts[:, 2])
    z_max = np.max(pts[:, 2])
    pts_xy = pts[:, :2]
    hull = ConvexHull(pts_xy)
    contour = pts_xy[hull.vertices].astype(pts_xy.dtype, copy=True)
    x_mean, y_mean = np.mean(contour, axis=0)
    contour[:, 0] -= x_mean
    contour[:, 1] -= y_mean
    edges = (contour[1:] - contour[:-1]).astype(np.float64)
    angles = np.array([abs(math.atan2(e[1], e[0]) % (math.pi / 2)) for e in edges])
    angles = np.unique(angles)
    # all candidate rotations at once (the reference loops; np.matmul runs the same 2x2 @ 2xV product per angle)
    ca = np.array([[math.cos(a), math.cos(a - (math.pi / 2)), math.cos(a + (math.pi / 2))] for a in angles]).reshape(-1, 3)
    Rs = np.stack([ca[:, [0, 1]], ca[:, [2, 0]]], axis=1)                 # [A, 2, 2]
    rot = np.matmul(Rs, np.transpose(contour))                            # [A, 2, V]
    mins, maxs = np.nanmin(rot, axis=2), np.nanmax(rot, axis=2)           # [A, 2]
    areas = (maxs[:, 0] - mins[:, 0]) * (maxs[:, 1] - mins[:, 1])
    best = (0, 10000000000, 0, 0, 0, 0)
    ok = areas < best[1]                                                  # NaN areas never win
    if ok.any():
        i = int(np.flatnonzero(areas == areas[ok].min())[0])              # the first smallest area wins
        best = (angles[i], areas[i], mins[i, 0], maxs[i, 0], mins[i, 1], maxs[i, 1])
    a, _, min_x, max_x, min_y, max_y = best
    R = np.array([[math.cos(a), math.cos(a - (math.pi / 2))], [math.cos(a + (math.pi / 2)), math.cos(a)]])
    c2 = np.zeros((4, 2))
    c2[0] = np.dot([max_x, max_y], R)
    c2[1] = np.dot([max_x, min_y], R)
    c2[2] = np.dot([min_x, min_y], R)
    c2[3] = np.dot([min_x, max_y], R)
    c2[:, 0] += x_mean
    c2[:, 1] += y_mean
    upper = np.concatenate([c2, np.array([[z_max] * 4]).T], axis=1)
    lower = np.concatenate([c2, np.array([[z_min] * 4]).T], axis=1)
    return np.concatenate([upper, lower], axis=0)


def compute_oriented_bboxes(points):
    """compute_oriented_bbox for a batch: points [n, N, 3] float32 -> list of n [8, 3] float64 boxes.

    The library's host routine (include/odam_sq.h, odam_sq_oriented_bbox; csrc/hull2d.h) follows qhull's 2-D construction so that
    the hull's vertex ORDER -- which decides the edge the reference's open polygon leaves out -- is qhull's; an object that sits
    inside qhull's round-off tolerance band (status 1: exact coincidences, cube-like surfaces) is recomputed here with
    scipy's qhull, the library the reference itself calls.  Returns (boxes, n_recomputed)."""
    import ctypes
    from . import _lib
    pts = np.ascontiguousarray(points, np.float32)
    n = len(pts)
    if n == 0:
        return [], 0
    corners = np.empty((n, 8, 3), np.float64)
    status = np.ones(n, np.int32)
    _lib.check(_lib.lib().odam_sq_oriented_bbox(pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(n), ctypes.c_int(pts.shape[1]),
                                                corners.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p)),
               "odam_sq_oriented_bbox")
    redo = np.flatnonzero(status)
    for i in redo:
        corners[i] = compute_oriented_bbox(pts[i])
    return [corners[i] for i in range(n)], len(redo)


def _edge_lines(bbox, img_h, img_w, thr=EDGE_THRESHOLD):
    """bbox [[x_min,y_min],[x_max,y_max]] -> {name: [a, b, -value]} for edges farther than `thr`
    pixels from the image border (quadric_helper.py:69-109)."""
    (x_min, y_min), (x_max, y_max) = bbox
    out = {}
    for name, v, lim in (("x_min", x_min, img_w), ("y_min", y_min, img_h),
                         ("x_max", x_max, img_w), ("y_max", y_max, img_h)):
        if v > thr and v < lim - thr:
            out[name] = np.array([1, 0, -v]) if name[0] == "x" else np.array([0, 1, -v])
    return out


def _object_constraints(track, frame_to_img, img_h, img_w, thr=EDGE_THRESHOLD, with_rows=False):
    """Per observed frame of one track, in image order, vectorised over the observations.

    tracking_gt_utils.py:145-211 walks every image, tests membership and builds per-frame dicts; here the
    membership is one dictionary lookup per observation (first row of a frame id wins, as
    np.where(...)[0][0] does) and the bbox-edge constraints go straight into arrays:
      tgt[n,4], mask[n,4] in the order x_min, x_max, y_min, y_max (sq_libs.py:438): mask = edge farther
      than `thr` px from the border (quadric_helper.py:87-107); tgt = float32(-float32(-pixel)), i.e. what
      `-gt` is after sq_libs.py:448 stores the line's last entry in a float32 tensor.
    Returns class, image ids [n], tgt, mask, rotation matrices [n,3,3], t_wo [3], dims [n,3]; with_rows: and the track row of
    every observation [n] (closed_form_quadrics reads the float64 edge values there).
    """
    frames = track[:, 0].astype(np.int32)
    if isinstance(frame_to_img, _UniqueFrames):
        # every frame id names ONE image (the usual sequence): first row of each id by np.unique, image index by binary search,
        # image order by one argsort -- the same (img_id, row) list as the walk below, without a Python loop per observation
        uniq, first = np.unique(frames, return_index=True)
        pos = np.searchsorted(frame_to_img.ids, uniq)
        pos[pos >= len(frame_to_img.ids)] = 0
        hit = frame_to_img.ids[pos] == uniq
        img_ids = frame_to_img.order[pos[hit]]
        rows = first[hit].astype(np.int64)
        o = np.argsort(img_ids, kind="stable")
        img_ids, rows = img_ids[o], rows[o]
    else:
        first_row = {}
        for r, fid in enumerate(frames.tolist()):
            first_row.setdefault(fid, r)
        obs = sorted((img_id, r) for fid, r in first_row.items() for img_id in frame_to_img.get(fid, ()))
        img_ids = np.array([o[0] for o in obs], np.int64)
        rows = np.array([o[1] for o in obs], np.int64)
    obj_class = int(np.median(track[:, 1]))
    t_wo = np.mean(track[:, 9:12], axis=0)
    sub = track[rows]
    c, s_ = np.cos(sub[:, 12]), np.sin(sub[:, 12])          # box_utils.rotz per observation
    R = np.zeros((len(rows), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, -s_, s_, c, 1.0
    vals = sub[:, [2, 4, 3, 5]]                              # x_min, x_max, y_min, y_max
    lims = np.array([img_w, img_w, img_h, img_h], np.float64)
    mask = ((vals > thr) & (vals < lims - thr)).astype(np.float32)
    tgt = np.where(mask > 0, (-((-vals).astype(np.float32))), np.float32(0)).astype(np.float32)
    if with_rows:
        return obj_class, img_ids, tgt, mask, R, t_wo, sub[:, 6:9], rows
    return obj_class, img_ids, tgt, mask, R, t_wo, sub[:, 6:9]


class _UniqueFrames:
    """frame id -> image index for a sequence whose frame ids are all different: ids sorted, order[i] = image index of ids[i] --
    sq.frame_tables, the tables the prelude kernel searches, under sq.unique_frame_ids, the one statement of the rule"""

    def __init__(self, img_names):
        self.ids, order = _sq.frame_tables(img_names)
        self.order = order.astype(np.int64)

    @staticmethod
    def applies(img_names):
        return _sq.unique_frame_ids(img_names) is not None


def averaging_T_wos_batch(R_list, t_list):
    """averaging_T_wos for many objects with ONE conversion of all rotation matrices, one batched symmetric eigen-decomposition and
    one conversion back -- the same operations scipy's Rotation.mean applies per object (quaternions q of the observations,
    K = q^T q by np.dot, eigenvector of the largest eigenvalue from np.linalg.eigh, taken as the mean quaternion WITHOUT
    renormalising), so every matrix equals the per-object call bit for bit (tests/test_multi_view_host.py checks 400 objects)."""
    n = len(R_list)
    out = np.tile(np.eye(4), (n, 1, 1))
    if n == 0:
        return out
    lens = [len(R) for R in R_list]
    q_all = Rotation.from_matrix(np.concatenate(R_list)).as_quat()
    K = np.empty((n, 4, 4))
    o = 0
    for i, k in enumerate(lens):
        q = q_all[o:o + k]
        K[i] = np.dot(q.T, q)
        o += k
    _, v = np.linalg.eigh(K)
    out[:, :3, :3] = Rotation(np.ascontiguousarray(v[:, :, -1]), normalize=False).as_matrix()
    for i, (t, k) in enumerate(zip(t_list, lens)):
        out[i, :3, 3] = np.mean(np.repeat(t[None, :], k, axis=0), axis=0)
    return out


def averaging_T_wos(R_wos, t_wo):
    """tracking_gt_utils.py:59-66 for T_wos that all carry the same translation (load_pred_object gives every
    per-frame T_wo the track's mean t_wo, :148/:186-189): mean rotation by scipy, mean of n equal vectors."""
    out = np.eye(4)
    out[:3, :3] = Rotation.from_matrix(R_wos).mean().as_matrix()
    out[:3, 3] = np.mean(np.repeat(t_wo[None, :], len(R_wos), axis=0), axis=0)
    return out


class SuperQuadric:
    """Result object with the attribute surface of the reference's SuperQuadric
    (sq_libs.py:531-595): translate[3], angle[], scales[3], shapes[2] as float32 numpy, obj_class,
    and compute_ellipsoid_points(use_numpy) -> ([1000,3] float32, None)."""

    def __init__(self, params, obj_class, points=None, fitter=None):
        p = np.asarray(params, np.float32)
        self.translate = p[0:3].copy()
        self.angle = np.float32(p[3])
        self.scales = p[4:7].copy()
        self.shapes = p[7:9].copy()
        self.obj_class = obj_class
        self._points = points
        self._fitter = fitter

    @property
    def params(self):
        return np.concatenate([self.translate, [self.angle], self.scales, self.shapes]).astype(np.float32)

    # run_processor.py:85-92 pickles the result dict; eval_scan2cad.py:191-215 and result_viewer.py:25-43 load it and
    # call compute_ellipsoid_points.  The device context does not travel: a loaded object without cached points
    # computes them with the default fitter.
    def __getstate__(self):
        st = dict(self.__dict__)
        st["_fitter"] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)

    def compute_ellipsoid_points(self, use_numpy=True):
        if self._points is None:
            fitter = self._fitter or default_fitter()
            self._points = fitter.points(self.params[None])[0].cpu().numpy()
        return self._points, None


_DEFAULT_FITTER = {}


def default_fitter(device="cuda:0"):
    if device not in _DEFAULT_FITTER:
        _DEFAULT_FITTER[device] = _sq.SqFitter(device, 200)
    return _DEFAULT_FITTER[device]


def _finish_dual(tracks, pre, n_iters, fitter, return_params):
    """The fit and result half of optim_process for representation "dual_quadric": all eligible objects in one fit_dual call
    (an object whose discriminant goes negative raises AssertionError there, as sq_libs.py:129,136 does), DualQuadric results,
    bboxes_qc from compute_oriented_bbox of the 2500 ellipsoid points (run_multi_view.py:66-67) through the native box path.
    `pre`: what _host_prelude / _device_prelude return."""
    n_objs = len(pre["classes"])      # (tracks may be None: optim_process(rows=...))
    fit_ids = pre["fit_ids"]
    out = None
    if fit_ids:
        out = fitter.fit_dual(pre["fit_init"][0], pre["fit_init"][1], pre["fit_counts"], pre["P"], pre["tgt"], pre["mask"], n_iters=n_iters)
    inits, bboxes_dl = pre["host"]()
    params = {i: inits[i][0] for i in range(n_objs)}
    Qs = {}
    if fit_ids:
        fp, fq = out["params"].cpu().numpy(), out["Q"].cpu().numpy()
        for j, i in enumerate(fit_ids):
            params[i] = fp[j]
            Qs[i] = fq[j]
    quadrics = [_sq.DualQuadric(Qs[i] if i in Qs else _sq.dual_params2mat(*inits[i])) for i in range(n_objs)]
    boxes = {}
    if fit_ids:
        bl, _ = compute_oriented_bboxes(np.stack([quadrics[i].compute_ellipsoid_points(use_numpy=True)[0] for i in fit_ids]))
        boxes = dict(zip(fit_ids, bl))
    bboxes_qc = [boxes[i] if i in boxes else bboxes_dl[i] for i in range(n_objs)]
    out_dict = {"tracks": tracks, "bboxes_qc": bboxes_qc, "bboxes_dl": bboxes_dl, "quadrics": quadrics}
    if return_params:
        out_dict["params"] = np.stack([params[i] for i in range(n_objs)]) if n_objs else np.zeros((0, 5), np.float32)
        out_dict["fitted"] = np.array([i in Qs for i in range(n_objs)], bool)
    return out_dict


def _frame_index(img_names):
    """frame id -> image indices, in the form _object_constraints takes"""
    if _UniqueFrames.applies(img_names):
        return _UniqueFrames(img_names)
    frame_to_img = {}
    for i, fid in enumerate(img_names):
        frame_to_img.setdefault(int(fid), []).append(i)  # every image whose id is in the track
    return frame_to_img


def _check_resume(resume, representation, n_objs):
    """the refusals of optim_process(resume=...), before any work: -> (state rows, track indices) or (None, None)"""
    if representation == "dual_quadric":
        raise ValueError('resume / return_state: the "dual_quadric" fit is not resumable (super_quadric, cube and quadric are)')
    if resume is None:
        return None, None
    if resume["representation"] != representation:
        raise ValueError(f"resume holds the state of a {resume['representation']!r} fit, this call fits {representation!r}")
    ids = np.asarray(resume["track_ids"], np.int64).reshape(-1)
    if len(ids) and (ids.min() < 0 or ids.max() >= n_objs):
        raise ValueError(f"resume refers to track {int(ids.max() if ids.max() >= n_objs else ids.min())}, the list has {n_objs} tracks "
                         "(state is keyed by track index: it does not survive merge_process)")
    if len(resume["state"]) != len(ids):
        raise ValueError(f"resume: {len(resume['state'])} state rows for {len(ids)} track indices")
    return resume["state"], ids


def _host_prelude(tracks, img_names, P_cws, img_h, img_w, representation, prior, n_views):
    """The prelude of a fit pass on the host, per track (run_multi_view.py:44-62): class, detector box, initial parameters, and the
    packed constraint rows of the tracks with at least n_views constrained views."""
    n_objs = len(tracks)
    frame_to_img = _frame_index(img_names)
    P_all = np.asarray(P_cws)

    inits, classes, bboxes_dl, fit_ids = [], [], [], []
    fit_P, fit_tgt, fit_mask, fit_counts = [], [], [], []
    cons = [_object_constraints(np.asarray(tracks[obj_id]), frame_to_img, img_h, img_w) for obj_id in range(n_objs)]
    # mean pose of every object (tracking_gt_utils.py:59-66) and its yaw: the scipy conversions once for all objects
    if n_objs and all(len(c[4]) for c in cons):
        T_wos = averaging_T_wos_batch([c[4] for c in cons], [c[5] for c in cons])
        yaws = Rotation.from_matrix(T_wos[:, :3, :3]).as_euler("zxy")[:, 0]
    else:       # an object without an observed frame: the per-object calls (and their errors) as they were
        T_wos = yaws = None
    for obj_id in range(n_objs):
        obj_class, img_ids, tgt, mask, R_wos, t_wo, dims = cons[obj_id]
        T_wo = T_wos[obj_id] if T_wos is not None else averaging_T_wos(R_wos, t_wo)
        scales = np.mean(np.asarray(dims), axis=0)
        bboxes_dl.append(get_3d_box(scales, T_wo[:3, :3], T_wo[:3, 3]))
        yaw = yaws[obj_id] if yaws is not None else Rotation.from_matrix(T_wo[:3, :3]).as_euler("zxy")[0]
        if representation == "dual_quadric":      # QuadricOptimizer.__init__ (sq_libs.py:41-58): no class, no prior
            inits.append(_sq.init_dual(T_wo[:3, 3], yaw, scales))
        else:
            if prior and obj_class not in _sq.CLASS_MAPPER:
                raise KeyError(obj_class)  # sq_libs.py:464 (CLASS_MAPPER covers classes 0..7 only)
            inits.append(_sq.init_params(T_wo[:3, 3], yaw, scales, representation))
        classes.append(obj_class)
        valid = mask.any(axis=1)       # frames with at least one constrained edge (run_multi_view.py:51-54)
        if int(valid.sum()) >= n_views:
            fit_ids.append(obj_id)
            fit_P.append(P_all[img_ids[valid]].astype(np.float32).reshape(-1, 12))
            fit_tgt.append(tgt[valid])
            fit_mask.append(mask[valid])
            fit_counts.append(int(valid.sum()))
    pre = {"classes": classes, "fit_ids": fit_ids, "fit_counts": fit_counts, "host": lambda: (inits, bboxes_dl)}
    if fit_ids:
        if representation == "dual_quadric":
            pre["fit_init"] = (np.stack([inits[i][0] for i in fit_ids]), np.stack([inits[i][1] for i in fit_ids]))
        else:
            pre["fit_init"] = np.stack([inits[i] for i in fit_ids])
        pre["P"], pre["tgt"], pre["mask"] = np.concatenate(fit_P), np.concatenate(fit_tgt), np.concatenate(fit_mask)
    return pre


def _device_prelude(tracks, img_names, P_cws, img_h, img_w, representation, prior, n_views, fitter):
    """The same prelude through SqFitter.prepare: ONE concatenate of the tracks' first 14 columns, one upload, one launch for all
    tracks, one small copy back (class, view counts, status); the tracks to fit are picked on the host from the counts and their
    constrained views are gathered on the device into the packed rows fit / fit_dual take as device tensors.  Returns the dict of
    _host_prelude, or None where this call has to take the host path: frame ids that are not all different, no track, a track
    the kernel refuses (no view, a class that is no integer in 0..63, more than sq.PREPARE_MAX_ROWS rows), or a track that is not a
    float64 array of at least 14 columns -- the host path then raises what it always raised.  Class, views, counts, tgt, mask, P, translate and scales are the host path's bits; the yaw is the closed form
    atan2(sum sin, sum cos) of the same mean rotation: a float32 init row can differ by one unit in the last place of
    its angle, bboxes_dl in the last digits of a float64."""
    n_objs = len(tracks)
    if n_objs == 0 or not _UniqueFrames.applies(img_names):
        return None
    arrs = [np.asarray(t) for t in tracks]
    if any(a.ndim != 2 or a.shape[1] < 14 or a.dtype != np.float64 for a in arrs):
        return None      # the kernel reads float64 rows of 14 columns; the host path computes in the dtype it is given, or raises
    offs = np.zeros(n_objs + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a in arrs])
    rows = np.concatenate([a[:, :14] for a in arrs]).astype(np.float64, copy=False)
    return _prelude_from_rows(rows, offs, img_names, P_cws, img_h, img_w, representation, prior, n_views, fitter)


def _prelude_from_rows(rows, offs, img_names, P_cws, img_h, img_w, representation, prior, n_views, fitter, check=None):
    """_device_prelude from the upload on, shared by its two entries: `rows` [R, 14] float64 track after track -- the host array
    _device_prelude concatenated, or a track_store.TrackRows block's rows, already on the device -- and their host offsets [n + 1].
    check: called behind prepare's one synchronisation (the block's own status word arrives with it).  None where a track comes
    back with a status."""
    import torch
    n_objs = len(offs) - 1
    lens = np.diff(offs)
    prep = fitter.prepare(rows, offs, img_names, P_cws, img_h, img_w, representation)
    if check is not None:
        check()
    if prep["status"].any():
        return None
    dual = representation == "dual_quadric"
    classes = [int(c) for c in prep["cls"]]
    if prior and not dual:
        for c in classes:
            if c not in _sq.CLASS_MAPPER:
                raise KeyError(c)  # sq_libs.py:464, where the host path raises it: at the first such track
    fit = prep["n_valid"] >= n_views
    fit_ids = [int(i) for i in np.flatnonzero(fit)]
    fit_counts = [int(c) for c in prep["n_valid"][fit]]

    def host():      # the rows of the result dict: one copy each, taken after the fit has been launched
        box = prep["bboxes_dl"].cpu().numpy()
        init = prep["init"].cpu().numpy()
        if dual:
            half = prep["half_dims"].cpu().numpy()
            return [(init[i], half[i]) for i in range(n_objs)], [box[i] for i in range(n_objs)]
        return [init[i] for i in range(n_objs)], [box[i] for i in range(n_objs)]
    pre = {"classes": classes, "fit_ids": fit_ids, "fit_counts": fit_counts, "host": host}
    if fit_ids:
        dev = prep["valid"].device
        R, K = len(rows), int(sum(fit_counts))
        # place of every constrained view of a fitted track among the packed rows: a running count, no read-back.  A track has
        # n_obs <= its rows views (a frame id can repeat or name no image); prepare hands "valid" out as 0 in the words past them,
        # so exactly K rows are selected
        sel = (prep["valid"] != 0) & torch.from_numpy(np.repeat(fit, lens)).to(dev)
        pos = torch.cumsum(sel, 0) - 1
        idx = torch.empty(K + 1, device=dev, dtype=torch.int64)      # slot K takes every row that is not packed
        idx.scatter_(0, torch.where(sel, pos, torch.full_like(pos, K)), torch.arange(R, device=dev))
        idx = idx[:K]
        pre["P"], pre["tgt"], pre["mask"] = prep["P"].index_select(0, idx), prep["tgt"].index_select(0, idx), prep["mask"].index_select(0, idx)
        ids_dev = torch.as_tensor(fit_ids, device=dev)
        if dual:
            pre["fit_init"] = (prep["init"].index_select(0, ids_dev), prep["half_dims"].index_select(0, ids_dev))
        else:
            p0 = prep["init"].index_select(0, ids_dev)
            pre["fit_init"] = p0

            def cold_state():      # sq.cold_state on the device
                st = torch.zeros(len(fit_ids), _sq.STATE_FLOATS, device=dev, dtype=torch.float32)
                st[:, 0:9] = p0
                st[:, 27:30] = p0[:, 4:7]
                st[:, 31] = _sq.REPRESENTATIONS[representation]
                return st
            pre["cold_state"] = cold_state
    return pre


def optim_process(tracks, img_names, T_wcs, P_cws, img_h, img_w, K, representation, prior, n_iters, n_views,
                  fitter=None, return_params=False, resume=None, return_state=False, prelude="host", rows=None):
    """run_multi_view.py:22-76 with the per-object fits batched on the GPU.

    Resumable (SqFitter.fit's state): with return_state the dict also holds "state" = {"state": [k, 32] rows, "track_ids": the k
    tracks fitted, "representation"}; passed back as `resume`, every track in it that is fitted again continues from its row for
    n_iters MORE steps on its current views (the constraint rows are rebuilt from the track as always), every other track starts
    cold.  State is keyed by track index: valid while association only appends tracks, invalid after merge_process.

    prelude: "host" (default) builds the constraint rows and initial shapes per track in numpy / scipy; "device" builds them for
    all tracks in one launch (_device_prelude, SqFitter.prepare) and falls back to the host path for this call, with one debug log
    line, where that does not apply: frame ids that are not all different, a track the kernel refuses (no view, a class that is no
    integer in 0..63, more than 16384 rows), no track, or a track that is not a float64 array of at least 14 columns.

    rows: a packed block of track_store.TrackRows ({"rows14" [R, 14] float64 on the device, "row_offsets" host offsets, "n_tracks", ...;
    DESIGN 6p) standing for [t[:, :14] for t in tracks]: the prelude is the device prelude run on that block -- no concatenate, no
    upload, the same bits as prelude="device" on the same rows.  `tracks` is then only passed through to the result dict and may be
    None -- or a callable without arguments that returns the list: it is called once, after the fit has been enqueued, so that a
    caller's host work on the list (merge.tracks_from_packed) runs under the fit.  Where the device prelude does not apply the call
    takes the host path if `tracks` is a host list, and raises ValueError naming the condition if it is not."""
    if prelude not in ("host", "device"):
        raise ValueError(f'prelude must be "host" or "device", got {prelude!r}')
    fitter = fitter or default_fitter()
    later = tracks if rows is not None and callable(tracks) else None
    if later is not None:
        tracks = None
    if rows is not None and tracks is not None and len(tracks) != rows["n_tracks"]:
        raise ValueError(f"optim_process: rows holds {rows['n_tracks']} tracks, the list {len(tracks)}")
    n_objs = int(rows["n_tracks"]) if tracks is None and rows is not None else len(tracks)
    res_state = res_ids = None
    if resume is not None or return_state:
        res_state, res_ids = _check_resume(resume, representation, n_objs)
    pre = None
    if rows is not None:
        why = None
        if n_objs == 0:
            why = "the block holds no track"
        elif not _UniqueFrames.applies(img_names):
            why = "the frame ids of img_names are not all different integers inside int32"
        else:
            pre = _prelude_from_rows(rows["rows14"], np.asarray(rows["row_offsets"], np.int64), img_names, P_cws, img_h, img_w, representation,
                                     prior, n_views, fitter, check=rows.get("check"))
            if pre is None:
                why = "a track came back from the prelude kernel with a status (no view, a class that is no integer in 0..63, too many rows)"
        if pre is None:
            if later is not None:
                tracks, later = later(), None
            if tracks is None:
                raise ValueError("optim_process(rows=...): the device prelude does not apply -- " + why + " -- and there is no host track list to fall back on")
            _log.debug("optim_process: the device prelude does not apply to the packed rows (%s), taking the host path", why)
    elif prelude == "device":
        pre = _device_prelude(tracks, img_names, P_cws, img_h, img_w, representation, prior, n_views, fitter)
        if pre is None:
            _log.debug("optim_process: the device prelude does not apply to this call (%d tracks), taking the host path", n_objs)
    if pre is None:
        pre = _host_prelude(tracks, img_names, P_cws, img_h, img_w, representation, prior, n_views)
    classes, fit_ids, fit_counts = pre["classes"], pre["fit_ids"], pre["fit_counts"]

    if representation == "dual_quadric":
        return _finish_dual(later() if later is not None else tracks, pre, n_iters, fitter, return_params)
    points = {}
    state_out = None
    out = None
    if fit_ids:
        more = {}
        if resume is not None or return_state:
            import torch
            # rows of fits that have not begun: the device prelude makes them where its init rows are
            st = pre["cold_state"]() if "cold_state" in pre else torch.from_numpy(_sq.cold_state(pre["fit_init"], representation))
            if res_ids is not None and len(res_ids):
                row_of = {int(t): j for j, t in enumerate(res_ids)}
                dst = [j for j, i in enumerate(fit_ids) if i in row_of]
                if dst:      # these continue; the rest of st stays the row of a fit that has not begun
                    rs = res_state if torch.is_tensor(res_state) else torch.as_tensor(np.asarray(res_state, np.float32))
                    st = st.to(rs.device)
                    st[torch.as_tensor(dst, device=rs.device)] = rs[torch.as_tensor([row_of[fit_ids[j]] for j in dst], device=rs.device)].to(torch.float32)
            more = dict(state=st, want_state=bool(return_state))
        out = fitter.fit(pre["fit_init"], [classes[i] for i in fit_ids], fit_counts, pre["P"], pre["tgt"], pre["mask"],
                         n_iters=n_iters, representation=representation, prior=bool(prior), want_points=True, **more)
        state_out = out.get("state") if return_state else None
    if later is not None:
        tracks = later()
    inits, bboxes_dl = pre["host"]()
    params = {i: inits[i] for i in range(n_objs)}
    if fit_ids:
        fp = out["params"].cpu().numpy()
        fpts = out["points"].cpu().numpy()
        for j, i in enumerate(fit_ids):
            params[i] = fp[j]
            points[i] = fpts[j]

    quadrics, bboxes_qc = [], []
    boxes = {}
    if fit_ids:       # oriented boxes of all fitted surfaces in one native call (run_multi_view.py:66-67)
        bl, _ = compute_oriented_bboxes(np.stack([points[i] for i in fit_ids]))
        boxes = dict(zip(fit_ids, bl))
    for obj_id in range(n_objs):
        if obj_id in points:  # run_multi_view.py:64-69
            quadrics.append(SuperQuadric(params[obj_id], classes[obj_id], points[obj_id], fitter))
            bboxes_qc.append(boxes[obj_id])
        else:                 # fewer than n_views constrained frames: keep the detector box (:59-62)
            quadrics.append(SuperQuadric(params[obj_id], classes[obj_id], None, fitter))
            bboxes_qc.append(bboxes_dl[obj_id])
    out_dict = {"tracks": tracks, "bboxes_qc": bboxes_qc, "bboxes_dl": bboxes_dl, "quadrics": quadrics}
    if return_params:
        out_dict["params"] = np.stack([params[i] for i in range(n_objs)]) if n_objs else np.zeros((0, 9), np.float32)
        out_dict["fitted"] = np.array([i in points for i in range(n_objs)], bool)
    if return_state:
        out_dict["state"] = {"state": state_out if state_out is not None else np.zeros((0, _sq.STATE_FLOATS), np.float32),
                             "track_ids": np.asarray(fit_ids, np.int64), "representation": representation}
    return out_dict


def optim_process_scenes(scenes, rows, representation, prior, n_iters, n_views, fitter=None):
    """optim_process(..., return_params=True, rows=block) for MANY scenes in the launches of one: ONE SqFitter.prepare_scenes
    for the tracks of all scenes, the device-side packing of the constrained views, ONE SqFitter.fit for the fitted tracks of all
    scenes, ONE compute_oriented_bboxes, and a split into one dict per scene -- each equal to the single-scene call's, key for key and
    bit for bit.

    scenes: one dict per scene: "img_names", "P_cws", "img_h", "img_w", and "tracks": the host list, None, or a callable without
    arguments that returns it (called once, after the fit has been enqueued).  rows: the combined packed block of the scenes' tracks
    (track_store.pack_scenes), scene s owning tracks trk_off[s] .. trk_off[s + 1] - 1.  representation ("super_quadric", "cube" or
    "quadric"; "dual_quadric" is refused), prior, n_iters and n_views are shared.

    A scene takes no part in the fit where the single-scene call would leave the device prelude: it holds no track, its frame ids are
    not all different, or one of its tracks comes back from the prelude kernel with a status.  Such scenes are decided from the one
    copy prepare_scenes makes anyway and REPORTED, not host-pathed here.  Returns (outs, left): outs[s] the scene's dict, or None for a
    scene that was left out; left = {s: reason}."""
    import torch
    if representation == "dual_quadric":
        raise ValueError('optim_process_scenes: representation "dual_quadric" is not fitted over scenes (super_quadric, cube and quadric are)')
    if representation not in _sq.REPRESENTATIONS:
        raise ValueError(f"optim_process_scenes: unknown representation {representation!r}")
    fitter = fitter or default_fitter()
    S = len(scenes)
    trk = np.asarray(rows["trk_off"], np.int64)
    offs = np.asarray(rows["row_offsets"], np.int64)
    if len(trk) != S + 1 or int(trk[-1]) != int(rows["n_tracks"]):
        raise ValueError(f"optim_process_scenes: the block holds {len(trk) - 1} scenes and {int(rows['n_tracks'])} tracks, {S} scenes were given")
    later = [sc["tracks"] if callable(sc.get("tracks")) else None for sc in scenes]
    tracks = [None if later[s] is not None else scenes[s].get("tracks") for s in range(S)]
    for s in range(S):
        if tracks[s] is not None and len(tracks[s]) != trk[s + 1] - trk[s]:
            raise ValueError(f"optim_process_scenes: rows holds {int(trk[s + 1] - trk[s])} tracks of scene {s}, the list {len(tracks[s])}")
    left = {}
    for s, sc in enumerate(scenes):
        if trk[s + 1] == trk[s]:
            left[s] = "the block holds no track"
        elif not _UniqueFrames.applies(sc["img_names"]):
            left[s] = "the frame ids of img_names are not all different integers inside int32"
    n_all = int(trk[-1])
    lens = np.diff(offs)
    scene_of = np.repeat(np.arange(S), np.diff(trk))
    # a scene that is out already keeps its tracks in the launch with an empty image table: no view, a status, nothing to decide twice
    prep = fitter.prepare_scenes(rows["rows14"], offs, trk, [None if s in left else sc["img_names"] for s, sc in enumerate(scenes)],
                                 [None if s in left else sc["P_cws"] for s, sc in enumerate(scenes)], [sc["img_h"] for sc in scenes],
                                 [sc["img_w"] for sc in scenes], representation)
    if rows.get("check") is not None:
        rows["check"]()
    for s in np.unique(scene_of[prep["status"] != 0]).tolist():
        left.setdefault(int(s), "a track came back from the prelude kernel with a status (no view, a class that is no integer in 0..63, too many rows)")
    keep = np.array([s not in left for s in range(S)], bool)
    in_fit = keep[scene_of] if n_all else np.zeros(0, bool)
    classes = [int(c) for c in prep["cls"]]
    if prior:
        for i in np.flatnonzero(in_fit):
            if classes[i] not in _sq.CLASS_MAPPER:
                raise KeyError(classes[i])  # sq_libs.py:464, where the single-scene call raises it
    fit = in_fit & (prep["n_valid"] >= n_views)
    fit_ids = [int(i) for i in np.flatnonzero(fit)]
    fit_counts = [int(c) for c in prep["n_valid"][fit]]
    out = None
    if fit_ids:      # _prelude_from_rows's packing, over the tracks of all scenes
        dev = prep["valid"].device
        R, K = int(offs[-1]), int(sum(fit_counts))
        sel = (prep["valid"] != 0) & torch.from_numpy(np.repeat(fit, lens)).to(dev)
        pos = torch.cumsum(sel, 0) - 1
        idx = torch.empty(K + 1, device=dev, dtype=torch.int64)
        idx.scatter_(0, torch.where(sel, pos, torch.full_like(pos, K)), torch.arange(R, device=dev))
        idx = idx[:K]
        p0 = prep["init"].index_select(0, torch.as_tensor(fit_ids, device=dev))
        out = fitter.fit(p0, [classes[i] for i in fit_ids], fit_counts, prep["P"].index_select(0, idx), prep["tgt"].index_select(0, idx),
                         prep["mask"].index_select(0, idx), n_iters=n_iters, representation=representation, prior=bool(prior), want_points=True)
    for s in range(S):
        if later[s] is not None and keep[s]:
            tracks[s] = later[s]()
    box = prep["bboxes_dl"].cpu().numpy()
    init = prep["init"].cpu().numpy()
    params = {i: init[i] for i in range(n_all)}
    points, boxes = {}, {}
    if fit_ids:
        fp, fpts = out["params"].cpu().numpy(), out["points"].cpu().numpy()
        for j, i in enumerate(fit_ids):
            params[i], points[i] = fp[j], fpts[j]
        bl, _ = compute_oriented_bboxes(fpts)
        boxes = dict(zip(fit_ids, bl))
    outs = []
    for s in range(S):
        if not keep[s]:
            outs.append(None)
            continue
        ids = range(int(trk[s]), int(trk[s + 1]))
        quadrics = [SuperQuadric(params[i], classes[i], points.get(i), fitter) for i in ids]
        outs.append({"tracks": tracks[s], "bboxes_qc": [boxes[i] if i in points else box[i] for i in ids], "bboxes_dl": [box[i] for i in ids],
                     "quadrics": quadrics, "params": np.stack([params[i] for i in ids]), "fitted": np.array([i in points for i in ids], bool)})
    return outs, left


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def closed_form_quadrics(tracks, img_names, T_wcs, P_cws, img_h, img_w, K, n_views=3, fitter=None):
    """The closed-form dual quadric of every track from its 2D box edges alone: the reference's compute_quadric_svd
    (sq_libs.py:30-36) over load_pred_object's plane vectors (tracking_gt_utils.py:198-205), which its driver collects
    (run_multi_view.py:25,36) and never uses.  No 3D guess enters -- translate, angle and dims of the detector only make
    bboxes_dl -- and there is no iteration: all tracks with at least n_views valid views go to the GPU in ONE
    SqFitter.quadric_svd call (float64; fixed accumulation order, so the result does not depend on the host's BLAS / LAPACK).

    The rows are those of the fit (_object_constraints: same views, masks, first row of a frame), but the edge values are the
    float64 pixels of the track columns [2, 4, 3, 5], not the fit's float32 targets, and P_cws is used in float64.
    Returns {"quadrics", "bboxes_qc", "bboxes_dl", "status", "eig"}: bboxes_dl as optim_process; status [n] int32 and eig [n, 3]
    (smallest, second smallest, largest eigenvalue of A; NaN where nothing was computed) as include/odam_sq.h gives them, with
    status 2 also for a track that was not sent (fewer than n_views valid views).  Status 0: quadrics[i] is an sq.DualQuadric
    (float64 Q, Q[3,3] = -1) and bboxes_qc[i] the oriented box of its compute_ellipsoid_points; otherwise quadrics[i] is None
    and bboxes_qc[i] = bboxes_dl[i], the rule optim_process has for the tracks it does not fit."""
    fitter = fitter or default_fitter()
    n_objs = len(tracks)
    frame_to_img = _frame_index(img_names)
    P_all = np.asarray(P_cws, np.float64)
    bboxes_dl, ids, counts, rows_P, rows_e, rows_m = [], [], [], [], [], []
    for obj_id in range(n_objs):
        track = np.asarray(tracks[obj_id])
        _, img_ids, _, mask, R_wos, t_wo, dims, rows = _object_constraints(track, frame_to_img, img_h, img_w, with_rows=True)
        T_wo = averaging_T_wos(R_wos, t_wo)
        bboxes_dl.append(get_3d_box(np.mean(np.asarray(dims), axis=0), T_wo[:3, :3], T_wo[:3, 3]))
        valid = mask.any(axis=1)       # frames with at least one constrained edge, as the fit counts them
        if int(valid.sum()) >= n_views:
            ids.append(obj_id)
            counts.append(int(valid.sum()))
            rows_P.append(P_all[img_ids[valid]].reshape(-1, 12))
            rows_e.append(track[rows[valid]][:, [2, 4, 3, 5]].astype(np.float64))      # x_min, x_max, y_min, y_max
            rows_m.append(mask[valid])
    status = np.full(n_objs, 2, np.int32)
    eig = np.full((n_objs, 3), np.nan)
    quadrics = [None] * n_objs
    bboxes_qc = list(bboxes_dl)
    if ids:
        out = fitter.quadric_svd(counts, np.concatenate(rows_P), np.concatenate(rows_e), np.concatenate(rows_m))
        Q, st = _host(out["Q"]), np.asarray(out["status"], np.int32)
        status[ids] = st
        eig[ids] = _host(out["eig"])
        good = [i for j, i in enumerate(ids) if st[j] == 0]
        for j, i in enumerate(ids):
            if st[j] == 0:
                quadrics[i] = _sq.DualQuadric(Q[j].copy())
        if good:      # oriented boxes of all ellipsoids in one native call (run_multi_view.py:66-67)
            bl, _ = compute_oriented_bboxes(np.stack([quadrics[i].compute_ellipsoid_points(use_numpy=True)[0] for i in good]))
            for i, b in zip(good, bl):
                bboxes_qc[i] = b
    return {"quadrics": quadrics, "bboxes_qc": bboxes_qc, "bboxes_dl": bboxes_dl, "status": status, "eig": eig}


def reprojection(tracks, quadrics, img_names, T_wcs, P_cws, img_h, img_w, K, fitter=None):
    """How well every fitted object explains the 2D detections of its track, view by view -- one yardstick for all five shapes.

    quadrics[i] belongs to tracks[i] and is a SuperQuadric (any of "super_quadric", "cube", "quadric": scored from its surface
    points through the forward half of constraint_2d, sq_libs.py:395-430, float32; an object without cached points gets them
    from ONE fitter.points call on the parameter rows), an sq.DualQuadric (the iterative fit's float32 Q or the closed form's
    float64 Q: scored through get_bbox, sq_libs.py:289-314, in float64), or None (skipped).  The rows are the fit's
    (_object_constraints: first row of a frame, the 20 px mask rule, only views with at least one constrained edge); the
    super-quadric group sees P_cws and the track columns [2, 4, 3, 5] as float32, as its fit did, the dual group as float64.
    One reprojection launch and one score launch per group (SqFitter.reproject / reproject_dual / reprojection_score).

    Returns a dict of numpy arrays.  Per object, length len(tracks): loss_2d (what the fits log), mean_abs_px, mean_iou, min_iou,
    worst_img (image index of the first view with the smallest IoU), n_views, n_edges, n_bad (views without a prediction: no
    surface point in front of the camera / a negative discriminant); an object that was skipped or has no valid view holds
    NaN / -1 / 0.  Per view, flattened in track order: view_offsets [len(tracks) + 1], img_ids, pred [., 4] (x_min, x_max, y_min,
    y_max), residual [., 4], iou."""
    fitter = fitter or default_fitter()
    n_objs = len(tracks)
    if len(quadrics) != n_objs:
        raise ValueError(f"{len(quadrics)} quadrics for {n_objs} tracks")
    frame_to_img = _frame_index(img_names)
    P_all = np.asarray(P_cws)
    P_all64 = np.asarray(P_cws, np.float64)
    counts = np.zeros(n_objs, np.int64)
    img_of, group = {}, {"sq": [], "dq": []}
    rows_P, rows_b, rows_m = {}, {}, {}
    for i, q in enumerate(quadrics):
        if q is None:
            continue
        if isinstance(q, SuperQuadric):
            kind = "sq"
        elif isinstance(q, _sq.DualQuadric):
            kind = "dq"
        else:
            raise TypeError(f"quadrics[{i}] is a {type(q).__name__}: expected multi_view.SuperQuadric, sq.DualQuadric or None")
        track = np.asarray(tracks[i])
        _, img_ids, _, mask, _, _, _, rows = _object_constraints(track, frame_to_img, img_h, img_w, with_rows=True)
        valid = mask.any(axis=1)       # frames with at least one constrained edge, as the fit counts them
        if not valid.any():
            continue
        counts[i] = int(valid.sum())
        img_of[i] = img_ids[valid]
        group[kind].append(i)
        edges = track[rows[valid]][:, [2, 4, 3, 5]]      # x_min, x_max, y_min, y_max
        if kind == "sq":
            rows_P[i] = P_all[img_ids[valid]].astype(np.float32).reshape(-1, 12)
            rows_b[i] = edges.astype(np.float32)
        else:
            rows_P[i] = P_all64[img_ids[valid]].reshape(-1, 12)
            rows_b[i] = edges.astype(np.float64)
        rows_m[i] = mask[valid]
    offs = np.zeros(n_objs + 1, np.int64)
    offs[1:] = np.cumsum(counts)
    total = int(offs[-1])
    out = {"loss_2d": np.full(n_objs, np.nan), "mean_abs_px": np.full(n_objs, np.nan), "mean_iou": np.full(n_objs, np.nan),
           "min_iou": np.full(n_objs, np.nan), "worst_img": np.full(n_objs, -1, np.int64), "n_views": counts,
           "n_edges": np.zeros(n_objs, np.int64), "n_bad": np.zeros(n_objs, np.int64), "view_offsets": offs,
           "img_ids": np.full(total, -1, np.int64), "pred": np.full((total, 4), np.nan), "residual": np.full((total, 4), np.nan),
           "iou": np.full(total, np.nan)}
    for kind, ids in group.items():
        if not ids:
            continue
        vc = [int(counts[i]) for i in ids]
        P, boxes, mask = (np.concatenate([r[i] for i in ids]) for r in (rows_P, rows_b, rows_m))
        if kind == "sq":
            pts = {i: quadrics[i]._points for i in ids if quadrics[i]._points is not None}
            need = [i for i in ids if i not in pts]
            if need:      # one call for all of them
                got = _host(fitter.points(np.stack([quadrics[i].params for i in need])))
                pts.update(zip(need, got))
            r = fitter.reproject(np.stack([np.asarray(pts[i], np.float32) for i in ids]), vc, P)
            bad = r["n_valid"] == 0
        else:
            r = fitter.reproject_dual(np.stack([np.asarray(quadrics[i].Q, np.float64) for i in ids]), vc, P)
            bad = r["status"]
        s = fitter.reprojection_score(r["ext"], bad, vc, boxes, mask, float(img_w), float(img_h))
        dst = np.concatenate([np.arange(offs[i], offs[i + 1]) for i in ids])
        out["img_ids"][dst] = np.concatenate([img_of[i] for i in ids])
        out["pred"][dst] = _host(r["ext"])
        out["residual"][dst] = _host(s["residual"])
        out["iou"][dst] = _host(s["iou"])
        for key in ("loss_2d", "mean_abs_px", "mean_iou", "min_iou", "n_edges", "n_bad"):
            out[key][ids] = _host(s[key])
        worst = _host(s["worst_view"]).astype(np.int64)
        out["worst_img"][ids] = [out["img_ids"][offs[i] + w] if w >= 0 else -1 for i, w in zip(ids, worst)]
    return out
