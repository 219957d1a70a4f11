"""OdamProcess -- the plugin surface of the reference (likojack/ODAM src/processor.py:15-368) over the
MI355X detector and super-quadric fitter.

Same constructor, attributes (`tracks`, `T_wcs`, `P_cws`, `usable_frames`, `sequence_meta`) and methods
(`init_sequence`, `process_frame`, `run_detector`, `optim_process`, `merge_process`) so that
src/scripts/run_processor.py:61-83 runs unchanged with `from odam_amd.processor import OdamProcess`.

What is different underneath:
  * `detector` is an odam_amd.detector.Detector (gfx950 kernels); `run_detector` can also be fed
    detections computed ahead of time in batches / on other ranks (`detect_frames`, `process_frame(...,
    detections=...)`): detection is stateless per frame (processor.py:259-289), association is not.
  * `_prepare_tracks` evaluates the surface of ALL live tracks in one odam_sq_points_batch launch
    instead of one CPU sampler call per track (processor.py:181-207).
  * `optim_process` batches every object's 200-step fit into one kernel launch (odam_amd.multi_view).
The associator (src/models/associator.py) is the reference's own and stays caller-supplied; the track merge
between the two fit passes is restated in odam_amd/merge.py (run_merge.py:79-130).
"""
import ctypes
import logging

import numpy as np
import torch

from . import merge, multi_view


class _Meta(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def get_homogeneous(pts):  # geometry_utils.py:7-49 (numpy, [N,3] -> [N,4])
    return np.concatenate([pts, np.ones_like(pts[:, 2:])], axis=1)


def projection(pts, intr_mat):  # geometry_utils.py:276-316, unbatched, keep_z=False
    pts = pts @ intr_mat.T
    z = np.ones_like(pts[:, -1])
    pts = pts / pts[:, -1:]
    pts[:, -1] *= z
    return pts


def _track_mark(track, k):
    """what identifies the first k rows of a track for the running sums of _prepare_tracks: frame id and centre of its first
    and its k-th observation (a slot of the track list that now holds another track, or an edited prefix, does not match)"""
    return (track[0, 0], track[0, 9], track[0, 10], track[k - 1, 0], track[k - 1, 9], track[k - 1, 10])


def get_cam_azi(T_wc):  # scannet_utils.py:213-222
    o = np.array([[0, 0, 1], [0, 0, 0]])
    o = (get_homogeneous(o) @ T_wc.T)[:, :3]
    o = o[0] - o[1]
    o[2] = 0
    o = o / np.linalg.norm(o)
    return np.arctan2(o[1], o[0])


def detection_array(out_objects, b, frame_id, seq_w, seq_h):
    """processor.py:269-288 for one frame, all detections at once: [n, 79] float64.  Same arithmetic as the reference's
    per-detection loop (float32 boxes divided in place by the sequence size, float32 angle -> sin / cos, every value
    widened to float64, 64 code columns of -1)."""
    bb = out_objects["bboxes"][b]
    n = len(bb)
    rows = np.full((n, 79), -1.0)
    if n == 0:
        return rows
    angles = np.asarray(out_objects["angles"][b]) / 180. * np.pi
    bb[:, :, 0] /= seq_w
    bb[:, :, 1] /= seq_h
    rows[:, 0] = frame_id
    rows[:, 1] = out_objects["classes"][b]
    rows[:, 2:6] = bb.reshape(n, 4)
    rows[:, 6:9] = out_objects["dimensions"][b]
    rows[:, 9:12] = out_objects["translates"][b]
    rows[:, 12] = np.sin(angles)
    rows[:, 13] = np.cos(angles)
    rows[:, 14] = out_objects["scores"][b]
    return rows


def detection_rows(out_objects, b, frame_id, seq_w, seq_h):
    """processor.py:269-288: one frame's post-processed detections -> list of 79-float rows."""
    return detection_array(out_objects, b, frame_id, seq_w, seq_h).tolist()


class OdamProcess:
    def __init__(self, detector, associator, transforms, scale_prior, detect_threshold=0.6, match_threshold=0.1,
                 score_threshold=0.8, representation="super_quadric", no_code=True, fitter=None):
        self.detector = detector
        self.associator = associator
        self.transforms = transforms
        self.scale_prior = scale_prior
        self.detect_threshold = detect_threshold
        self.match_threshold = match_threshold
        self.score_threshold = score_threshold
        self.representation = representation
        self.no_code = no_code
        self.run_associator = False
        self._tracks = None
        self._pending = []          # fast path: (track ids, [k, 82] rows) attached per frame, not yet concatenated into self._tracks
        self._pending_app = None    # fast path: the last frame's attach, not yet appended to the device mirror (goes with the next step)
        self._n_tracks = 0
        self._exposed = True        # somebody may hold (and edit) the list self.tracks returned: the mirror is re-checked before the next fast frame
        self.sequence_meta = None
        self.fitter = fitter
        self.refine_fitter = None   # refine(): its own context, with a bias-correction table long enough for a whole scan (REFINE_MAX_ITERS)
        self._refine_state = None   # refine(): what multi_view.optim_process(return_state=True) returned last, keyed by track index
        self.device_prelude = False  # optim_process / refine with prelude=None: True builds the fits' constraint rows on the device (multi_view.optim_process, prelude="device")
        self.resident_rows = False   # ... with prelude=None: True keeps the tracks' rows on the device between calls and uploads only the new ones (prelude="resident", track_store.TrackRows)
        self._rows = None            # the row store, made by the first call that needs it
        self._store_auth = False     # True: the row store IS the record of the tracks (track_frames_packed(resident=True)) and `tracks` a view of it
        self.logger = logging.getLogger('OdamProcess')

    # `tracks` is the reference's attribute (src/processor.py:300; a list of [n, 82] arrays, index = track id).  The fast path of
    # process_frames keeps what a frame attaches as (ids, rows) records and concatenates them into the arrays only when somebody asks
    # for the list -- a concatenate per matched track per frame is a third of that path's host time otherwise.
    # While track_frames_packed(resident=True) feeds the sequence, the rows exist on the device only (self._rows) and `tracks` is a VIEW:
    # reading it returns self._rows.host_tracks(), one download that the store caches until it changes.  Assigning `tracks`, or a
    # non-resident process_frames / track_frames_packed call, makes the host list the record again (_release_store).
    @property
    def tracks(self):
        if self._store_auth:
            return self._rows.host_tracks()
        self._sync_host_view()
        self._exposed = True
        return self._tracks

    @tracks.setter
    def tracks(self, value):
        self._store_auth = False
        self._pending = []
        self._pending_app = None
        self._tracks = value
        self._n_tracks = len(value) if value is not None else 0
        self._exposed = True

    def _sync_host_view(self):
        """fold the fast path's records into self._tracks and bring the device mirror's host-side bookkeeping (lengths, marks) in step"""
        if self._pending:
            add = {}
            for ids, rows in self._pending:
                for j, t in enumerate(ids):
                    add.setdefault(t, []).append(rows[j:j + 1])
            for t in sorted(add):
                if t < len(self._tracks):
                    self._tracks[t] = np.concatenate([self._tracks[t]] + add[t], axis=0)
                else:
                    assert t == len(self._tracks), (t, len(self._tracks))
                    self._tracks.append(np.concatenate(add[t], axis=0))
            self._pending = []
        win = getattr(self, "_win", None)
        if self._pending_app is not None:       # the last fast frame's attach has not reached the mirror yet
            ids, rows = self._pending_app
            self._pending_app = None
            if win is not None:
                win.append_raw(ids, rows)
        if win is not None and getattr(self, "_win_meta_stale", False):
            win.lengths = [len(t) for t in self._tracks]
            win.marks = win._marks_of(self._tracks)
            self._win_meta_stale = False

    def _fitter(self):
        if self.fitter is None:
            self.fitter = multi_view.default_fitter(str(getattr(self.detector, "device", "cuda:0")))
        return self.fitter

    # ---- sequence state (processor.py:291-304) ---------------------------------------------------
    def init_sequence(self, intrinsics, img_h, img_w):
        self.run_associator = False
        self.sequence_meta = _Meta(K=intrinsics, img_h=img_h, img_w=img_w)
        self.tracks = []
        self._win_meta_stale = False
        self.T_wcs = []
        self.P_cws = []
        self.usable_frames = []
        self._sum_cache = []
        self._win_checked = None
        self._frame_token = None
        self._refine_state = None
        if getattr(self, "_win", None) is not None:
            self._win.reset()
        if getattr(self, "_rows", None) is not None:
            self._rows.reset()
        if getattr(self.associator, "iou_tracker", False):
            self._iou_tracker().reset()

    # ---- detection (processor.py:259-289) ----------------------------------------------------------
    def detect_frames(self, rgbs, frame_ids):
        """Batched, stateless run_detector over several frames: list (per frame) of lists of 79-float rows.
        Frames of one size go through the detector in batches of max_batch; frames of DIFFERENT sizes are batched the
        way the reference's DETR.forward batches a list of tensors (padded NestedTensor with a key-padding mask,
        misc.py:303-320) and post-processed each with its own size."""
        size_of = lambda rgb: tuple(rgb.size) if hasattr(rgb, "size") and not isinstance(rgb, np.ndarray) else rgb.shape[1::-1]
        sizes = [size_of(rgb) for rgb in rgbs]
        out = []
        mb = getattr(self.detector, "max_batch", 1)
        on_device = getattr(self.transforms, "on_device", False)
        if on_device:
            self.detector.resize = (self.transforms.size, self.transforms.max_size)
        for b0 in range(0, len(rgbs), mb):
            chunk = rgbs[b0:b0 + mb]
            if len(set(sizes[b0:b0 + mb])) > 1:
                xs = [self.transforms(rgb, None)[0] for rgb in chunk]
                pred = self.detector.forward_nested(xs)
                for b in range(len(chunk)):
                    one = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in pred.items()}
                    objs = self.detector.postprocess(one, sizes[b0 + b], float(self.detect_threshold), self.sequence_meta.K)
                    out.append(detection_rows(objs, 0, frame_ids[b0 + b], self.sequence_meta.img_w, self.sequence_meta.img_h))
                continue
            if on_device:   # raw uint8 frames up, transform + forward on the GPU
                raw = np.stack([np.asarray(rgb, np.uint8) for rgb in chunk])
                pred = self.detector.forward_u8(torch.from_numpy(raw).to(self.detector.device))
                nb = raw.shape[0]
            else:
                x = torch.stack([self.transforms(rgb, None)[0] for rgb in chunk])
                pred = self.detector(x)
                nb = x.shape[0]
            objs = self.detector.postprocess(pred, sizes[b0], float(self.detect_threshold), self.sequence_meta.K)
            for b in range(nb):
                out.append(detection_rows(objs, b, frame_ids[b0 + b], self.sequence_meta.img_w,
                                          self.sequence_meta.img_h))
        return out

    def run_detector(self, rgb, frame_id, T_wc):
        return self.detect_frames([rgb], [frame_id])[0]

    def detect_frames_packed(self, rgbs, frame_ids):
        """detect_frames with threshold, NMS and the rows on the device (Detector.select_pack): returns device tensors
        (block float32 [N,30,15], count int32 [N]) equal, bit for bit, to parallel.pack_detections(self.detect_frames(rgbs,
        frame_ids)) -- what the all-gather of the sharded chain sends -- without the [N,Q,16] rows coming to the host.
        For frames of ONE size only: a mixed-size list raises ValueError and keeps using detect_frames (its padded batches are
        post-processed frame by frame, each with its own size)."""
        size_of = lambda rgb: tuple(rgb.size) if hasattr(rgb, "size") and not isinstance(rgb, np.ndarray) else rgb.shape[1::-1]
        sizes = {size_of(rgb) for rgb in rgbs}
        if len(sizes) > 1:
            raise ValueError(f"detect_frames_packed: frames of one size only, got {sorted(sizes)}; use detect_frames")
        det = self.detector
        N = len(rgbs)
        blk = torch.empty(N, 30, 15, device=det.device, dtype=torch.float32)
        cnt = torch.empty(N, device=det.device, dtype=torch.int32)
        mb = getattr(det, "max_batch", 1)
        on_device = getattr(self.transforms, "on_device", False)
        if on_device:
            det.resize = (self.transforms.size, self.transforms.max_size)
        m = self.sequence_meta
        for b0 in range(0, N, mb):
            chunk = rgbs[b0:b0 + mb]
            if on_device:   # raw uint8 frames up, transform + forward on the GPU
                raw = np.stack([np.asarray(rgb, np.uint8) for rgb in chunk])
                pred = det.forward_u8(torch.from_numpy(raw).to(det.device))
            else:
                pred = det(torch.stack([self.transforms(rgb, None)[0] for rgb in chunk]))
            rows = det.postprocess_rows(pred, next(iter(sizes)), m.K, on_device=True)
            det.select_pack(rows, frame_ids[b0:b0 + len(chunk)], (m.img_w, m.img_h), float(self.detect_threshold),
                            out=(blk[b0:b0 + len(chunk)], cnt[b0:b0 + len(chunk)]))
        return blk, cnt

    # ---- tracks (processor.py:95-257) --------------------------------------------------------------
    def _img_size_row(self):
        m = self.sequence_meta
        return np.array([[m.img_w, m.img_h, m.img_w, m.img_h]])

    def _track_rows(self, det, T_wc, with_code):
        """[n,79] detection rows of one frame -> [n,82] track rows (layout processor.py:98-108): boxes in pixels, centre
        and azimuth moved from the camera to the world frame, the detected box repeated as the projected one."""
        rows = np.full((len(det), 82), -1.0)
        px = det[:, 2:6] * self._img_size_row()
        rows[:, :9] = det[:, :9]
        rows[:, 2:6] = px
        rows[:, 9:12] = (get_homogeneous(det[:, 9:12]) @ T_wc.T)[:, :3]
        rows[:, 12] = np.arctan2(det[:, 12], det[:, 13]) + get_cam_azi(T_wc)
        rows[:, 13] = det[:, 14]
        if with_code:
            rows[:, 14:78] = det[:, 15:79]
        rows[:, 78:82] = px
        return rows

    def _init_tracks(self, detections, T_wc):
        """processor.py:95-131: every detection of the first frame with detections starts a track"""
        return [r[None, :] for r in self._track_rows(detections, T_wc, with_code=False)]

    # ---- device-resident track windows (odam_amd.associator.TrackWindows) ------------------------------------------------
    def _windows(self):
        """the device mirror of self.tracks' observations, or None where it does not apply (a caller-supplied associator
        or fitter without the native entry points, shape codes in use, more tracks than the native store holds)"""
        self._win_checked = None      # set again below only when the mirror was checked against self.tracks in THIS frame
        if not (getattr(self.associator, "native_windows", False) and self.no_code and hasattr(self._fitter(), "project_extents")):
            return None
        if getattr(self, "_win", None) is None:
            from .associator import TrackWindows
            self._win = TrackWindows(str(getattr(self.associator, "device", "cuda:0")))
        w = self._win
        if len(self.tracks) > w.max_tracks:
            return None
        # the window kernel reads the fitter's projected extents through a raw pointer on the window store's stream: both must
        # live on one device (a detector + fitter on cuda:0 with the associator on cuda:1 takes the host path)
        fdev = getattr(self._fitter(), "device", None)
        if fdev is not None and torch.device(fdev) != w.device:
            return None
        if not w.in_step(self.tracks):                        # first use, or somebody edited self.tracks: rebuild the mirror
            w.load(self.tracks)
        self._win_checked = getattr(self, "_frame_token", None)   # _attach_to_tracks of this frame need not check again
        return w

    def _preprocess_tracks(self, tracks, T_wc, cam_azi, n_times=100, proj_px=None):
        """processor.py:133-170: the last `n_times` observations of every track in the CURRENT camera frame,
        [T, n_times, 79] float32 padded with -1.  All observations of all tracks go through numpy at once (the
        reference loops over tracks; every row is computed by the same operations), and nothing here is a torch CPU
        op: on a many-core host those fork the whole OpenMP pool, which costs milliseconds per frame in this loop."""
        in_ = np.full((len(tracks), n_times, 79), -1.0, np.float32)
        if not len(tracks):
            return in_
        tails = [t[-n_times:] for t in tracks]                       # only the window that is used (rows are independent)
        lens = np.array([len(t) for t in tails])
        ends = np.cumsum(lens)
        cat = np.concatenate(tails, axis=0)                          # [sum min(n, n_times), 82]
        # the box projected by _prepare_tracks: handed over directly, or (reference calling convention) in the last row
        proj = cat[ends - 1, -4:] if proj_px is None else proj_px
        assert not np.any(np.all(proj == -1, axis=1)), "wrong projected bbox"
        proj = np.clip(proj / self._img_size_row()[0], a_min=-1, a_max=2)
        obs = np.full((len(cat), 79), -1.0)
        obs[:, :9] = cat[:, :9]
        obs[:, 2:6] = proj[np.repeat(np.arange(len(tracks)), lens)]
        obs[:, 9:12] = (get_homogeneous(cat[:, 9:12]) @ np.linalg.inv(T_wc).T)[:, :3]
        rel = cat[:, 12] - cam_azi
        obs[:, 12], obs[:, 13] = np.sin(rel), np.cos(rel)
        obs[:, 14] = cat[:, 13]
        obs[:, 15:79] = cat[:, 14:78]
        obs = obs.astype(np.float32)                                 # torch.tensor(., dtype=float32): round to nearest
        for idx, (n, e) in enumerate(zip(lens, ends)):
            k = min(int(n), n_times)
            in_[idx, :k] = obs[e - k:e]
        return in_

    def _prepare_tracks(self, T_wc, n_times=100):
        cam_azi = get_cam_azi(T_wc)
        tracks = self.tracks                         # read-only here (the reference deep-copies and scribbles on the copy)
        fitter = self._fitter()
        win = self._windows() if len(tracks) and n_times == getattr(getattr(self, "_win", None), "WINDOW", 100) else None
        if win is not None and hasattr(fitter, "build_track_windows"):
            # the device mirror is in step with `tracks` (checked by _windows()): the per-track means below come from its running
            # sums, and surface extents + window tensor follow in the same native call (odam_trackwin_build_tracks) -- nothing
            # of this frame's track input is computed or touched on the host
            m = self.sequence_meta
            return fitter.build_track_windows(win, np.linalg.inv(T_wc), m.K, cam_azi, m.img_w, m.img_h)
        # one batched surface evaluation for all tracks (reference: one SuperQuadric + sampler call each);
        # parameters as sq.init_params builds them: mean centre, mean azimuth, sqrt(mean dims / 2), shapes -0
        params = np.zeros((len(tracks), 9))
        params[:, 7:] = -0.0
        # np.mean = np.add.reduce / n.  Over axis 0 of an [n, 3] block numpy adds the rows one after the other, so a running sum
        # per track (extended by the rows a frame appends) gives the same bits as reducing the whole track again; the 1-D
        # azimuth column is reduced pairwise by numpy and is therefore reduced afresh.
        cache = getattr(self, "_sum_cache", None)
        if cache is None:
            cache = self._sum_cache = []
        del cache[len(tracks):]
        for i, track in enumerate(tracks):
            n = len(track)
            if i < len(cache) and cache[i][0] == n and cache[i][3] == _track_mark(track, n):
                _, s_t, s_d = cache[i][:3]
            elif i < len(cache) and 0 < cache[i][0] < n and cache[i][3] == _track_mark(track, cache[i][0]):
                k, s_t, s_d = cache[i][:3]
                s_t = s_t.copy(); s_d = s_d.copy()
                for r in range(k, n):
                    s_t += track[r, 9:12]; s_d += track[r, 6:9]
                cache[i] = (n, s_t, s_d, _track_mark(track, n))
            else:
                s_t = np.add.reduce(track[:, 9:12], axis=0); s_d = np.add.reduce(track[:, 6:9], axis=0)
                entry = (n, s_t, s_d, _track_mark(track, n))
                if i < len(cache):
                    cache[i] = entry
                else:
                    cache.append(entry)
            params[i, :3] = s_t / n
            params[i, 3] = np.add.reduce(track[:, 12], axis=0) / n
            params[i, 4:7] = np.maximum(s_d / n, 0.05)    # np.clip(., 0.05, inf)
        params[:, 4:7] = np.sqrt(params[:, 4:7] / 2)
        params = params.astype(np.float32)
        if win is not None:
            # everything after the per-track means on the device: surface extents (odam_sq_project_extents), then the
            # [T, 79, n_times] window tensor in the current camera frame (odam_trackwin_build) -- nothing comes back to the host
            T_cw = np.linalg.inv(T_wc)
            proj_dev = fitter.project_extents(params, T_cw, self.sequence_meta.K, on_device=True)
            return win.build(proj_dev, T_cw, cam_azi, self.sequence_meta.img_w, self.sequence_meta.img_h)
        if len(tracks) and hasattr(fitter, "project_extents"):
            # surface points, camera transform, projection and min / max on the device (odam_sq_project_extents): the same
            # float64 products per point as below; 32 bytes per track come back
            proj_px = fitter.project_extents(params, np.linalg.inv(T_wc), self.sequence_meta.K)
        elif len(tracks):
            # (a fitter without the device projection -- the oracle-backed test double: tests/test_processor.py)
            pts_all = fitter.points(params).cpu().numpy()
            T_cw = np.linalg.inv(T_wc)
            cam = (np.concatenate([pts_all, np.ones_like(pts_all[..., 2:])], axis=2) @ T_cw.T)[..., :3]
            pix = cam @ np.asarray(self.sequence_meta.K).T
            pix = np.ascontiguousarray((pix / pix[..., -1:]).transpose(0, 2, 1))      # [T, 3, 1000]
            lo, hi = pix.min(axis=2), pix.max(axis=2)
            proj_px = np.concatenate([lo[:, :2], hi[:, :2]], axis=1)                  # x_min, y_min, x_max, y_max
        else:
            proj_px = np.zeros((0, 4))
        in_ = self._preprocess_tracks(tracks, T_wc, cam_azi, n_times, proj_px=proj_px)
        return torch.from_numpy(np.ascontiguousarray(in_.transpose(0, 2, 1)))   # [T, 79, n_times], as .permute(0, 2, 1)

    def _collater(self, data_list):
        max_dets = 30
        n_features = data_list[0]['detections'].shape[0]
        detections = np.full((len(data_list), n_features, max_dets), -1.0, np.float32)
        tracks, poses, tsplit, dsplit, valid = [], [], [], [], []
        for b_id, data in enumerate(data_list):
            tracks.append(data['tracks'])
            poses.append(data['pose'])
            nt, nd = data['tracks'].shape[0], data['detections'].shape[1]
            tsplit.append(nt); dsplit.append(nd); valid.append((nt, nd))
            detections[b_id, :, :nd] = np.asarray(data['detections'], np.float32)
        gt_masks = np.zeros((sum(tsplit), sum(dsplit)), np.float32)
        t0 = d0 = 0
        for nt, nd in zip(tsplit, dsplit):
            gt_masks[t0:t0 + nt, d0:d0 + nd] = 1
            t0 += nt; d0 += nd
        return {"tracks": tracks[0] if len(tracks) == 1 else torch.cat(tracks, dim=0),
                "detections": torch.from_numpy(detections), "gt_masks": torch.from_numpy(gt_masks),
                "track_batch_split": tsplit, "detection_batch_split": dsplit, "poses": poses, "valid_list": valid}

    def _attach_to_tracks(self, pred_match, detections, T_wc, score_mat):
        """processor.py:212-257: a matched detection extends its track, an unmatched one (-1) starts a new one;
        matches scoring below `score_threshold` are dropped (index -1 reads the dustbin row, as in the reference)."""
        rows = self._track_rows(detections, T_wc, with_code=not self.no_code)
        win = getattr(self, "_win", None)
        # the device mirror matches the tracks as they stand: checked by _windows() in this very frame, or checked now
        tok = getattr(self, "_frame_token", None)
        in_step = win is not None and ((tok is not None and getattr(self, "_win_checked", None) is tok) or win.in_step(self.tracks))
        ids, picked = [], []
        for det_id, track_id in enumerate(pred_match):
            if score_mat[track_id, det_id] < self.score_threshold:
                continue
            if track_id == -1:
                ids.append(len(self.tracks))
                self.tracks.append(rows[det_id:det_id + 1])
            else:
                ids.append(int(track_id))
                self.tracks[track_id] = np.concatenate([self.tracks[track_id], rows[det_id:det_id + 1]], axis=0)
            picked.append(det_id)
        if in_step and ids and len(set(ids)) == len(ids) and max(ids) < win.max_tracks:
            win.append(ids, rows[picked])       # keep the mirror in step (whenever it is not, _windows() rebuilds it from self.tracks)

    # ---- per-frame driver (processor.py:306-345) ---------------------------------------------------
    def process_frame(self, rgb, frame_id, T_wc, detections=None):
        """`detections`: optional rows for this frame computed earlier by `detect_frames` (here or on another
        rank); None -> run the detector now, as the reference does."""
        if getattr(self.associator, "iou_tracker", False):
            if detections is None:
                detections = self.run_detector(rgb, frame_id, T_wc)
            return self._track_frames_iou([frame_id], [T_wc], detections_list=[detections])
        if detections is not None and self._fast_ok():
            return self.process_frames([frame_id], [T_wc], [detections])
        return self._process_frame_host(rgb, frame_id, T_wc, detections)

    def _process_frame_host(self, rgb, frame_id, T_wc, detections=None):
        """process_frame with every step a separate call, as the reference has them (src/processor.py:306-345): what runs when the
        associator or the fitter is the caller's own (no native track store), with shape codes, or with the detector in the loop"""
        self._frame_token = object()      # one per call: what "_windows() checked the device mirror in this very frame" is keyed on
        self.usable_frames.append(frame_id)
        self.T_wcs.append(T_wc)
        self.P_cws.append(self.sequence_meta.K @ np.linalg.inv(T_wc)[:3, :])
        if detections is None:
            detections = self.run_detector(rgb, frame_id, T_wc)
        if len(detections) == 0:
            return None
        detections = np.asarray(detections)
        if len(detections) > 30:
            detections = detections[:30, :]
        if not self.run_associator:
            self.run_associator = True
            self.tracks = self._init_tracks(detections, T_wc)
            return None
        dev = getattr(self.detector, "device", "cuda")
        track_tensors = self._prepare_tracks(T_wc)
        data = self._collater([{"detections": detections.astype(np.float32).T, "tracks": track_tensors, "pose": T_wc}])
        n_tracks, n_detections = data['valid_list'][0]
        with torch.no_grad():
            predictions = self.associator(data, self.match_threshold, eval_only=True)
        pred_matches = predictions['matches'][0].astype(np.int32)
        score_mat = predictions['pred'][0][0].cpu().exp().numpy()
        dets = data['detections'][0, :, :n_detections].numpy().T
        self._attach_to_tracks(pred_matches, dets, T_wc, score_mat)

    # ---- the same loop for frames whose detections are at hand, with the host out of the device's way -------------------------------
    def _fast_ok(self):
        """process_frames' fast path applies: the associator and the fitter are this package's (native track store, odam_assoc_step),
        no shape codes, one device, the Hungarian step on the host (scipy, the default)"""
        a = self.associator
        if not (self.no_code and getattr(a, "native_windows", False) and hasattr(a, "step_launch") and self._tracks is not None):
            return False      # (decided before the fitter is touched: a caller with its own associator may have no GPU fitter at all)
        if "assignment" in vars(a) or "_attach_to_tracks" in vars(self) or "_prepare_tracks" in vars(self):
            return False      # somebody hooked a step of the per-frame path on this object (tests do): keep the steps separate
        f = self._fitter()
        if not (hasattr(f, "build_track_windows") and hasattr(f, "_h")):
            return False
        from . import _lib
        if _lib.get_config("assoc.hungarian"):
            return False
        adev, fdev = getattr(a, "device", None), getattr(f, "device", None)
        return adev is not None and fdev is not None and torch.device(adev) == torch.device(fdev)

    def process_frames(self, frame_ids, T_wcs, detections_list):
        """process_frame(None, frame_ids[k], T_wcs[k], detections=detections_list[k]) for k = 0, 1, ... -- the loop of
        run_processor.py:70-79 for frames whose detections were computed ahead (detect_frames, another rank's all-gather) -- and the same
        results: the same library calls on the same values in the same order.  What changes is where the host's work sits.  Per frame the
        device runs one chain (mirror append -> track input -> association network -> Sinkhorn, ~0.47 ms at 40 tracks) and the host has
        ~0.25 ms of its own (camera quantities, track rows, Hungarian step, list bookkeeping); frame by frame the two alternate, each
        idle while the other works.  Here a frame's device work is ONE native call (odam_assoc_step), everything the host can know
        before the assignment arrives -- the NEXT frame's camera quantities and track rows included -- is computed while the device works,
        and the track list is extended lazily (self.tracks folds the records in when it is read).  Only the Hungarian step and the
        threshold tests stay between one frame's result and the next frame's launch.

        With an odam_amd.tracker.IouTracker as the associator the frames take _track_frames_iou instead: one launch for all of them."""
        if getattr(self.associator, "iou_tracker", False):
            return self._track_frames_iou(frame_ids, T_wcs, detections_list=detections_list)
        n = len(frame_ids)
        if not self._fast_ok():
            for k in range(n):
                self._process_frame_host(None, frame_ids[k], T_wcs[k], detections_list[k])
            return None
        m = self.sequence_meta
        K = np.asarray(m.K, np.float64)
        K9 = K[:3, :3].reshape(-1)
        assoc, fitter = self.associator, self._fitter()

        def prep(k):
            """everything of frame k the host can compute without the association result (numpy, as the per-frame path computes it)"""
            T_wc = T_wcs[k]
            det = detections_list[k]
            T_cw = np.linalg.inv(T_wc)
            P = {"T_wc": T_wc, "P_cw": m.K @ T_cw[:3, :], "n": len(det)}
            if len(det) == 0:
                return P
            det = np.asarray(det)
            if len(det) > 30:
                det = det[:30, :]
            # the float32 round trip of the collater (processor.py:49-68, 337-339): the attach reads the detections back from the
            # float32 tensor the associator was given
            det32T = det.astype(np.float32).T
            P["det32T"] = det32T
            P["det"] = det
            P["rows82"] = self._track_rows(det32T.T, T_wc, with_code=False)
            P["cam_azi"] = get_cam_azi(T_wc)
            P["cam21"] = np.ascontiguousarray(np.concatenate([T_cw[:3].reshape(-1), K9]))
            return P

        nxt = prep(0) if n else None
        for k in range(n):
            cur, nxt = nxt, None
            self.usable_frames.append(frame_ids[k])
            self.T_wcs.append(cur["T_wc"])
            self.P_cws.append(cur["P_cw"])
            launched = False
            if cur["n"]:
                if not self.run_associator:
                    # the first frame with detections starts the tracks (processor.py:320-323): host rows, the mirror is loaded below
                    self.run_associator = True
                    self.tracks = self._init_tracks(cur["det"], cur["T_wc"])
                else:
                    win = self._fast_mirror()
                    if win is None:      # more tracks than the native store holds: this frame takes the host path
                        self._rewind_frame()
                        self._process_frame_host(None, frame_ids[k], T_wcs[k], detections_list[k])
                        if k + 1 < n:
                            nxt = prep(k + 1)
                        continue
                    app = self._pending_app or ((), np.zeros((0, 82)))
                    self._pending_app = None
                    try:
                        assoc.step_launch(win, fitter, app[0], np.asarray(app[1])[:, :14], self._n_tracks, cur["cam21"], float(cur["cam_azi"]),
                                          float(m.img_w), float(m.img_h), cur["det32T"])
                    except BaseException:
                        self._mirror_unknown()
                        raise
                    launched = True
            if k + 1 < n:
                nxt = prep(k + 1)                 # under the device's work on frame k
            if launched:
                try:
                    Z = assoc.step_finish()
                except BaseException:
                    self._mirror_unknown()
                    raise
                self._attach_fast(Z, cur)
        return None

    def _mirror_unknown(self):
        """a native call of the fast path failed: what the device mirror holds is not known any more (the append of the last attach may or may
        not have run) -- forget its host-side bookkeeping, so that whoever uses it next (either path) rebuilds it from the track list"""
        self._pending_app = None
        self._exposed = True
        self._win_meta_stale = False
        win = getattr(self, "_win", None)
        if win is not None:
            win.lengths = [-1]          # no track list has this: in_step() fails, load() follows

    def _rewind_frame(self):
        self.usable_frames.pop(); self.T_wcs.pop(); self.P_cws.pop()

    def _fast_mirror(self):
        """the device mirror, in step with the tracks as the fast path knows them; None where the native store does not apply"""
        if getattr(self, "_win", None) is None:
            from .associator import TrackWindows
            self._win = TrackWindows(str(getattr(self.associator, "device", "cuda:0")))
        w = self._win
        if self._exposed:
            # the list was handed out (or replaced) since the last fast frame: fold everything in and check the mirror against it once
            self._sync_host_view()
            self._n_tracks = len(self._tracks)
            if self._n_tracks + 30 > w.max_tracks:
                return None
            if not w.in_step(self._tracks):
                w.load(self._tracks)
            self._exposed = False
        elif self._n_tracks + 30 > w.max_tracks:
            return None
        return w

    def _attach_fast(self, Z, cur):
        """hungarian_matching + _attach_to_tracks (src/models/associator.py:19-35, src/processor.py:212-257) on the assignment of a
        fast frame: the same tests on the same float32 values; the rows go to the record list and to the mirror's next append"""
        from . import _lib
        n_det = cur["det32T"].shape[1]
        # hungarian_matching (associator.py:19-35) on the float32 scores torch computes -- linear_sum_assignment(1 - scores), kept where the
        # matched score exceeds the match threshold -- and _attach_to_tracks' test (processor.py:228-231: a detection is dropped if the score
        # of its pair, for an unmatched one the dustbin row, is below the score threshold; a NaN is not below anything: kept, as in the
        # loop): ONE native host call on ONE exponential (odam_assoc_attach restates scipy's solver with its tie order;
        # tests/test_assoc_host.py holds it to scipy on random, tie-ridden and fixture matrices)
        score_mat = Z.exp()
        att = getattr(self, "_att", None)
        if att is None:      # result buffers and their addresses, once (numpy's .ctypes.data_as costs 3 us a call, np.empty + two of them 7)
            m_, k_ = np.empty(32, np.int32), np.empty(32, np.uint8)
            att = self._att = (m_, k_, ctypes.c_void_p(m_.ctypes.data), ctypes.c_void_p(k_.ctypes.data), _lib.lib().odam_assoc_attach)
        rc = att[4](ctypes.c_void_p(score_mat.data_ptr()), Z.shape[0] - 1, n_det, Z.shape[1], ctypes.c_double(self.match_threshold),
                    ctypes.c_double(self.score_threshold), att[2], att[3])
        if rc in (4, 5):      # what scipy raises for the same matrices
            raise ValueError("matrix contains invalid numeric entries" if rc == 4 else "cost matrix is infeasible")
        _lib.check(rc, "odam_assoc_attach")
        match, keep = att[0][:n_det], att[1][:n_det]
        picked = np.flatnonzero(keep)
        mk = match[picked]
        new = mk == -1
        n_tracks = self._n_tracks
        ids_a = mk.astype(np.int64)
        ids_a[new] = n_tracks + np.arange(int(new.sum()))
        n_tracks += int(new.sum())
        ids = ids_a.tolist()
        rows = cur["rows82"]
        if ids:
            assert len(set(ids)) == len(ids), ids      # a track receives at most one observation per frame (the Hungarian step's matching)
            sel = rows[picked]
            self._pending.append((ids, sel))
            self._pending_app = (ids, sel)
            self._n_tracks = n_tracks
            self._win_meta_stale = True

    # ---- network-free association (odam_amd.tracker.IouTracker; the reference's src/scripts/run_tracking.py) ----------------------------
    def _iou_tracker(self):
        t = self.associator
        if t.fitter is None and hasattr(self._fitter(), "_h") and torch.device(self._fitter().device) == torch.device(t.device):
            t.fitter = self._fitter()      # one device context for the tracker and the fits
        return t

    def _track_frames_iou(self, frame_ids, T_wcs, detections_list=None, packed=None):
        """The frames' association by the IoU tracker: ONE IouTracker.step call (one launch) for all of them, then the track rows on the
        host -- _track_rows(..., with_code=False) of every frame, grouped by the returned ids into self.tracks, the same [n, 82] layout as
        the network path builds, so optim_process, merge_process, refine, closed_form_quadrics, reprojection and evaluate work on them
        unchanged.  usable_frames, T_wcs and P_cws get every frame, as always.

        The rules are the reference TRACKER's (run_tracking.py), not the processor's: the first frame is not special (its detections start
        tracks only where their score reaches the tracker's track_threshold, like any other frame's), and a detection below that threshold
        that matches nothing is dropped.  This object's match_threshold / score_threshold belong to the network path and are not used.
        The tracker's device state decides the matching; self.tracks is its host record and must not be edited between frames.
        A frame that would exceed the tracker's max_tracks raises tracker.TrackOverflow: the frames before it are attached, that frame and
        the later ones of the call are not (nor appended to usable_frames)."""
        from . import parallel, tracker as _tracker
        trk = self._iou_tracker()
        m = self.sequence_meta
        n = len(frame_ids)
        if n == 0:
            return None
        if trk._state is None:
            trk.reset()
        self._release_store()      # host rows are built here: the host list is the record from now on
        if self._tracks is None or len(self._tracks) != trk.n_tracks[0]:
            raise _tracker._lib.OdamError(f"the IoU tracker holds {trk.n_tracks[0]} tracks, self.tracks "
                                          f"{None if self._tracks is None else len(self._tracks)}: init_sequence first, and do not edit the list between frames")
        if packed is None:
            blk, cnt = parallel.pack_detections([d if isinstance(d, np.ndarray) else np.asarray(d, np.float64).reshape(-1, 79)
                                                 for d in detections_list])
            step_in = (blk, cnt)
        else:
            step_in = packed
        T_all = np.ascontiguousarray(np.stack([np.asarray(T, np.float64) for T in T_wcs]))
        done, err = n, None
        try:
            ids = trk.step(step_in[0], step_in[1], np.asarray(frame_ids, np.int64), T_all, m.img_w, m.img_h)[0]
        except _tracker.TrackOverflow as e:
            ids, done, err = e.outputs[0], e.frame, e
        ids = ids.cpu().numpy()
        if packed is not None:
            blk, cnt = packed[0].cpu().numpy(), packed[1].cpu().numpy()
        for k in range(done):
            self.usable_frames.append(frame_ids[k])
            self.T_wcs.append(T_wcs[k])
            self.P_cws.append(m.K @ np.linalg.inv(T_wcs[k])[:3, :])
        tracks = self.tracks
        add = {}
        for k in range(done):
            nk = int(min(max(int(cnt[k]), 0), parallel.MAX_DETS))
            if nk == 0:
                continue
            self.run_associator = True
            rows = self._track_rows(blk[k, :nk].astype(np.float64), np.asarray(T_wcs[k]), with_code=False)
            for d in range(nk):
                if ids[k, d] >= 0:
                    add.setdefault(int(ids[k, d]), []).append(rows[d:d + 1])
        for t in sorted(add):
            if t < len(tracks):
                tracks[t] = np.concatenate([tracks[t]] + add[t], axis=0)
            else:
                assert t == len(tracks), (t, len(tracks))
                tracks.append(np.concatenate(add[t], axis=0))
        self._n_tracks = len(tracks)
        if err is not None:
            raise err
        return None

    def _release_store(self):
        """the end of the resident mode: the list the store stands for becomes self.tracks (downloaded here unless somebody read it
        already), and the store follows the host list through TrackRows.sync as before"""
        if self._store_auth:
            self.tracks = self._rows.host_tracks()

    def _track_frames_resident(self, blk, cnt, frame_ids, T_wcs):
        """_track_frames_iou with the track rows made on the device: IouTracker.step, then TrackRows.append_tracked on the ids as they
        lie on the device.  No detection, id or row visits the host; the poses' azimuths (get_cam_azi) go up with the poses."""
        from . import tracker as _tracker
        trk = self._iou_tracker()
        m = self.sequence_meta
        n = len(frame_ids)
        if n == 0:
            return None
        if trk._state is None:
            trk.reset()
        if self._rows is None:
            from .track_store import TrackRows
            self._rows = TrackRows(self._fitter())
        if not self._store_auth:      # the store takes over from the host list: in step with it first (nothing to send in a new sequence)
            if self._tracks is None or self._rows.sync(self.tracks) is None:
                raise _tracker._lib.OdamError("track_frames_packed(resident=True): init_sequence first; the row store does not take this track list")
            self._store_auth = True
        if len(self._rows.lengths) != trk.n_tracks[0]:
            raise _tracker._lib.OdamError(f"the IoU tracker holds {trk.n_tracks[0]} tracks, the row store {len(self._rows.lengths)}: "
                                          "init_sequence first, and do not edit the tracks between frames")
        T_all = np.ascontiguousarray(np.stack([np.asarray(T, np.float64) for T in T_wcs]))
        done, err = n, None
        try:
            ids = trk.step(blk, cnt, np.asarray(frame_ids, np.int64), T_all, m.img_w, m.img_h)[0]
        except _tracker.TrackOverflow as e:      # the slots from the overflow frame on are -1: emitting over all frames adds nothing for them
            ids, done, err = e.outputs[0], e.frame, e
        azi = np.array([get_cam_azi(T) for T in T_all])
        self._rows.append_tracked(blk, cnt, ids, T_all, azi, m.img_w, m.img_h, trk.n_tracks[0])
        for k in range(done):
            self.usable_frames.append(frame_ids[k])
            self.T_wcs.append(T_wcs[k])
            self.P_cws.append(m.K @ np.linalg.inv(T_wcs[k])[:3, :])
        if not self.run_associator and done:      # (four bytes back, until the first frame with a detection)
            self.run_associator = bool((torch.as_tensor(cnt)[:done] > 0).any())
        self._n_tracks = trk.n_tracks[0]
        if err is not None:
            raise err
        return None

    def track_frames_packed(self, blk, cnt, frame_ids, T_wcs, resident=False):
        """process_frames for an IouTracker on detect_frames_packed's device block (float32 [N, 30, 15] + int32 [N]): the block goes into
        the tracker's launch as it is -- the detections do not visit the host before the tracks are built; they are read back once,
        afterwards, for the host's track rows.  Same tracks as process_frames on the unpacked rows.

        resident=True builds no host rows at all: the ids stay on the device and the track rows are written there, straight into the
        row store (track_store.TrackRows.append_tracked); usable_frames, T_wcs, P_cws, run_associator and TrackOverflow are
        as above.  From then on the STORE is the record of the tracks and `self.tracks` a view of it: reading it downloads the list
        (TrackRows.host_tracks, cached until the next frames arrive; equal to the host path's list up to the rounding DESIGN 6t
        states) and edits of that list reach nobody.  refine / optim_process with prelude="resident" and
        pipeline.map_scene(resident_rows=True, loaded=True) take the store as it stands, without a sync and without the list.
        The view ends, and the host list is the record again with the store following it through sync, as soon as `tracks` is
        assigned (nothing is downloaded: the assigned list replaces the rows), a non-resident process_frames / process_frame /
        track_frames_packed call is made, or the store is asked to stand for another list (optim_process(prelude="resident") on a
        list that is not the view, map_scene's merge); all but the assignment download the list first."""
        if not getattr(self.associator, "iou_tracker", False):
            raise TypeError("track_frames_packed needs an odam_amd.tracker.IouTracker as the associator")
        if resident:
            return self._track_frames_resident(blk, cnt, frame_ids, T_wcs)
        return self._track_frames_iou(frame_ids, T_wcs, packed=(blk, cnt))

    # ---- back end (processor.py:347-368) -----------------------------------------------------------
    def merge_process(self, data, on_device=False):
        """on_device: clustering and assembly on the device too (merge.merge_scenes); the same merged tracks"""
        self.logger.info("Merging tracks")
        if self._refine_state is not None:      # keyed by track index, and merging renumbers the tracks
            self.logger.info("Dropping the fit state of %d refined tracks: track indices change in merge_process",
                             len(self._refine_state["track_ids"]))
            self._refine_state = None
        if on_device:
            return merge.merge_process(data, self.usable_frames, fitter=self._fitter(), on_device=True)
        return merge.merge_process(data, self.usable_frames)

    REFINE_MAX_ITERS = 4000     # steps one track can take over all refine() calls of a sequence (rows of the context's Adam table)

    def refine(self, n_iters=50, return_params=False, prelude=None):
        """The online call: current shapes of the live tracks while the scan is running.  Fits every track with enough views for
        n_iters steps, CONTINUING every track an earlier refine() of this sequence fitted (parameters, Adam moments, step count and
        the scales the prior is measured from are kept here, per track index) on the views it has now; a new track, or one that had
        too few views last time, starts cold.  Returns optim_process's dict.  Reads the tracks and nothing else: association, and
        optim_process at the end of the scan, go on as if it had never been called.  init_sequence clears the state, merge_process
        drops it (track indices change there).  Not for representation "dual_quadric".  prelude: "host", "device" (multi_view.optim_process),
        "resident" (the device prelude on the row store: only the rows the scan added since the last call are uploaded), or None for what
        self.resident_rows / self.device_prelude say."""
        if self.representation == "dual_quadric":
            raise ValueError('refine: the "dual_quadric" fit is not resumable')
        if self.refine_fitter is None:
            self.refine_fitter = multi_view._sq.SqFitter(str(getattr(self.detector, "device", "cuda:0")), self.REFINE_MAX_ITERS)
        m = self.sequence_meta
        # (a resident sequence fitted from its store needs the list for the result dict only: it is downloaded under the fit)
        tracks = (lambda: self.tracks) if self._store_auth and self._prelude(prelude) == "resident" else self.tracks
        out = multi_view.optim_process(tracks, self.usable_frames, self.T_wcs, self.P_cws, m.img_h, m.img_w, m.K,
                                       self.representation, prior=True, n_iters=int(n_iters), n_views=10,
                                       fitter=self.refine_fitter, return_params=return_params,
                                       resume=self._refine_state, return_state=True, **self._prelude_args(prelude, tracks, self.refine_fitter))
        # (a track fitted once is fitted every time after: its views only grow, so the new rows cover the old ones)
        self._refine_state = out.pop("state")
        return out

    def closed_form_quadrics(self, n_views=3):
        """The detector-independent shapes of the live tracks: multi_view.closed_form_quadrics (the closed-form dual quadric from
        the 2D box edges, one launch, no iteration) on the views the tracks have now, from n_views valid views on.  Reads the tracks
        and nothing else, like refine(), and keeps no state: association, refine() and optim_process go on as if it had never
        been called.  Works for every representation."""
        m = self.sequence_meta
        return multi_view.closed_form_quadrics(self.tracks, self.usable_frames, self.T_wcs, self.P_cws, m.img_h, m.img_w, m.K,
                                               n_views=int(n_views), fitter=self._fitter())

    def reprojection(self, tracks, quadrics):
        """How well quadrics[i] (a multi_view.SuperQuadric, an sq.DualQuadric or None) explains the detections of tracks[i], view by
        view: multi_view.reprojection with this sequence's frames, poses and intrinsics -- the output of optim_process, refine() or
        closed_form_quadrics scored on one scale.  Reads its arguments and the sequence and nothing else, and keeps no state."""
        m = self.sequence_meta
        return multi_view.reprojection(tracks, quadrics, self.usable_frames, self.T_wcs, self.P_cws, m.img_h, m.img_w, m.K,
                                       fitter=self._fitter())

    def evaluate(self, out, gt_boxes, gt_classes, threshold=0.25, min_views=1):
        """A result dict of optim_process / refine against the ground truth of its scene (corners [k, 8, 3], class ids [k]):
        evaluate.evaluate for the one scene -- the reference's eval_scan2cad.py matching and F1 table, two launches.  Reads its
        arguments and nothing else, and keeps no state."""
        from . import evaluate
        return evaluate.evaluate([out], [(gt_boxes, gt_classes)], threshold, min_views, fitter=self._fitter())

    def evaluate_ap(self, out, gt_boxes, gt_classes, ovthresh=0.25, use_07_metric=False, iou="aabb", min_views=1):
        """A result dict of optim_process / refine against the ground truth of its scene, score-ranked: evaluate.evaluate_ap for the
        one scene -- the reference's eval_det_cls / voc_ap curves and average precision per class, objects ranked by the mean score
        of their detections.  Reads its arguments and nothing else, and keeps no state."""
        from . import evaluate
        return evaluate.evaluate_ap([out], [(gt_boxes, gt_classes)], ovthresh, use_07_metric, iou, min_views, fitter=self._fitter())

    def detections_ap(self, blk, cnt, other_blk, other_cnt, iou="aabb3d", ovthresh=0.25, use_07_metric=False):
        """The detections of one run (detect_frames_packed's block and counts) against those of another run of the same frames as
        the ground truth, frame by frame, on the device: evaluate.detections_ap -- what a narrower number type costs at the level of
        detections, before association and fitting.  Reads its arguments and nothing else, and keeps no state."""
        from . import evaluate
        return evaluate.detections_ap(blk, cnt, other_blk, other_cnt, iou, ovthresh, use_07_metric, fitter=self._fitter())

    def _prelude(self, prelude):
        if prelude is None:
            return "resident" if self.resident_rows else "device" if self.device_prelude else "host"
        return prelude

    def _prelude_args(self, prelude, tracks, fitter):
        """the prelude keywords of multi_view.optim_process; "resident": the row store is brought in step with `tracks` (only rows that
        were appended since the last call go up) and its packed block stands for them; a list the store refuses takes the device prelude.
        Where the store is the record itself (track_frames_packed(resident=True)) and `tracks` is its view -- the list self.tracks
        returned, or a callable that will return it -- the store is taken as it stands: no sync, and the list is not needed"""
        prelude = self._prelude(prelude)
        if prelude != "resident":
            return {"prelude": prelude}
        if self._store_auth:
            if callable(tracks) or self._rows.is_view(tracks):
                return {"prelude": "device", "rows": self._rows.packed()}
            self._release_store()      # the store is to stand for another list
        if self._rows is None:
            from .track_store import TrackRows
            self._rows = TrackRows(fitter)
        if self._rows.sync(tracks) is None:
            return {"prelude": "device"}
        return {"prelude": "device", "rows": self._rows.packed()}

    def fit_settings(self):
        """what optim_process hands multi_view.optim_process besides the sequence: the settings processes must share to be fitted in
        one call (pipeline.map_scenes)"""
        # (QuadricOptimizer.run takes 500 steps whatever it is told, sq_libs.py:227)
        return {"representation": self.representation, "prior": True, "n_iters": 500 if self.representation == "dual_quadric" else 200,
                "n_views": 10}

    def optim_process(self, tracks, return_params=False, prelude=None, rows=None):
        """prelude: "host", "device" (multi_view.optim_process), "resident" (the device prelude on the row store, self._rows), or None for
        what self.resident_rows / self.device_prelude say.  rows: a packed block that stands for the tracks' rows (multi_view.optim_process;
        pipeline.map_scene passes its store's), whatever prelude says"""
        m = self.sequence_meta
        fit = self.fit_settings()
        return multi_view.optim_process(tracks, self.usable_frames, self.T_wcs, self.P_cws, m.img_h, m.img_w, m.K,
                                        fit["representation"], prior=fit["prior"], n_iters=fit["n_iters"], n_views=fit["n_views"],
                                        fitter=self._fitter(), return_params=return_params,
                                        **({"rows": rows} if rows is not None else self._prelude_args(prelude, tracks, self._fitter())))

    def optim_process_params(self, tracks):
        """optim_process + the fitted parameter rows and the fitted / not-fitted flags (what a rank sends to the others:
        odam_amd/pipeline.py)"""
        return self.optim_process(tracks, return_params=True)
