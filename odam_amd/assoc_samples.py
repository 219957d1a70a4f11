"""Validation samples of the association network, cut from a per-scene ground-truth track table: what the reference's dataset builds per
sampled frame (likojack/ODAM src/datasets/scan_net_track.py:285-341 ScanNetTrack.get_by_sequence, :34-97 collater), without its three file
reads -- the caller supplies the axis-aligned T_wc per frame and the image size per scene.

    table `tracks` [n_obj, n_frames, 83] float64 (scan_net_track.py:4-5):
        0 image id (-1: not observed in this frame) | 1 class | 2-5 detected box | 6-8 dims | 9-11 t_wo | 12 azimuth | 13 score |
        14 ground-truth id | 15-78 shape code | 79-82 the object's projected box in this frame, pixels
    `unmatched`: {str(img_name): [79-vector, ...]} -- detections of that frame that belong to no object (same first 79 columns)

plan() decides everything discrete on the host (pure numpy); SceneTable keeps the compacted scene on the device (include/odam_samples.h)
and cut() builds a whole batch in one launch, straight into the layout Associator.forward_batch takes; cut_host() is the same batch
through numpy.  The one deviation from the reference: "poses" holds the caller's T_wc of the frame (the reference returns the un-aligned
T_cw it read from the pose file, which this interface never sees)."""
import ctypes
import time

import numpy as np
import torch

from . import _lib

MAX_DETS = 30          # ScanNetTrack.max_objs / the collater's max_dets
MAX_BATCH = 64         # odam_samples_cut's and odam_assoc_forward_batch's limits
MAX_SUM_T = 1024
_COLS78 = np.r_[0:14, 15:79]      # a row without its ground-truth id (np.delete(row, 14): scan_net_track.py:294, 307-308)


class _Index:
    """the host's discrete view of a scene: who is valid where, and where each row went in the compacted arrays"""

    def __init__(self, tracks, unmatched, img_names=None):
        tracks = np.asarray(tracks)
        if tracks.ndim != 3 or tracks.shape[2] != 83:
            raise ValueError(f"assoc_samples: the table is [n_obj, n_frames, 83], got {tracks.shape}")
        self.n_obj, self.n_frames = tracks.shape[:2]
        self.valid = tracks[:, :, 0] != -1                                   # _get_objs_from_tracks / _get_objs_from_frame: obj[0] != -1
        self.cum = np.zeros((self.n_obj, self.n_frames + 1), np.int32)       # cum[o, f]: valid rows of o in frames < f
        np.cumsum(self.valid, axis=1, out=self.cum[:, 1:])
        self.obs_off = np.zeros(self.n_obj + 1, np.int64)
        np.cumsum(self.cum[:, -1], out=self.obs_off[1:])
        first = np.argmax(self.valid, axis=1)
        self.gid = np.where(self.valid.any(axis=1), tracks[np.arange(self.n_obj), first, 14], -1).astype(np.int64)      # int(t[0, 14]), :306
        self.img_names = [str(f) for f in range(self.n_frames)] if img_names is None else [str(n) for n in img_names]
        if len(self.img_names) != self.n_frames:
            raise ValueError("assoc_samples: one image name per frame")
        rows = [np.asarray(unmatched.get(n, []), np.float64).reshape(-1, 79) for n in self.img_names]
        self.unm_off = np.zeros(self.n_frames + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=self.unm_off[1:])
        self.unm = np.ascontiguousarray(np.concatenate(rows, axis=0)[:, _COLS78[:78]])

    def n_tracks(self, frames):
        return (self.cum[:, np.asarray(frames, np.int64)] > 0).sum(axis=0)

    def n_detections(self, frames, use_gt_det=False):
        f = np.asarray(frames, np.int64)
        n = self.valid[:, f].sum(axis=0)
        return n if use_gt_det else n + (self.unm_off[f + 1] - self.unm_off[f])


def _plan(ix, frame_ids, use_gt_det=False, n_times=100):
    out = []
    for f in [int(f) for f in frame_ids]:
        if not 0 <= f < ix.n_frames:
            raise IndexError(f"assoc_samples: frame {f} outside the scene's {ix.n_frames}")
        cnt = ix.cum[:, f]
        tr = np.flatnonzero(cnt > 0)                       # the tracks: objects seen before f, in object order
        fo = np.flatnonzero(ix.valid[:, f])                # the frame's objects
        pos = np.full(ix.n_obj, -1, np.int64)
        pos[fo] = np.arange(len(fo))
        new = fo[cnt[fo] == 0]
        # _get_match_list (:142-171): a pair per track, then the frame objects that are no track
        match = np.concatenate([np.stack([np.arange(len(tr)), pos[tr]], axis=1),
                                np.stack([np.full(len(new), -1), pos[new]], axis=1)]).astype(np.int64)
        det_src = ix.obs_off[fo] + cnt[fo]                 # the row of o in frame f stands behind its cnt earlier ones
        if not use_gt_det:                                 # _concat_unmatched (:271-283)
            u = np.arange(ix.unm_off[f], ix.unm_off[f + 1])
            if len(u):
                match = np.concatenate([match, np.stack([np.full(len(u), -1), len(fo) + np.arange(len(u))], axis=1)])
                det_src = np.concatenate([det_src, -(u + 1)])
            if len(det_src) > MAX_DETS:                    # the detections AND the pair list are cut to 30: restated, not repaired
                match, det_src = match[:MAX_DETS], det_src[:MAX_DETS]
        k = np.minimum(cnt[tr], n_times)
        scores = np.zeros((len(tr), len(det_src)), np.float32)
        for i, j in match:
            if i != -1 and j != -1:
                scores[i, j] = 1.0                         # (an IndexError here is the reference's: a matched pair past the cap)
        out.append({"frame": f, "track_objs": tr, "row0": (ix.obs_off[tr] + cnt[tr] - k).astype(np.int64), "k": k.astype(np.int64),
                    "det_src": det_src.astype(np.int64), "valid": (len(tr), len(det_src)), "match": match, "scores": scores,
                    "global_track_ids": [int(g) for g in ix.gid[tr]]})
    return out


def plan(tracks, unmatched, frame_ids, use_gt_det=False, n_times=100, img_names=None):
    """Everything discrete about the samples of `frame_ids`, from the dense table, without a device.  Per sample a dict: "frame";
    "track_objs" [T] (objects with a valid row in a frame before it, in object order); "row0" / "k" [T] (the kept rows of a track are rows
    row0 .. row0 + k of the compacted observation array: its last min(count, n_times) valid rows before the frame); "det_src" [n] (>= 0:
    that row of the compacted observations, the frame's own objects in object order; < 0: row -(src + 1) of the frame-ordered unmatched
    rows); "valid" (T, n); "match" [pairs, 2]; "scores" [T, n] float32; "global_track_ids"."""
    return _plan(_Index(tracks, unmatched, img_names), frame_ids, use_gt_det, n_times)


def channels(rows78, cam13, box):
    """[m, 78] float64 rows (ground-truth id removed) -> [m, 79] float32 network input rows (_preprocess_tracks :219-238, _preprocess
    :184-198) in the kernel's operation order: t_co = ((x c0 + y c1) + z c2) + c3 per camera row -- every product and sum a float64
    operation of its own --, sin / cos of azimuth - cam_azi, rounded to float32 once.  cam13 [13] or [m, 13]; box [m, 4] or [4]."""
    rows78 = np.asarray(rows78, np.float64)
    cam = np.broadcast_to(np.asarray(cam13, np.float64), (len(rows78), 13))
    out = np.empty((len(rows78), 79), np.float64)
    out[:, 0:2] = rows78[:, 0:2]
    out[:, 2:6] = box
    out[:, 6:9] = rows78[:, 6:9]
    x, y, z = rows78[:, 9], rows78[:, 10], rows78[:, 11]
    for i in range(3):
        out[:, 9 + i] = ((x * cam[:, 4 * i] + y * cam[:, 4 * i + 1]) + z * cam[:, 4 * i + 2]) + cam[:, 4 * i + 3]
    rel = rows78[:, 12] - cam[:, 12]
    out[:, 12], out[:, 13] = np.sin(rel), np.cos(rel)
    out[:, 14] = rows78[:, 13]
    out[:, 15:] = rows78[:, 14:]
    return out.astype(np.float32)


def camera_block(T_wcs):
    """[n_frames, 13]: rows 0-2 of inv(T_wc) and the camera azimuth (processor.get_cam_azi = scannet_utils.get_cam_azi)"""
    from .processor import get_cam_azi
    T_wcs = np.asarray(T_wcs, np.float64).reshape(-1, 4, 4)
    cam = np.empty((len(T_wcs), 13))
    for f, T in enumerate(T_wcs):
        cam[f, :12] = np.linalg.inv(T)[:3].reshape(-1)
        cam[f, 12] = get_cam_azi(T)
    return cam


class SceneTable:
    """One labelled scene, compacted once: the valid rows object after object [n_obs, 78], their offsets, the projected boxes
    [n_obj, n_frames, 4], the camera block [n_frames, 13] and the unmatched rows -- the dense table is mostly -1 and is never uploaded.
    device=None keeps the scene on the host only (cut_host)."""

    def __init__(self, tracks, unmatched, T_wcs, img_size, img_names=None, device="cuda:0"):
        tracks = np.asarray(tracks, np.float64)
        self.ix = _Index(tracks, unmatched, img_names)
        self.obs = np.ascontiguousarray(tracks[self.ix.valid][:, _COLS78])      # (a boolean mask walks the table row-major: object, then frame)
        self.proj = np.ascontiguousarray(tracks[:, :, 79:83])
        self.T_wcs = np.asarray(T_wcs, np.float64).reshape(-1, 4, 4)
        if len(self.T_wcs) != self.ix.n_frames:
            raise ValueError("assoc_samples: one T_wc per frame")
        self.cam = camera_block(self.T_wcs)
        self.img_w, self.img_h = float(img_size[0]), float(img_size[1])
        self.wh = np.array([self.img_w, self.img_h, self.img_w, self.img_h])
        self.device = None if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        self.plan_seconds = 0.0      # host time spent planning (tools/assoc_samples_timing.py reads it)
        if self.device is not None:
            if len(self.obs) == 0:
                raise ValueError("assoc_samples: a scene without a single observation")
            L, ix = _lib.lib(), self.ix
            _lib.check(L.odam_samples_create(ix.n_obj, ix.n_frames, len(self.obs), len(ix.unm), ctypes.byref(self._h)), "odam_samples_create")
            a = lambda x: x.ctypes.data
            with torch.cuda.device(self.device):
                _lib.check(L.odam_samples_load(self._h, a(self.obs), a(ix.obs_off), a(self.proj), a(self.cam), a(ix.unm) if len(ix.unm) else None,
                                               a(ix.unm_off), self.img_w, self.img_h, torch.cuda.current_stream(self.device).cuda_stream),
                           "odam_samples_load")

    def close(self):
        if self._h:
            _lib.lib().odam_samples_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def usable_frames(self, use_gt_det=False):
        """the frames with at least one track and one detection: the only ones the batched forward accepts"""
        f = np.arange(self.ix.n_frames)
        return [int(x) for x in f[(self.ix.n_tracks(f) >= 1) & (self.ix.n_detections(f, use_gt_det) >= 1)]]

    def batches(self, frame_ids, batch_size):
        """frame_ids in order, split so that no batch has more than min(batch_size, 64) samples or more than 1024 tracks"""
        frame_ids = [int(f) for f in frame_ids]
        size = max(1, min(int(batch_size), MAX_BATCH))
        out, cur, t_cur = [], [], 0
        for f, t in zip(frame_ids, self.ix.n_tracks(frame_ids).tolist() if frame_ids else []):
            if t > MAX_SUM_T:
                raise _lib.OdamError(f"assoc_samples: frame {f} has {t} tracks, a batch holds {MAX_SUM_T}")
            if cur and (len(cur) == size or t_cur + t > MAX_SUM_T):
                out.append(cur)
                cur, t_cur = [], 0
            cur.append(f)
            t_cur += t
        if cur:
            out.append(cur)
        return out

    def plan(self, frame_ids, use_gt_det=False, n_times=100):
        return _plan(self.ix, frame_ids, use_gt_det, n_times)

    def _batch_dict(self, plans, tracks, detections):
        """collate()'s key set (associator.py) around the two tensors, plus "scores", "global_track_ids" and "frames" per sample"""
        valid = [p["valid"] for p in plans]
        gt_masks = torch.zeros((sum(t for t, _ in valid), sum(n for _, n in valid)), dtype=torch.float)
        t0 = d0 = 0
        for t, n in valid:
            gt_masks[t0:t0 + t, d0:d0 + n] = 1
            t0, d0 = t0 + t, d0 + n
        return {"tracks": tracks, "detections": detections, "gt_matches": [p["match"] for p in plans], "gt_masks": gt_masks,
                "img_names": [self.ix.img_names[p["frame"]] for p in plans], "track_batch_split": [t for t, _ in valid],
                "detection_batch_split": [n for _, n in valid], "poses": [self.T_wcs[p["frame"]] for p in plans], "valid_list": valid,
                "scores": [p["scores"] for p in plans], "global_track_ids": [p["global_track_ids"] for p in plans],
                "frames": [p["frame"] for p in plans]}

    def cut_raw(self, plans, n_times=100):
        """the launch alone: (tracks [sum T, 79, n_times], detections [B, 79, 30], status [B] int32), all on the device, stream-ordered"""
        if self.device is None or not self._h:
            raise _lib.OdamError("SceneTable: no native store (device=None, or closed); use cut_host")
        B = len(plans)
        sum_t = sum(p["valid"][0] for p in plans)
        i32 = lambda xs: np.ascontiguousarray(np.concatenate(xs) if len(xs) else np.zeros(0), np.int32)
        frames = np.ascontiguousarray([p["frame"] for p in plans], np.int32)
        n_det = np.ascontiguousarray([p["valid"][1] for p in plans], np.int32)
        det_src = np.zeros((max(B, 1), MAX_DETS), np.int32)
        for b, p in enumerate(plans):
            det_src[b, :min(len(p["det_src"]), MAX_DETS)] = p["det_src"][:MAX_DETS]
        slot_sample = i32([np.full(p["valid"][0], b) for b, p in enumerate(plans)])
        slot_obj, slot_row0, slot_k = i32([p["track_objs"] for p in plans]), i32([p["row0"] for p in plans]), i32([p["k"] for p in plans])
        dev = self.device
        ok = 1 <= B <= MAX_BATCH and 1 <= sum_t <= MAX_SUM_T and 1 <= n_times <= 128      # (the library refuses the rest by name)
        with torch.cuda.device(dev):
            tracks = torch.empty((sum_t if ok else 0, 79, n_times), device=dev, dtype=torch.float32)
            dets = torch.empty((B if ok else 0, 79, MAX_DETS), device=dev, dtype=torch.float32)
            status = torch.empty(max(B, 1), device=dev, dtype=torch.int32)
            a = lambda x: x.ctypes.data if x.size else 16      # (a non-null address for an empty array: the sizes refuse the call)
            _lib.check(_lib.lib().odam_samples_cut(self._h, B, a(frames), a(n_det), a(det_src), sum_t, a(slot_sample), a(slot_obj), a(slot_row0),
                                                   a(slot_k), n_times, tracks.data_ptr() or 16, dets.data_ptr() or 16, status.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "odam_samples_cut")
        return tracks, dets, status[:B]

    def cut(self, frame_ids, use_gt_det=False, n_times=100):
        """The batch of `frame_ids` as Associator.__call__ takes it: collate()'s keys, "tracks" [sum T, 79, n_times] and "detections"
        [B, 79, 30] float32 DEVICE tensors built by one launch.  Raises AssertionError("wrong projected bbox") where the reference does."""
        t0 = time.perf_counter()
        plans = self.plan(frame_ids, use_gt_det, n_times)
        self.plan_seconds += time.perf_counter() - t0
        tracks, dets, status = self.cut_raw(plans, n_times)
        bad = np.flatnonzero(status.cpu().numpy() & 1)
        assert len(bad) == 0, "wrong projected bbox (frame %d)" % plans[int(bad[0])]["frame"]
        return self._batch_dict(plans, tracks, dets)

    def cut_host(self, frame_ids, use_gt_det=False, n_times=100):
        """cut() through numpy: the same plan, the arithmetic of channels(); host tensors, and "gt_scores" [sum T, sum n] with every
        sample's score block on the diagonal, as the reference's collater fills it (scan_net_track.py:72-83)"""
        plans = self.plan(frame_ids, use_gt_det, n_times)
        B = len(plans)
        ks = np.concatenate([p["k"] for p in plans]) if B else np.zeros(0, np.int64)
        row0 = np.concatenate([p["row0"] for p in plans]) if B else np.zeros(0, np.int64)
        objs = np.concatenate([p["track_objs"] for p in plans]) if B else np.zeros(0, np.int64)
        fr = np.concatenate([np.full(p["valid"][0], p["frame"], np.int64) for p in plans]) if B else np.zeros(0, np.int64)
        sum_t = len(ks)
        pb = self.proj[objs, fr]                                                   # [sum T, 4]
        bad = np.flatnonzero((pb == -1).all(axis=1))
        assert len(bad) == 0, "wrong projected bbox (frame %d)" % int(fr[bad[:1]].sum())
        box = np.clip(pb / self.wh, -1, 2)
        slot = np.repeat(np.arange(sum_t), ks)
        t = np.arange(len(slot)) - np.repeat(np.cumsum(ks) - ks, ks)              # time step of every kept row inside its slot
        tracks = np.full((sum_t, 79, n_times), -1.0, np.float32)
        tracks[slot, :, t] = channels(self.obs[np.repeat(row0, ks) + t], self.cam[fr[slot]], box[slot])
        dets = np.full((B, 79, MAX_DETS), -1.0, np.float32)
        for b, p in enumerate(plans):
            src = p["det_src"]
            if len(src) > MAX_DETS:
                raise _lib.OdamError(f"assoc_samples: frame {p['frame']} has {len(src)} detections (use_gt_det applies no cap), the batch holds 30")
            rows = np.where((src >= 0)[:, None], self.obs[np.maximum(src, 0)], self.ix.unm[np.maximum(-(src + 1), 0)] if len(self.ix.unm) else 0.0)
            dets[b, :, :len(src)] = channels(rows, self.cam[p["frame"]], rows[:, 2:6] / self.wh).T
        out = self._batch_dict(plans, torch.from_numpy(tracks), torch.from_numpy(dets))
        gt_scores = torch.zeros_like(out["gt_masks"])
        t0 = d0 = 0
        for p in plans:
            tt, n = p["valid"]
            gt_scores[t0:t0 + tt, d0:d0 + n] = torch.from_numpy(p["scores"])
            t0, d0 = t0 + tt, d0 + n
        out["gt_scores"] = gt_scores
        return out
