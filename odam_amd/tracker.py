"""Network-free association: the reference's IoU tracker (likojack/ODAM src/scripts/run_tracking.py:106-170 match_tracks, :37-52
convert_det_to_list, :55-103 init_tracks without its ORB / depth side data) with the frame loop of a whole sequence in ONE launch
(include/odam_track.h, csrc/track_iou.hip; restated in numpy by tests/track_iou_ref.py).

It needs no checkpoint: detect -> IouTracker -> optim_process -> merge_process -> evaluate runs with the detector's weights alone, and the
tracks it builds are the baseline the association network (odam_amd.associator) is compared with (evaluate.compare_maps).

The rule is the reference tracker's, decision for decision -- see odam_track.h for all of it.  Each detection of a frame, in descending
score order, scans the tracks in index order; a track updates the scan's state when its 2D and its 3D IoU both exceed the running maxima
(3D alone for a track last seen more than max_gap frame ids ago) and the classes agree; the detection joins the last track that did, if the
final maxima pass match_threshold (2D) or iou3d_threshold (3D); unmatched detections whose score is not below track_threshold start tracks.
Equal scores are taken by descending index (np.argsort(kind="stable")[::-1]; the reference's own order of ties is unspecified).  A NaN IoU
compares false and never matches, where the reference asserts.

The match confidence a caller gets instead of the network's score matrix: per detection the deciding (max_iou_2d, max_iou_3d).
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_DETS = 30
DET_COLS = 15
HEADER_WORDS = 8
MAX_TRACKS_LIMIT = 65536

_VP, _CI, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
TRACK_ARGTYPES = {
    "odam_track_iou_state_bytes": ([_CI], ctypes.c_longlong),
    "odam_track_iou_reset": ([_VP, _VP, _CI, _CI, _VP], _CI),
    "odam_track_iou_step": ([_VP, _CI, _VP, _CI, _VP, _VP, _VP, _VP, _D, _D, _D, _D, _D, _CI, _VP, _CI, _VP, _VP, _VP, _VP, _VP], _CI),
}


def _entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = TRACK_ARGTYPES[name]
    return f


class TrackOverflow(_lib.OdamError):
    """a frame would have taken a sequence past max_tracks: the kernel stopped before it.  `.frame` is the frame's index in the call's
    frame arrays, `.frame_id` its frame id, `.sequence` the sequence; `.outputs` the call's (ids, iou2d, iou3d), -1 from that frame on.
    The state is as after the frame before: reset() with a larger max_tracks, or go on with other frames."""

    def __init__(self, sequence, frame, frame_id, max_tracks, outputs):
        super().__init__(f"IouTracker: frame index {frame} (frame id {frame_id}) of sequence {sequence} would exceed max_tracks = {max_tracks}; "
                         "the sequence stopped before it")
        self.sequence, self.frame, self.frame_id, self.outputs = sequence, frame, frame_id, outputs


class IouTracker:
    iou_tracker = True      # what OdamProcess dispatches on (process_frames, process_frame -> _track_frames_iou)

    def __init__(self, match_threshold=0.5, track_threshold=0.8, iou3d_threshold=0.2, max_gap=5, max_tracks=1024, device="cuda:0", fitter=None):
        self.match_threshold = float(match_threshold)
        self.track_threshold = float(track_threshold)
        self.iou3d_threshold = float(iou3d_threshold)
        self.max_gap = int(max_gap)
        self.max_tracks = int(max_tracks)
        if not 1 <= self.max_tracks <= MAX_TRACKS_LIMIT:
            raise ValueError(f"max_tracks must be 1 .. {MAX_TRACKS_LIMIT}, got {max_tracks}")
        self.device = torch.device(device)
        self.fitter = fitter
        self._state = None
        self._n_seq = 0
        self._stepped = False
        self.n_tracks = []          # per sequence, after the last call

    def to(self, device):
        self.device = torch.device(device)
        self._state = None
        return self

    def eval(self):
        return self

    def _ctx(self):
        if self.fitter is None:
            from . import multi_view
            self.fitter = multi_view.default_fitter(str(self.device))
        if torch.device(self.fitter.device) != self.device:
            raise _lib.OdamError(f"IouTracker on {self.device} with a fitter context on {self.fitter.device}")
        return self.fitter._h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def state_bytes(self):
        b = _entry("odam_track_iou_state_bytes")(self.max_tracks)
        if b < 0:
            raise _lib.OdamError(f"odam_track_iou_state_bytes({self.max_tracks}) is invalid")
        return int(b)

    def reset(self, n_seq=1):
        """empty sequences: n_seq state blocks of capacity max_tracks (the buffer is allocated here, never inside a step)"""
        n_seq = int(n_seq)
        if n_seq < 1:
            raise ValueError("reset: at least one sequence")
        per = self.state_bytes()
        if self._state is None or self._state.numel() != n_seq * per or self._state.device != self.device:
            self._state = torch.empty(n_seq * per, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            _lib.check(_entry("odam_track_iou_reset")(self._ctx(), _lib.ptr(self._state), n_seq, self.max_tracks, self._stream()),
                       "odam_track_iou_reset")
        self._n_seq, self._stepped, self.n_tracks = n_seq, False, [0] * n_seq

    def header(self):
        """[n_seq, 3] int32 on the host: n_tracks, the overflow record of the last call (-1 = none), max_tracks"""
        per = self.state_bytes()
        return self._state.view(torch.int32).reshape(self._n_seq, per // 4)[:, :3].cpu().numpy()

    def _dev(self, x, dtype, shape):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=dtype))
        t = t.to(device=self.device, dtype=getattr(torch, np.dtype(dtype).name)).reshape(shape).contiguous()
        return t

    def step_scenes(self, blks, cnts, frame_ids, T_wcs, img_w, img_h):
        """The next frames of several sequences in ONE launch: lists with one entry per sequence (blk [N_s, 30, 15] float32, cnt [N_s]
        int32, frame ids [N_s], T_wc [N_s, 4, 4] float64; device tensors are taken as they are, host arrays are uploaded; N_s may be 0).
        The state holds len(blks) sequences: call reset(len(blks)) first (a tracker that has not stepped yet is reset here).
        Returns a list of (ids [N_s, 30] int32, iou2d, iou3d [N_s, 30] float64) device tensors; raises TrackOverflow for the first sequence
        that did not fit."""
        n_seq = len(blks)
        if not (len(cnts) == len(frame_ids) == len(T_wcs) == n_seq):
            raise ValueError("one entry per sequence in all four lists")
        if n_seq == 0:
            return []
        if self._state is None or (self._n_seq != n_seq and not self._stepped):
            self.reset(n_seq)
        if self._n_seq != n_seq:
            raise ValueError(f"the state holds {self._n_seq} sequences, the call has {n_seq}: reset({n_seq}) first")
        d_cnt = [self._dev(c, np.int32, (-1,)) for c in cnts]
        sizes = [int(c.shape[0]) for c in d_cnt]
        d_blk = [self._dev(b, np.float32, (-1, MAX_DETS, DET_COLS)) for b in blks]
        d_fid = [self._dev(f, np.int32, (-1,)) for f in frame_ids]
        d_T = [self._dev(T, np.float64, (-1, 4, 4)) for T in T_wcs]
        for s in range(n_seq):
            if not (d_blk[s].shape[0] == d_fid[s].shape[0] == d_T[s].shape[0] == sizes[s]):
                raise ValueError(f"sequence {s}: block, counts, frame ids and poses disagree about the number of frames")
        off = np.zeros(n_seq + 1, np.int64)
        off[1:] = np.cumsum(sizes)
        N = int(off[-1])
        if N >= 2 ** 31 // (MAX_DETS * DET_COLS):
            raise _lib.OdamError(f"{N} frames in one call: the offsets are 32-bit")
        one = lambda parts: parts[0] if n_seq == 1 else torch.cat(parts)
        blk, cnt, fid, T = one(d_blk), one(d_cnt), one(d_fid), one(d_T)
        d_off = torch.from_numpy(off.astype(np.int32)).to(self.device)
        ids = torch.full((max(N, 1), MAX_DETS), -1, device=self.device, dtype=torch.int32)
        iou2d = torch.full((max(N, 1), MAX_DETS), -1.0, device=self.device, dtype=torch.float64)
        iou3d = torch.full((max(N, 1), MAX_DETS), -1.0, device=self.device, dtype=torch.float64)
        n_tracks = torch.empty(n_seq, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(_entry("odam_track_iou_step")(
                self._ctx(), n_seq, _lib.ptr(d_off), N, _lib.ptr(blk), _lib.ptr(cnt), _lib.ptr(fid), _lib.ptr(T), float(img_w), float(img_h),
                self.match_threshold, self.track_threshold, self.iou3d_threshold, self.max_gap, _lib.ptr(self._state), self.max_tracks,
                _lib.ptr(ids), _lib.ptr(iou2d), _lib.ptr(iou3d), _lib.ptr(n_tracks), self._stream()), "odam_track_iou_step")
        self._stepped = True
        out = [(ids[off[s]:off[s + 1]], iou2d[off[s]:off[s + 1]], iou3d[off[s]:off[s + 1]]) for s in range(n_seq)]
        hdr = self.header()                       # the one read-back of a call: 12 bytes per sequence
        self.n_tracks = [int(x) for x in hdr[:, 0]]
        for s in range(n_seq):
            if hdr[s, 1] == -2 or hdr[s, 2] != self.max_tracks:
                raise _lib.OdamError(f"IouTracker: the state block of sequence {s} was not reset for max_tracks = {self.max_tracks}")
            if hdr[s, 1] >= 0:
                f = int(hdr[s, 1]) - int(off[s])
                raise TrackOverflow(s, f, int(d_fid[s][f].item()), self.max_tracks, out[s])
        return out

    def step(self, blk, cnt, frame_ids, T_wcs, img_w, img_h):
        """The next frames of the one sequence, in one launch: blk [N, 30, 15] float32 + cnt [N] int32 (parallel.pack_detections /
        OdamProcess.detect_frames_packed), frame ids [N], T_wc [N, 4, 4] float64.  Returns device tensors (ids [N, 30] int32: track id of
        every detection slot, -1 = dropped or unused; iou2d, iou3d [N, 30] float64: the deciding maxima, -1 where the scan never updated).
        The state persists: a scene fed in chunks continues where it stopped.  Raises TrackOverflow with the frame index when a frame
        would exceed max_tracks."""
        if self._state is not None and self._n_seq != 1 and not self._stepped:
            self.reset(1)
        return self.step_scenes([blk], [cnt], [frame_ids], [T_wcs], img_w, img_h)[0]


def build(args=None):
    """beside associator.build: the tracker from a config (dict or namespace) with any of match_threshold, track_threshold,
    iou3d_threshold, max_gap, max_tracks, device; the reference's defaults (run_tracking.py:357-359) otherwise"""
    g = (lambda k: args[k]) if isinstance(args, dict) else (lambda k: getattr(args, k))
    kw = {}
    for k in ("match_threshold", "track_threshold", "iou3d_threshold", "max_gap", "max_tracks", "device"):
        try:
            kw[k] = g(k)
        except (KeyError, AttributeError, TypeError):
            pass
    return IouTracker(**kw)
