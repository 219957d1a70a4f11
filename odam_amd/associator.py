"""Host side of the association network: drop-in for the reference's Associator object as OdamProcess calls it
(likojack/ODAM src/models/associator.py:163-268, src/processor.py:327-341):
    out = associator(data, match_threshold, eval_only=True)
    out["matches"][0]  -> track id per detection (-1 = new track)      (hungarian_matching, :19-35)
    out["pred"][0][0]  -> log assignment [(T+1), (n_det+1)] tensor      (log_optimal_transport, :283-298)
The network forward and the 100 Sinkhorn iterations run in the gfx950 library (include/odam_assoc.h).  The Hungarian step is scipy's on
the host, exactly as the reference does (odam_config assoc.hungarian = 0, the default), or the library's (assoc.hungarian = 1:
odam_assoc_hungarian restates scipy's shortest-augmenting-path solver with its tie order on one wavefront, launched behind the Sinkhorn
loop; same matching on every fixture and on matrices full of ties -- tests/test_assoc_gpu.py -- but 0.01 ms per frame slower, because the
host has to wait for the device either way)."""
import contextlib
import ctypes
import math

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import _lib


def hungarian_matching(scores, matching_threshold):  # associator.py:19-35
    scores = scores.detach().cpu().numpy()
    match = np.zeros(scores.shape[1]) - 1
    rows, cols = linear_sum_assignment(1 - scores)
    for r, c in zip(rows, cols):
        if scores[r, c] > matching_threshold:
            match[c] = r
    return match


class TrackWindows:
    """Device-resident observations of the live tracks (include/odam_assoc.h, odam_trackwin_*): what
    OdamProcess._preprocess_tracks (src/processor.py:133-170) rebuilds on the host every frame is built by one launch here."""

    WINDOW = 100

    def __init__(self, device="cuda:0", max_tracks=1024):
        self.device = torch.device(device)
        self.max_tracks = max_tracks
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().odam_trackwin_create(max_tracks, self.WINDOW, ctypes.byref(self._h)), "odam_trackwin_create")
        self.lengths = []           # observations per track, as appended (the host's check against its own track list)
        self.marks = np.zeros((0, 3))      # per track: frame id of its first observation, frame id and world x of its last -- see in_step()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().odam_trackwin_reset(self._h, self._stream()), "odam_trackwin_reset")
        self.lengths = []
        self.marks = np.zeros((0, 3))

    @staticmethod
    def _marks_of(tracks):
        """[T, 3] float64: frame id of the first observation, frame id and world x of the last one (one pass over the list)"""
        n = len(tracks)
        out = np.empty((n, 3))
        out[:, 0] = np.fromiter((t[0, 0] for t in tracks), np.float64, n)
        out[:, 1] = np.fromiter((t[-1, 0] for t in tracks), np.float64, n)
        out[:, 2] = np.fromiter((t[-1, 9] for t in tracks), np.float64, n)
        return out

    def in_step(self, tracks):
        """True when the mirror holds exactly `tracks` as far as the host can tell without reading rows back: the same number of
        observations per track AND the same first / last observation (frame ids, world x of the last one) -- a track list that was
        replaced or edited at equal lengths (a restore, a test) is caught as well."""
        if [len(t) for t in tracks] != self.lengths:
            return False
        return len(tracks) == 0 or np.array_equal(self._marks_of(tracks), self.marks[:len(tracks)])

    def load(self, tracks):
        """(re)build the mirror from a host track list in one upload (include/odam_assoc.h, odam_trackwin_load)"""
        T = len(tracks)
        if T > self.max_tracks:
            raise _lib.OdamError(f"TrackWindows: {T} tracks exceed the store's {self.max_tracks}")
        lens = np.ascontiguousarray([len(t) for t in tracks], np.int32)
        tails = [np.asarray(t, np.float64)[-self.WINDOW:, :14] for t in tracks if len(t)]
        rows = np.ascontiguousarray(np.concatenate(tails, axis=0)) if tails else np.zeros((0, 14))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().odam_trackwin_load(self._h, ctypes.c_int(T), lens.ctypes.data_as(ctypes.c_void_p),
                                                     rows.ctypes.data_as(ctypes.c_void_p), self._stream()), "odam_trackwin_load")
        self.lengths = lens.tolist()
        if any(n == 0 for n in self.lengths):
            raise _lib.OdamError("TrackWindows: a track without observations")
        self.marks = self._marks_of(tracks)
        # ... and the store's running sums (odam_trackwin_load_sums): dims, centre and azimuth of EVERY observation
        cols = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64)[:, 6:13] for t in tracks], axis=0)) if T else np.zeros((0, 7))
        _lib.check(_lib.lib().odam_trackwin_load_sums(self._h, ctypes.c_int(T), lens.ctypes.data_as(ctypes.c_void_p),
                                                      cols.ctypes.data_as(ctypes.c_void_p)), "odam_trackwin_load_sums")

    def append(self, track_ids, rows82):
        """rows82 [n, 82] float64 track rows (processor.py:98-108); track_ids [n]: existing index or len(lengths) + j for new ones"""
        rows = np.ascontiguousarray(np.asarray(rows82, np.float64)[:, :14])
        ids = np.ascontiguousarray(track_ids, np.int32)
        for i0 in range(0, len(ids), 32):
            n = min(32, len(ids) - i0)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().odam_trackwin_append(self._h, ctypes.c_int(n), ids[i0:].ctypes.data_as(ctypes.c_void_p),
                                                           rows[i0:].ctypes.data_as(ctypes.c_void_p), self._stream()), "odam_trackwin_append")
        r = np.asarray(rows82, np.float64)
        n_new = int((ids >= len(self.lengths)).sum())
        if n_new:
            self.marks = np.concatenate([self.marks, np.zeros((n_new, 3))])
        for t, row in zip(ids.tolist(), r):
            if t == len(self.lengths):
                self.lengths.append(1)
                self.marks[t, 0] = row[0]
            else:
                self.lengths[t] += 1
            self.marks[t, 1] = row[0]; self.marks[t, 2] = row[9]

    def append_raw(self, track_ids, rows82):
        """append() without the host-side lengths / marks: OdamProcess's fast path keeps those stale while it runs and rebuilds them from
        its track list when somebody looks (processor.py::_sync_host_view)"""
        rows = np.ascontiguousarray(np.asarray(rows82, np.float64)[:, :14])
        ids = np.ascontiguousarray(track_ids, np.int32)
        for i0 in range(0, len(ids), 32):
            n = min(32, len(ids) - i0)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().odam_trackwin_append(self._h, ctypes.c_int(n), ids[i0:].ctypes.data_as(ctypes.c_void_p),
                                                           rows[i0:].ctypes.data_as(ctypes.c_void_p), self._stream()), "odam_trackwin_append")

    def build(self, proj_px_dev, T_cw, cam_azi, img_w, img_h):
        T = len(self.lengths)
        out = torch.empty(T, 79, self.WINDOW, device=self.device, dtype=torch.float32)
        cam = np.ascontiguousarray(np.concatenate([np.asarray(T_cw, np.float64)[:3].reshape(-1), [cam_azi, img_w, img_h]]))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().odam_trackwin_build(self._h, ctypes.c_int(T), _lib.ptr(proj_px_dev), cam.ctypes.data_as(ctypes.c_void_p),
                                                      _lib.ptr(out), self._stream()), "odam_trackwin_build")
        return out

    def params(self):
        """[T, 9] float32 parameter rows of the track surfaces from the store's running sums (odam_trackwin_params) -- what
        OdamProcess._prepare_tracks computes from the host track list (src/processor.py:172-180), bit for bit"""
        T = len(self.lengths)
        out = np.zeros((T, 9), np.float32)
        _lib.check(_lib.lib().odam_trackwin_params(self._h, ctypes.c_int(T), out.ctypes.data_as(ctypes.c_void_p)), "odam_trackwin_params")
        return out

    def close(self):
        if self._h:
            _lib.lib().odam_trackwin_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Associator:
    native_windows = True       # OdamProcess may hand this associator a device tensor built by TrackWindows

    def __init__(self, config=None, max_tracks=256, device="cuda:0"):
        cfg = config or {"GNN_layers": ["self", "cross"] * 6, "self_GNN_layers": ["self"] * 4, "sinkhorn_iterations": 100}
        self.gnn_layers = list(cfg["GNN_layers"])
        self.n_self = len(cfg["self_GNN_layers"])
        self.iters = int(cfg["sinkhorn_iterations"])
        self.max_tracks = max_tracks
        self.device = torch.device(device)
        self._h = None
        self._sd = None
        self.lost_launches = 0      # frames whose persistent matching launch was abandoned and re-run (see assignment_checked)
        self._lost_seen = 0

    def to(self, device):
        self.device = torch.device("cuda:0" if str(device) == "cuda" else device)
        return self

    def cuda(self):
        return self.to("cuda:0")

    def eval(self):
        return self

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in sd.items() if torch.is_tensor(v)}
        self.close()
        return self

    def close(self):
        if self._h:
            _lib.lib().odam_assoc_destroy(self._h)
            self._h = None
            self._lost_seen = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h:
            return self._h
        if self._sd is None:
            raise _lib.OdamError("Associator: load_state_dict() first")
        L = _lib.lib()
        h = ctypes.c_void_p()
        cross = (ctypes.c_int * len(self.gnn_layers))(*[1 if n == "cross" else 0 for n in self.gnn_layers])
        with torch.cuda.device(self.device):
            _lib.check(L.odam_assoc_create(self.max_tracks, self.n_self, cross, len(self.gnn_layers), self.iters,
                                           ctypes.byref(h)), "odam_assoc_create")
            try:
                tensors = dict(self._sd)
                # PositionalEncoding.div_term (associator.py:320), torch CPU float32 ops
                tensors["pe_div_term"] = torch.exp(torch.arange(0, 256, 2).float() * (-math.log(10000.0) / 256))
                for name, t in tensors.items():
                    t = t.reshape(t.shape[0], t.shape[1]) if t.dim() == 3 else t     # Conv1d weight [N, K, 1]
                    t = t.contiguous()
                    shape = (ctypes.c_longlong * max(t.dim(), 1))(*t.shape)
                    _lib.check(L.odam_assoc_set_weight(h, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()),
                               f"odam_assoc_set_weight({name})")
                _lib.check(L.odam_assoc_finalize(h), "odam_assoc_finalize")
            except Exception:
                L.odam_assoc_destroy(h)      # a half-built handle is not kept
                raise
        self._h = h
        return h

    MAX_TRACKS = 1024      # odam_assoc_create's limit (the Sinkhorn kernel keeps the whole matrix in LDS)

    def _grow(self, n_tracks):
        """the reference has no track limit (associator.py:202-268): the native workspace is sized per handle, so a scene
        with more live tracks gets a new handle with at least twice the room (weights are kept in self._sd)"""
        if n_tracks > self.MAX_TRACKS:
            raise _lib.OdamError(f"Associator: {n_tracks} live tracks exceed the native limit of {self.MAX_TRACKS}")
        old, old_h = self.max_tracks, self._h
        self.max_tracks = min(self.MAX_TRACKS, max(n_tracks, 2 * self.max_tracks))
        torch.cuda.synchronize(self.device)
        self._h = None
        try:
            self._handle()
        except Exception:
            self.max_tracks, self._h = old, old_h      # the old handle stays usable for smaller frames
            raise
        if old_h:
            _lib.lib().odam_assoc_destroy(old_h)
        self._lost_seen = 0

    def set_persistent(self, on):
        """matching GNN as one persistent launch (the default where the device can hold its 256 workgroups at once) or as the launch
        sequence.  A caller that runs the association on a stream restricted to a share of the compute units
        (hipExtStreamCreateWithCUMask; tests/native/cumask_probe.hip) should switch the persistent launch off: its workgroups wait for each other and would
        never all become resident (the bounded wait would abandon every launch and re-run it through the sequence)."""
        _lib.check(_lib.lib().odam_assoc_set_persistent(self._handle(), ctypes.c_int(1 if on else 0)), "odam_assoc_set_persistent")

    def assignment(self, tracks, detections, n_tracks, n_det, sequence=False, threshold=None):
        """tracks [T,79,100], detections [1,79,30] or [79,30] (any device) -> Z [(T+1),(n_det+1)] device tensor.
        Stream-ordered; sequence=True takes the launch-sequence path (no device-wide barrier).

        This is the RAW entry: an abandoned persistent launch (include/odam_assoc.h) leaves Z all NaN and is reported only
        through odam_assoc_lost_launches -- use assignment_checked() (what __call__ does) unless the caller synchronises and
        checks that counter itself, as the timing scripts do.  A loss taken here is attributed to the next checked call."""
        dev = self.device
        if n_tracks > self.max_tracks:
            self._grow(n_tracks)
        tr = tracks.to(dev, torch.float32).contiguous()
        _pinned = getattr(self, "_pin_mode", False) and (not detections.is_cuda) and detections.dtype == torch.float32
        if _pinned:
            # (inside assignment_checked only.)  The kernels read the detections from, and write Z to, pinned host memory themselves --
            # no copy command either way; this call then waits for the stream itself, so what it returns is valid host data and the
            # two buffers are free for the next frame
            if getattr(self, "_pin", None) is None:
                self._pin = (torch.empty(79 * 30, dtype=torch.float32).pin_memory(), torch.empty((self.MAX_TRACKS + 1) * 31, dtype=torch.float32).pin_memory())
            de = self._pin[0].view(79, 30)
            de.copy_(detections.reshape(79, 30))
            Z = self._pin[1][:(n_tracks + 1) * (n_det + 1)].view(n_tracks + 1, n_det + 1)
        else:
            de = detections.to(dev, torch.float32).reshape(79, 30).contiguous()
            Z = torch.empty(n_tracks + 1, n_det + 1, device=dev, dtype=torch.float32)
        L = _lib.lib()
        fn, what = (L.odam_assoc_forward_sequence, "odam_assoc_forward_sequence") if sequence else (L.odam_assoc_forward, "odam_assoc_forward")
        with torch.cuda.device(dev):
            _lib.check(fn(self._handle(), _lib.ptr(tr), ctypes.c_int(n_tracks), _lib.ptr(de), ctypes.c_int(n_det), _lib.ptr(Z),
                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), what)
            self._match = None
            if threshold is not None and _lib.get_config("assoc.hungarian") and min(n_tracks, n_det) <= 32 and max(n_tracks, n_det) <= 128 \
                    and n_det <= 31:      # the pinned result is 31 match words + the status word
                # the Hungarian step behind the Sinkhorn loop on the same stream: match [n_det] + status into pinned memory next to Z
                if getattr(self, "_pin_match", None) is None:
                    self._pin_match = torch.empty(32, dtype=torch.int32).pin_memory()
                _lib.check(L.odam_assoc_hungarian(_lib.ptr(Z), ctypes.c_int(n_tracks), ctypes.c_int(n_det), ctypes.c_int(n_det + 1),
                                                  ctypes.c_double(float(threshold)), ctypes.c_int(1), _lib.ptr(self._pin_match),
                                                  ctypes.c_void_p(self._pin_match.data_ptr() + 4 * 31),
                                                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "odam_assoc_hungarian")
                self._match = (self._pin_match, n_det)
        if _pinned or self._match is not None:
            torch.cuda.current_stream(dev).synchronize()
        return Z

    def assignment_checked(self, tracks, detections, n_tracks, n_det, threshold=None):
        """assignment() + synchronisation + the lost-launch check: if the persistent matching kernel could not get all its
        workgroups resident within the barrier bound (a foreign kernel held the CUs), this frame is run again through the
        launch sequence in the same process and counted in self.lost_launches.  The reference cannot fail this way
        (associator.py:202-268), so neither may the drop-in.  Returns Z on the host when the detections came from the host (the
        kernels then read them from, and write Z to, pinned memory: no copy commands), on the device otherwise."""
        self._pin_mode = True
        try:
            Z = self.assignment(tracks, detections, n_tracks, n_det, threshold=threshold)
            torch.cuda.current_stream(self.device).synchronize()
            n = ctypes.c_uint(0)
            _lib.check(_lib.lib().odam_assoc_lost_launches(self._handle(), ctypes.byref(n)), "odam_assoc_lost_launches")
            if n.value != self._lost_seen:
                self._lost_seen = n.value
                self.lost_launches += 1
                self._lost_in_a_row = getattr(self, "_lost_in_a_row", 0) + 1
                Z = self.assignment(tracks, detections, n_tracks, n_det, sequence=True, threshold=threshold)
                torch.cuda.current_stream(self.device).synchronize()
                if self._lost_in_a_row >= 3:
                    # three abandoned launches in a row are not a busy device but a condition that will not pass (the row-partitioned
                    # kernel's placement check, a stream confined to a share of the compute units): stay on the launch sequence
                    self.set_persistent(False)
                    self.persistent_given_up = True
            else:
                self._lost_in_a_row = 0
        finally:
            self._pin_mode = False
        return Z if Z.is_cuda else Z.clone()      # (the pinned buffer is the next frame's)

    # ---- one frame's device work behind one native call (include/odam_assoc.h, odam_assoc_step) -------------------------------------
    def step_launch(self, win, fitter, app_ids, app_rows14, n_tracks, cam21, cam_azi, img_w, img_h, det32T):
        """Enqueue, for one frame: the mirror append of what the previous frame attached (app_ids / app_rows14, may be empty), the
        track input for this frame's camera and the association forward on it -- OdamProcess's fast path (processor.py::process_frames).
        det32T [79, n_det] float32 (the frame's detection rows transposed, as process_frame hands them to the collater).  Nothing is
        synchronised here; step_finish() waits and returns the log assignment."""
        dev = self.device
        n_det = det32T.shape[1]
        if n_tracks > self.max_tracks:
            self._grow(n_tracks)
        if getattr(self, "_pin", None) is None:
            self._pin = (torch.empty(79 * 30, dtype=torch.float32).pin_memory(), torch.empty((self.MAX_TRACKS + 1) * 31, dtype=torch.float32).pin_memory())
        de = self._pin[0].view(79, 30).numpy()
        de[:, n_det:] = -1.0                      # the collater's padding (processor.py:49-68)
        de[:, :n_det] = det32T
        buf = getattr(self, "_tracks_buf", None)
        if buf is None or buf.shape[0] < n_tracks:
            self._tracks_buf = buf = torch.empty(max(64, 2 * n_tracks), 79, TrackWindows.WINDOW, device=dev, dtype=torch.float32)
        L = _lib.lib()
        n_app = len(app_ids)
        ids = np.ascontiguousarray(app_ids, np.int32)
        rows = np.ascontiguousarray(app_rows14, np.float64)
        # (per-frame host cost matters here -- the device is idle until the call below: the device context is entered only when another
        # device is current, and the completion event is one object, recorded again every frame)
        dev_t = torch.device(dev)
        ctx = torch.cuda.device(dev_t) if torch.cuda.current_device() != (dev_t.index or 0) else contextlib.nullcontext()
        with ctx, fitter._lock:
            cur = torch.cuda.current_stream(dev_t)
            stream = cur.cuda_stream
            if fitter._last is not None and fitter._last[0] != stream:
                cur.wait_event(fitter._last[1])
            _lib.check(L.odam_assoc_step(self._handle(), win._h, fitter._h, ctypes.c_int(n_app), ctypes.c_void_p(ids.ctypes.data),
                                         ctypes.c_void_p(rows.ctypes.data), ctypes.c_int(n_tracks), ctypes.c_void_p(cam21.ctypes.data),
                                         ctypes.c_double(cam_azi), ctypes.c_double(img_w), ctypes.c_double(img_h), _lib.ptr(self._pin[0]),
                                         ctypes.c_int(n_det), _lib.ptr(buf), _lib.ptr(self._pin[1]), ctypes.c_void_p(stream)), "odam_assoc_step")
            ev = getattr(self, "_step_ev", None)
            if ev is None:
                ev = self._step_ev = torch.cuda.Event()
            ev.record(cur)
            fitter._last = (stream, ev)
        self._step = (n_tracks, n_det, fitter)

    def step_finish(self):
        """Wait for the frame enqueued by step_launch and return its log assignment [(T + 1), (n_det + 1)] -- a view of the pinned buffer,
        valid until the next step_launch.  An abandoned persistent launch is re-run through the launch sequence, as in assignment_checked."""
        n_tracks, n_det, fitter = self._step
        dev = self.device
        cur = torch.cuda.current_stream(dev)
        cur.synchronize()
        fitter._last = None                    # synchronised: no cross-stream wait is owed
        n = ctypes.c_uint(0)
        _lib.check(_lib.lib().odam_assoc_lost_launches(self._handle(), ctypes.byref(n)), "odam_assoc_lost_launches")
        if n.value != self._lost_seen:
            self._lost_seen = n.value
            self.lost_launches += 1
            self._lost_in_a_row = getattr(self, "_lost_in_a_row", 0) + 1
            self._pin_mode = True
            try:
                self.assignment(self._tracks_buf[:n_tracks], self._pin[0].view(79, 30), n_tracks, n_det, sequence=True)
                cur.synchronize()
            finally:
                self._pin_mode = False
            if self._lost_in_a_row >= 3:
                self.set_persistent(False)
                self.persistent_given_up = True
        else:
            self._lost_in_a_row = 0
        return self._pin[1][:(n_tracks + 1) * (n_det + 1)].view(n_tracks + 1, n_det + 1)

    def __call__(self, in_data, threshold, eval_only=False, device="cuda"):
        """Associator.forward (associator.py:202-268) for any batch: in_data["tracks"] [sum T, 79, 100], ["detections"] [B, 79, 30],
        ["valid_list"] [(T_b, n_det_b)] * B and, unless eval_only, ["gt_matches"] [[k_b, 2] (track, detection) index pairs] * B, where -1
        (like T_b / n_det_b) names the dustbin.  Returns "pred" [Z_b[None]] * B, "loss" (0-dim float64 tensor: sum over the samples of
        sum_pairs -Z_b[track, detection]), "matches" [per detection: track id, -1 = new] * B and "loss_terms" (float64 [B]).
        The batch-of-one inference call of OdamProcess (eval_only=True) keeps its own path: the persistent matching kernel."""
        valid = in_data["valid_list"]
        if len(valid) != 1 or not eval_only:
            return self._call_batch(in_data, threshold, eval_only)
        n_tracks, n_det = valid[0]
        # ONE download of the log assignment: both consumers -- the Hungarian step here and process_frame's score matrix
        # (processor.py:337-339: predictions['pred'][0][0].cpu().exp()) -- read it on the host
        self._match = None      # (set by assignment() when the Hungarian step ran on the device behind it)
        Z = self.assignment_checked(in_data["tracks"], in_data["detections"][0], n_tracks, n_det, threshold=threshold).cpu()
        pred = [Z[None]]
        m = getattr(self, "_match", None)
        if m is not None and int(m[0][31]) == 0:      # solved on the device behind the Sinkhorn loop (status word 0)
            match = [m[0][:n_det].numpy().astype(np.float64)]
        else:
            match = [hungarian_matching(Z[:-1, :-1].exp(), threshold)]
        return {"pred": pred, "loss": 0, "matches": match}

    MAX_BATCH = 64         # odam_assoc_forward_batch's limits (include/odam_assoc.h)
    MAX_DETS = 30

    def forward_batch(self, tracks, detections, valid_list, gt_matches=None):
        """The batched forward on the device, stream-ordered (odam_assoc_forward_batch): -> (Z flat float32 device tensor, Z_off
        [B + 1] element offsets of the dense (T_b + 1) x (n_b + 1) blocks, loss_terms float64 [B] device, status int32 [B] device).
        gt_matches None: no pairs (the loss terms are 0)."""
        dev = self.device
        valid = [(int(t), int(n)) for t, n in valid_list]
        B = len(valid)
        sum_t, t_max = sum(t for t, _ in valid), max([t for t, _ in valid] + [1])
        tr = tracks.to(dev, torch.float32).contiguous()
        de = detections.to(dev, torch.float32).contiguous()
        if tuple(tr.shape) != (sum_t, 79, TrackWindows.WINDOW) or tuple(de.shape) != (B, 79, self.MAX_DETS):
            raise _lib.OdamError(f"Associator: tracks {tuple(tr.shape)} / detections {tuple(de.shape)} do not fit valid_list "
                                 f"({sum_t} tracks, {B} samples): expected [{sum_t}, 79, 100] and [{B}, 79, 30]")
        T = np.ascontiguousarray([t for t, _ in valid], np.int32)
        n = np.ascontiguousarray([k for _, k in valid], np.int32)
        gt = gt_off = None
        if gt_matches is not None:
            if len(gt_matches) != B:
                raise _lib.OdamError(f"Associator: {len(gt_matches)} gt_matches for {B} samples")
            pairs = [np.asarray(g.cpu() if torch.is_tensor(g) else g).astype(np.int32).reshape(-1, 2) for g in gt_matches]
            gt = np.ascontiguousarray(np.concatenate(pairs, axis=0) if pairs else np.zeros((0, 2)), np.int32)
            if gt.shape[0] == 0:
                gt = np.zeros((1, 2), np.int32)      # (a non-null address; gt_off says it holds nothing)
            gt_off = np.ascontiguousarray(np.r_[0, np.cumsum([len(p) for p in pairs])], np.int32)
        z_off = np.ascontiguousarray(np.r_[0, np.cumsum([(t + 1) * (k + 1) for t, k in valid])], np.int64)
        if 1 <= sum_t <= self.MAX_TRACKS and sum_t > self.max_tracks:
            self._grow(sum_t)
        h = self._handle()
        L = _lib.lib()
        addr = lambda a: None if a is None else a.ctypes.data
        with torch.cuda.device(dev):
            if 1 <= B <= self.MAX_BATCH and t_max <= self.MAX_TRACKS and B * (t_max + self.MAX_DETS) > (self._batch_rows if getattr(self, "_batch_h", None) is h else 0):
                # the padded block's workspaces, sized the way _grow sizes the handle: at least twice the room that ran out
                b_cap, t_cap = getattr(self, "_batch_cap", (0, 0))
                b_cap, t_cap = min(self.MAX_BATCH, max(B, b_cap)), min(self.MAX_TRACKS, max(t_max, t_cap))
                _lib.check(L.odam_assoc_reserve_batch(h, b_cap, t_cap), "odam_assoc_reserve_batch")
                self._batch_cap, self._batch_rows, self._batch_h = (b_cap, t_cap), b_cap * (t_cap + self.MAX_DETS), h
            Z = torch.empty(max(int(z_off[-1]), 1), device=dev, dtype=torch.float32)
            terms = torch.zeros(max(B, 1), device=dev, dtype=torch.float64)
            status = torch.zeros(max(B, 1), device=dev, dtype=torch.int32)
            _lib.check(L.odam_assoc_forward_batch(h, tr.data_ptr(), addr(T), de.data_ptr(), addr(n), B, addr(gt), addr(gt_off), Z.data_ptr(),
                                                  addr(z_off), terms.data_ptr(), status.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "odam_assoc_forward_batch")
        return Z, z_off, terms[:B], status[:B]

    def _call_batch(self, in_data, threshold, eval_only):
        if "valid_list" not in in_data or (not eval_only and "gt_matches" not in in_data):
            raise KeyError("Associator: valid_list is required, and gt_matches unless eval_only")
        valid = [(int(t), int(n)) for t, n in in_data["valid_list"]]
        B = len(valid)
        dev = self.device
        Z, z_off, terms, status = self.forward_batch(in_data["tracks"], in_data["detections"], valid, None if eval_only else in_data["gt_matches"])
        # matches: with assoc.hungarian = 1 the samples inside the device solver's 32 x 128 are solved behind the transport, one wavefront
        # each; every other sample by scipy on the host, from the one download of all Z blocks below
        on_device = []
        if _lib.get_config("assoc.hungarian"):
            on_device = [b for b, (t, n) in enumerate(valid) if min(t, n) <= 32 and max(t, n) <= 128]
        if on_device:
            pin = torch.empty(B * 33, dtype=torch.int32).pin_memory()      # 32 match words + the status word per sample
            L = _lib.lib()
            with torch.cuda.device(dev):
                stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                for b in on_device:
                    t, n = valid[b]
                    _lib.check(L.odam_assoc_hungarian(ctypes.c_void_p(Z.data_ptr() + 4 * int(z_off[b])), ctypes.c_int(t), ctypes.c_int(n),
                                                      ctypes.c_int(n + 1), ctypes.c_double(float(threshold)), ctypes.c_int(1),
                                                      ctypes.c_void_p(pin.data_ptr() + 4 * 33 * b), ctypes.c_void_p(pin.data_ptr() + 4 * (33 * b + 32)),
                                                      stream), "odam_assoc_hungarian")
        Zh, terms_h, status_h = Z.cpu(), terms.cpu(), status.cpu()      # (synchronises the stream)
        torch.cuda.current_stream(dev).synchronize()
        pred, matches = [], []
        for b, (t, n) in enumerate(valid):
            if int(status_h[b]) & 1:
                raise ValueError(f"Associator: the log assignment of sample {b} ({t} tracks, {n} detections) holds a NaN")
            if int(status_h[b]):
                raise _lib.OdamError(f"Associator: sample {b} was refused by odam_assoc_ot_batch (status {int(status_h[b])})")
            Zb = Zh[int(z_off[b]):int(z_off[b + 1])].view(t + 1, n + 1)
            pred.append(Zb[None])
            if b in on_device and int(pin[33 * b + 32]) == 0:
                matches.append(pin[33 * b:33 * b + n].numpy().astype(np.float64))
            else:
                matches.append(hungarian_matching(Zb[:-1, :-1].exp(), threshold))
        total = 0.0
        for x in terms_h.tolist():      # in sample order: loss == sum(loss_terms)
            total += x
        return {"pred": pred, "loss": torch.tensor(total, dtype=torch.float64), "matches": matches, "loss_terms": terms_h}

    forward = __call__


def collate(data_list):
    """The reference's collater (src/scripts/run_association.py:68-123, src/datasets/scan_net_track.py): samples
    {"tracks" [T, 79, 100], "detections" [79, n <= 30], "match" [k, 2], "img_path", "pose"} -> one batch with its key set.  The
    detection slots past n are padded with -1 up to max_dets = 30; gt_masks [sum T, sum n] is 1 inside every sample's own block."""
    max_dets = Associator.MAX_DETS
    B = len(data_list)
    n_features = data_list[0]["detections"].shape[0]
    detections = torch.full((B, n_features, max_dets), -1.0, dtype=torch.float)
    track_split = [int(d["tracks"].shape[0]) for d in data_list]
    det_split = [int(d["detections"].shape[1]) for d in data_list]
    for b, d in enumerate(data_list):
        detections[b, :, :det_split[b]] = torch.as_tensor(d["detections"], dtype=torch.float)
    gt_masks = torch.zeros((sum(track_split), sum(det_split)), dtype=torch.float)
    t0 = d0 = 0
    for nt, nd in zip(track_split, det_split):
        gt_masks[t0:t0 + nt, d0:d0 + nd] = 1
        t0, d0 = t0 + nt, d0 + nd
    return {"tracks": torch.cat([torch.as_tensor(d["tracks"]) for d in data_list], dim=0),
            "detections": detections,
            "gt_matches": [d["match"] for d in data_list],
            "gt_masks": gt_masks,
            "img_names": [d.get("img_path") for d in data_list],
            "track_batch_split": track_split,
            "detection_batch_split": det_split,
            "poses": [d.get("pose") for d in data_list],
            "valid_list": list(zip(track_split, det_split))}


def gt_track_of_detections(match, n_tracks, n_det):
    """[n_det] ground-truth track of every detection from the (track, detection) pairs of a sample: -1 (new) where the pair names the
    track dustbin (-1 or n_tracks) or no pair names the detection; pairs on the detection dustbin say nothing about a detection"""
    out = np.full(n_det, -1.0)
    for t, d in np.asarray(match).reshape(-1, 2).astype(np.int64):
        if 0 <= d < n_det:
            out[d] = t if 0 <= t < n_tracks else -1
    return out


def validate(model, samples, threshold, batch_size):
    """Scores `model` (an Associator with its weights loaded) on recorded samples (collate()'s input) in batches of batch_size:
    "loss" = the mean over the samples of sum_pairs -Z[track, detection] -- the unit of the reference's training log per sample --, "accuracy"
    = the share of detections whose predicted track equals the ground-truth track (-1 = new); per sample: "loss_terms", "correct", "n_det"."""
    terms, correct, n_dets = [], [], []
    for i0 in range(0, len(samples), batch_size):
        chunk = samples[i0:i0 + batch_size]
        batch = collate(chunk)
        out = model(batch, threshold, eval_only=False)
        terms += out["loss_terms"].tolist()
        for (t, n), match, pred in zip(batch["valid_list"], batch["gt_matches"], out["matches"]):
            correct.append(int((np.asarray(pred) == gt_track_of_detections(match, t, n)).sum()))
            n_dets.append(n)
    return {"loss": float(np.sum(terms) / max(len(terms), 1)), "accuracy": float(sum(correct) / max(sum(n_dets), 1)),
            "loss_terms": terms, "correct": correct, "n_det": n_dets}


def validate_scene(model, scene, threshold, batch_size=16, frames=None, use_gt_det=False):
    """validate() on a labelled scene (assoc_samples.SceneTable): every batch of frames is cut on the device (SceneTable.cut: one launch,
    straight into the batched forward's layout) and scored by model(batch, threshold, eval_only=False); the tracks tensor never visits the
    host.  frames None: every usable frame of the scene.  Returns validate()'s dict plus "frames"."""
    frames = scene.usable_frames(use_gt_det) if frames is None else [int(f) for f in frames]
    terms, correct, n_dets = [], [], []
    for chunk in scene.batches(frames, batch_size):
        batch = scene.cut(chunk, use_gt_det=use_gt_det)
        out = model(batch, threshold, eval_only=False)
        terms += out["loss_terms"].tolist()
        for (t, n), match, pred in zip(batch["valid_list"], batch["gt_matches"], out["matches"]):
            correct.append(int((np.asarray(pred) == gt_track_of_detections(match, t, n)).sum()))
            n_dets.append(n)
    return {"loss": float(np.sum(terms) / max(len(terms), 1)), "accuracy": float(sum(correct) / max(sum(n_dets), 1)),
            "loss_terms": terms, "correct": correct, "n_det": n_dets, "frames": frames}


def build(args):
    """src/models/associator.py:330-340"""
    g = (lambda k: args[k]) if isinstance(args, dict) else (lambda k: getattr(args, k))
    try:
        max_tracks = int(g("max_tracks"))      # optional: initial workspace size (grows on demand)
    except (KeyError, AttributeError):
        max_tracks = 256
    return Associator({"GNN_layers": g("GNN_layers"), "self_GNN_layers": g("self_GNN_layers"),
                       "sinkhorn_iterations": g("sinkhorn_iterations")}, max_tracks=max_tracks)
