"""Device-resident track rows: what a fit pass needs of the map stays on the device between calls, and a refresh uploads only what the
scan added since the last one.

`TrackRows` keeps the first 14 columns of every track row in ARRIVAL order -- a log [N, 14] float64 and the track id of every row --
and hands them out track after track, as SqFitter.prepare and SqFitter.merge_assemble take them: `packed()` is the block
{"rows14", "row_offsets", "max_rows", "n_tracks"} that multi_view.optim_process(rows=...) and merge.merge_packed(rows=...) accept
in place of the np.concatenate([t[:, :14] for t in tracks]) + upload they otherwise make on every call.  The order by track is made on
the device (include/odam_rows.h: odam_rows_group, an LSD radix sort of the row indices on the id, and odam_rows_gather14), and only
when rows were appended since the last time.

The host keeps what it needs to decide WITHOUT reading rows back: rows per track and the marks associator.TrackWindows keeps (frame id
of a track's first row, frame id and world x of its last).  Nothing here is on the per-frame path: the store catches up at the
call that needs it (`sync`).
"""
import ctypes

import numpy as np

from . import _lib

_VP, _CI, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
# the entry points as include/odam_rows.h declares them (tests/test_track_rows_host.py and tests/test_track_emit_host.py hold the two
# together)
ROWS_ARGTYPES = {
    "odam_rows_group_workspace": [_CI, _CI, _VP],
    "odam_rows_group": [_VP, _CI, _CI, _VP, _VP, _VP, _VP, ctypes.c_size_t, _VP],
    "odam_rows_gather14": [_VP, _VP, _CI, _VP, _VP],
    "odam_rows_emit_workspace": [_CI, _VP],
    "odam_rows_emit_tracked": [_VP, _VP, _VP, _VP, _VP, _CI, _D, _D, _CI, _VP, _VP, _CI, _CI, _VP, _VP, _VP, _VP, _VP, _VP, ctypes.c_size_t, _VP],
    "odam_rows_marks": [_VP, _CI, _VP, _VP, _VP, _VP, _VP, _CI, _VP, _VP],
}
MAX_ROWS = 1 << 24       # ODAM_ROWS_MAX_ROWS
MAX_TRACKS = 65536       # ODAM_ROWS_MAX_TRACKS
CHUNK = 4096             # ODAM_ROWS_CHUNK: rows one workgroup of the sort takes
ONE_PASS_TRACKS = 256    # up to here the sort is one 8-bit pass, beyond it two
STATUS_OK, STATUS_BAD_ID, STATUS_BAD_COUNT = 0, 1, 2
EMIT_DETS = 30           # ODAM_ROWS_EMIT_DETS: detection slots of a frame
EMIT_BAD_ID, EMIT_OVERFLOW = 1, 2      # odam_rows_emit_tracked's status word is a sum of these


def _entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = ROWS_ARGTYPES[name], ctypes.c_int
    return f


def group_workspace(n_rows, n_tracks):
    """bytes of working memory odam_rows_group needs"""
    b = ctypes.c_size_t(0)
    _lib.check(_entry("odam_rows_group_workspace")(int(n_rows), int(n_tracks), ctypes.cast(ctypes.byref(b), _VP)), "odam_rows_group_workspace")
    return int(b.value)


def group(tid, n_tracks, row_off, src_out=None, status=None):
    """odam_rows_group on device tensors, on the current stream: tid [N] int32, row_off [n_tracks + 1] int32 -> (src [N] int32, status
    [1] int32), both on the device; nothing is read back"""
    import torch
    N = int(tid.shape[0])
    dev = tid.device
    if src_out is None:
        src_out = torch.empty(max(N, 1), device=dev, dtype=torch.int32)
    if status is None:
        status = torch.zeros(1, device=dev, dtype=torch.int32)
    nbytes = group_workspace(N, n_tracks)
    work = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(_entry("odam_rows_group")(_lib.ptr(tid), N, int(n_tracks), _lib.ptr(row_off), _lib.ptr(src_out), _lib.ptr(status),
                                             _lib.ptr(work), nbytes, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "odam_rows_group")
    return src_out[:N], status


def gather14(log, src, out=None):
    """odam_rows_gather14 on device tensors, on the current stream: out[i] = log[src[i]] on whole rows, bit for bit"""
    import torch
    N = int(src.shape[0])
    if out is None:
        out = torch.empty(max(N, 1), 14, device=log.device, dtype=torch.float64)
    with torch.cuda.device(log.device):
        _lib.check(_entry("odam_rows_gather14")(_lib.ptr(log), _lib.ptr(src), N, _lib.ptr(out),
                                                ctypes.c_void_p(torch.cuda.current_stream(log.device).cuda_stream)), "odam_rows_gather14")
    return out[:N]


def _marks_of(tracks):
    from .associator import TrackWindows
    return TrackWindows._marks_of(tracks)


def _acceptable(tracks):
    """what multi_view._device_prelude takes: float64 arrays of at least 14 columns, none of them empty"""
    return all(isinstance(t, np.ndarray) and t.ndim == 2 and t.shape[1] >= 14 and t.dtype == np.float64 and len(t) for t in tracks)


class TrackRows:
    """The row store of one sequence on `fitter`'s device (see the module text).  Counters for tests and tools: rows_uploaded (rows sent
    from the host, in all), loads (full uploads), groupings (runs of the sort)."""

    def __init__(self, fitter, capacity_rows=65536):
        self.fitter = fitter
        self.device = fitter.device
        self.capacity = max(int(capacity_rows), 1)
        self._log = self._tid = None          # [capacity, 14] float64, [capacity] int32: made at the first upload
        self._stage = None                    # pinned staging: (rows [k, 14] float64, ids [k] int32), grown on demand
        self._stage_event = None              # the newest copy out of it
        self._word = None                     # pinned: the sort's status word lands here
        self.rows_uploaded = self.loads = self.groupings = 0
        self.rows_emitted = 0                 # rows the device wrote itself (append_tracked)
        self._host = None                     # (the packed block, the host list made from it): host_tracks' cache
        self.reset()

    def reset(self):
        """empty the store (the device buffers are kept)"""
        self.n_rows = 0
        self.lengths = []
        self.marks = np.zeros((0, 3))
        self._grouped = True                  # the log itself is track after track (a load, an adopted block, nothing at all)
        self._block = None

    # ---- the two places that touch the device on the way in (a test's stub overrides them) ---------------------------------------------
    def _reserve(self, n_rows):
        """room for n_rows rows in all: doubling, a new tensor and one device-to-device copy of the rows held"""
        import torch
        if self._log is not None and n_rows <= self.capacity:
            return
        while self.capacity < n_rows:
            self.capacity *= 2
        log = torch.empty(self.capacity, 14, device=self.device, dtype=torch.float64)
        tid = torch.empty(self.capacity, device=self.device, dtype=torch.int32)
        if self._log is not None and self.n_rows:
            log[:self.n_rows].copy_(self._log[:self.n_rows])
            tid[:self.n_rows].copy_(self._tid[:self.n_rows])
        self._log, self._tid = log, tid

    def _upload(self, pieces, ids, at):
        """pieces: list of [k_i, >= 14] float64 arrays, ids: the track of each piece -> log rows at .. at + sum k_i - 1, through the pinned
        staging buffer: the rows in one copy, their ids (4 bytes a row) in a second"""
        import torch
        k = int(sum(len(p) for p in pieces))
        if k == 0:
            return
        if self._stage_event is not None:
            self._stage_event.synchronize()      # the copy before this one has left the buffer
        if self._stage is None or self._stage[0].shape[0] < k:
            cap = max(k, 2 * (self._stage[0].shape[0] if self._stage is not None else 512))
            self._stage = (torch.empty(cap, 14, dtype=torch.float64).pin_memory(), torch.empty(cap, dtype=torch.int32).pin_memory())
        rows, tid = self._stage[0].numpy(), self._stage[1].numpy()
        o = 0
        for p, t in zip(pieces, ids):
            rows[o:o + len(p)] = p[:, :14]
            tid[o:o + len(p)] = t
            o += len(p)
        with torch.cuda.device(self.device):
            self._log[at:at + k].copy_(self._stage[0][:k], non_blocking=True)
            self._tid[at:at + k].copy_(self._stage[1][:k], non_blocking=True)
            self._stage_event = torch.cuda.Event()
            self._stage_event.record(torch.cuda.current_stream(self.device))

    # ---- bringing the store in step -------------------------------------------------------------------------------------------------------
    def load(self, tracks):
        """One upload of all rows, track after track: the log is then grouped as it stands and no kernel is needed.  Returns the rows
        uploaded, or None -- with the store emptied -- for a list _device_prelude would refuse (a track that is not a float64 array of
        at least 14 columns, an empty track, more rows or tracks than the sort takes): the caller takes its host path."""
        tracks = list(tracks)
        self.reset()
        lens = [len(t) for t in tracks] if _acceptable(tracks) else None
        if lens is None or sum(lens) > MAX_ROWS or len(lens) > MAX_TRACKS:
            return None
        n = int(sum(lens))
        self.loads += 1
        if n:
            self._reserve(n)
            self._upload(tracks, range(len(tracks)), 0)
        self.n_rows, self.lengths = n, lens
        self.marks = _marks_of(tracks) if tracks else np.zeros((0, 3))
        self.rows_uploaded += n
        return n

    def _extends(self, tracks):
        """True where every stored track is a prefix of the list's track as far as the host can tell without reading rows back, and
        tracks were only appended: TrackWindows.in_step's test with "the same length" widened to "the same or longer", the marks taken at
        the rows the store holds"""
        T = len(self.lengths)
        if T == 0 or len(tracks) < T or not _acceptable(tracks):
            return False
        if any(len(t) < k for t, k in zip(tracks, self.lengths)):
            return False
        m = np.empty((T, 3))
        m[:, 0] = np.fromiter((t[0, 0] for t in tracks[:T]), np.float64, T)
        m[:, 1] = np.fromiter((t[k - 1, 0] for t, k in zip(tracks, self.lengths)), np.float64, T)
        m[:, 2] = np.fromiter((t[k - 1, 9] for t, k in zip(tracks, self.lengths)), np.float64, T)
        return np.array_equal(m, self.marks)

    def sync(self, tracks):
        """Bring the store in step with a host track list; returns the rows uploaded (None: load's refusal).  Rows and tracks that were
        only appended go up alone, at the end of the log; anything else -- a track shortened, replaced or edited at its first or last
        stored row, fewer tracks, an empty store -- is a load."""
        tracks = list(tracks)
        if not self._extends(tracks):
            return self.load(tracks)
        T = len(self.lengths)
        pieces, ids = [], []
        for i, t in enumerate(tracks):
            k = self.lengths[i] if i < T else 0
            if len(t) > k:
                pieces.append(t[k:])
                ids.append(i)
        add = int(sum(len(p) for p in pieces))
        if self.n_rows + add > MAX_ROWS or len(tracks) > MAX_TRACKS:
            self.reset()
            return None
        if add:
            self._reserve(self.n_rows + add)
            self._upload(pieces, ids, self.n_rows)
            self.n_rows += add
            self.lengths = [len(t) for t in tracks]
            self.marks = _marks_of(tracks)
            self.rows_uploaded += add
            self._grouped = False
            self._block = None
        return add

    def adopt(self, block):
        """merge.merge_packed's block as the new content: its rows are track after track and already on the device, nothing is uploaded.
        One small copy back: the offsets and the marks of the merged tracks."""
        import torch
        rows = block["rows14"]
        off_d = block["row_offsets"].to(torch.int64)
        T = int(off_d.shape[0]) - 1
        self.reset()
        if T > 0 and rows.shape[0]:
            first, last = rows.index_select(0, off_d[:-1]), rows.index_select(0, off_d[1:] - 1)
            small = torch.cat([off_d.to(torch.float64), first[:, 0], last[:, 0], last[:, 9]]).cpu().numpy()
            off = small[:T + 1].astype(np.int64)
            self.marks = np.ascontiguousarray(small[T + 1:].reshape(3, T).T)
        else:
            off = np.zeros(T + 1, np.int64)
        self.lengths = np.diff(off).astype(np.int64).tolist()
        self.n_rows = int(off[-1])
        self._log = rows[:self.n_rows].contiguous()
        self.capacity = max(self.n_rows, 1)
        lens_d = (off_d[1:] - off_d[:-1])
        self._tid = torch.repeat_interleave(torch.arange(T, device=rows.device, dtype=torch.int32), lens_d, output_size=self.n_rows)

    def _take(self, rows, lengths, marks, lens_d=None):
        """the end of adopt_scenes for one store: `rows` [n_rows, 14] on the device, track after track, is the log from now on; lengths
        and marks are the host's -- the state adopt leaves"""
        self.reset()
        self.lengths = [int(k) for k in lengths]
        self.marks = np.ascontiguousarray(marks, np.float64).reshape(len(self.lengths), 3)
        self.n_rows = int(sum(self.lengths))
        self.capacity = max(self.n_rows, 1)
        self._set_log(rows, lens_d)

    def _set_log(self, rows, lens_d=None):
        """(device side of _take; lens_d: the lengths where they lie on the device already, so that nothing is uploaded)"""
        import torch
        self._log = rows[:self.n_rows].contiguous()
        if lens_d is None:
            lens_d = torch.as_tensor(self.lengths, dtype=torch.int64).to(rows.device)
        self._tid = torch.repeat_interleave(torch.arange(len(self.lengths), device=rows.device, dtype=torch.int32), lens_d, output_size=self.n_rows)

    # ---- rows that are born on the device (include/odam_rows.h: odam_rows_emit_tracked, odam_rows_marks) -----------------------------------
    def _emit(self, blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks, base):
        """the device side of append_tracked (a test's stub overrides it): both launches on the current stream, then the ONE copy back,
        [n_tracks + 1, 4] float64 -- per track the rows added and the frame id of the first, the frame id and world x of the last of
        them; in the last row the rows added in all and the status word"""
        import torch
        dev = self.device
        as_dev = lambda x, dt, shape: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=dt))).to(
            device=dev, dtype=getattr(torch, np.dtype(dt).name)).reshape(shape).contiguous()
        N = int(blk.shape[0])
        blk, cnt, ids = as_dev(blk, np.float32, (N, EMIT_DETS, 15)), as_dev(cnt, np.int32, (N,)), as_dev(ids, np.int32, (N, EMIT_DETS))
        T, azi = as_dev(T_wcs, np.float64, (N, 4, 4)), as_dev(cam_azi, np.float64, (N,))
        b = ctypes.c_size_t(0)
        _lib.check(_entry("odam_rows_emit_workspace")(N, ctypes.cast(ctypes.byref(b), _VP)), "odam_rows_emit_workspace")
        work = torch.empty(max(int(b.value), 16), device=dev, dtype=torch.uint8)
        words = torch.empty(3 * max(n_tracks, 1) + 2, device=dev, dtype=torch.int32)      # counts, first, last; n_emitted, status
        nt = max(n_tracks, 1)
        counts, first, last, n_emitted, status = words[:nt], words[nt:2 * nt], words[2 * nt:3 * nt], words[3 * nt:3 * nt + 1], words[3 * nt + 1:]
        out = torch.empty(n_tracks + 1, 4, device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_entry("odam_rows_emit_tracked")(
                _lib.ptr(blk), _lib.ptr(cnt), _lib.ptr(ids), _lib.ptr(T), _lib.ptr(azi), N, float(img_w), float(img_h), int(n_tracks),
                _lib.ptr(self._log), _lib.ptr(self._tid), int(base), int(self.capacity), _lib.ptr(n_emitted), _lib.ptr(counts), _lib.ptr(first),
                _lib.ptr(last), _lib.ptr(status), _lib.ptr(work), int(b.value), stream), "odam_rows_emit_tracked")
            _lib.check(_entry("odam_rows_marks")(_lib.ptr(self._log), int(self.capacity), _lib.ptr(counts), _lib.ptr(first), _lib.ptr(last),
                                                 _lib.ptr(n_emitted), _lib.ptr(status), int(n_tracks), _lib.ptr(out), stream), "odam_rows_marks")
        return out.cpu().numpy()

    def append_tracked(self, blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks):
        """The track rows of N frames' detections, made ON the device from the tracker's ids and appended to the log: blk [N, 30, 15]
        float32 + cnt [N] int32 (OdamProcess.detect_frames_packed), ids [N, 30] int32 (IouTracker.step; -1 = no row), T_wcs [N, 4, 4]
        and cam_azi [N] float64 (processor.get_cam_azi of every pose), n_tracks = the tracks after these frames.  Device tensors are taken
        as they are, host arrays are uploaded (the poses are host data; no track row is).  Room is reserved for the worst case, 30 N
        rows.  One small copy back brings the rows per track and their marks; returns the rows added.  Raises OdamError -- the store
        as it was -- where the kernel answered a status (an id >= n_tracks)."""
        N = int(blk.shape[0])
        n_tracks = int(n_tracks)
        if n_tracks < len(self.lengths):
            raise ValueError(f"append_tracked: n_tracks = {n_tracks}, the store holds {len(self.lengths)} tracks")
        if n_tracks > MAX_TRACKS or self.n_rows + EMIT_DETS * N > MAX_ROWS:
            raise _lib.OdamError(f"append_tracked: {n_tracks} tracks / {self.n_rows} + 30 x {N} rows are more than the store takes")
        if N == 0:
            return 0
        self._reserve(self.n_rows + EMIT_DETS * N)
        small = self._emit(blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks, self.n_rows)
        added, status = int(small[n_tracks, 0]), int(small[n_tracks, 1])
        if status != 0:
            raise _lib.OdamError(f"TrackRows: odam_rows_emit_tracked answered status {status} (1: an id that is not below n_tracks = {n_tracks}, "
                                 "2: more rows than the log holds)")
        counts = small[:n_tracks, 0].astype(np.int64)
        old = np.zeros(n_tracks, np.int64)
        old[:len(self.lengths)] = self.lengths
        marks = np.zeros((n_tracks, 3))
        marks[:len(self.marks)] = self.marks
        got = counts > 0
        new = got & (old == 0)
        marks[new, 0] = small[:n_tracks, 1][new]
        marks[got, 1:] = small[:n_tracks, 2:4][got]
        self.marks = marks
        self.lengths = (old + counts).tolist()
        self.n_rows += added
        self.rows_emitted += added
        if added:
            self._grouped = False
        self._block = self._host = None
        return added

    def is_view(self, tracks):
        """True where `tracks` is the very list host_tracks() returned for the store as it stands"""
        return self._host is not None and self._block is not None and self._host[0] is self._block and tracks is self._host[1]

    def host_tracks(self):
        """The host list the store stands for: [n, 82] float64 per track, as OdamProcess._track_rows(with_code=False) lays them out
        (columns 14:78 are -1, 78:82 repeat 2:6).  Groups the store (packed()), downloads rows14 ONCE and caches the list until the
        store changes; sync() of this list finds the store in step."""
        block = self.packed()
        if self._host is not None and self._host[0] is block:
            return self._host[1]
        rows14 = block["rows14"].cpu().numpy()
        block["check"]()
        full = np.full((len(rows14), 82), -1.0)
        full[:, :14] = rows14
        full[:, 78:82] = rows14[:, 2:6]
        off = block["row_offsets"]
        tracks = [full[off[t]:off[t + 1]] for t in range(block["n_tracks"])]
        self._host = (block, tracks)
        return tracks

    # ---- handing the rows out ----------------------------------------------------------------------------------------------------------------
    def packed(self):
        """{"rows14" [R, 14] float64 on the device, track after track; "row_offsets" [n + 1] int64 numpy; "max_rows"; "n_tracks"; "check"}.
        Runs the sort and the gather only if rows were appended since the last grouping, and caches the block.  block["check"]() raises
        OdamError where the sort answered a status: it reads a word whose copy to the host was enqueued HERE, so call it behind a
        synchronisation the consumer makes anyway (SqFitter.prepare's one small copy) -- it makes none of its own."""
        import torch
        if self._block is not None:
            return self._block
        T, R = len(self.lengths), self.n_rows
        off = np.zeros(T + 1, np.int64)
        off[1:] = np.cumsum(self.lengths)
        check = lambda: None
        if R == 0:
            rows14 = torch.zeros(0, 14, device=self.device, dtype=torch.float64)
        elif self._grouped:
            rows14 = self._log[:R]
        else:
            with torch.cuda.device(self.device):
                d_off = torch.from_numpy(off.astype(np.int32)).to(self.device, non_blocking=True)
                src, status = group(self._tid[:R], T, d_off)
                rows14 = gather14(self._log[:R], src)
                if self._word is None:
                    self._word = torch.zeros(1, dtype=torch.int32).pin_memory()
                word = self._word
                word.copy_(status, non_blocking=True)
            self.groupings += 1

            def check():
                if int(word[0]) != 0:
                    raise _lib.OdamError(f"TrackRows: odam_rows_group answered status {int(word[0])} "
                                         "(1: a track id outside the list, 2: a track whose row count is not the host's)")
        self._block = {"rows14": rows14, "row_offsets": off, "max_rows": int(max(self.lengths)) if T else 0, "n_tracks": T, "check": check}
        return self._block


# ---- many scenes in one block (pipeline.map_scenes) ---------------------------------------------------------------------------

def _concat_rows(pieces):
    """the rows of several blocks one after the other, device to device (a test's stub overrides it)"""
    import torch
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces)


def _adopt_copy(rows, off_d):
    """adopt_scenes' ONE copy back (a test's stub overrides it): off_d [T + 1] on the device -> float64 numpy [T + 1 + 3 T]: the offsets, then
    the frame id of every track's first row, the frame id of its last row, the world x of its last row"""
    import torch
    off_d = off_d.to(torch.int64)
    first, last = rows.index_select(0, off_d[:-1]), rows.index_select(0, off_d[1:] - 1)
    return torch.cat([off_d.to(torch.float64), first[:, 0], last[:, 0], last[:, 9]]).cpu().numpy()


def pack_scenes(stores):
    """The packed blocks of S stores as ONE block, scene after scene: {"rows14", "row_offsets", "trk_off", "max_rows", "n_tracks", "check"}
    -- what packed() returns, plus "trk_off" [S + 1] int64: scene s owns tracks trk_off[s] .. trk_off[s + 1] - 1 (an empty store is an
    empty scene).  The rows are concatenated on the device; nothing is uploaded or read back.  check() calls every block's own."""
    blocks = [st.packed() for st in stores]
    trk_off = np.zeros(len(blocks) + 1, np.int64)
    trk_off[1:] = np.cumsum([b["n_tracks"] for b in blocks])
    offs, base = [np.zeros(1, np.int64)], 0
    for b in blocks:
        o = np.asarray(b["row_offsets"], np.int64)
        offs.append(o[1:] + base)
        base += int(o[-1])
    pieces = [b["rows14"] for b in blocks if int(b["row_offsets"][-1])]
    rows14 = _concat_rows(pieces) if pieces else (blocks[0]["rows14"] if blocks else None)
    checks = [b["check"] for b in blocks]

    def check():
        for c in checks:
            c()
    return {"rows14": rows14, "row_offsets": np.concatenate(offs), "trk_off": trk_off, "max_rows": max([b["max_rows"] for b in blocks], default=0),
            "n_tracks": int(trk_off[-1]), "check": check}


def adopt_scenes(stores, merged):
    """TrackRows.adopt for S stores from ONE merged block (merge.merge_packed_scenes): "rows14" and "row_offsets" on the device for the
    merged tracks of all scenes one after the other, "n_out" [S] on the host: merged tracks per scene.  Every store gets what adopt
    would have given it from its own scene's block -- lengths, marks, n_rows, and a log that holds the same bits -- with ONE copy back
    for all scenes (the offsets and the marks).  stores[s] = None leaves scene s alone (its rows are in the block all the same)."""
    n_out = [int(k) for k in merged["n_out"]]
    if len(n_out) != len(stores):
        raise ValueError(f"adopt_scenes: {len(stores)} stores for the {len(n_out)} scenes of the block")
    T = int(sum(n_out))
    rows = merged["rows14"]
    if T > 0 and rows.shape[0]:
        small = _adopt_copy(rows, merged["row_offsets"][:T + 1])
        off = small[:T + 1].astype(np.int64)
        marks = np.ascontiguousarray(small[T + 1:].reshape(3, T).T)
    else:
        off, marks = np.zeros(T + 1, np.int64), np.zeros((T, 3))
    lens_d = None
    if T > 0:
        off_d = merged["row_offsets"][:T + 1].to(merged["rows14"].device).long()
        lens_d = off_d[1:] - off_d[:-1]
    o = 0
    for st, k in zip(stores, n_out):
        if st is not None:
            st._take(rows[int(off[o]):int(off[o + k])], np.diff(off[o:o + k + 1]), marks[o:o + k], None if lens_d is None else lens_d[o:o + k])
        o += k
