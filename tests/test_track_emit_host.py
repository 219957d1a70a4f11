"""Track rows written on the device, without a device: the numpy restatement tests/track_emit_ref.py against the host path it replaces
(OdamProcess._track_rows), its flag and rank rules, the entry points of include/odam_rows.h against what odam_amd.track_store gives
ctypes and their argument checks (which come before any device work), TrackRows.append_tracked's bookkeeping on a stub whose device
side is the restatement, and OdamProcess's view rule on a stub store.  CPU only.

Contract of the restatement against _track_rows: columns 0-8 and 13 bit for bit; columns 9-11 within
track_emit_ref.centre_bound (derived: two evaluations of one 4-term sum); column 12 within ATAN_ULPS of test_track_emit_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_emit_ref as R
from conftest import REPO

C_TO_CTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
K = np.array([[1170.0, 0, 648.0], [0, 1170.0, 484.0], [0, 0, 1.0]])
W, H = 1296, 968


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _proc():
    from odam_amd.processor import OdamProcess
    proc = OdamProcess(None, None, None, None)
    proc.init_sequence(K, H, W)
    return proc


# ---- the restatement against the host path ---------------------------------------------------------------------------------------------
def test_restatement_against_track_rows():
    from odam_amd import processor
    from test_track_emit_gpu import ATAN_ULPS
    proc = _proc()
    worst9 = worst12 = 0.0
    for seed in range(4):
        blk, cnt, ids, T, azi = R.scene(25, 40, seed)
        assert np.array_equal(bits(azi), bits(np.array([processor.get_cam_azi(t) for t in T])))
        got = R.rows_of(blk, T, azi, W, H)
        bound = R.centre_bound(blk, T)
        for k in range(len(cnt)):
            n = int(np.clip(cnt[k], 0, 30))
            want = proc._track_rows(blk[k, :n].astype(np.float64), T[k], with_code=False)
            g = got[k, :n]
            for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13):
                assert np.array_equal(bits(g[:, c]), bits(want[:, c])), (seed, k, c)
            d = np.abs(g[:, 9:12] - want[:, 9:12])
            assert (d <= bound[k, :n]).all(), (seed, k)
            worst9 = max(worst9, float((d / bound[k, :n]).max()) if n else 0.0)
            u = np.abs(g[:, 12] - want[:, 12]) / np.spacing(np.abs(want[:, 12]))
            assert (u <= ATAN_ULPS).all(), (seed, k)
            worst12 = max(worst12, float(u.max()) if n else 0.0)
            assert (want[:, 14:78] == -1).all() and np.array_equal(want[:, 78:82], want[:, 2:6])
    print("restatement vs _track_rows: columns 9-11 at %.3g of the bound, column 12 %.3g ulp" % (worst9, worst12))


# ---- flags, ranks, the per-track outputs --------------------------------------------------------------------------------------------------
def _call(blk, cnt, ids, T, azi, n_tracks, cap, base=0):
    log = np.full((cap, 14), -7.5)
    tid = np.full(cap, -9, np.int32)
    res = R.emit(blk, cnt, ids, T, azi, W, H, n_tracks, log, tid, base)
    return log, tid, res


def test_flag_and_rank_rules():
    blk, _, _, T, azi = R.scene(4, 5, 1)
    cnt = np.array([2, -3, 40, 0], np.int32)
    ids = np.full((4, 30), -1, np.int32)
    ids[0, :5] = [3, -1, 4, 4, 4]        # slot 1 is live with -1; slots 2 .. 4 lie beyond the count: ignored although their ids are good
    ids[1, :3] = [0, 1, 2]               # a negative count is 0 live slots
    ids[2, :] = np.where(np.arange(30) % 3 == 0, -1, np.arange(30) % 5)      # a count of 40 is 30 live slots, -1 interleaved
    ids[3, :] = 2                        # count 0
    on, bad = R.flags(cnt, ids, 5)
    assert not bad and on[0].tolist() == [True] + [False] * 29 and not on[1].any() and not on[3].any()
    assert on[2].tolist() == [d % 3 != 0 for d in range(30)]
    log, tid, res = _call(blk, cnt, ids, T, azi, 5, 40, base=3)
    assert res["status"] == 0 and res["n_emitted"] == 21
    assert (log[:3] == -7.5).all() and (log[24:] == -7.5).all() and (tid[:3] == -9).all() and (tid[24:] == -9).all()
    want_t = [3] + [d % 5 for d in range(30) if d % 3]
    assert tid[3:24].tolist() == want_t                                        # (k, d) lexicographic
    rows = R.rows_of(blk, T, azi, W, H)
    assert np.array_equal(bits(log[3]), bits(rows[0, 0])) and np.array_equal(bits(log[4:24]), bits(rows[2][on[2]]))
    assert res["counts"].tolist() == np.bincount(want_t, minlength=5).tolist()
    pos = 3 + np.arange(21)
    for t in range(5):
        p = pos[np.array(want_t) == t]
        assert (res["first_pos"][t], res["last_pos"][t]) == (p.min(), p.max())
    m = R.marks(log, res)
    assert m.shape == (6, 4) and m[5].tolist() == [21, 0, 0, 0]
    assert m[3].tolist() == [res["counts"][3], log[3, 0], log[res["last_pos"][3], 0], log[res["last_pos"][3], 9]]
    # an id that is not below n_tracks: status, the slot is left out, the others are as they were
    ids2 = ids.copy()
    ids2[2, 4] = 5
    log2, tid2, res2 = _call(blk, cnt, ids2, T, azi, 5, 40, base=3)
    assert res2["status"] == R.BAD_ID and res2["n_emitted"] == 20
    keep = np.ones(21, bool)
    keep[1 + [d for d in range(30) if d % 3].index(4)] = False
    assert tid2[3:23].tolist() == np.array(want_t)[keep].tolist() and np.array_equal(bits(log2[3:23]), bits(log[3:24][keep]))
    ids2[0, 3] = 99                                                             # beyond the count: not even looked at
    assert R.emit(blk, cnt, ids2, T, azi, W, H, 5, log2.copy(), tid2.copy(), 3)["status"] == R.BAD_ID
    ids2[2, 4] = 4
    assert R.emit(blk, cnt, ids2, T, azi, W, H, 5, log2.copy(), tid2.copy(), 3)["status"] == 0
    # one row short: nothing at all is written
    log3, tid3, res3 = _call(blk, cnt, ids, T, azi, 5, 23, base=3)
    assert res3["status"] == R.OVERFLOW and res3["n_emitted"] == 21 and (log3 == -7.5).all() and (tid3 == -9).all()
    assert (res3["counts"] == 0).all() and (res3["first_pos"] == -1).all() and (res3["last_pos"] == -1).all()
    assert R.marks(log3, res3)[:5].tolist() == [[0, -1, -1, -1]] * 5 and R.marks(log3, res3)[5].tolist() == [21, 2, 0, 0]
    assert _call(blk, cnt, ids, T, azi, 5, 24, base=3)[2]["status"] == 0
    # no frames
    res0 = R.emit(blk[:0], cnt[:0], ids[:0], T[:0], azi[:0], W, H, 5, log3, tid3, 3)
    assert res0["n_emitted"] == 0 and res0["status"] == 0 and (log3 == -7.5).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_rows.h")).read(), flags=re.S)


def _header_args(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/odam_rows.h"
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return names, want


def test_prototypes_are_the_headers():
    from odam_amd import _lib, track_store as ts, tracker
    txt = _header()
    for name in ("odam_rows_emit_workspace", "odam_rows_emit_tracked", "odam_rows_marks"):
        names, want = _header_args(txt, name)
        assert ts.ROWS_ARGTYPES[name] == want, name
        assert hasattr(_lib.lib(), name)
        f = ts._entry(name)
        assert list(f.argtypes) == want and f.restype is ctypes.c_int
    assert _header_args(txt, "odam_rows_emit_tracked")[0] == [
        "det_block", "det_count", "ids", "T_wc", "cam_azi", "N", "img_w", "img_h", "n_tracks", "rows", "tid", "base", "cap", "n_emitted", "counts",
        "first_pos", "last_pos", "status", "work", "work_bytes", "stream"]
    assert _header_args(txt, "odam_rows_marks")[0] == ["rows", "n_log", "counts", "first_pos", "last_pos", "n_emitted", "status", "n_tracks", "out",
                                                       "stream"]
    for name, value in (("ODAM_ROWS_EMIT_DETS", ts.EMIT_DETS), ("ODAM_ROWS_EMIT_BAD_ID", ts.EMIT_BAD_ID), ("ODAM_ROWS_EMIT_OVERFLOW", ts.EMIT_OVERFLOW)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) == value, name
    assert (ts.EMIT_DETS, ts.EMIT_BAD_ID, ts.EMIT_OVERFLOW) == (R.DETS, R.BAD_ID, R.OVERFLOW) and ts.EMIT_DETS == tracker.MAX_DETS


def test_argument_checks_come_before_any_device_work():
    from odam_amd import _lib, track_store as ts
    L = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    size = ctypes.c_size_t(12345)
    ps = ctypes.cast(ctypes.byref(size), ctypes.c_void_p)
    most = 2 ** 24 // 30                                                          # frames whose slots still fit
    fw = ts._entry("odam_rows_emit_workspace")
    assert fw(10, None) == 1 and b"odam_rows_emit_workspace" in L.odam_last_error()      # ODAM_E_INVALID
    assert fw(-1, ps) == 1 and fw(most + 1, ps) == 3 and b"2^24" in L.odam_last_error()   # ODAM_E_LIMIT
    assert fw(0, ps) == 0 and size.value == 0
    for n in (1, 136, 137, 274, most):
        assert fw(n, ps) == 0
        assert size.value == -(-4 * 2 * -(-n * 30 // ts.CHUNK) // 16) * 16, n             # a count and a flag per chunk
    fe = ts._entry("odam_rows_emit_tracked")
    ptrs = ("blk", "cnt", "ids", "T", "azi", "rows", "tid", "n_emitted", "counts", "first", "last", "status", "work")
    g = lambda kw, k: kw.get(k, p)

    def args(**kw):
        return [g(kw, "blk"), g(kw, "cnt"), g(kw, "ids"), g(kw, "T"), g(kw, "azi"), kw.get("N", 4), 640.0, 480.0, kw.get("n_tracks", 2), g(kw, "rows"),
                g(kw, "tid"), kw.get("base", 0), kw.get("cap", 200), g(kw, "n_emitted"), g(kw, "counts"), g(kw, "first"), g(kw, "last"),
                g(kw, "status"), g(kw, "work"), kw.get("bytes", 16), None]
    for k in ptrs:
        assert fe(*args(**{k: None})) == 1 and b"odam_rows_emit_tracked: null" in L.odam_last_error(), k
    assert fe(*args(N=-1)) == 1 and fe(*args(n_tracks=-1)) == 1
    assert fe(*args(N=most + 1)) == 3 and b"2^24" in L.odam_last_error()
    assert fe(*args(n_tracks=65537)) == 3 and b"65536" in L.odam_last_error()
    assert fe(*args(N=most + 1, blk=None)) == 3                                    # the limit is answered before anything else is looked at
    assert fe(*args(base=-1)) == 1 and b"base" in L.odam_last_error() and fe(*args(base=201)) == 1 and fe(*args(cap=-1)) == 1
    assert fe(*args(bytes=15)) == 1 and b"workspace" in L.odam_last_error()
    assert fe(*args(N=274, bytes=16)) == 1 and b"workspace" in L.odam_last_error()   # three chunks: 24 bytes, 32 as the query rounds them
    assert fe(*args(work=ctypes.c_void_p(p.value + 8))) == 1 and b"aligned" in L.odam_last_error()
    assert fe(*args(rows=ctypes.c_void_p(p.value + 8))) == 1 and b"aligned" in L.odam_last_error()
    assert fe(*args(N=0)) == 0 and fe(*args(N=0, blk=None, work=None, rows=None)) == 0      # the empty call launches nothing
    fm = ts._entry("odam_rows_marks")
    okm = lambda **kw: [g(kw, "rows"), kw.get("n_log", 10), g(kw, "counts"), g(kw, "first"), g(kw, "last"), g(kw, "n_emitted"), g(kw, "status"),
                        kw.get("n_tracks", 2), g(kw, "out"), None]
    for k in ("rows", "counts", "first", "last", "n_emitted", "status", "out"):
        assert fm(*okm(**{k: None})) == 1 and b"odam_rows_marks" in L.odam_last_error(), k
    assert fm(*okm(n_log=-1)) == 1 and fm(*okm(n_tracks=-1)) == 1 and fm(*okm(n_tracks=65537)) == 3


# ---- TrackRows.append_tracked: the bookkeeping, the device side played by the restatement -----------------------------------------------
class _Fitter:
    device = "cpu"


def _stub(capacity=65536):
    from odam_amd.track_store import TrackRows

    class Stub(TrackRows):
        """a host log; _emit is the restatement; uploads are recorded"""

        def __init__(self):
            self.uploads, self.emits = [], 0
            self.log, self.ids = np.zeros((0, 14)), np.zeros(0, np.int32)
            super().__init__(_Fitter(), capacity_rows=capacity)

        def _reserve(self, n_rows):
            while self.capacity < n_rows:
                self.capacity *= 2
            if len(self.log) < self.capacity:
                log, ids = np.full((self.capacity, 14), -7.5), np.full(self.capacity, -9, np.int32)
                log[:self.n_rows], ids[:self.n_rows] = self.log[:self.n_rows], self.ids[:self.n_rows]
                self.log, self.ids = log, ids

        def _upload(self, pieces, ids, at):
            self.uploads.append((at, [int(i) for i in ids]))

        def _emit(self, blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks, base):
            self.emits += 1
            assert base == self.n_rows and len(self.log) == self.capacity >= base + 30 * len(cnt)
            res = R.emit(blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks, self.log, self.ids, base)
            return R.marks(self.log, res)
    return Stub()


def test_append_tracked_bookkeeping():
    from odam_amd import _lib
    from odam_amd.track_store import _marks_of
    blk, cnt, _, T, azi = R.scene(80, 200, 3)
    ids, n = R.tracker_ids(cnt, 200, 3)
    assert 20 < n <= 80
    whole, halves = _stub(), _stub(capacity=64)
    added = whole.append_tracked(blk, cnt, ids, T, azi, W, H, n)
    assert added == whole.n_rows == whole.rows_emitted == int((ids >= 0).sum()) > 500 and whole.emits == 1
    assert whole.rows_uploaded == 0 and whole.loads == 0 and not whole._grouped and whole._block is None and whole.capacity == 65536
    want = R.host_tracks(whole.log, whole.ids, whole.n_rows, n)
    assert whole.lengths == [len(t) for t in want] and all(isinstance(x, int) for x in whole.lengths)
    assert np.array_equal(whole.marks, _marks_of(want))
    assert whole.sync(want) == 0 and whole.uploads == [] and whole.loads == 0      # the list the store stands for finds it in step
    # two calls of 40 frames: the same log, counts and marks; the tracks known after the first call are fewer
    n1 = int(ids[:40].max()) + 1
    assert 0 < n1 < n
    a = halves.append_tracked(blk[:40], cnt[:40], ids[:40], T[:40], azi[:40], W, H, n1)
    assert halves.capacity == 2048 and len(halves.lengths) == n1 and halves.n_rows == a
    b = halves.append_tracked(blk[40:], cnt[40:], ids[40:], T[40:], azi[40:], W, H, n)
    assert a + b == added and halves.capacity == (2048 if a + 1200 <= 2048 else 4096) and halves.emits == 2
    assert np.array_equal(bits(halves.log[:added]), bits(whole.log[:added])) and np.array_equal(halves.ids[:added], whole.ids[:added])
    assert halves.lengths == whole.lengths and np.array_equal(halves.marks, whole.marks) and halves.rows_emitted == added
    # no frames: nothing happens; fewer tracks than the store holds, or a status: refused, the store as it was
    assert halves.append_tracked(blk[:0], cnt[:0], ids[:0], T[:0], azi[:0], W, H, n) == 0 and halves.emits == 2
    with pytest.raises(ValueError):
        halves.append_tracked(blk[:1], cnt[:1], ids[:1], T[:1], azi[:1], W, H, n - 1)
    before = (halves.n_rows, list(halves.lengths), halves.marks.copy(), halves.rows_emitted)
    with pytest.raises(_lib.OdamError, match="status 1"):
        halves.append_tracked(blk[:40], cnt[:40], ids[:40] + n - n1 + 1, T[:40], azi[:40], W, H, n)
    assert (halves.n_rows, halves.lengths, halves.rows_emitted) == (before[0], before[1], before[3]) and np.array_equal(halves.marks, before[2])
    # rows appended by the device and rows uploaded from the host live in one log
    more = [np.concatenate([t, t[-1:] + 1.0]) for t in want]
    assert whole.sync(more) == n and whole.rows_uploaded == n and whole.rows_emitted == added and whole.uploads == [(added, list(range(n)))]
    whole.reset()
    assert whole.n_rows == 0 and whole.lengths == [] and whole.rows_emitted == added


# ---- OdamProcess: `tracks` as a view of the store ----------------------------------------------------------------------------------------
class _StubTracker:
    """two detections per frame, the first always track 0, the second track 1"""
    iou_tracker = True
    device = "cpu"
    fitter = object()
    _state = object()

    def __init__(self):
        self.n_tracks = [0]

    def reset(self, n_seq=1):
        self.n_tracks = [0]

    def step(self, blk, cnt, frame_ids, T_wcs, img_w, img_h):
        import torch
        ids = torch.full((len(frame_ids), 30), -1, dtype=torch.int32)
        ids[:, :2] = torch.tensor([0, 1], dtype=torch.int32)
        self.n_tracks = [2]
        return ids, None, None


class _StubStore:
    def __init__(self):
        self.lengths, self.downloads, self.appends, self.syncs, self.packs = [], 0, [], [], 0
        self._list = None

    def reset(self):
        self.lengths, self._list = [], None

    def sync(self, tracks):
        self.syncs.append([len(t) for t in tracks])
        return 0

    def append_tracked(self, blk, cnt, ids, T_wcs, cam_azi, img_w, img_h, n_tracks):
        self.appends.append((len(cnt), int(n_tracks), np.asarray(cam_azi).copy()))
        self.lengths = [sum(a[0] for a in self.appends)] * n_tracks
        self._list = None

    def host_tracks(self):
        if self._list is None:
            self.downloads += 1
            self._list = [np.full((k, 82), float(t)) for t, k in enumerate(self.lengths)]
        return self._list

    def is_view(self, tracks):
        return tracks is self._list and tracks is not None

    def packed(self):
        self.packs += 1
        return {"n_tracks": len(self.lengths)}


def test_tracks_is_a_view_of_the_store_until_the_host_takes_over():
    import torch
    from odam_amd import processor
    from odam_amd.processor import OdamProcess
    proc = OdamProcess(None, _StubTracker(), None, None, fitter=object())
    proc._rows = store = _StubStore()
    proc.init_sequence(K, H, W)
    blk, cnt = torch.zeros(5, 30, 15), torch.full((5,), 2, dtype=torch.int32)
    T = list(R.scene(5, 2, 0)[3])
    proc.track_frames_packed(blk[:3], cnt[:3], [10, 11, 12], T[:3], resident=True)
    assert proc._store_auth and store.syncs == [[]] and [a[:2] for a in store.appends] == [(3, 2)] and store.downloads == 0
    assert np.array_equal(store.appends[0][2], [processor.get_cam_azi(t) for t in T[:3]])
    assert proc.usable_frames == [10, 11, 12] and len(proc.T_wcs) == len(proc.P_cws) == 3 and proc.run_associator and proc._n_tracks == 2
    assert proc._tracks == []                                                       # no host rows were built
    a = proc.tracks
    assert proc.tracks is a and store.downloads == 1 and [len(t) for t in a] == [3, 3]      # materialised once, cached
    assert proc._store_auth
    # "resident" takes the store as it stands for the view (or a callable), without a sync
    assert proc._prelude_args("resident", a, None) == {"prelude": "device", "rows": {"n_tracks": 2}}
    assert proc._prelude_args("resident", lambda: proc.tracks, None)["rows"] == {"n_tracks": 2}
    assert store.syncs == [[]] and store.downloads == 1 and proc._store_auth and store.packs == 2
    proc.track_frames_packed(blk[3:4], cnt[3:4], [13], T[3:4], resident=True)       # more frames: the cached list is stale
    assert store.syncs == [[]] and [len(t) for t in proc.tracks] == [4, 4] and store.downloads == 2
    # a non-resident call hands the record back to the host list: it is downloaded first (here: cached), then extended on the host
    view = proc.tracks
    proc.track_frames_packed(blk[4:], cnt[4:], [14], T[4:])
    assert not proc._store_auth and store.downloads == 2 and proc._tracks is view and [t.shape for t in proc.tracks] == [(5, 82), (5, 82)]
    assert proc.usable_frames == [10, 11, 12, 13, 14] and len(store.appends) == 2
    # ... and the store catches up through sync when it is needed again
    assert proc._prelude_args("resident", proc.tracks, None)["rows"] == {"n_tracks": 2} and store.syncs[-1] == [5, 5]
    # resident again: the store takes over from the list it is in step with
    store.lengths = [5, 5]
    proc.track_frames_packed(blk[:1], cnt[:1], [15], T[:1], resident=True)
    assert proc._store_auth and store.syncs[-1] == [5, 5] and len(store.syncs) == 3
    # a list that is not the view: the host list becomes the record first, then the store is synced to the OTHER list
    other = [np.zeros((2, 82))]
    assert proc._prelude_args("resident", other, None)["rows"] == {"n_tracks": 2}
    assert not proc._store_auth and store.syncs[-1] == [2] and [len(t) for t in proc.tracks] == [5, 5]
    # assigning ends the view without a download
    proc.track_frames_packed(blk[:1], cnt[:1], [16], T[:1], resident=True)
    n = store.downloads
    proc.tracks = []
    assert not proc._store_auth and store.downloads == n and proc.tracks == []
    # the default is the host path, and the keyword is refused without a tracker
    with pytest.raises(TypeError):
        OdamProcess(None, None, None, None).track_frames_packed(blk, cnt, [0] * 5, T, resident=True)
