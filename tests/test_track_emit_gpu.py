"""Track rows written on the device (odam_amd/csrc/track_emit.hip through include/odam_rows.h, track_store.TrackRows.append_tracked,
OdamProcess.track_frames_packed(resident=True) and pipeline.map_scene(loaded=True)) against the numpy restatement
tests/track_emit_ref.py and the host path they replace.

What is asked:
  kernel == restatement   bit for bit in the log, the ids, n_emitted, the per-track counts and positions, the status word and the
                          marks block -- except column 12 of the log, where the device library's atan2 meets np.arctan2: ATAN_ULPS.
  untouched words         the log starts as sentinels: positions outside base .. base + n_emitted - 1 keep them; a bad id stores
                          nothing for its slot; a log one row short stores nothing at all.
  downstream              rows taken from a device-fed store through host_tracks() and loaded into a second store give the same packed
                          block bit for bit, so map_scene on either gives the same bits: the chain does not depend on ATAN_ULPS.
Sizes: 1 frame; 137 and 274 frames (4110 and 8220 slots: one and two chunk boundaries of 4096); the fixture scene's first 60 frames."""
import ctypes

import numpy as np
import pytest

import track_emit_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = np.array([[1170.0, 0, 648.0], [0, 1170.0, 484.0], [0, 0, 1.0]])
W, H = 1296, 968
SENT_D, SENT_I = -1234.5, -77

# Column 12 = atan2(sin, cos) + cam_azi: the device library's atan2 against np.arctan2, in ulps of the binary64 result.
# MEASURED on an MI355X over every input of this file (the cases below and the fixture scene, 80 comparisons): 2048 ulp at the worst (the
# fixture scene; 1024 on the synthetic cases), always a power of two.  The two atan2 differ in the LAST BIT of their own result in
# places; the result here is the SUM with cam_azi, and where the two nearly cancel, one ulp of the angle is 2^10 - 2^11 ulp of a sum
# that many binades smaller: the figure counts the cancellation (which is why it is a power of two), and is taken for what an atan2
# that is one ulp off does to these inputs.  The bound is twice the measured value.
ATAN_ULPS = 4096.0
_worst = {"ulp": 0.0}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _col12(got, want, what):
    """column 12 within ATAN_ULPS ulps of the restatement's (or the host path's) value; the figure is printed before it is asserted"""
    if len(got):
        u = np.abs(got - want) / np.spacing(np.abs(want))
        _worst["ulp"] = max(_worst["ulp"], float(u.max()))
        print("%s: column 12 differs by %.4g ulp at the worst (so far %.4g)" % (what, float(u.max()), _worst["ulp"]))
        assert (u <= ATAN_ULPS).all(), (what, float(u.max()))


def _same_rows(got, want, what):
    """log rows: every column but 12 bit for bit, column 12 within ATAN_ULPS"""
    assert got.shape == want.shape, what
    cols = [c for c in range(got.shape[1]) if c != 12]
    assert np.array_equal(bits(got[:, cols]), bits(want[:, cols])), what
    _col12(got[:, 12], want[:, 12], what)


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 200)
    yield f
    f.close()


def _raw(blk, cnt, ids, T, azi, n_tracks, cap, base=0, log=None, tid=None):
    """odam_rows_emit_tracked + odam_rows_marks on a sentinel-filled log -> dict of host arrays"""
    import torch
    from odam_amd import _lib, track_store as ts
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(DEV)
    N = len(cnt)
    if log is None:
        log = torch.full((cap, 14), SENT_D, device=DEV, dtype=torch.float64)
        tid = torch.full((cap,), SENT_I, device=DEV, dtype=torch.int32)
    nt = max(n_tracks, 1)
    counts, first, last = (torch.full((nt + 2,), SENT_I, device=DEV, dtype=torch.int32) for _ in range(3))      # two guard words each
    n_em, status = torch.full((3,), SENT_I, device=DEV, dtype=torch.int32), torch.full((3,), SENT_I, device=DEV, dtype=torch.int32)
    out = torch.full((n_tracks + 2, 4), SENT_D, device=DEV, dtype=torch.float64)
    b = ctypes.c_size_t(0)
    assert ts._entry("odam_rows_emit_workspace")(N, ctypes.cast(ctypes.byref(b), ctypes.c_void_p)) == 0
    work = torch.zeros(max(b.value, 16) + 16, device=DEV, dtype=torch.uint8)
    work[b.value:] = 0x5A
    t_blk, t_cnt, t_ids, t_T, t_azi = d(blk, np.float32), d(cnt, np.int32), d(ids, np.int32), d(T, np.float64), d(azi, np.float64)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ts._entry("odam_rows_emit_tracked")(_lib.ptr(t_blk), _lib.ptr(t_cnt), _lib.ptr(t_ids), _lib.ptr(t_T), _lib.ptr(t_azi), N, float(W), float(H),
                                             n_tracks, _lib.ptr(log), _lib.ptr(tid), base, cap, _lib.ptr(n_em), _lib.ptr(counts), _lib.ptr(first),
                                             _lib.ptr(last), _lib.ptr(status), _lib.ptr(work), b.value, stream)
    assert rc == 0, _lib.lib().odam_last_error()
    if N:
        assert ts._entry("odam_rows_marks")(_lib.ptr(log), cap, _lib.ptr(counts), _lib.ptr(first), _lib.ptr(last), _lib.ptr(n_em), _lib.ptr(status),
                                            n_tracks, _lib.ptr(out), stream) == 0
    torch.cuda.synchronize()
    assert (work[b.value:].cpu().numpy() == 0x5A).all()                            # nothing behind the workspace
    h = lambda x: x.cpu().numpy()
    return {"log": h(log), "tid": h(tid), "n_emitted": h(n_em), "counts": h(counts), "first_pos": h(first), "last_pos": h(last),
            "status": h(status), "marks": h(out), "dev": (log, tid)}


def _check(got, blk, cnt, ids, T, azi, n_tracks, cap, base, what, log0=None, tid0=None):
    """a raw call against the restatement run on the same starting log"""
    log = np.full((cap, 14), SENT_D) if log0 is None else log0.copy()
    tid = np.full(cap, SENT_I, np.int32) if tid0 is None else tid0.copy()
    want = R.emit(blk, cnt, ids, T, azi, W, H, n_tracks, log, tid, base)
    assert got["n_emitted"].tolist() == [want["n_emitted"], SENT_I, SENT_I] and got["status"].tolist() == [want["status"], SENT_I, SENT_I], what
    for k in ("counts", "first_pos", "last_pos"):
        assert np.array_equal(got[k][:n_tracks], want[k]) and (got[k][max(n_tracks, 1):] == SENT_I).all(), (what, k)
    assert np.array_equal(got["tid"], tid), what
    _same_rows(got["log"], log, what)                                              # the sentinels outside the written range included
    m = R.marks(got["log"], want)                                                  # (on the device's own log: the gather is exact)
    assert np.array_equal(bits(got["marks"][:n_tracks + 1]), bits(m)) and (got["marks"][n_tracks + 1:] == SENT_D).all(), what
    return want


# ---- 1. the kernels against the restatement ------------------------------------------------------------------------------------------------
CASES = [(137, 40, (), 0.5), (137, 40, (1,), 0.5), (274, 40, (), 0.5), (274, 40, (1,), 0.5), (274, 40, (0,), 0.5), (274, 1, (), 0.9), (274, 65536, (), 0.5)]


@pytest.mark.parametrize("N,n_tracks,empty,live", CASES)
def test_emit_equals_the_restatement(N, n_tracks, empty, live):
    blk, cnt, ids, T, azi = R.scene(N, n_tracks, 11 + N + len(empty), live=live, empty_chunks=empty)
    cap, base = N * 30 + 5, 3
    got = _raw(blk, cnt, ids, T, azi, n_tracks, cap, base)
    want = _check(got, blk, cnt, ids, T, azi, n_tracks, cap, base, "N = %d, %d tracks, empty chunks %r" % (N, n_tracks, empty))
    live_slots = int(np.clip(cnt, 0, 30).sum())
    assert want["status"] == 0 and 0.3 * live_slots < want["n_emitted"] < live_slots
    for c in empty:                                                                # the chunk really is empty, the ones beside it are not
        on = R.flags(cnt, ids, n_tracks)[0].reshape(-1)
        assert not on[c * 4096:(c + 1) * 4096].any() and on.any()
    # repeated launches give identical bits
    again = _raw(blk, cnt, ids, T, azi, n_tracks, cap, base)
    for k in ("log", "tid", "n_emitted", "counts", "first_pos", "last_pos", "status", "marks"):
        assert got[k].tobytes() == again[k].tobytes(), k


def test_one_frame():
    blk, cnt, ids, T, azi = R.scene(1, 7, 2, live=1.0)
    for count, what in ((0, "count 0"), (30, "30 emitted"), (45, "count 45"), (-1, "count -1")):
        cnt[:] = count
        got = _raw(blk, cnt, ids, T, azi, 7, 30, 0)
        want = _check(got, blk, cnt, ids, T, azi, 7, 30, 0, "one frame, " + what)
        assert want["n_emitted"] == (30 if count >= 30 else 0) and want["status"] == 0
    # no frames at all: no launch, nothing is written, not even the count
    got = _raw(blk[:0], cnt[:0], ids[:0], T[:0], azi[:0], 7, 30, 0)
    assert (got["log"] == SENT_D).all() and got["n_emitted"].tolist() == [SENT_I] * 3 and got["status"].tolist() == [SENT_I] * 3
    # no tracks yet: every id is -1
    cnt[:] = 30
    ids[:] = -1
    got = _raw(blk, cnt, ids, T, azi, 0, 30, 0)
    _check(got, blk, cnt, ids, T, azi, 0, 30, 0, "one frame, no track")
    assert got["marks"][0].tolist() == [0, 0, 0, 0]


def test_a_bad_id_and_a_log_one_row_short():
    blk, cnt, ids, T, azi = R.scene(137, 40, 5)
    on = R.flags(cnt, ids, 40)[0]
    k, d = [int(x[len(x) // 2]) for x in np.nonzero(on)]
    bad = ids.copy()
    bad[k, d] = 40                                                                 # an id equal to n_tracks
    beyond = np.nonzero(np.arange(30)[None, :] >= np.clip(cnt, 0, 30)[:, None])
    bad[beyond[0][0], beyond[1][0]] = 70000                                        # beyond its frame's count: not looked at
    cap = 137 * 30
    got = _raw(blk, cnt, bad, T, azi, 40, cap)
    want = _check(got, blk, cnt, bad, T, azi, 40, cap, 0, "an id equal to n_tracks")
    ok = R.emit(blk, cnt, ids, T, azi, W, H, 40, np.zeros((cap, 14)), np.zeros(cap, np.int32), 0)
    assert want["status"] == R.BAD_ID and want["n_emitted"] == ok["n_emitted"] - 1 and want["counts"].sum() == want["n_emitted"]
    assert (got["log"][want["n_emitted"]:] == SENT_D).all() and (got["tid"][:want["n_emitted"]] < 40).all()
    # both at once, and the log one row short alone: nothing is stored
    n = ok["n_emitted"]
    for these, base, room, status in ((ids, 7, n - 1, R.OVERFLOW), (bad, 0, n - 2, R.BAD_ID | R.OVERFLOW), (ids, 7, n, 0)):
        got = _raw(blk, cnt, these, T, azi, 40, base + room, base)
        want = _check(got, blk, cnt, these, T, azi, 40, base + room, base, "room for %d of %d rows" % (room, n))
        assert want["status"] == status
        if status:
            assert (got["log"] == SENT_D).all() and (got["tid"] == SENT_I).all() and (got["counts"][:40] == 0).all()
            assert (got["first_pos"][:40] == -1).all() and (got["last_pos"][:40] == -1).all() and got["marks"][40, 1] == status


# ---- 2. through TrackRows ----------------------------------------------------------------------------------------------------------------
def _store_state(s):
    return s._log[:s.n_rows].cpu().numpy(), s._tid[:s.n_rows].cpu().numpy(), list(s.lengths), s.marks.copy()


def _same_store(a, b, what):
    assert a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[3]), bits(b[3])), what


def test_two_calls_equal_one_and_the_store_grows(fitter):
    import torch
    from odam_amd.track_store import TrackRows, _marks_of
    blk, cnt, _, T, azi = R.scene(80, 200, 3)
    ids, n = R.tracker_ids(cnt, 200, 3)
    n1 = int(ids[:40].max()) + 1
    assert 0 < n1 < n
    whole, halves = TrackRows(fitter), TrackRows(fitter, capacity_rows=64)
    added = whole.append_tracked(blk, cnt, ids, T, azi, W, H, n)
    a = halves.append_tracked(torch.from_numpy(blk[:40]).to(DEV), torch.from_numpy(cnt[:40]).to(DEV), torch.from_numpy(ids[:40]).to(DEV), T[:40],
                              azi[:40], W, H, n1)
    assert halves.capacity == 2048 and tuple(halves._log.shape) == (2048, 14)
    b = halves.append_tracked(blk[40:], cnt[40:], ids[40:], T[40:], azi[40:], W, H, n)
    assert a + b == added == int((ids >= 0).sum()) and halves.capacity == (2048 if a + 1200 <= 2048 else 4096)      # growth kept the rows
    _same_store(_store_state(whole), _store_state(halves), "two calls of 40 frames against one of 80")
    assert whole.rows_uploaded == halves.rows_uploaded == 0 and whole.rows_emitted == halves.rows_emitted == added and not whole._grouped
    # ... and it is the restatement's log, and the host's marks of it
    log, tid = np.zeros((added, 14)), np.zeros(added, np.int32)
    R.emit(blk, cnt, ids, T, azi, W, H, n, log, tid, 0)
    got = _store_state(whole)
    assert np.array_equal(got[1], tid)
    _same_rows(got[0], log, "TrackRows.append_tracked")
    tracks = whole.host_tracks()
    assert whole.host_tracks() is tracks and whole.groupings == 1                  # cached
    assert [len(t) for t in tracks] == whole.lengths and np.array_equal(whole.marks, _marks_of(tracks))
    for t, w in zip(tracks, R.host_tracks(got[0], got[1], added, n)):
        assert t.shape == w.shape and np.array_equal(bits(t), bits(w))
    assert whole.sync(tracks) == 0 and whole.rows_uploaded == 0 and whole.loads == 0
    whole.append_tracked(blk[:1], cnt[:1], ids[:1], T[:1], azi[:1], W, H, n)
    assert whole.host_tracks() is not tracks                                       # ... until the next append


def test_packed_equals_a_store_loaded_with_host_tracks(fitter):
    """more than 256 tracks: the sort's two-pass range"""
    from odam_amd.track_store import TrackRows
    blk, cnt, _, T, azi = R.scene(137, 400, 9)
    ids, n = R.tracker_ids(cnt, 400, 9, grow=6)
    assert n > 256
    fed = TrackRows(fitter)
    fed.append_tracked(blk, cnt, ids, T, azi, W, H, n)
    tracks = fed.host_tracks()
    a = fed.packed()
    other = TrackRows(fitter)
    assert other.load(tracks) == fed.n_rows
    b = other.packed()
    assert fed.groupings == 1 and other.groupings == 0 and a["n_tracks"] == b["n_tracks"] == n and a["max_rows"] == b["max_rows"]
    assert np.array_equal(a["row_offsets"], b["row_offsets"])
    assert np.array_equal(bits(a["rows14"].cpu().numpy()), bits(b["rows14"].cpu().numpy()))
    a["check"]()


# ---- 3. end to end: the fixture scene through OdamProcess ----------------------------------------------------------------------------------
class _Det:
    device = DEV


N_E2E = 60


@pytest.fixture(scope="module")
def scene60(golden):
    import track_iou_ref
    z = golden("iou_tracking.npz")
    s = {q["name"]: q for q in track_iou_ref.fixture_scenes(z)}["many"]
    return {"blk": s["blk"][:N_E2E], "cnt": s["cnt"][:N_E2E], "fids": [int(x) for x in s["frame_ids"][:N_E2E]], "T": [t for t in s["T_wcs"][:N_E2E]],
            "ids": s["ids"][:N_E2E], "thr": track_iou_ref.fixture_thresholds(z), "w": float(z["img_w"]), "h": float(z["img_h"])}


def _proc(sc, fitter, **kw):
    from odam_amd import tracker
    from odam_amd.processor import OdamProcess
    proc = OdamProcess(_Det(), tracker.IouTracker(device=DEV, fitter=fitter, **sc["thr"], **kw), None, None, fitter=fitter)
    proc.init_sequence(K, int(sc["h"]), int(sc["w"]))
    return proc


def _feed(proc, sc, spans, resident):
    import torch
    for a, b in spans:
        proc.track_frames_packed(torch.from_numpy(sc["blk"][a:b]).to(DEV), torch.from_numpy(sc["cnt"][a:b]).to(DEV), sc["fids"][a:b], sc["T"][a:b],
                                 **({"resident": True} if resident else {}))
    return proc


def test_resident_tracking_equals_the_host_path(scene60, fitter):
    sc = scene60
    host = _feed(_proc(sc, fitter), sc, [(0, N_E2E)], False)
    res = _feed(_proc(sc, fitter), sc, [(0, N_E2E)], True)
    assert res._store_auth and res._tracks == [] and res.associator.n_tracks == host.associator.n_tracks and res._n_tracks == host._n_tracks > 10
    assert res.usable_frames == host.usable_frames == sc["fids"] and res.run_associator and len(res.T_wcs) == len(res.P_cws) == N_E2E
    assert np.array_equal(res.P_cws[7], host.P_cws[7])
    store = res._rows
    assert store.rows_uploaded == 0 and store.rows_emitted == store.n_rows == sum(len(t) for t in host.tracks)
    # the ids: the log's are the fixture's, slot by slot in arrival order
    T = np.stack(sc["T"])
    azi = np.array([R.cam_azi(t) for t in T])
    n = host._n_tracks
    log, tid = np.zeros((store.n_rows, 14)), np.zeros(store.n_rows, np.int32)
    want = R.emit(sc["blk"], sc["cnt"], sc["ids"], T, azi, int(sc["w"]), int(sc["h"]), n, log, tid, 0)
    assert want["n_emitted"] == store.n_rows and np.array_equal(store._tid[:store.n_rows].cpu().numpy(), tid)
    _same_rows(store._log[:store.n_rows].cpu().numpy(), log, "the fixture scene")
    # proc.tracks against the host path's list, within the contract
    got = res.tracks
    assert res.tracks is got and store.rows_uploaded == 0 and len(got) == len(host.tracks) == n
    order = np.argsort(tid, kind="stable")
    on = R.flags(sc["cnt"], sc["ids"], n)[0]
    bound = R.centre_bound(sc["blk"], T)[on][order]
    o = 0
    for g, w in zip(got, host.tracks):
        assert g.shape == w.shape and g.dtype == w.dtype
        cols = [c for c in range(82) if c not in (9, 10, 11, 12)]
        assert np.array_equal(bits(g[:, cols]), bits(w[:, cols]))
        assert (np.abs(g[:, 9:12] - w[:, 9:12]) <= bound[o:o + len(g)]).all()
        _col12(g[:, 12], w[:, 12], "proc.tracks against the host path, a track of %d rows" % len(g))
        o += len(g)
    # chunked feeding gives the same store
    parts = _feed(_proc(sc, fitter), sc, [(0, 20), (20, 40), (40, 60)], True)
    _same_store(_store_state(store), _store_state(parts._rows), "3 x 20 frames")
    assert parts.usable_frames == sc["fids"] and parts._rows.rows_uploaded == 0


def test_overflow_keeps_the_frames_before_it(scene60, fitter):
    from odam_amd import tracker
    sc = scene60
    host, res = _proc(sc, fitter, max_tracks=12), _proc(sc, fitter, max_tracks=12)
    with pytest.raises(tracker.TrackOverflow) as eh:
        _feed(host, sc, [(0, N_E2E)], False)
    with pytest.raises(tracker.TrackOverflow) as er:
        _feed(res, sc, [(0, N_E2E)], True)
    f = er.value.frame
    assert 0 < f == eh.value.frame < N_E2E and res.usable_frames == host.usable_frames == sc["fids"][:f] and res._n_tracks == host._n_tracks <= 12
    assert [len(t) for t in res.tracks] == [len(t) for t in host.tracks] and res._rows.rows_uploaded == 0


def _same_result(a, b):
    for k in ("params", "bboxes_qc", "bboxes_dl"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert np.array_equal(a["fitted"], b["fitted"])


def test_refine_evaluate_and_map_scene_on_the_resident_sequence(scene60):
    from odam_amd import multi_view, pipeline
    sc = scene60
    fitter = multi_view.default_fitter(DEV)
    res = _feed(_proc(sc, fitter), sc, [(0, N_E2E)], True)
    store = res._rows
    # refine from the store as it stands: no sync, no upload; the list arrives for the result dict only
    out = res.refine(n_iters=20, return_params=True, prelude="resident")
    assert res._store_auth and store.rows_uploaded == 0 and store.loads == 1 and out["tracks"] is res.tracks and out["fitted"].sum() > 3
    ref = _feed(_proc(sc, fitter), sc, [(0, N_E2E)], False)
    ref.tracks = [t.copy() for t in res.tracks]                                    # the reloaded rows: the host list is the record there
    _same_result(out, ref.refine(n_iters=20, return_params=True, prelude="device"))
    res.refine_fitter.close(); ref.refine_fitter.close()
    assert res.closed_form_quadrics() is not None and res.reprojection(res.tracks, out["quadrics"]) is not None
    fit = np.nonzero(out["fitted"])[0]
    ev = res.evaluate(out, np.asarray(out["bboxes_qc"])[fit], np.array([out["quadrics"][i].obj_class for i in fit]))
    assert ev is not None and res._store_auth
    # map_scene from the store against map_scene on the reloaded rows
    st_a, st_b = {}, {}
    a = pipeline.map_scene(res, resident_rows=True, loaded=True, stages=st_a)
    assert store.rows_uploaded == 0 and store.loads == 1 and not res._store_auth
    b = pipeline.map_scene(ref, resident_rows=True, stages=st_b)
    _same_result(st_a["first_pass"], st_b["first_pass"])
    _same_result(a, b)
    assert len(a["tracks"]) == len(b["tracks"]) <= len(ref.tracks)
    for x, y in zip(a["tracks"], b["tracks"]):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    # proc.tracks is the unmerged host list now
    assert len(res.tracks) == len(ref.tracks) and all(x.tobytes() == y.tobytes() for x, y in zip(res.tracks, ref.tracks))
    with pytest.raises(ValueError):
        pipeline.map_scene(ref, loaded=True)
