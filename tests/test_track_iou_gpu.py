"""The gfx950 IoU tracker (odam_amd/csrc/track_iou.hip through odam_amd/tracker.py, OdamProcess and the raw entry points of
include/odam_track.h) against its numpy restatement tests/track_iou_ref.py and the reference-run fixture iou_tracking.npz
(make_golden_tracking.py: the reference's own match_tracks / convert_det_to_list).

What is asked:
  kernel == restatement   bit for bit in ids, iou2d and iou3d, on every fixture scene: the same binary64 operations in the same order,
                          no contraction, IEEE division.
  kernel == reference     ids exactly (the fixture's margin >= 1e-9 makes that a fair demand, see iou_tracking.md).
  resumable, batched      one call == calls over chunks of 1, 7 and N - 1 frames on one state; several sequences in one launch == each
                          alone; all bit for bit.
  untouched words         output buffers are 3 frames longer than needed and start as sentinels: words no slot owns keep them, and so do
                          the slots from an overflow frame on.
Sizes are the fixture's: <= 150 frames (210 for the scene that must reach a track of 200 observations, 1 - 3 detections per frame),
<= 30 detections per frame, 99 tracks in the largest scene (the second lane chunk)."""
import ctypes

import numpy as np
import pytest

import track_iou_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = np.array([[1170.0, 0, 648.0], [0, 1170.0, 484.0], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 200)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fx(golden):
    """the fixture's scenes and the restatement's run of each, computed once and left unchanged"""
    z = golden("iou_tracking.npz")
    scenes = R.fixture_scenes(z)
    thr = R.fixture_thresholds(z)
    w, h = float(z["img_w"]), float(z["img_h"])
    for s in scenes:
        s["want"] = R.run(s["blk"], s["cnt"], s["frame_ids"], s["T_wcs"], w, h, **thr)[:3]
    return {"scenes": scenes, "thr": thr, "w": w, "h": h, "by": {s["name"]: s for s in scenes}}


def _tracker(fx, fitter, **kw):
    from odam_amd import tracker
    return tracker.IouTracker(device=DEV, fitter=fitter, **fx["thr"], **kw)


def _inputs(s, a=0, b=None):
    return s["blk"][a:b], s["cnt"][a:b], s["frame_ids"][a:b], s["T_wcs"][a:b]


def _same(got, want, what):
    for k, name in enumerate(("ids", "iou2d", "iou3d")):
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, name)
        assert g.tobytes() == want[k].tobytes(), (what, name, int((g != want[k]).sum()))


# ---- 1. the kernel against the restatement and the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_kernel_equals_restatement_and_reference(fx, fitter, k):
    s = fx["scenes"][k]
    trk = _tracker(fx, fitter)
    trk.reset()
    got = trk.step(*_inputs(s), fx["w"], fx["h"])
    assert got[0].is_cuda and tuple(got[0].shape) == (len(s["cnt"]), 30)
    _same(got, s["want"], s["name"])
    ids = got[0].cpu().numpy()
    assert np.array_equal(ids, s["ids"]), s["name"]                                   # the reference's ids
    assert np.array_equal(R.member_rows(ids, s["cnt"]), s["members"])                  # ... and track membership
    assert trk.n_tracks == [s["n_tracks"]]
    e2 = np.abs(got[1].cpu().numpy() - s["iou2d"]).max(); e3 = np.abs(got[2].cpu().numpy() - s["iou3d"]).max()
    print("%s: kernel vs the reference's deciding IoUs: 2D %.3g, 3D %.3g" % (s["name"], e2, e3))
    assert max(e2, e3) <= 1e-12
    if s["name"] == "many":
        assert 64 < trk.n_tracks[0] < 128 and (ids >= 64).sum() > 20


# ---- 2. one state, many calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, -1])
def test_chunked_calls_equal_one_call(fx, fitter, chunk):
    s = fx["by"]["many"]
    N = len(s["cnt"])
    step = N - 1 if chunk < 0 else chunk
    trk = _tracker(fx, fitter)
    trk.reset()
    parts = [trk.step(*_inputs(s, a, min(N, a + step)), fx["w"], fx["h"]) for a in range(0, N, step)]
    got = [np.concatenate([p[k].cpu().numpy() for p in parts]) for k in range(3)]
    _same(got, s["want"], "chunks of %d" % step)
    assert trk.n_tracks == [s["n_tracks"]]


# ---- 3. several sequences in one launch -------------------------------------------------------------------------------------------
def test_sequences_in_one_launch(fx, fitter):
    many, long_, ordered = fx["by"]["many"], fx["by"]["long"], fx["by"]["ordered"]
    empty = {"blk": many["blk"][:0], "cnt": many["cnt"][:0], "frame_ids": many["frame_ids"][:0], "T_wcs": many["T_wcs"][:0],
             "want": tuple(x[:0] for x in many["want"]), "n_tracks": 0}
    for seqs in ([many, ordered], [ordered, empty, many, long_, ordered]):
        trk = _tracker(fx, fitter)
        trk.reset(len(seqs))
        out = trk.step_scenes([q["blk"] for q in seqs], [q["cnt"] for q in seqs], [q["frame_ids"] for q in seqs], [q["T_wcs"] for q in seqs],
                              fx["w"], fx["h"])
        assert len(out) == len(seqs)
        for i, (q, o) in enumerate(zip(seqs, out)):
            _same(o, q["want"], "sequence %d of %d" % (i, len(seqs)))
        assert trk.n_tracks == [q["n_tracks"] for q in seqs]
        # ... and they continue independently: the second half of `many` after its first half, beside a fresh `ordered`
    trk = _tracker(fx, fitter)
    trk.reset(2)
    a = trk.step_scenes([many["blk"][:70], ordered["blk"][:0]], [many["cnt"][:70], ordered["cnt"][:0]], [many["frame_ids"][:70], []],
                        [many["T_wcs"][:70], ordered["T_wcs"][:0]], fx["w"], fx["h"])
    b = trk.step_scenes([many["blk"][70:], ordered["blk"]], [many["cnt"][70:], ordered["cnt"]], [many["frame_ids"][70:], ordered["frame_ids"]],
                        [many["T_wcs"][70:], ordered["T_wcs"]], fx["w"], fx["h"])
    _same([np.concatenate([a[0][k].cpu().numpy(), b[0][k].cpu().numpy()]) for k in range(3)], many["want"], "many in two calls")
    _same(b[1], ordered["want"], "ordered beside it")


def test_no_frames_and_no_detections(fx, fitter):
    many = fx["by"]["many"]
    trk = _tracker(fx, fitter)
    trk.reset()
    got = trk.step(*_inputs(many, 0, 0), fx["w"], fx["h"])                       # a sequence of 0 frames
    assert tuple(got[0].shape) == (0, 30) and trk.n_tracks == [0]
    blk = many["blk"][:5].copy()                                                 # frames of 0 detections: rows present, counts 0
    got = trk.step(blk, np.zeros(5, np.int32), many["frame_ids"][:5], many["T_wcs"][:5], fx["w"], fx["h"])
    assert (got[0].cpu().numpy() == -1).all() and (got[1].cpu().numpy() == -1).all() and (got[2].cpu().numpy() == -1).all()
    assert trk.n_tracks == [0]
    # the fixture's own empty frames sit between frames with detections; after the two calls above the state is still that of an empty sequence
    assert (many["cnt"][:20] == 0).any()
    got = trk.step(*_inputs(many, 0, 20), fx["w"], fx["h"])
    _same(got, [x[:20] for x in many["want"]], "after empty calls")


def _edge_scene():
    """12 frames the fixture cannot have: score ties (scores drawn from four values, 30 detections on six places of two classes), NaN
    scores, boxes over and wholly outside the image (zero area after the clip), detections without volume (0 / 0 = NaN IoUs with the
    tracks they start), counts outside 0 .. 30"""
    rs = np.random.RandomState(5)
    N = 12
    T = np.tile(np.eye(4), (N, 1, 1))
    for f in range(N):
        c, s_ = np.cos(0.1 * f), np.sin(0.1 * f)
        T[f, :3, :3] = [[c, -s_, 0], [s_, c, 0], [0, 0, 1]]
        T[f, :3, 3] = [0.3 * f, -0.2 * f, 1.0]
    place = rs.uniform(-2, 2, (6, 3)); dims = rs.uniform(0.5, 1.0, (6, 3)); bc = rs.uniform(0.2, 0.8, (6, 2))
    blk = np.full((N, 30, 15), -1.0, np.float32)
    for f in range(N):
        for d in range(30):
            o = rs.randint(0, 6)
            c2 = bc[o] + rs.normal(0, 0.06, 2)
            t_co = T[f, :3, :3].T @ (place[o] + rs.normal(0, 0.3, 3) - T[f, :3, 3])
            blk[f, d] = np.r_[f, o % 2, c2 - 0.1, c2 + 0.1, dims[o] * (1 + rs.normal(0, 0.03, 3)), t_co, 0, 1, rs.choice([0.7, 0.8, 0.85, 0.9])]
    blk[1, 3, 14] = np.nan; blk[4, 0, 14] = np.nan; blk[4, 7, 14] = np.nan                  # NaN scores: first in the order, "not below" the threshold
    blk[2, 5, 2:6] = [-0.3, -0.2, 0.1, 0.15]; blk[2, 6, 2:6] = [0.9, 0.85, 1.4, 1.2]        # over the border
    blk[3, 2, 2:6] = [1.1, 1.2, 1.3, 1.4]; blk[3, 2, 14] = 0.95                              # wholly outside: zero area, starts a track
    blk[3, 9, 6:9] = 0.0; blk[3, 9, 14] = 0.95                                               # no volume
    blk[5, 1, 2:6] = [1.1, 1.2, 1.3, 1.4]; blk[5, 1, 6:9] = 0.0                              # meets both: NaN IoUs, never matches
    blk[6, 4, 9:12] = np.nan                                                                 # a NaN centre
    cnt = np.array([30, 30, 30, 30, 35, 30, 30, -2, 0, 30, 7, 30], np.int32)
    fid = np.array([0, 1, 2, 3, 4, 9, 10, 11, 12, 20, 21, 22], np.int32)
    return blk, cnt, fid, T


@pytest.mark.parametrize("thr", [{}, dict(match_threshold=0.3, track_threshold=0.75, iou3d_threshold=0.1, max_gap=2)])
def test_ties_nan_degenerate_inputs_and_other_thresholds(fx, fitter, thr):
    from odam_amd import tracker
    blk, cnt, fid, T = _edge_scene()
    with np.errstate(all="ignore"):
        want = R.run(blk, cnt, fid, T, fx["w"], fx["h"], **thr)
    assert want[3].n > 64 and np.isnan(want[3].lo[:, :want[3].n]).any()       # a second lane chunk; a track with a NaN box
    assert len(np.unique(blk[0, :, 14])) <= 4                                  # ties
    trk = tracker.IouTracker(device=DEV, fitter=fitter, **thr)
    trk.reset()
    got = trk.step(blk, cnt, fid, T, fx["w"], fx["h"])
    _same(got, want[:3], "edge scene %r" % (thr,))
    assert trk.n_tracks == [want[3].n]
    if thr:      # the thresholds are honoured: the default run differs
        with np.errstate(all="ignore"):
            base = R.run(blk, cnt, fid, T, fx["w"], fx["h"])
        assert not np.array_equal(base[0], want[0])


# ---- 4. raw entry points: untouched words, overflow, argument checks -------------------------------------------------------------
SENT_I, SENT_D = -77, -1234.5
TAIL = 3


def _raw(fitter, fx, s, cap, prefill=None, state=None, **bad):
    """odam_track_iou_step on one sequence with output buffers TAIL frames longer than the frames; the frames' slots start as `prefill`
    (-1, what a caller pre-fills; or the sentinel), the tail as sentinels -> rc, ids, iou2d, iou3d, n_tracks, header, state"""
    import torch
    from odam_amd import _lib, tracker
    N = len(s["cnt"])
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(DEV)
    blk, cnt, fid, T = d(s["blk"], np.float32), d(s["cnt"], np.int32), d(s["frame_ids"], np.int32), d(s["T_wcs"], np.float64)
    off = d(np.array([0, N]), np.int32)
    per = tracker._entry("odam_track_iou_state_bytes")(cap)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if state is None:
        state = torch.zeros(max(per, 16) + 64, device=DEV, dtype=torch.uint8)
        state[max(per, 0):] = 0x5A                                               # 64 guard bytes behind the block
        if per > 0:
            assert tracker._entry("odam_track_iou_reset")(fitter._h, _lib.ptr(state), 1, cap, stream) == 0
    ids = torch.full((N + TAIL, 30), SENT_I, device=DEV, dtype=torch.int32)
    o2 = torch.full((N + TAIL, 30), SENT_D, device=DEV, dtype=torch.float64)
    o3 = torch.full((N + TAIL, 30), SENT_D, device=DEV, dtype=torch.float64)
    if prefill is not None:
        ids[:N] = prefill; o2[:N] = prefill; o3[:N] = prefill
    nt = torch.full((1 + TAIL,), SENT_I, device=DEV, dtype=torch.int32)
    a = dict(ctx=fitter._h, n_seq=1, off=_lib.ptr(off), n_frames=N, blk=_lib.ptr(blk), cnt=_lib.ptr(cnt), fid=_lib.ptr(fid), T=_lib.ptr(T),
             state_ptr=_lib.ptr(state), max_tracks=cap, ids=_lib.ptr(ids), o2=_lib.ptr(o2), o3=_lib.ptr(o3), nt=_lib.ptr(nt))
    a.update(bad)
    t = fx["thr"]
    rc = tracker._entry("odam_track_iou_step")(a["ctx"], a["n_seq"], a["off"], a["n_frames"], a["blk"], a["cnt"], a["fid"], a["T"], fx["w"], fx["h"],
                                               t["match_threshold"], t["track_threshold"], t["iou3d_threshold"], t["max_gap"], a["state_ptr"],
                                               a["max_tracks"], a["ids"], a["o2"], a["o3"], a["nt"], stream)
    torch.cuda.synchronize()
    hdr = state[:32].view(torch.int32).cpu().numpy()
    return rc, ids.cpu().numpy(), o2.cpu().numpy(), o3.cpu().numpy(), nt.cpu().numpy(), hdr, state


def test_untouched_words(fx, fitter):
    s = fx["by"]["many"]
    N = len(s["cnt"])
    rc, ids, o2, o3, nt, hdr, state = _raw(fitter, fx, s, 128)
    assert rc == 0
    _same((ids[:N], o2[:N], o3[:N]), s["want"], "raw call")                       # every slot of every processed frame is written
    assert (ids[N:] == SENT_I).all() and (o2[N:] == SENT_D).all() and (o3[N:] == SENT_D).all()
    assert nt[0] == s["n_tracks"] and (nt[1:] == SENT_I).all() and hdr[:3].tolist() == [s["n_tracks"], -1, 128]
    assert (state[-64:].cpu().numpy() == 0x5A).all()                              # nothing behind the state block


def test_overflow_stops_before_the_frame(fx, fitter):
    from odam_amd import tracker
    s = fx["by"]["many"]
    N = len(s["cnt"])
    S = R.State(64)
    with pytest.raises(R.Overflow) as e:
        R.step(S, s["blk"], s["cnt"], s["frame_ids"], s["T_wcs"], fx["w"], fx["h"], **fx["thr"])
    f = e.value.frame
    assert 0 < f < N
    rc, ids, o2, o3, nt, hdr, state = _raw(fitter, fx, s, 64, prefill=-1)
    assert rc == 0 and hdr[1] == f and hdr[0] == nt[0] == S.n <= 64               # the call reports the overflow frame
    _same((ids[:f], o2[:f], o3[:f]), [x[:f] for x in s["want"]], "before the overflow frame")      # == the unlimited run
    assert (ids[f:N] == -1).all() and (o2[f:N] == -1).all() and (o3[f:N] == -1).all()              # the pre-filled -1, untouched
    assert (ids[N:] == SENT_I).all() and (o2[N:] == SENT_D).all() and (state[-64:].cpu().numpy() == 0x5A).all()
    # the host raises with that frame; the state is as after frame f - 1: frames without new tracks still go through
    trk = _tracker(fx, fitter, max_tracks=64)
    trk.reset()
    with pytest.raises(tracker.TrackOverflow) as te:
        trk.step(*_inputs(s), fx["w"], fx["h"])
    assert te.value.frame == f and te.value.frame_id == int(s["frame_ids"][f]) and te.value.sequence == 0 and str(f) in str(te.value)
    _same([x[:f] for x in te.value.outputs], [x[:f] for x in s["want"]], "TrackOverflow.outputs")
    assert trk.n_tracks == [S.n]
    again = trk.step(*_inputs(fx["by"]["many"], 0, 0), fx["w"], fx["h"])
    assert tuple(again[0].shape) == (0, 30) and trk.header()[0].tolist() == [S.n, -1, 64]


def test_abi_argument_checks(fx, fitter):
    from odam_amd import _lib, tracker
    s = fx["by"]["ordered"]
    null = ctypes.c_void_p(0)
    assert tracker._entry("odam_track_iou_state_bytes")(0) == -1 and tracker._entry("odam_track_iou_state_bytes")(-5) == -1
    assert tracker._entry("odam_track_iou_state_bytes")(65537) == -1
    b1, b1024 = tracker._entry("odam_track_iou_state_bytes")(1), tracker._entry("odam_track_iou_state_bytes")(1024)
    assert b1 % 16 == 0 and b1 >= 32 + 140 and b1024 % 16 == 0 and b1024 >= 32 + 140 * 1024
    _, _, _, _, _, _, state = _raw(fitter, fx, s, 16)
    for bad in (dict(ctx=null), dict(off=null), dict(blk=null), dict(cnt=null), dict(fid=null), dict(T=null), dict(state_ptr=null), dict(ids=null),
                dict(o2=null), dict(o3=null), dict(nt=null), dict(n_seq=-1), dict(n_frames=-1), dict(max_tracks=0), dict(max_tracks=-3)):
        rc, ids, o2, o3, nt, hdr, _ = _raw(fitter, fx, s, 16, state=state, **bad)
        assert rc == 1 and b"odam_track_iou_step" in _lib.lib().odam_last_error(), bad      # ODAM_E_INVALID, and no launch:
        assert (ids == SENT_I).all() and (o2 == SENT_D).all() and (o3 == SENT_D).all() and (nt == SENT_I).all(), bad
    rc, ids, _, _, nt, _, _ = _raw(fitter, fx, s, 16, state=state, max_tracks=65537)
    assert rc == 3 and (ids == SENT_I).all()                                              # ODAM_E_LIMIT
    import torch
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    reset = tracker._entry("odam_track_iou_reset")
    assert reset(null, _lib.ptr(state), 1, 16, stream) == 1 and reset(fitter._h, null, 1, 16, stream) == 1
    assert reset(fitter._h, _lib.ptr(state), -1, 16, stream) == 1 and reset(fitter._h, _lib.ptr(state), 1, 0, stream) == 1
    # a state block that was reset for another capacity is refused by the kernel, which then writes nothing but the sequence's -1
    rc, ids, o2, o3, nt, hdr, _ = _raw(fitter, fx, s, 8, state=state)
    assert rc == 0 and nt[0] == -1 and hdr[1] == -2 and (ids == SENT_I).all() and (o2 == SENT_D).all()
    with pytest.raises(ValueError):
        tracker.IouTracker(max_tracks=0)


# ---- 5. through OdamProcess -------------------------------------------------------------------------------------------------------
class _Det:
    device = DEV


def _proc(fx, fitter, **kw):
    from odam_amd.processor import OdamProcess
    proc = OdamProcess(_Det(), _tracker(fx, fitter, **kw), None, None, fitter=fitter)
    proc.init_sequence(K, int(fx["h"]), int(fx["w"]))
    return proc


def _check_tracks(proc, s):
    """rows == _track_rows of the member detections, membership == the fixture's"""
    tracks = proc.tracks
    assert len(tracks) == s["n_tracks"]
    rows_of = {}
    for t, f, d in s["members"]:
        if f not in rows_of:
            n = int(s["cnt"][f])
            rows_of[f] = proc._track_rows(s["blk"][f, :n].astype(np.float64), s["T_wcs"][f], with_code=False)
        rows_of.setdefault(("t", t), []).append(rows_of[f][d])
    for t in range(s["n_tracks"]):
        want = np.asarray(rows_of[("t", t)])
        assert tracks[t].shape == want.shape == (len(want), 82) and tracks[t].tobytes() == want.tobytes(), t


def test_process_frames_with_the_iou_tracker(fx, fitter):
    import torch
    from odam_amd import parallel
    s = fx["by"]["many"]
    N = len(s["cnt"])
    dets = parallel.unpack_detections(s["blk"], s["cnt"])
    T = [s["T_wcs"][i] for i in range(N)]
    fids = [int(x) for x in s["frame_ids"]]
    proc = _proc(fx, fitter)
    assert not proc._fast_ok()
    proc.process_frames(fids[:60], T[:60], dets[:60])                              # two calls: the tracker's state carries over
    proc.process_frames(fids[60:], T[60:], dets[60:])
    _check_tracks(proc, s)
    assert proc.usable_frames == fids and len(proc.T_wcs) == len(proc.P_cws) == N
    assert np.array_equal(proc.P_cws[7], K @ np.linalg.inv(T[7])[:3, :])
    # frame by frame, the reference's call (detections at hand, as a list of rows)
    one = _proc(fx, fitter)
    for i in range(25):
        one.process_frame(None, fids[i], T[i], detections=[list(r) for r in dets[i]])
    upto = [t[t[:, 0] <= fids[24]] for t in proc.tracks]
    assert len(one.tracks) == sum(len(t) > 0 for t in upto) > 10
    for a, b in zip(one.tracks, upto):
        assert a.tobytes() == b.tobytes()
    # the device block without a visit to the host before the launch
    packed = _proc(fx, fitter)
    packed.track_frames_packed(torch.from_numpy(s["blk"]).to(DEV), torch.from_numpy(s["cnt"]).to(DEV), fids, T)
    _check_tracks(packed, s)
    assert packed.usable_frames == fids
    # the back end works on the result unchanged
    out = proc.optim_process(proc.tracks)
    assert len(out["bboxes_qc"]) == len(out["quadrics"]) == s["n_tracks"] and np.asarray(out["bboxes_qc"]).shape == (s["n_tracks"], 8, 3)
    merged = proc.merge_process(out)
    assert 0 < len(merged) <= s["n_tracks"] and all(t.shape[1] == 82 for t in merged)
    # a new sequence starts from an empty tracker
    proc.init_sequence(K, int(fx["h"]), int(fx["w"]))
    proc.process_frames(fids[:3], T[:3], dets[:3])
    assert len(proc.tracks) == len(set(s["members"][s["members"][:, 1] < 3][:, 0].tolist()))


def test_process_overflow_raises_with_the_frame(fx, fitter):
    from odam_amd import parallel, tracker
    s = fx["by"]["many"]
    N = len(s["cnt"])
    proc = _proc(fx, fitter, max_tracks=64)
    with pytest.raises(tracker.TrackOverflow) as e:
        proc.process_frames([int(x) for x in s["frame_ids"]], list(s["T_wcs"]), parallel.unpack_detections(s["blk"], s["cnt"]))
    f = e.value.frame
    assert len(proc.usable_frames) == f and len(proc.tracks) <= 64
    assert sum(len(t) for t in proc.tracks) == int((s["members"][:, 1] < f).sum())


def test_run_scene_with_the_iou_tracker(fx, fitter):
    from odam_amd import parallel, pipeline
    s = fx["by"]["many"]
    n = 60
    dets = parallel.unpack_detections(s["blk"][:n], s["cnt"][:n])
    proc = _proc(fx, fitter)
    stages = {}
    out = pipeline.run_scene(proc, n, [int(x) for x in s["frame_ids"][:n]], list(s["T_wcs"][:n]), detect=lambda f0, f1: dets[f0:f1], chunk=25,
                             stages=stages)
    want = s["members"][s["members"][:, 1] < n]
    assert len(proc.tracks) == len(set(want[:, 0].tolist())) and sum(len(t) for t in proc.tracks) == len(want)
    assert set(out) >= {"tracks", "bboxes_qc", "bboxes_dl", "quadrics"} and 0 < len(out["tracks"]) <= len(proc.tracks)
    assert len(out["bboxes_qc"]) == len(out["tracks"]) and "associate" in stages


def test_the_network_associator_keeps_its_path(golden):
    """an OdamProcess with the association network still takes the fast path it took (its flag, not its time), and no tracker branch"""
    import os, sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import scene_weights
    from odam_amd import associator, sq
    from odam_amd.processor import OdamProcess
    z = golden("process_tracks.npz")
    ids = [int(f) for f in z["img_names"]][:6]
    T = [z["scene_T_wcs"][i] for i in range(len(ids))]
    dets = [np.asarray(z[f"det{f}"], np.float64).reshape(-1, 79) for f in ids]
    net = associator.Associator({"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                max_tracks=64, device=DEV)
    net.load_state_dict(scene_weights.make_scene_associator_state_dict(2, 8, seed=0))
    f = sq.SqFitter(DEV, 1)
    proc = OdamProcess(_Det(), net, None, None, fitter=f)
    proc.init_sequence(z["K"], 480, 640)
    assert not getattr(net, "iou_tracker", False) and proc._fast_ok()
    called = []
    proc._track_frames_iou = lambda *a, **k: called.append(1)
    proc.process_frames(ids, T, dets)
    assert proc._fast_ok() and getattr(proc, "_win", None) is not None and len(proc.tracks) >= 1 and not called
    net.close(); f.close()
