"""The device-resident row store on the device: odam_rows_group / odam_rows_gather14 (csrc/track_rows.hip) against their
numpy restatement (tests/track_rows_ref.py), track_store.TrackRows against the host track list it mirrors, and the consumers --
SqFitter.prepare(max_rows=), multi_view.optim_process(rows=), OdamProcess.refine(prelude="resident"), pipeline.map_scene(resident_rows=True)
-- against the paths they stand in for.  Every comparison is exact: integers equal, rows compared as uint64 words.

Raw calls run on buffers that hold a fill value, with canary words on both sides of src_out and behind the workspace."""
import ctypes

import numpy as np
import pytest
import torch

import e2e_lib
import sq_prepare_ref as P
import track_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 200)
    yield f
    f.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def raw_group(tid, n_tracks, row_off, N=None):
    """odam_rows_group on canaried buffers -> (return code, status word, src [N], canaries intact)"""
    from odam_amd import _lib, track_store as ts
    tid = np.ascontiguousarray(tid, np.int32)
    N = len(tid) if N is None else N
    d_tid = torch.from_numpy(tid).to(DEV) if len(tid) else torch.zeros(1, device=DEV, dtype=torch.int32)
    d_off = torch.from_numpy(np.ascontiguousarray(row_off, np.int32)).to(DEV)
    src = torch.full((N + 2 * PAD,), R.FILL_I, device=DEV, dtype=torch.int32) if N <= 2 ** 24 else torch.full((2 * PAD,), R.FILL_I, device=DEV, dtype=torch.int32)
    status = torch.full((1 + 2 * PAD,), R.FILL_I, device=DEV, dtype=torch.int32)
    nbytes = ts.group_workspace(min(N, ts.MAX_ROWS), min(n_tracks, ts.MAX_TRACKS))
    work = torch.full((nbytes + 256,), 0x5A, device=DEV, dtype=torch.uint8)
    rc = ts._entry("odam_rows_group")(_lib.ptr(d_tid), N, n_tracks, _lib.ptr(d_off), _lib.ptr(src[PAD:]), _lib.ptr(status[PAD:]), _lib.ptr(work),
                                      nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h, st = src.cpu().numpy(), status.cpu().numpy()
    keep = N if N <= 2 ** 24 else 0
    intact = bool((h[:PAD] == R.FILL_I).all() and (h[PAD + keep:] == R.FILL_I).all() and (st[:PAD] == R.FILL_I).all() and (st[PAD + 1:] == R.FILL_I).all()
                  and (work[nbytes:] == 0x5A).all().item())
    return rc, int(st[PAD]), h[PAD:PAD + keep], intact


def raw_gather(rows, src):
    from odam_amd import track_store as ts
    n = len(src)
    out = torch.full((n + 4, 14), float("nan"), device=DEV, dtype=torch.float64)
    got = ts.gather14(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(np.ascontiguousarray(src, np.int32)).to(DEV), out=out)
    torch.cuda.synchronize()
    assert got.shape[0] == n and np.isnan(out[n:].cpu().numpy()).all()
    return got.cpu().numpy()


def _ids(n_rows, n_tracks, seed):
    """ids over a random ~70 % of the tracks (the rest stay empty), the last track among them"""
    rs = np.random.RandomState(seed)
    live = np.flatnonzero(rs.uniform(size=n_tracks) < 0.7)
    live = np.union1d(live, [n_tracks - 1])
    if n_tracks > 2:
        live = live[live != 1]
    return rs.choice(live, n_rows).astype(np.int32)


def _shapes():
    from odam_amd.track_store import CHUNK      # the implementation's chunk: the sizes around it follow it
    one = [(n, 1) for n in (1, 63, 64, 65)]
    around = [(n, 5) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)]
    tracks = [(3000, t) for t in (1, 2, 255, 256, 257, 4097)]
    return one + around + tracks + [(3 * CHUNK + 17, 4097)]


@pytest.mark.parametrize("n_rows,n_tracks", _shapes())
def test_group_and_gather_equal_the_restatement(n_rows, n_tracks):
    tid = _ids(n_rows, n_tracks, n_rows + n_tracks)
    off = R.offsets(tid, n_tracks)
    if n_tracks > 2:
        assert (np.diff(off) == 0).any()      # some tracks are empty
    st, want = R.group(tid, n_tracks, off)
    assert st == R.OK
    rc, status, src, intact = raw_group(tid, n_tracks, off)
    assert rc == 0 and status == R.OK and intact
    assert np.array_equal(src, want)
    rows = R.bit_rows(n_rows, seed=n_tracks)
    assert np.array_equal(bits(raw_gather(rows, src)), bits(R.gather14(rows, want)))


def test_an_empty_log_launches_nothing():
    from odam_amd import track_store as ts
    rc, status, src, intact = raw_group(np.zeros(0, np.int32), 1, [0, 0])
    assert rc == 0 and status == R.FILL_I and intact and len(src) == 0      # not even the status word is written
    rc, status, src, intact = raw_group(np.zeros(5, np.int32), 0, [0], N=5)
    assert rc == 0 and status == R.FILL_I and (src == R.FILL_I).all() and intact
    assert ts.gather14(torch.zeros(1, 14, device=DEV, dtype=torch.float64), torch.zeros(0, device=DEV, dtype=torch.int32)).shape[0] == 0


@pytest.fixture(scope="module")
def scan():
    """700 tracks, 70,000 rows in frame order; rows with ordinary numbers (the frame id in column 0) so that they can be a track list too"""
    tid, frame, n_tracks = R.scan_log()
    rs = np.random.RandomState(8)
    rows = rs.standard_normal((len(tid), 14))
    rows[:, 0] = frame
    return tid, rows, n_tracks


def test_an_interleaved_scan(scan):
    tid, rows, n_tracks = scan
    off = R.offsets(tid, n_tracks)
    rc, status, src, intact = raw_group(tid, n_tracks, off)
    assert rc == 0 and status == R.OK and intact
    assert np.array_equal(src, np.argsort(tid, kind="stable"))
    brows = R.bit_rows(len(tid), seed=1)
    assert np.array_equal(bits(raw_gather(brows, src)), bits(brows[np.argsort(tid, kind="stable")]))


@pytest.mark.parametrize("n_tracks", [40, 700])
def test_statuses_and_bounds(n_tracks):
    """one and two passes: a bad id or a row count that is not the host's is a status; nothing is written outside src_out"""
    n = 5000
    tid = _ids(n, n_tracks, 9)
    off = R.offsets(tid, n_tracks)
    for bad_id in (-1, n_tracks, 2 ** 31 - 1, -2 ** 31):
        t = tid.copy()
        t[[17, n - 1]] = bad_id
        assert R.group(t, n_tracks, off)[0] == R.BAD_ID
        rc, status, src, intact = raw_group(t, n_tracks, off)
        assert rc == 0 and status == R.BAD_ID and intact, bad_id
    # one track a row short of what the host counted: the row belongs to its neighbour
    k = int(np.flatnonzero(np.diff(off) > 1)[3])
    t = tid.copy()
    t[np.flatnonzero(tid == k)[0]] = k + 1 if k + 1 < n_tracks else k - 1
    assert R.group(t, n_tracks, off)[0] == R.BAD_COUNT
    rc, status, src, intact = raw_group(t, n_tracks, off)
    assert rc == 0 and status == R.BAD_COUNT and intact
    # ... or is missing altogether (the offsets speak of one row more than the log has), or the offsets do not start at 0
    o2 = off.copy()
    o2[k + 1:] += 1
    assert R.group(tid, n_tracks, o2)[0] == R.BAD_COUNT
    rc, status, src, intact = raw_group(tid, n_tracks, o2)
    assert rc == 0 and status == R.BAD_COUNT and intact
    rc, status, src, intact = raw_group(tid, n_tracks, off + 1)
    assert rc == 0 and status == R.BAD_COUNT and intact
    # offsets that are wild numbers are only ever compared
    rc, status, src, intact = raw_group(tid, n_tracks, np.full(n_tracks + 1, -2 ** 31, np.int64))
    assert rc == 0 and status == R.BAD_COUNT and intact
    # and a bad id wins over a bad count
    t = tid.copy()
    t[0] = -5
    rc, status, src, intact = raw_group(t, n_tracks, o2)
    assert rc == 0 and status == R.BAD_ID and intact


def test_limits_are_refused_before_any_launch():
    from odam_amd import _lib, track_store as ts
    tid = np.zeros(8, np.int32)
    rc, status, src, intact = raw_group(tid, 1, [0, 8], N=2 ** 24 + 1)
    assert rc == 3 and status == R.FILL_I and intact and b"2^24" in _lib.lib().odam_last_error()      # ODAM_E_LIMIT
    rc, status, src, intact = raw_group(tid, 65537, np.zeros(4, np.int32))
    assert rc == 3 and status == R.FILL_I and (src == R.FILL_I).all() and intact
    z = torch.zeros(4, 14, device=DEV, dtype=torch.float64)
    rc = ts._entry("odam_rows_gather14")(_lib.ptr(z), _lib.ptr(torch.zeros(4, device=DEV, dtype=torch.int32)), 2 ** 24 + 1, _lib.ptr(z), None)
    assert rc == 3


# ---- TrackRows ----------------------------------------------------------------------------------------------------------------------------

def _tracks_at(tid, rows, k):
    """the host track list after the first k rows of the log: tracks are numbered in order of first appearance, so the list only grows"""
    t, r = tid[:k], rows[:k]
    n = int(t.max()) + 1 if k else 0
    order = np.argsort(t, kind="stable")
    cuts = np.cumsum(np.bincount(t, minlength=n))[:-1]
    return [np.ascontiguousarray(a) for a in np.split(r[order], cuts)] if k else []


def _block_is(block, tracks):
    rows, offs = P.pack(tracks)
    assert block["n_tracks"] == len(tracks) and np.array_equal(block["row_offsets"], offs) and block["row_offsets"].dtype == np.int64
    assert block["max_rows"] == (max(len(t) for t in tracks) if tracks else 0)
    got = block["rows14"]
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(rows), 14)
    torch.cuda.synchronize()
    block["check"]()
    assert np.array_equal(bits(got.cpu().numpy()), bits(rows))


def test_incremental_equals_whole(fitter, scan):
    from odam_amd.track_store import TrackRows
    tid, rows, n_tracks = scan
    store = TrackRows(fitter)
    cuts = [4000, 4100, 17000, 17001, 40321, 66000, 70000]      # seven uneven refreshes
    done = 0
    for i, k in enumerate(cuts):
        tracks = _tracks_at(tid, rows, k)
        assert store.sync(tracks) == k - done
        done = k
        assert store.rows_uploaded == k and store.loads == 1
        _block_is(store.packed(), tracks)
        assert store.groupings == i      # the first block is the load itself; every later one is sorted on the device
        assert store.packed() is store.packed() and store.groupings == i      # cached until rows are appended
    assert len(tracks) == n_tracks
    assert store.sync(tracks) == 0 and store.groupings == 6


@pytest.mark.parametrize("case", ["shortened", "first row replaced", "fewer tracks", "empty list"])
def test_sync_fallbacks_reload(fitter, scan, case):
    from odam_amd.track_store import TrackRows
    tid, rows, _ = scan
    store = TrackRows(fitter, capacity_rows=64)
    tracks = _tracks_at(tid, rows, 3000)
    assert store.sync(_tracks_at(tid, rows, 50)) == 50 and store.capacity == 64
    assert store.sync(_tracks_at(tid, rows, 300)) == 250 and store.capacity == 512      # grown past the 64 rows it began with: the content is kept
    _block_is(store.packed(), _tracks_at(tid, rows, 300))
    assert store.sync(tracks) == 2700 and store.loads == 1 and store.capacity == 4096
    _block_is(store.packed(), tracks)
    nxt = [t.copy() for t in tracks]
    if case == "shortened":
        nxt[3] = nxt[3][:-1]
    elif case == "first row replaced":
        nxt[5][0, 0] += 0.5
    elif case == "fewer tracks":
        nxt = nxt[:-2]
    else:
        nxt = []
    n = sum(len(t) for t in nxt)
    assert store.sync(nxt) == n and store.loads == 2 and store.rows_uploaded == 3000 + n
    _block_is(store.packed(), nxt)
    assert store.groupings == 2      # a load needs no kernel
    store.reset()
    assert store.n_rows == 0 and store.packed()["n_tracks"] == 0
    assert store.load([np.zeros((3, 14), np.float32)]) is None and store.load([np.zeros((0, 14))]) is None and store.loads == 2


def test_a_status_raises_behind_the_consumers_synchronisation(fitter, scan):
    from odam_amd import _lib
    from odam_amd.track_store import TrackRows
    tid, rows, _ = scan
    store = TrackRows(fitter)
    store.sync(_tracks_at(tid, rows, 500))
    store.sync(_tracks_at(tid, rows, 900))
    store.lengths[0] += 1      # the host's count and the log disagree
    store.lengths[1] -= 1
    block = store.packed()
    torch.cuda.synchronize()
    with pytest.raises(_lib.OdamError, match="status 2"):
        block["check"]()


# ---- the consumers ------------------------------------------------------------------------------------------------------------------------

def test_prepare_with_device_offsets_and_max_rows(fitter):
    tracks, img_names, P_cws, img_h, img_w = P.random_tracks(13, 40)
    rows, offs = P.pack(tracks)
    d_rows = torch.from_numpy(rows).to(DEV)
    most = int(np.diff(offs).max())
    for rep in ("super_quadric", "dual_quadric"):
        a = fitter.prepare(d_rows, offs, img_names, P_cws, img_h, img_w, rep)
        b = fitter.prepare(d_rows, torch.from_numpy(offs).to(DEV), img_names, P_cws, img_h, img_w, rep, max_rows=most)
        assert not a["status"].any()
        for k in ("cls", "n_obs", "n_valid", "status"):
            assert np.array_equal(a[k], b[k]), k
        views = np.zeros(len(rows), bool)
        for o in range(len(tracks)):
            views[int(offs[o]):int(offs[o]) + int(a["n_obs"][o])] = True
        for k in ("init", "half_dims", "pose", "bboxes_dl", "row_offsets"):
            if a[k] is not None:
                assert np.array_equal(bits(a[k].cpu().numpy()), bits(b[k].cpu().numpy())), k
        assert np.array_equal(a["valid"].cpu().numpy(), b["valid"].cpu().numpy())
        for k in ("view_img", "view_row", "tgt", "mask", "P"):      # (words past a track's views are not written by either)
            assert np.array_equal(bits(a[k].cpu().numpy()[views]), bits(b[k].cpu().numpy()[views])), k
        # a launch sized for fewer rows than a track has refuses that track, as the header says
        small = 1 << ((most - 1).bit_length() - 1)      # (the launch holds a power of two of rows)
        c = fitter.prepare(d_rows, torch.from_numpy(offs).to(DEV), img_names, P_cws, img_h, img_w, rep, max_rows=small)
        assert small < most and np.array_equal(c["status"] == P.TOO_MANY_ROWS, np.diff(offs) > small)


class Spy:
    """wraps fit / fit_dual of the test's own fitter object: keeps host copies of what the prelude handed over"""

    def __init__(self, fitter):
        self.fitter, self.calls = fitter, []
        self._fit, self._fit_dual = fitter.fit, fitter.fit_dual
        fitter.fit, fitter.fit_dual = self.fit, self.fit_dual

    def restore(self):
        del self.fitter.fit, self.fitter.fit_dual

    @staticmethod
    def _np(x):
        return x.detach().cpu().numpy().copy() if torch.is_tensor(x) else np.array(x)

    def fit(self, params0, class_ids, view_counts, P, tgt, mask, **kw):
        self.calls.append(dict(init=self._np(params0), cls=[int(c) for c in class_ids], counts=[int(c) for c in view_counts], P=self._np(P).reshape(-1, 12),
                               tgt=self._np(tgt), mask=self._np(mask), state=None if kw.get("state") is None else self._np(kw["state"])))
        return self._fit(params0, class_ids, view_counts, P, tgt, mask, **kw)

    def fit_dual(self, init5, half_dims, view_counts, P, tgt, mask, **kw):
        self.calls.append(dict(init=self._np(init5), half=self._np(half_dims), cls=None, counts=[int(c) for c in view_counts],
                               P=self._np(P).reshape(-1, 12), tgt=self._np(tgt), mask=self._np(mask), state=None))
        return self._fit_dual(init5, half_dims, view_counts, P, tgt, mask, **kw)


def _same_call(a, b):
    assert a["counts"] == b["counts"] and a["cls"] == b["cls"]
    for k in ("init", "half", "P", "tgt", "mask", "state"):
        if a.get(k) is not None or b.get(k) is not None:
            assert a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]), bits(b[k])), k


def _same_result(a, b, keys=("params", "bboxes_qc", "bboxes_dl")):
    for k in keys:
        assert np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k]))), k
    assert np.array_equal(a["fitted"], b["fitted"])


@pytest.fixture(scope="module")
def fixture_scene(golden):
    z = golden("e2e.npz")
    seq, K, T_wcs, P_cws = e2e_lib.sequence_geometry()
    return z, seq, K, T_wcs, P_cws


@pytest.mark.parametrize("rep,w", [("super_quadric", 1), ("super_quadric", 2), ("dual_quadric", 1), ("dual_quadric", 2)])
def test_optim_process_from_the_block(fitter, fixture_scene, rep, w):
    """the block comes from a store that was fed in two refreshes, so its rows went through the sort and the gather"""
    from odam_amd import multi_view
    from odam_amd.track_store import TrackRows
    z, seq, K, T_wcs, P_cws = fixture_scene
    tracks = e2e_lib.reference_tracks(z, w)
    n_iters = 500 if rep == "dual_quadric" else 200
    store = TrackRows(fitter)
    store.sync([t[:max(1, len(t) // 2)] for t in tracks])
    assert store.sync(tracks) == sum(len(t) - max(1, len(t) // 2) for t in tracks)
    block = store.packed()
    assert store.groupings == 1 and store.loads == 1
    args = (seq["img_names"], T_wcs, P_cws, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"], K, rep, True, n_iters, 10)
    spy = Spy(fitter)
    try:
        dev = multi_view.optim_process([t.copy() for t in tracks], *args, fitter=fitter, return_params=True, prelude="device")
        res = multi_view.optim_process(None, *args, fitter=fitter, return_params=True, rows=block)
        late = multi_view.optim_process(lambda: tracks, *args, fitter=fitter, return_params=True, rows=block)
    finally:
        spy.restore()
    assert len(spy.calls) == 3 and dev["fitted"].sum() >= 9
    _same_call(spy.calls[0], spy.calls[1])
    _same_call(spy.calls[0], spy.calls[2])
    _same_result(dev, res)
    _same_result(dev, late)
    assert res["tracks"] is None and late["tracks"] is tracks and len(res["quadrics"]) == len(tracks)
    # where the device prelude does not apply: a host list is the fall-back, without one the call says which condition failed
    names2, P2 = list(seq["img_names"]) + [seq["img_names"][0]], np.concatenate([P_cws, P_cws[:1]])
    args2 = (names2, None, P2) + args[3:8] + (20, 10)
    with pytest.raises(ValueError, match="not all different"):
        multi_view.optim_process(None, *args2, fitter=fitter, rows=block)
    if rep == "super_quadric" and w == 2:
        a = multi_view.optim_process([t.copy() for t in tracks], *args2, fitter=fitter, return_params=True, rows=block)
        b = multi_view.optim_process([t.copy() for t in tracks], *args2, fitter=fitter, return_params=True, prelude="host")
        _same_result(a, b)
        with pytest.raises(ValueError, match="rows holds"):
            multi_view.optim_process(tracks[:-1], *args, fitter=fitter, rows=block)
        lost = [t.copy() for t in tracks]
        lost[1][:, 0] = 10 ** 6      # a track without a view: the kernel's status
        gone = TrackRows(fitter)
        gone.load(lost)
        with pytest.raises(ValueError, match="status"):
            multi_view.optim_process(None, *args, fitter=fitter, rows=gone.packed())


def test_refine_twice_resident_equals_device(fixture_scene):
    from odam_amd.processor import OdamProcess
    z, seq, K, T_wcs, P_cws = fixture_scene
    full = e2e_lib.reference_tracks(z, 1)
    early = [t[:max(1, 2 * len(t) // 3)] for t in full]
    states = {}
    for prelude in ("device", "resident"):
        proc = OdamProcess(None, None, None, None)
        proc.init_sequence(K, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"])
        proc.usable_frames, proc.T_wcs, proc.P_cws = seq["img_names"], T_wcs, P_cws
        assert proc.resident_rows is False and proc._rows is None and proc._prelude(None) == "host"
        proc.tracks = [t.copy() for t in early]
        a = proc.refine(n_iters=50, return_params=True, prelude=prelude)
        first = proc._refine_state
        if prelude == "resident":
            assert proc._rows.rows_uploaded == sum(len(t) for t in early) and proc._rows.loads == 1
            proc.resident_rows = True      # refine(prelude=None) reads the attribute
            assert proc._prelude(None) == "resident"
        proc.tracks = [t.copy() for t in full]
        b = proc.refine(n_iters=50, return_params=True, prelude=None if prelude == "resident" else prelude)
        if prelude == "resident":      # the second call sent the rows the scan added, and nothing else
            assert proc._rows.rows_uploaded == sum(len(t) for t in full) and proc._rows.loads == 1 and proc._rows.groupings == 1
        st = proc._refine_state
        states[prelude] = (first["track_ids"].tolist(), torch.as_tensor(first["state"]).cpu().numpy(), st["track_ids"].tolist(),
                           torch.as_tensor(st["state"]).cpu().numpy(), a, b)
        if prelude == "resident":
            proc.init_sequence(K, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"])
            assert proc._rows.n_rows == 0 and proc._rows.lengths == []
        proc.refine_fitter.close()
    d, r = states["device"], states["resident"]
    assert d[0] == r[0] and d[2] == r[2] and len(d[2]) > len(d[0]) > 0
    assert np.array_equal(bits(d[1]), bits(r[1])) and np.array_equal(bits(d[3]), bits(r[3]))      # every state row, both calls
    _same_result(d[4], r[4])
    _same_result(d[5], r[5])


class _CountingNumpy:
    """numpy with a concatenate that counts the calls made on track rows: a list of [k, 14] arrays"""

    def __init__(self):
        self.track_row_calls = 0

    def __getattr__(self, name):
        return getattr(np, name)

    def concatenate(self, arrays, *a, **k):
        if isinstance(arrays, (list, tuple)) and len(arrays) and all(isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[1] == 14 for x in arrays):
            self.track_row_calls += 1
        return np.concatenate(arrays, *a, **k)


def test_map_scene_resident_equals_map_scene(fixture_scene, monkeypatch):
    from odam_amd import merge, multi_view, pipeline, track_store
    from odam_amd.processor import OdamProcess
    z, seq, K, T_wcs, P_cws = fixture_scene
    tracks = e2e_lib.reference_tracks(z, 1)
    outs = {}
    for resident in (False, True):
        proc = OdamProcess(None, None, None, None, fitter=multi_view.default_fitter(DEV))
        proc.init_sequence(K, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"])
        proc.usable_frames, proc.T_wcs, proc.P_cws = seq["img_names"], T_wcs, P_cws
        proc.device_prelude = True
        proc.tracks = [t.copy() for t in tracks]
        counter = _CountingNumpy()
        for mod in (merge, multi_view, pipeline, track_store):
            monkeypatch.setattr(mod, "np", counter)
        stages = {}
        out2 = pipeline.map_scene(proc, resident_rows=resident, device_merge=True, stages=stages)
        monkeypatch.undo()
        outs[resident] = (stages["first_pass"], out2, counter.track_row_calls)
        assert set(stages) == {"fit1", "merge", "fit2", "first_pass"}
        if resident:
            assert proc._rows.loads == 1 and proc._rows.rows_uploaded == sum(len(t) for t in tracks) and proc._rows.groupings == 0
            # the store holds the merged tracks now: a refresh from the host list finds it in step
            assert proc._rows.sync(out2["tracks"]) == 0 and proc._rows.loads == 1
        else:
            assert proc._rows is None
    (a1, a2, n_host), (b1, b2, n_res) = outs[False], outs[True]
    assert n_host >= 3 and n_res == 0      # pass 1, the merge and pass 2 each concatenate the rows on the default path; none does here
    _same_result(a1, b1)
    _same_result(a2, b2)
    assert len(a2["tracks"]) == len(b2["tracks"]) < len(tracks)
    for x, y in zip(a2["tracks"], b2["tracks"]):
        assert x.shape == y.shape and x.shape[1] == 82 and np.array_equal(bits(x), bits(y))
    assert all(np.array_equal(x, y) for x, y in zip(b1["tracks"], tracks))
