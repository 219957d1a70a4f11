"""What the association network is fed about the tracks, against references that share no code with the kernels:
(A) odam_sq_project_extents (csrc/sq_fit.hip, project_extent_kernel: channels 2..5 of every track row) against the longdouble
    restatement of tests/track_input_ref.py, from the surface points that tests/test_sq_gpu.py pins bit for bit to the oracle;
(B) the track-window store (odam_trackwin_*) at window sizes other than the associator's 100 against
    OdamProcess._preprocess_tracks, bit for bit, and the append that names a track twice."""
import ctypes

import numpy as np
import pytest
import torch

import track_input_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_FIX = np.array([[577.87, 0, 319.5], [0, 577.87, 239.5], [0, 0, 1.0]])
# every entry non-zero and different: skew, and a last row that makes the "depth" a combination of all three camera coordinates
K_GEN = np.array([[577.87, 1.7, 319.5], [-0.9, 561.3, 239.5], [1e-4, -2e-4, 1.0]])


def _camera(rs, t_scale=1.0):
    Q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    T_wc = np.eye(4); T_wc[:3, :3] = Q; T_wc[:3, 3] = rs.normal(size=3) * t_scale
    return T_wc


def _objects(rs, n, T_wc, depth=(2.0, 6.0), dims=(0.1, 2.0), lateral=1.5, shapes=True):
    """[n, 9] float32 parameter rows (sq.init_params: centre, azimuth, sqrt(dims / 2), shape exponents) of objects whose centres lie at
    the given depth range in FRONT of the camera T_wc (negative depths: behind it)"""
    c_cam = np.concatenate([rs.uniform(-lateral, lateral, (n, 2)), rs.uniform(depth[0], depth[1], (n, 1))], axis=1)
    c_w = c_cam @ T_wc[:3, :3].T + T_wc[:3, 3]
    d = rs.uniform(dims[0], dims[1], (n, 3))
    p = np.zeros((n, 9))
    p[:, :3] = c_w
    p[:, 3] = rs.uniform(-3.5, 3.5, n)
    p[:, 4:7] = np.sqrt(np.maximum(d, 0.05) / 2)
    p[:, 7:] = rs.normal(0, 1.5, (n, 2)) if shapes else -0.0      # -0: what _prepare_tracks evaluates; others: other point sets
    return p.astype(np.float32)


def _cases():
    """(name, params [n, 9], T_cw, K, ordinary).  `ordinary`: every point well in front of the camera -- the cases the coverage condition is
    counted over and the fixed bounds (B <= 1e-6 px, agreement with float64 numpy) apply to; the test checks the depth itself."""
    rs = np.random.RandomState(20240611)
    out = []
    for n in (1, 4, 65, 129, 300):              # in this order on ONE fitter: the point buffer (128 objects at first) is grown at 129 and at 300
        T_wc = _camera(rs)
        out.append(("random-%d" % n, _objects(rs, n, T_wc, shapes=n != 65), np.linalg.inv(T_wc), K_FIX, True))
    T_wc = _camera(rs)
    out.append(("general-K", _objects(rs, 24, T_wc), np.linalg.inv(T_wc), K_GEN, True))
    T_wc = _camera(rs)
    out.append(("dims-at-the-clamp", _objects(rs, 12, T_wc, dims=(0.05, 0.05)), np.linalg.inv(T_wc), K_FIX, True))
    T_wc = _camera(rs)
    out.append(("dims-5m", _objects(rs, 12, T_wc, depth=(4.0, 8.0), dims=(5.0, 5.0)), np.linalg.inv(T_wc), K_GEN, True))
    T_wc = _camera(rs)
    out.append(("straddling", _objects(rs, 16, T_wc, depth=(-0.3, 0.3), dims=(1.0, 3.0)), np.linalg.inv(T_wc), K_FIX, False))
    T_wc = _camera(rs)
    out.append(("behind", _objects(rs, 12, T_wc, depth=(-6.0, -2.0)), np.linalg.inv(T_wc), K_GEN, False))
    # 1e4 m between camera and objects (depth 1e4: the division shrinks every error); the whole scene 1 km and 10 km from the world origin,
    # objects 2..6 m in front of the camera: T_cw's translation is then 1e3 / 1e4 m and the camera coordinates are differences of terms of
    # that size -- the cancellation is what the bound's S_k measures
    T_wc = _camera(rs)
    out.append(("objects-1e4m-away", _objects(rs, 12, T_wc, depth=(1e4, 1.0001e4), lateral=3e3), np.linalg.inv(T_wc), K_GEN, False))
    T_wc = _camera(rs); T_wc[:3, 3] += np.array([6e2, -7e2, 4e2])
    out.append(("scene-at-1e3m", _objects(rs, 12, T_wc), np.linalg.inv(T_wc), K_FIX, False))
    T_wc = _camera(rs); T_wc[:3, 3] += np.array([6e3, -7e3, 4e3])
    T_cw = np.linalg.inv(T_wc)
    assert np.linalg.norm(T_cw[:3, 3]) > 1e4
    out.append(("scene-at-1e4m", _objects(rs, 12, T_wc), T_cw, K_FIX, False))
    return out


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    return sq.SqFitter(DEV, 1)


def test_projected_extents_vs_longdouble(fitter, measured):
    """odam_sq_project_extents against tests/track_input_ref.py.  For each of the four extents of each object (a) some surface point's
    longdouble (u, v) lies within that point's own float64 rounding bound B of the device's value, and (b) no point lies beyond the device's
    value by more than its own B -- so the value is the extreme over ALL 1000 points (a dropped wave or stride fails (b)), computed by the
    stated formula to float64 rounding (a wrong entry of K or T fails (a)).  Where every point is at least 0.5 deep the bound itself is at most
    1e-6 px and the device agrees with the float64 numpy code of the host path to rtol 1e-12 / atol 1e-9.  The arg-extremes of the reference
    must fall in each of the kernel's four waves and in its last, partial stride (points 768..999), for minima and for maxima."""
    cases = _cases()
    # all calls first, back to back behind ~20 ms of work on the stream (a grown buffer must not be freed under a queued kernel), one synchronisation
    busy = torch.randn(2048, 2048, device=DEV)
    for _ in range(20):
        busy = busy @ busy * 1e-3
    dev = [fitter.project_extents(p, T_cw, K, on_device=True) for _, p, T_cw, K, _ in cases]
    torch.cuda.synchronize()
    del busy
    assert fitter.project_extents(np.zeros((0, 9), np.float32), cases[0][2], K_FIX).shape == (0, 4)       # n = 0: nothing to do, no error
    waves_lo, waves_hi, tail_lo, tail_hi, n_obj, problems = set(), set(), 0, 0, 0, []
    for (name, p, T_cw, K, ordinary), d in zip(cases, dev):
        d = d.cpu().numpy()
        pts = fitter.points(p).cpu().numpy()
        r = ref.extents(pts, T_cw, K)
        n = len(p)
        n_obj += n
        assert d.shape == (n, 4) and np.isfinite(d).all(), name
        deep = bool((r["depth"] >= 0.5).all())
        assert deep or not ordinary, name
        worst = 0.0
        for o in range(4):
            c, sign = o & 1, (1.0 if o < 2 else -1.0)                 # outputs 0, 1: minima of u, v; 2, 3: maxima
            x = r["uv"][:, :, c]                                       # [n, 1000] longdouble
            B = r["bound"][:, :, c]
            dd = d[:, o].astype(ref.LD)[:, None]
            near = (np.abs(dd - x) <= B).any(axis=1)
            if not near.all():
                problems.append("%s output %d: no point within its bound of the device's value for %d objects, first %d" % (name, o, (~near).sum(), np.flatnonzero(~near)[0]))
            beyond = sign * (dd - x) - B                               # > 0: the point lies past the device's extreme by more than its bound
            if not (beyond <= 0).all():
                i, j = np.argwhere(beyond > 0)[0]
                problems.append("%s output %d: %d points beyond the device's extreme, by up to %.3e px (first: object %d point %d, wave %d)"
                                % (name, o, (beyond > 0).sum(), float(beyond.max()), i, j, (j & 255) >> 6))
            a = r["arg"][:, o]
            ratio = np.abs(d[:, o].astype(ref.LD) - r["ext"][:, o]) / B[np.arange(n), a]
            worst = max(worst, float(ratio.max()))
            if ordinary:
                (waves_lo if o < 2 else waves_hi).update(((a & 255) >> 6).tolist())
                if o < 2:
                    tail_lo += int((a >= 768).sum())
                else:
                    tail_hi += int((a >= 768).sum())
        print("extents %-20s n %3d  max |device - longdouble| / B %.4f  max B %.3e px  min depth %.3g" % (name, n, worst, r["bound"].max(), r["depth"].min()))
        measured("track_input.extents." + name, worst)
        if deep:
            if not r["bound"].max() <= 1e-6:
                problems.append("%s: bound %.3e px above 1e-6" % (name, r["bound"].max()))
            f64 = ref.extents_f64(pts, T_cw, K)
            print("extents %-20s max |device - float64 numpy| %.3e px, largest |difference| / (1e-9 + 1e-12 |numpy|) %.3f"
                  % (name, np.abs(d - f64).max(), (np.abs(d - f64) / (1e-9 + 1e-12 * np.abs(f64))).max()))
            measured("track_input.extents_vs_numpy." + name, (np.abs(d - f64) / (1e-9 + 1e-12 * np.abs(f64))).max())
            if not np.allclose(d, f64, rtol=1e-12, atol=1e-9):
                problems.append("%s: differs from the float64 numpy code of the host path by up to %.3e px" % (name, np.abs(d - f64).max()))
    for line in problems:
        print("extents FAILS", line)
    assert not problems, problems
    assert n_obj >= 300
    assert waves_lo == {0, 1, 2, 3} and waves_hi == {0, 1, 2, 3}, (waves_lo, waves_hi)
    assert tail_lo >= 4 and tail_hi >= 4, (tail_lo, tail_hi)


# ---- (B) the track-window store at every window size -------------------------------------------------------------------------------
def _random_tracks(rs, lengths):
    tracks = []
    for n in lengths:
        t = rs.normal(0, 1, (n, 82)); t[:, 14:78] = -1
        t[:, 0] = np.arange(n) + rs.randint(0, 50)         # frame ids ascend inside a track
        tracks.append(t)
    return tracks


def _edge_proj(img_w, img_h):
    """[6, 4] projected boxes in pixels whose quotient by the image size sits on the clip's edges -1 and 2, one float64 ulp either side of
    them, and far outside (+-inf, +-1e300).  The ulp rows check that nothing goes wrong AT the edge; once the quotient is stored as float32
    they all read -1 or 2, so they cannot tell a clip done in double from one done in float."""
    iw, ih = float(img_w), float(img_h)
    e = np.nextafter
    rows = [[-iw, -ih, 2 * iw, 2 * ih],
            [e(-iw, -np.inf), e(-ih, -np.inf), e(2 * iw, np.inf), e(2 * ih, np.inf)],
            [e(-iw, np.inf), e(-ih, np.inf), e(2 * iw, -np.inf), e(2 * ih, -np.inf)],
            [-np.inf, np.inf, np.inf, -np.inf],
            [1e300, -1e300, -1e300, 1e300],
            [2 * iw, -ih, -iw, 2 * ih]]
    return np.array(rows)


@pytest.mark.parametrize("W", [1, 37, 64, 128])
def test_track_windows_at_other_window_sizes(W):
    """odam_trackwin_create accepts windows of 1..128 observations; the associator uses 100 and so did every test.  A store of window W, filled
    by odam_trackwin_load and again by appends (one observation per track and call), against _preprocess_tracks(n_times=W) on the host: the
    [T, 79, W] tensor bit for bit, for tracks of 1, W-1, W, W+1 and 3W+1 observations (ring wrap) and projected boxes on, beside and far
    outside the clip range [-1, 2] of proj / image size."""
    from odam_amd.associator import TrackWindows
    from odam_amd.processor import OdamProcess, get_cam_azi

    class Win(TrackWindows):
        WINDOW = W
    rs = np.random.RandomState(100 + W)
    proc = OdamProcess(None, None, None, None)
    proc.init_sequence(K_FIX, 480, 640)
    T_wc = _camera(rs)
    cam_azi = get_cam_azi(T_wc)
    lengths = [n for n in (1, W - 1, W, W + 1, 3 * W + 1) if n >= 1]
    lengths += list(rs.randint(1, 3 * W + 2, 12 - len(lengths)))
    tracks = _random_tracks(rs, lengths)
    assert len(tracks) == 12
    proj = rs.uniform(-200, 900, (12, 4))
    edge = _edge_proj(640, 480)
    proj[:len(edge)] = edge
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.ascontiguousarray(proc._preprocess_tracks(tracks, T_wc, cam_azi, n_times=W, proj_px=proj).transpose(0, 2, 1))
    assert want.shape == (12, 79, W)
    q = want[:, 2:6, 0]
    assert (q[:len(edge)] == -1).sum() >= 10 and (q[:len(edge)] == 2).sum() >= 10 and (np.abs(q[len(edge):] - 0.5) < 1.5).all()      # clipped and unclipped values both occur
    proj_dev = torch.from_numpy(proj).to(DEV)

    def device(win):
        return win.build(proj_dev, np.linalg.inv(T_wc), cam_azi, 640, 480).cpu().numpy()

    def same_bits(a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    win = Win(DEV, max_tracks=16)
    try:
        win.load(tracks)
        assert win.in_step(tracks)
        assert same_bits(device(win), want)
        win.reset()
        for j in range(max(lengths)):
            ids = [i for i, t in enumerate(tracks) if len(t) > j]
            win.append(ids, np.stack([tracks[i][j] for i in ids]))
        assert win.in_step(tracks)
        assert same_bits(device(win), want)
    finally:
        win.close()


def test_append_naming_a_track_twice_is_refused():
    """trackwin_append_kernel takes one workgroup per observation and reads the track's count once: two observations of one track in one call
    would be written to the same ring slot and counted once.  The entry refuses such a call (code 1) before it stages or launches anything; the
    store, its running sums and its staging ring are as they were, and the next valid append lands where it should."""
    from odam_amd import _lib
    from odam_amd.associator import TrackWindows
    from odam_amd.processor import OdamProcess, get_cam_azi
    rs = np.random.RandomState(3)
    proc = OdamProcess(None, None, None, None)
    proc.init_sequence(K_FIX, 480, 640)
    T_wc = _camera(rs)
    cam_azi = get_cam_azi(T_wc)
    tracks = _random_tracks(rs, [3, 120, 40, 7])
    proj = rs.uniform(-200, 900, (4, 4))
    proj_dev = torch.from_numpy(proj).to(DEV)

    def host(tr):
        return np.ascontiguousarray(proc._preprocess_tracks(tr, T_wc, cam_azi, proj_px=proj).transpose(0, 2, 1))
    win = TrackWindows(DEV, max_tracks=8)
    try:
        win.load(tracks)
        before = win.build(proj_dev, np.linalg.inv(T_wc), cam_azi, 640, 480).cpu().numpy()
        params_before = win.params()
        assert np.array_equal(before, host(tracks))
        extra = _random_tracks(rs, [3])[0]
        for ids in ([1, 1], [0, 2, 0], [3, 1, 2, 3]):
            ida = np.ascontiguousarray(ids, np.int32)
            rows = np.ascontiguousarray(np.repeat(extra[:1, :14], len(ids), 0))
            with torch.cuda.device(win.device):
                rc = _lib.lib().odam_trackwin_append(win._h, ctypes.c_int(len(ids)), ida.ctypes.data_as(ctypes.c_void_p),
                                                     rows.ctypes.data_as(ctypes.c_void_p), win._stream())
            assert rc == 1
            err = _lib.lib().odam_last_error().decode()
            assert err.startswith("odam_trackwin_append:") and "twice" in err, err
            with pytest.raises(_lib.OdamError, match="twice"):
                win.append(ids, np.repeat(extra[:1], len(ids), 0))
        torch.cuda.synchronize()
        assert np.array_equal(win.build(proj_dev, np.linalg.inv(T_wc), cam_azi, 640, 480).cpu().numpy(), before)
        assert np.array_equal(win.params().view(np.uint32), params_before.view(np.uint32))
        assert win.in_step(tracks)
        # the same rows, one call each: accepted
        win.append([1, 3], np.stack([extra[1], extra[2]]))
        grown = [t.copy() for t in tracks]
        grown[1] = np.concatenate([tracks[1], extra[1:2]]); grown[3] = np.concatenate([tracks[3], extra[2:3]])
        assert win.in_step(grown)
        assert np.array_equal(win.build(proj_dev, np.linalg.inv(T_wc), cam_azi, 640, 480).cpu().numpy(), host(grown))
    finally:
        win.close()
