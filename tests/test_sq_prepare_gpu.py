"""The fit prelude on the device: odam_sq_prepare_batch (csrc/sq_prepare.hip) against its numpy restatement (tests/sq_prepare_ref.py,
which tests/test_sq_prepare_host.py holds against the host path), and multi_view.optim_process / OdamProcess.refine with
prelude="device" against prelude="host" on the tracks of the whole-chain fixture.

Every raw call runs on buffers filled with the restatement's fill values, and whole buffers are compared: a word the kernel should not
have written shows like a wrong value does.  Bit for bit: the discrete outputs, tgt, mask, P, translate, scales, half_dims.  Yaw and
bboxes_dl: within 16 x the gap the host test measured between the restatement and scipy (sq_prepare_ref.YAW_GAP / BOX_GAP) -- both
sides are float64 evaluations of one quantity, the factor is for the device library's sin / cos / atan2 and the other summation order.
The float32 yaw entry: within 1 ulp."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import e2e_lib
import sq_prepare_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPS = ("super_quadric", "cube", "quadric", "dual_quadric")
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000]
YAW_TOL, BOX_TOL = 16 * R.YAW_GAP, 16 * R.BOX_GAP


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 200)
    yield f
    f.close()


def raw_prepare(fitter, rows, offs, img_names, P_cws, img_h, img_w, representation, thr=20.0, max_rows=None, n_obj=None):
    """odam_sq_prepare_batch on buffers that hold the restatement's fill values -> (return code, dict of numpy arrays)"""
    from odam_amd import _lib, sq
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 14)
    offs = np.asarray(offs, np.int64)
    n = len(offs) - 1 if n_obj is None else n_obj
    Rn = len(rows)
    ids, order = R.frame_tables(img_names)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dual = representation == "dual_quadric"
    fi = lambda *shape: torch.full(shape, R.FILL_I, device=DEV, dtype=torch.int32)
    ff = lambda dt, *shape: torch.full(shape, R.FILL_F, device=DEV, dtype=dt)
    b = {"cls": fi(max(n, 1)), "n_obs": fi(max(n, 1)), "n_valid": fi(max(n, 1)), "status": fi(max(n, 1)),
         "init": ff(torch.float32, max(n, 1), 5 if dual else 9), "half_dims": ff(torch.float32, max(n, 1), 3) if dual else None,
         "pose": ff(torch.float64, max(n, 1), 7), "bboxes_dl": ff(torch.float64, max(n, 1), 8, 3),
         "view_img": fi(Rn + 5), "view_row": fi(Rn + 5), "valid": fi(Rn + 5),
         "tgt": ff(torch.float32, Rn + 5, 4), "mask": ff(torch.float32, Rn + 5, 4), "P": ff(torch.float32, Rn + 5, 12)}
    d_rows = up(rows) if Rn else torch.zeros(1, 14, device=DEV, dtype=torch.float64)
    d_off, d_ids, d_ord, d_P = up(offs.astype(np.int32)), up(ids), up(order), up(np.asarray(P_cws, np.float64).reshape(-1, 12))
    if max_rows is None:
        max_rows = int(max(1, np.diff(offs).max())) if len(offs) > 1 else 1
    p = _lib.ptr
    rc = sq._prepare_entry()(fitter._h, n, p(d_off), p(d_rows), int(max_rows), len(ids), p(d_ids), p(d_ord), p(d_P), float(img_w), float(img_h),
                             float(thr), sq.REPRESENTATIONS[representation], p(b["cls"]), p(b["n_obs"]), p(b["n_valid"]), p(b["init"]),
                             p(b["half_dims"]), p(b["pose"]), p(b["bboxes_dl"]), p(b["status"]), p(b["view_img"]), p(b["view_row"]), p(b["tgt"]),
                             p(b["mask"]), p(b["P"]), p(b["valid"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: (None if v is None else v.cpu().numpy()) for k, v in b.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_against_ref(got, ref, n, Rn):
    """whole buffers: the first n per-track rows and Rn per-view rows against the restatement, the padding still the fill values"""
    for k in ("cls", "n_obs", "n_valid", "status"):
        assert np.array_equal(got[k][:n], ref[k]), (k, got[k][:n], ref[k])
        assert (got[k][n:] == R.FILL_I).all(), k
    # the status codes that leave a row unwritten leave the fill values there (the restatement has them too)
    for k in ("view_img", "view_row", "valid"):
        assert np.array_equal(got[k][:Rn], ref[k]), k
        assert (got[k][Rn:] == R.FILL_I).all(), k
    for k in ("tgt", "mask", "P"):
        assert np.array_equal(bits(got[k][:Rn]), bits(ref[k])), k
        assert np.isnan(got[k][Rn:]).all(), k
    a, b = got["init"][:n], ref["init"]
    exact = [c for c in range(a.shape[1]) if c != 3]
    assert np.array_equal(bits(a[:, exact]), bits(b[:, exact])), "translate / scales / shapes of the init rows"
    assert np.array_equal(np.isnan(a[:, 3]), np.isnan(b[:, 3]))
    w = ~np.isnan(b[:, 3])
    ulp = int(R.ulps32(a[w, 3], b[w, 3]).max()) if w.any() else 0
    assert ulp <= 1, "float32 yaw %d ulp from the restatement" % ulp
    if ref["half_dims"] is not None:
        assert np.array_equal(bits(got["half_dims"][:n]), bits(ref["half_dims"]))
    pa, pb = got["pose"][:n], ref["pose"]
    assert np.array_equal(bits(pa[:, [0, 1, 2, 4, 5, 6]]), bits(pb[:, [0, 1, 2, 4, 5, 6]])), "translation / scales in float64"
    assert np.array_equal(np.isnan(pa[:, 3]), np.isnan(pb[:, 3])) and np.array_equal(np.isnan(got["bboxes_dl"][:n]), np.isnan(ref["bboxes_dl"]))
    d = pa[w, 3] - pb[w, 3]
    yaw_gap = float(np.abs((d + np.pi) % (2 * np.pi) - np.pi).max()) if w.any() else 0.0
    box_gap = float(np.abs(got["bboxes_dl"][:n][w] - ref["bboxes_dl"][w]).max()) if w.any() else 0.0
    print("yaw gap %.3e rad (tolerance %.3e), bboxes_dl gap %.3e (tolerance %.3e), float32 yaw %d ulp" % (yaw_gap, YAW_TOL, box_gap, BOX_TOL, ulp))
    assert yaw_gap <= YAW_TOL and box_gap <= BOX_TOL
    for k in ("init", "pose", "bboxes_dl"):
        assert np.isnan(got[k][n:]).all(), k
    return yaw_gap, box_gap


@pytest.fixture(scope="module")
def sized():
    """tracks of every size at which the kernel changes shape (one wave, several waves, several sorted entries per thread), with
    6000 images so that the long tracks have thousands of views, and the restatement of all four representations (computed once)"""
    tracks, img_names, P_cws, img_h, img_w = R.random_tracks(17, len(SIZES), n_img=6000, sizes=SIZES)
    rows, offs = R.pack(tracks)
    ref = {rep: R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, rep) for rep in REPS}
    assert ref["super_quadric"]["n_obs"][-1] > 2048 and not ref["super_quadric"]["status"].any()
    return rows, offs, img_names, P_cws, img_h, img_w, ref


@pytest.mark.parametrize("rep", REPS)
def test_every_size_and_representation(fitter, sized, rep, measured):
    rows, offs, img_names, P_cws, img_h, img_w, ref = sized
    rc, got = raw_prepare(fitter, rows, offs, img_names, P_cws, img_h, img_w, rep)
    assert rc == 0
    yaw_gap, box_gap = check_against_ref(got, ref[rep], len(offs) - 1, len(rows))
    measured("sq_prepare.yaw_gap_vs_restatement", yaw_gap)
    measured("sq_prepare.box_gap_vs_restatement", box_gap)
    shapes = got["init"][:len(offs) - 1, 5 if rep == "dual_quadric" else 7:]
    if rep == "cube":
        assert (shapes == -10000.0).all()
    elif rep != "dual_quadric":
        assert (bits(shapes) == 0x80000000).all()      # -0.0 with its sign bit


def test_many_small_tracks_in_one_launch(fitter):
    """420 workgroups of mixed size -- the tracks of the host test -- in one launch"""
    tracks, img_names, P_cws, img_h, img_w = R.random_tracks(5, 420)
    rows, offs = R.pack(tracks)
    rc, got = raw_prepare(fitter, rows, offs, img_names, P_cws, img_h, img_w, "super_quadric")
    assert rc == 0
    check_against_ref(got, R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, "super_quadric"), len(tracks), len(rows))


def _special_tracks():
    """hand-made tracks, one per rule of the contract; image ids NOT sorted"""
    img_names = [40, 10, 30, 20, 50, 70, 60]      # image index of id 10 is 1, of 20 is 3, ...
    rs = np.random.RandomState(3)
    P_cws = rs.standard_normal((len(img_names), 3, 4))
    img_h, img_w = 480, 640

    def track(ids, cls=5):
        t = np.zeros((len(ids), 14))
        t[:, 0] = ids
        t[:, 1] = cls
        t[:, 2:6] = np.array([100.0, 120.0, 300.0, 330.0]) + rs.uniform(-20, 20, (len(ids), 4))
        t[:, 6:9] = rs.uniform(0.5, 1.5, (len(ids), 3))
        t[:, 9:12] = rs.uniform(-2, 2, (len(ids), 3))
        t[:, 12] = 0.7 + rs.uniform(-0.3, 0.3, len(ids))
        return t
    tracks = {}
    tracks["repeated id, the first row wins"] = track([10, 20, 10, 30, 20, 20])
    tracks["rows out of image order"] = track([70, 60, 50, 40, 30, 20, 10])
    tracks["ids the sequence does not have"] = track([11, 10, 99, 20, -5, 2.0 ** 31, 30])
    tracks["fractional ids truncate"] = track([10.9, 20.5, 30.0001])
    t = track([10, 20], cls=[4, 5])
    tracks["even median of 4 and 5 is 4"] = t
    t = track([10, 20, 30, 40])
    t[0, 2:6] = [20.0, 20.0, 620.0, 460.0]            # exactly thr and lim - thr: every edge out
    t[1, 2:6] = [np.nextafter(20.0, 21), np.nextafter(20.0, 21), np.nextafter(620.0, 0), np.nextafter(460.0, 0)]      # one ulp inside: all in
    t[2, 2:6] = [0.0, 5.0, 639.0, 479.0]              # the box fills the frame: a view without a constraint
    t[3, 2:6] = [20.0, 50.0, 620.0, 400.0]            # x edges on the band, y edges inside
    tracks["edges on the band"] = t
    tracks["no view at all"] = track([1, 2, 3])
    tracks["a class that is no integer"] = track([10, 20, 30], cls=[5, 5.5, 5])
    tracks["a class beyond 63"] = track([10, 20], cls=[64, 5])
    tracks["no view and a bad class"] = track([1, 2], cls=[np.nan, 5])
    tracks["one row"] = track([50])
    return tracks, img_names, P_cws, img_h, img_w


@pytest.mark.parametrize("rep", ("super_quadric", "dual_quadric"))
def test_every_rule_of_the_contract(fitter, rep):
    named, img_names, P_cws, img_h, img_w = _special_tracks()
    names, tracks = list(named), list(named.values())
    rows, offs = R.pack(tracks)
    ref = R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, rep)
    at = {k: i for i, k in enumerate(names)}
    # the restatement says what the case is meant to show
    g = lambda k, key: ref[key][int(offs[at[k]]):int(offs[at[k]]) + int(ref["n_obs"][at[k]])]
    assert g("repeated id, the first row wins", "view_row").tolist() == [0, 3, 1] and g("repeated id, the first row wins", "view_img").tolist() == [1, 2, 3]
    assert g("rows out of image order", "view_row").tolist() == [3, 6, 4, 5, 2, 0, 1]
    assert g("ids the sequence does not have", "view_row").tolist() == [1, 6, 3]
    assert g("fractional ids truncate", "view_img").tolist() == [1, 2, 3]
    assert ref["cls"][at["even median of 4 and 5 is 4"]] == 4
    m = {int(r): row for r, row in zip(g("edges on the band", "view_row"), g("edges on the band", "mask").tolist())}
    assert m[0] == [0, 0, 0, 0] and m[1] == [1, 1, 1, 1] and m[2] == [0, 0, 0, 0] and m[3] == [0, 0, 1, 1]
    assert ref["n_valid"][at["edges on the band"]] == 2 and ref["n_obs"][at["edges on the band"]] == 4
    want = {"no view at all": R.NO_VIEW, "a class that is no integer": R.BAD_CLASS, "a class beyond 63": R.BAD_CLASS, "no view and a bad class": R.NO_VIEW}
    assert ref["status"].tolist() == [want.get(k, 0) for k in names]
    rc, got = raw_prepare(fitter, rows, offs, img_names, P_cws, img_h, img_w, rep)
    assert rc == 0
    check_against_ref(got, ref, len(tracks), len(rows))


def test_too_many_rows_is_refused_from_the_offsets_alone(fitter):
    """a track of 16385 rows that do not exist: status 3 without a row being read; its neighbours are computed.  And a launch sized
    for fewer rows than a track has refuses that track the same way."""
    named, img_names, P_cws, img_h, img_w = _special_tracks()
    a, b = named["rows out of image order"], named["one row"]
    rows = np.concatenate([a, b])
    offs = np.array([0, len(a), len(a) + len(b), len(a) + len(b) + R.MAX_ROWS + 1])
    rc, got = raw_prepare(fitter, rows, offs, img_names, P_cws, img_h, img_w, "super_quadric", max_rows=R.MAX_ROWS + 1)
    assert rc == 0
    ref = R.prepare_ref(rows, offs[:3], img_names, P_cws, img_h, img_w)
    assert got["status"][:3].tolist() == [0, 0, R.TOO_MANY_ROWS] and got["cls"][2] == -1 and got["n_obs"][2] == 0 and got["n_valid"][2] == 0
    assert np.isnan(got["init"][2]).all() and np.isnan(got["pose"][2]).all() and np.isnan(got["bboxes_dl"][2]).all()
    assert np.array_equal(got["view_row"][:len(rows)], ref["view_row"]) and (got["view_row"][len(rows):] == R.FILL_I).all()
    assert np.array_equal(bits(got["init"][:2, [0, 1, 2, 4, 5, 6, 7, 8]]), bits(ref["init"][:, [0, 1, 2, 4, 5, 6, 7, 8]]))
    rc, got = raw_prepare(fitter, rows, offs[:3], img_names, P_cws, img_h, img_w, "super_quadric", max_rows=4)
    assert rc == 0
    ref = R.prepare_ref(rows, offs[:3], img_names, P_cws, img_h, img_w, cap=4)
    assert ref["status"].tolist() == [R.TOO_MANY_ROWS, 0]
    check_against_ref(got, ref, 2, len(rows))


def test_zero_objects(fitter):
    named, img_names, P_cws, img_h, img_w = _special_tracks()
    rc, got = raw_prepare(fitter, np.zeros((0, 14)), [0], img_names, P_cws, img_h, img_w, "super_quadric")
    assert rc == 0 and (got["status"] == R.FILL_I).all() and np.isnan(got["init"]).all() and (got["view_img"] == R.FILL_I).all()
    out = fitter.prepare(np.zeros((0, 14)), [0], img_names, P_cws, img_h, img_w)
    assert out["status"].shape == (0,) and tuple(out["init"].shape) == (0, 9) and tuple(out["P"].shape) == (0, 12)


def test_prepare_method(fitter):
    """SqFitter.prepare: host and device inputs, one read-back, the restatement's values where the status says they were written"""
    tracks, img_names, P_cws, img_h, img_w = R.random_tracks(9, 40, n_img=90, max_rows=150)
    tracks[3][:, 0] = 7.0          # no view
    rows, offs = R.pack(tracks)
    for rep in ("cube", "dual_quadric"):
        ref = R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, rep)
        a = fitter.prepare(rows, offs, img_names, P_cws, img_h, img_w, rep)
        b = fitter.prepare(torch.from_numpy(rows).to(DEV), torch.from_numpy(offs).to(DEV), img_names, torch.from_numpy(P_cws), img_h, img_w, rep)
        for out in (a, b):
            assert all(isinstance(out[k], np.ndarray) and out[k].dtype == np.int32 for k in ("cls", "n_obs", "n_valid", "status"))
            for k in ("cls", "n_obs", "n_valid", "status"):
                assert np.array_equal(out[k], ref[k]), k
            assert out["status"].tolist() == [R.NO_VIEW if i == 3 else 0 for i in range(len(tracks))]
            assert (out["half_dims"] is None) == (rep != "dual_quadric")
            ok = ref["status"] == 0
            exact = [c for c in range(ref["init"].shape[1]) if c != 3]
            assert np.array_equal(bits(out["init"].cpu().numpy()[ok][:, exact]), bits(ref["init"][ok][:, exact]))
            for o in np.flatnonzero(ok):
                g = slice(int(offs[o]), int(offs[o]) + int(ref["n_obs"][o]))
                for k in ("view_img", "view_row", "valid"):
                    assert np.array_equal(out[k][g].cpu().numpy(), ref[k][g])
                for k in ("tgt", "mask", "P"):
                    assert np.array_equal(bits(out[k][g].cpu().numpy()), bits(ref[k][g]))
        views = np.zeros(len(rows), bool)
        for o in np.flatnonzero(ok):
            views[int(offs[o]):int(offs[o]) + int(ref["n_obs"][o])] = True
        for k in ("init", "pose", "bboxes_dl", "tgt", "P"):      # the launch sized for 16384 rows gives the bits of the launch sized for 150
            ka, kb = a[k].cpu().numpy(), b[k].cpu().numpy()
            w = views if k in ("tgt", "P") else ok
            assert np.array_equal(bits(ka[w]), bits(kb[w])), k
    with pytest.raises(ValueError, match="all different"):
        fitter.prepare(rows, offs, list(img_names) + [img_names[0]], np.concatenate([P_cws, P_cws[:1]]), img_h, img_w)
    with pytest.raises(ValueError, match="row_offsets"):
        fitter.prepare(rows, offs[:-1], img_names, P_cws, img_h, img_w)


# ---- optim_process / refine with prelude="device" on the tracks of the whole-chain fixture ------------------------------------------

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


@pytest.fixture(scope="module")
def fixture_scene(golden):
    z = golden("e2e.npz")
    seq, K, T_wcs, P_cws = e2e_lib.sequence_geometry()
    return z, seq, K, T_wcs, P_cws


def _same_handover(h, d):
    """the packed rows and counts are identical; -> indices (among the fitted) whose init row is bit-equal"""
    assert h["counts"] == d["counts"] and h["cls"] == d["cls"]
    for k in ("P", "tgt", "mask"):
        assert h[k].dtype == np.float32 and d[k].dtype == np.float32 and np.array_equal(bits(h[k]), bits(d[k])), k
    if "half" in h:
        assert np.array_equal(bits(h["half"]), bits(d["half"]))
    exact = [c for c in range(h["init"].shape[1]) if c != 3]
    assert np.array_equal(bits(h["init"][:, exact]), bits(d["init"][:, exact]))
    assert R.ulps32(h["init"][:, 3], d["init"][:, 3]).max() <= 1
    return bits(h["init"][:, 3]) == bits(d["init"][:, 3])


@pytest.mark.parametrize("rep,w", [("super_quadric", 1), ("super_quadric", 2), ("dual_quadric", 1)])
def test_optim_process_device_prelude_on_the_fixture_tracks(fitter, fixture_scene, rep, w):
    from odam_amd import multi_view
    z, seq, K, T_wcs, P_cws = fixture_scene
    tracks = e2e_lib.reference_tracks(z, w)
    n_iters = 500 if rep == "dual_quadric" else 200
    spy = Spy(fitter)
    try:
        run = lambda prelude: multi_view.optim_process([t.copy() for t in tracks], seq["img_names"], T_wcs, P_cws, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"], K,
                                                       rep, True, n_iters, 10, fitter=fitter, return_params=True, prelude=prelude)
        host = run("host")
        dev = run("device")
    finally:
        spy.restore()
    assert len(spy.calls) == 2
    n = len(tracks)
    assert all(np.array_equal(a, b) for a, b in zip(host["tracks"], dev["tracks"])) and len(dev["tracks"]) == n
    assert np.array_equal(host["fitted"], dev["fitted"]) and host["fitted"].sum() >= 10 and not host["fitted"].all()
    if rep != "dual_quadric":
        assert [q.obj_class for q in host["quadrics"]] == [q.obj_class for q in dev["quadrics"]]
    gap = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in zip(host["bboxes_dl"], dev["bboxes_dl"]))
    print("bboxes_dl: device prelude against the host path %.3e (tolerance %.3e)" % (gap, BOX_TOL))
    assert gap <= BOX_TOL
    same = _same_handover(*spy.calls)
    fit_ids = np.flatnonzero(host["fitted"])
    clean = np.ones(n, bool)
    clean[fit_ids] = same
    # unfitted tracks: params are the init rows themselves
    for i in np.flatnonzero(~host["fitted"]):
        a, b = host["params"][i], dev["params"][i]
        exact = [c for c in range(len(a)) if c != 3]
        assert np.array_equal(bits(a[exact]), bits(b[exact])) and R.ulps32(a[3], b[3]) <= 1
        clean[i] = bits(a[3:4])[0] == bits(b[3:4])[0]
    print("%d of %d init rows differ from the host path's (one ulp of the angle)" % (int((~clean).sum()), n))
    assert (~clean).sum() <= 1
    for i in np.flatnonzero(clean):      # the same kernel on the same inputs
        assert np.array_equal(bits(host["params"][i]), bits(dev["params"][i])), i
        assert np.array_equal(bits(np.asarray(host["bboxes_qc"][i])), bits(np.asarray(dev["bboxes_qc"][i]))) or not host["fitted"][i], i
    # the restatement alone stays at zero on this fixture: its init rows are the host path's, all of them
    rows, offs = R.pack(tracks)
    ref = R.prepare_ref(rows, offs, seq["img_names"], P_cws, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"], rep)
    assert np.array_equal(bits(ref["init"][fit_ids]), bits(spy.calls[0]["init"]))
    assert np.array_equal(bits(ref["init"][~host["fitted"]]), bits(host["params"][~host["fitted"]]))


def test_n_valid_at_the_threshold(fitter):
    """a track with n_views - 1 constrained views is not fitted, one with n_views is: both paths"""
    from odam_amd import multi_view
    tracks, img_names, P_cws, img_h, img_w = R.random_tracks(21, 2, n_img=40, sizes=[30, 30])
    for t in tracks:
        t[:, 0] = img_names[:30]
        t[:, 1] = 5
        t[:, 2:6] = [5.0, 5.0, 639.0, 479.0]                 # no constrained edge
    tracks[0][:9, 2:6] = [100.0, 110.0, 300.0, 320.0]
    tracks[1][:10, 2:6] = [100.0, 110.0, 300.0, 320.0]
    P = np.tile(np.array([[500.0, 0, 320, 0], [0, 500.0, 240, 0], [0, 0, 1, 4.0]]), (40, 1, 1))
    out = {p: multi_view.optim_process([t.copy() for t in tracks], img_names, None, P, img_h, img_w, None, "super_quadric", True, 5, 10,
                                       fitter=fitter, return_params=True, prelude=p) for p in ("host", "device")}
    assert out["host"]["fitted"].tolist() == [False, True] and out["device"]["fitted"].tolist() == [False, True]
    prep = fitter.prepare(*R.pack(tracks), img_names, P, img_h, img_w)
    assert prep["n_valid"].tolist() == [9, 10] and prep["n_obs"].tolist() == [30, 30]


def test_gather_of_tracks_with_fewer_views_than_rows(fitter):
    """Fitted tracks whose frame ids repeat or name no image have n_obs below their row count: the kernel leaves the per-view words
    past their views unwritten, and the gather that packs the constrained views must not take anything from there.  The allocator is
    handed blocks of ones of the per-view buffers' size first and the call is made twice, so that stale words are not zero by luck;
    what reaches the fit is the host path's, bit for bit, both times."""
    from odam_amd import multi_view
    sizes = [40 + 9 * i for i in range(16)]
    tracks, img_names, _, img_h, img_w = R.random_tracks(31, len(sizes), n_img=120, sizes=sizes)
    tracks[0][5, 0] = tracks[0][0, 0]                       # a repeated id and an absent one for certain
    tracks[1][3, 0] = 1.0
    for t in tracks:                                        # most views constrained, so that the tracks are fitted
        keep = np.random.RandomState(len(t)).uniform(size=len(t)) < 0.8
        t[keep, 2:6] = np.array([100.0, 110.0, 300.0, 320.0]) + t[keep, 13:14] * 50.0
    P = np.tile(np.array([[500.0, 0, 320, 0], [0, 500.0, 240, 0], [0, 0, 1, 4.0]]), (len(img_names), 1, 1))
    P[:, 0, 3] = np.arange(len(img_names))                  # every image its own projection: a row packed from the wrong view shows
    rows, offs = R.pack(tracks)
    ref = R.prepare_ref(rows, offs, img_names, P, img_h, img_w)
    fit = ref["n_valid"] >= 10
    short = fit & (ref["n_obs"] < np.diff(offs))
    assert not ref["status"].any() and fit[0] and fit[1] and short[0] and short[1] and short.sum() >= 8
    assert (np.diff(offs) - ref["n_obs"])[fit].max() >= 3   # several unwritten words in one track
    run = lambda prelude: multi_view.optim_process([t.copy() for t in tracks], img_names, None, P, img_h, img_w, None, "super_quadric", True, 5, 10,
                                                   fitter=fitter, return_params=True, prelude=prelude)
    spy = Spy(fitter)
    try:
        host = run("host")
        outs = []
        for _ in range(2):
            stale = [torch.ones(len(rows), device=DEV, dtype=torch.int32) for _ in range(8)]
            torch.cuda.synchronize()
            del stale
            outs.append(run("device"))
    finally:
        spy.restore()
    assert len(spy.calls) == 3 and spy.calls[0]["counts"] == ref["n_valid"][fit].tolist() and host["fitted"].tolist() == fit.tolist()
    for dev, call in zip(outs, spy.calls[1:]):
        same = _same_handover(spy.calls[0], call)
        assert dev["fitted"].tolist() == fit.tolist()
        for j, i in enumerate(np.flatnonzero(fit)):
            if same[j]:      # the same kernel on the same inputs
                assert np.array_equal(bits(host["params"][i]), bits(dev["params"][i])), i
        gap = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in zip(host["bboxes_dl"], dev["bboxes_dl"]))
        assert gap <= BOX_TOL


def test_refine_twice_with_the_device_prelude(fixture_scene):
    from odam_amd.processor import OdamProcess
    z, seq, K, T_wcs, P_cws = fixture_scene
    full = e2e_lib.reference_tracks(z, 1)
    early = [t[:max(1, 2 * len(t) // 3)] for t in full]
    states, began_equal = {}, {}
    for prelude in ("host", "device"):
        proc = OdamProcess(None, None, None, None)
        proc.init_sequence(K, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"])
        proc.usable_frames, proc.T_wcs, proc.P_cws = seq["img_names"], T_wcs, P_cws
        assert proc.device_prelude is False
        if prelude == "device":
            proc.device_prelude = True      # refine(prelude=None) reads the attribute
        proc.tracks = [t.copy() for t in early]
        proc.refine(n_iters=50)
        spy = Spy(proc.refine_fitter)
        try:
            first = proc._refine_state
            proc.tracks = [t.copy() for t in full]
            proc.refine(n_iters=50, prelude=None if prelude == "device" else "host")
        finally:
            spy.restore()
        st = proc._refine_state
        states[prelude] = (first["track_ids"].tolist(), torch.as_tensor(first["state"]).cpu().numpy(),
                           st["track_ids"].tolist(), torch.as_tensor(st["state"]).cpu().numpy(), spy.calls[0]["state"])
        proc.refine_fitter.close()
    h, d = states["host"], states["device"]
    assert h[0] == d[0] and h[2] == d[2] and len(h[2]) > len(h[0]) > 0
    # an object's rows are the host path's bits wherever its init row was (words 27..29 keep the first launch's scales; word 3 of a
    # cold row is the init angle): at most one object of the fixture may differ, by one ulp of the angle
    first_equal = {t: np.array_equal(bits(h[1][j]), bits(d[1][j])) for j, t in enumerate(h[0])}
    cold = {t: bits(h[4][j, :9]).tolist() == bits(d[4][j, :9]).tolist() for j, t in enumerate(h[2]) if h[4][j, 30] == 0}
    differ = [t for t in h[2] if not np.array_equal(bits(h[3][h[2].index(t)]), bits(d[3][d[2].index(t)]))]
    print("refine twice: %d of %d state rows differ from the host path's" % (len(differ), len(h[2])))
    assert len(differ) <= 1
    for t in differ:      # only where the init row differed
        assert (t in first_equal and not first_equal[t]) or (t in cold and not cold[t])
    assert (h[3][:, 30] == [100.0 if t in h[0] else 50.0 for t in h[2]]).all() and np.array_equal(h[3][:, 30], d[3][:, 30])


def test_fallbacks_take_the_host_path(fitter, fixture_scene, caplog):
    from odam_amd import multi_view
    z, seq, K, T_wcs, P_cws = fixture_scene
    tracks = e2e_lib.reference_tracks(z, 2)
    args = lambda tr, names, P: ([t.copy() for t in tr], names, None, P, e2e_lib.SEQ["h"], e2e_lib.SEQ["w"], K, "super_quadric", True, 20, 10)
    called = []
    orig = fitter.prepare
    fitter.prepare = lambda *a, **k: (called.append(1), orig(*a, **k))[1]
    try:
        # duplicate image ids: the prelude kernel is not asked
        names2, P2 = list(seq["img_names"]) + [seq["img_names"][0]], np.concatenate([P_cws, P_cws[:1]])
        with caplog.at_level(logging.DEBUG, logger="odam_amd.multi_view"):
            a = multi_view.optim_process(*args(tracks, names2, P2), fitter=fitter, return_params=True, prelude="device")
        b = multi_view.optim_process(*args(tracks, names2, P2), fitter=fitter, return_params=True, prelude="host")
        assert not called and sum("device prelude does not apply" in r.getMessage() for r in caplog.records) == 1
        assert np.array_equal(bits(a["params"]), bits(b["params"])) and np.array_equal(a["fitted"], b["fitted"])
        assert all(np.array_equal(x, y) for x, y in zip(a["bboxes_dl"], b["bboxes_dl"])) and all(np.array_equal(x, y) for x, y in zip(a["bboxes_qc"], b["bboxes_qc"]))
        # a track without a view: the kernel says so (status 1) and the host path raises what it always raised
        lost = [t.copy() for t in tracks]
        lost[1][:, 0] = 10 ** 6
        errs = []
        for prelude in ("host", "device"):
            with pytest.raises(Exception) as e:
                multi_view.optim_process(*args(lost, seq["img_names"], P_cws), fitter=fitter, prelude=prelude)
            errs.append((type(e.value), str(e.value)))
        assert errs[0] == errs[1] and len(called) == 1
        # no track
        e0 = multi_view.optim_process(*args([], seq["img_names"], P_cws), fitter=fitter, return_params=True, prelude="device")
        assert e0["quadrics"] == [] and e0["params"].shape == (0, 9) and len(called) == 1
    finally:
        del fitter.prepare
    with pytest.raises(ValueError, match="prelude"):
        multi_view.optim_process(*args(tracks, seq["img_names"], P_cws), fitter=fitter, prelude="gpu")
