"""Reprojection, host side: the numpy restatement of the three kernels (tests/reproject_ref.py) against the reference-run fixtures that
already exist, the score arithmetic by hand, multi_view.reprojection / OdamProcess.reprojection behind the stand-in fitter, and the
C declarations against what odam_amd.sq gives ctypes.  tests/test_reproject_gpu.py asks the device for the same.

Tolerances (tests/golden/reproject.md, figures of tests/golden/make_reproject_figures.py), each 8 x the worst restatement-vs-reference
deviation measured on the CPU -- the margin DESIGN.md 6g uses for a restatement against a reference value:
  loss_2d of the reference's own points vs its logged value   1.12e-7 relative -> 9e-7
  float64 box of gt_Q vs exact box edges                      9.7e-13 px       -> 8e-12 px
  float64 box vs sq.DualQuadric.get_bbox (numpy's product)    1.2e-12 px       -> 1e-11 px"""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_ref
import quadric_svd_ref as S
import reproject_ref as R
from conftest import REPO

LOSS_RTOL = 9e-7
EXACT_PX = 8e-12
BBOX_PX = 1e-11


# ---- 1. sq_steps.npz: the reference's own points give the reference's own logged loss_2d ---------------------------------------
def test_loss_2d_of_the_references_points_is_its_logged_value(golden):
    z = golden("sq_steps.npz")
    worst, n = 0.0, 0
    for c in range(int(z["n_cases"])):
        P, tgt, mask = z[f"c{c}_P"], z[f"c{c}_tgt"], z[f"c{c}_mask"]
        for k in (0, 100, 199):
            r = R.reproject(z[f"c{c}_pts{k}"][None], [len(P)], P)
            assert (r["n_valid"] == 1000).all()
            s = R.reprojection_score(r["ext"], r["n_valid"] == 0, [len(P)], tgt, mask, 1e9, 1e9)
            assert s["loss_2d"].dtype == np.float32 and s["n_bad"][0] == 0 and s["n_edges"][0] == int((mask != 0).sum())
            ref = float(z[f"c{c}_l2d"][k])
            rel = abs(float(s["loss_2d"][0]) - ref) / abs(ref)
            print("case %d step %3d: %.9g vs %.9g, rel %.3e" % (c, k, s["loss_2d"][0], ref, rel))
            worst, n = max(worst, rel), n + 1
            assert rel <= LOSS_RTOL, (c, k, rel)
    assert n == 15
    print("worst %.3e (bound %.1e)" % (worst, LOSS_RTOL))


# ---- 2. quadric_svd.npz: exact objects project onto their own box edges --------------------------------------------------------
def test_exact_objects_project_onto_their_edges_and_noisy_ones_do_not(golden):
    z = golden("quadric_svd.npz")
    kind = z["kind"].astype(int)
    n_exact = n_noisy = 0
    for i in range(int(z["n_obj"])):
        P, edges = R.svd_track_views(z, i)
        ext, st = R.reproject_dq_one(z["gt_Q"][i], P)
        worst = float(np.abs(ext - edges).max())
        print("object %2d kind %d, %3d views: %.3e px" % (i, kind[i], len(P), worst))
        if kind[i] in (S.KIND_EXACT, S.KIND_TWO_VIEWS):
            n_exact += 1
            assert (st == 0).all() and worst <= EXACT_PX, (i, worst)
        elif kind[i] == S.KIND_NOISY:      # 1 px of noise per edge (noise_px): the worst of 12 .. 1200 edges is of pixel order
            n_noisy += 1
            assert z["noise_px"][i] == 1.0 and 1.0 <= worst <= 10.0, (i, worst)
    assert n_exact == 8 and n_noisy == 7


# ---- 3. the restatement against the reference's form through numpy's matrix product --------------------------------------------
def test_restated_box_vs_get_bbox(golden):
    worst32 = worst64 = 0.0
    d = golden("dq_fits.npz")
    for c in range(int(d["n_cases"])):      # the iterative fit's float32 Q, cast up
        Q, P = d[f"c{c}_Q"], d[f"c{c}_P"]
        assert Q.dtype == np.float32
        ext, st = R.reproject_dq_one(Q, P)
        assert (st == 0).all()
        worst32 = max(worst32, float(np.abs(ext - R.get_bbox_rows(Q, P)).max()))
    z = golden("quadric_svd.npz")
    for i in range(int(z["n_obj"])):        # float64 Q: the ground truth and the reference's closed form
        P, _ = R.svd_track_views(z, i)
        for Q in (z["gt_Q"][i], z["ref_Q"][i]):
            if not np.isfinite(Q).all():
                continue
            ext, st = R.reproject_dq_one(Q, P)
            ok = st == 0
            if ok.any():
                worst64 = max(worst64, float(np.abs(ext[ok] - R.get_bbox_rows(Q, P[ok])).max()))
    print("vs get_bbox: float32 Q %.3e px, float64 Q %.3e px (bound %.1e)" % (worst32, worst64, BBOX_PX))
    assert worst32 <= BBOX_PX and worst64 <= BBOX_PX


def test_status_of_a_camera_inside_the_ellipsoid(golden):
    """dq_ref.discriminant_problem: the status is 1 and the extents NaN for that view only"""
    d = dq_ref.case(golden("dq_fits.npz"), 0)
    Q = dq_ref.make_obj(d["init5"], d["half_dims"])["Q"].reshape(4, 4)
    P = dq_ref.discriminant_problem(d, view=3)
    ext, st = R.reproject_dq_one(Q, P)
    assert st.tolist() == [0, 0, 0, 1] + [0] * (len(P) - 4)
    assert np.isnan(ext[3]).all() and np.isfinite(np.delete(ext, 3, axis=0)).all()
    ext0, st0 = R.reproject_dq_one(Q, d["P"])
    assert (st0 == 0).all() and np.array_equal(np.delete(ext, 3, axis=0), np.delete(ext0, 3, axis=0))
    # c22 == 0: a projection whose third row is zero
    Pz = d["P"].astype(np.float64).reshape(-1, 3, 4).copy()
    Pz[1, 2] = 0.0
    ez, sz = R.reproject_dq_one(Q, Pz)
    assert sz[1] == 1 and np.isnan(ez[1]).all() and sz.sum() == 1


def test_sq_extents_fill_values_and_nan():
    rs = np.random.RandomState(5)
    pts = (rs.standard_normal((65, 3)) * 0.2 + [0, 0, 3.0]).astype(np.float32)
    M = np.array([[500, 0, 320, 0], [0, 500, 240, 0], [0, 0, 1, 0]], np.float32).reshape(1, 12)
    ext, nv = R.reproject_sq_one(pts, M)
    q = pts.astype(np.float64)
    u, v = 500 * q[:, 0] / q[:, 2] + 320, 500 * q[:, 1] / q[:, 2] + 240
    assert nv[0] == 65 and np.allclose(ext[0], [u.min(), u.max(), v.min(), v.max()], rtol=1e-5)
    behind = pts * np.float32([1, 1, -1])
    ext, nv = R.reproject_sq_one(behind, M)
    assert nv[0] == 0 and ext[0].tolist() == [1e6, -1e6, 1e6, -1e6]
    # depth must exceed 0.5, not reach it
    ext, nv = R.reproject_sq_one(np.float32([[0, 0, 0.5], [0.1, 0.1, 0.5000001]]), M)
    assert nv[0] == 1
    # a NaN coordinate of a point reaches its depth through the projection: the point is not valid, the others decide
    withnan = pts.copy()
    withnan[7, 0] = np.nan
    ext, nv = R.reproject_sq_one(withnan, M)
    assert nv[0] == 64 and np.isfinite(ext).all()
    assert np.array_equal(ext, R.reproject_sq_one(np.delete(pts, 7, axis=0), M)[0])
    # a NaN pixel coordinate of a VALID point (Inf / Inf: depth and x overflow, y does not): torch.min / max give NaN for that
    # axis only, as the default quiet NaN
    M2 = np.array([[500, 0, 320, 0], [0, 500, 0, 0], [0, 0, 2, 0]], np.float32).reshape(1, 12)
    far = pts.copy()
    far[7] = [0.1, 0.1, 3e38]
    ext, nv = R.reproject_sq_one(far, M2)
    assert nv[0] == 65 and np.isnan(ext[0, :2]).all() and np.isfinite(ext[0, 2:]).all()
    assert ext.view(np.uint32)[0, 0] == 0x7FC00000 and ext.view(np.uint32)[0, 1] == 0x7FC00000


# ---- 4. score arithmetic by hand ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score_arithmetic_by_hand(dtype):
    box = np.array([[100, 200, 50, 150]], dtype)      # x_min, x_max, y_min, y_max: 100 x 100
    one = np.ones((1, 4), np.float32)
    sc = lambda ext, m=one, bad=None, b=box: R.score_one(np.asarray(ext, dtype), bad, b, m, 640, 480, dtype)
    res, iou, obj, obj_i = sc(box)
    assert iou[0] == 1 and (res == 0).all() and obj.tolist() == [0, 0, 1, 1] and obj_i.tolist() == [0, 4, 0]
    assert sc([[300, 400, 50, 150]])[1][0] == 0                               # disjoint
    assert sc([[150, 250, 50, 150]])[1][0] == dtype(5000) / dtype(15000)      # half overlap: 1/3
    # a predicted box beyond the image is clipped: [-50, 700] x [-20, 500] -> the whole image
    whole = np.array([[0, 640, 0, 480]], dtype)
    assert sc([[-50, 700, -20, 500]], b=whole)[1][0] == 1
    assert sc([[-50, 200, 50, 150]])[1][0] == dtype(10000) / dtype(20000)
    # residuals: |ext - box| per edge; a masked edge gives 0 and is not counted
    m = np.array([[1, 0, 1, 1]], np.float32)
    res, iou, obj, obj_i = sc([[103, 250, 48, 150.5]], m)
    assert res.tolist() == [[3, 0, 2, 0.5]] and obj_i.tolist() == [0, 3, 0]
    assert obj[0] == dtype(5.5) and obj[1] == dtype(5.5) / dtype(3)           # loss_2d with F = 1; mean over 3 edges
    # all edges masked: no mean
    res, iou, obj, obj_i = sc([[103, 250, 48, 150.5]], np.zeros((1, 4), np.float32))
    assert (res == 0).all() and obj[0] == 0 and np.isnan(obj[1]) and obj_i[1] == 0
    # NaN edges (a status-1 view): residual 0, IoU 0, counted as bad; the fill values of an empty view: IoU 0
    res, iou, obj, obj_i = sc([[np.nan] * 4], bad=[1])
    assert (res == 0).all() and iou[0] == 0 and obj_i.tolist() == [0, 4, 1]
    assert sc([[1e6, -1e6, 1e6, -1e6]], bad=[1])[1][0] == 0 and sc([[1e6, -1e6, 1e6, -1e6]])[1][0] == 0
    assert sc(box, bad=[1])[1][0] == 0                                        # a bad view scores 0 whatever its numbers
    assert sc(box, b=np.array([[100, 100, 50, 150]], dtype))[1][0] == 0       # empty boxes on both sides: union 0
    # worst_view: the first of equal minima, at any distance across the lanes
    F = 131
    ext = np.tile(box, (F, 1))
    ext[[70, 5, 130]] = [150, 250, 50, 150]
    res, iou, obj, obj_i = R.score_one(ext, None, np.tile(box, (F, 1)), np.ones((F, 4), np.float32), 640, 480, dtype)
    assert obj_i[0] == 5 and obj[3] == dtype(5000) / dtype(15000) and obj_i[1] == 4 * F
    assert abs(obj[2] - (F - 3 + 1.0) / F) < 1e-6 and abs(obj[0] - 2 * 3 * 50.0 / F) < 1e-4
    # an object without views
    res, iou, obj, obj_i = R.score_one(np.zeros((0, 4), dtype), None, np.zeros((0, 4), dtype), np.zeros((0, 4), np.float32), 640, 480, dtype)
    assert np.isnan(obj).all() and obj_i.tolist() == [-1, 0, 0]


def test_wave_sums_is_dq_refs_order():
    rs = np.random.RandomState(2)
    for F in (1, 63, 64, 65, 129, 300):
        rows = rs.uniform(0, 30, (5, F)).astype(np.float32)
        assert np.array_equal(R.wave_sums(rows), dq_ref.wave_sums(rows))
        r64 = rows.astype(np.float64) + 1e-9
        got = R.wave_sums(r64)
        assert got.dtype == np.float64 and np.allclose(got, r64.sum(axis=1), rtol=(F + 8) * 2.0 ** -52, atol=0)


# ---- 5. multi_view.reprojection behind the stand-in fitter -------------------------------------------------------------------------
class Recorder(R.RefFitter):
    """the stand-in, keeping what it was sent"""

    def __init__(self):
        super().__init__()
        self.sent = []

    def reproject(self, points, view_counts, P):
        self.sent.append(("reproject", np.asarray(points), list(view_counts), np.asarray(P)))
        return R.reproject(points, view_counts, P)

    def reproject_dual(self, Q, view_counts, P):
        self.sent.append(("reproject_dual", np.asarray(Q), list(view_counts), np.asarray(P)))
        return R.reproject_dual(Q, view_counts, P)

    def reprojection_score(self, ext, bad, view_counts, boxes, mask, img_w, img_h):
        self.sent.append(("score", np.asarray(ext), list(view_counts), np.asarray(boxes), np.asarray(mask), img_w, img_h))
        return R.reprojection_score(ext, bad, view_counts, boxes, mask, img_w, img_h)


@pytest.fixture(scope="module")
def optim_scene(golden):
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    return z, tracks, ([int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], 480, 640, z["K"])


def test_reprojection_rows_are_the_fits_rows(optim_scene, oracle):
    """the super-quadric group: counts, P and mask are what optim_process sends to the fit, the boxes are its float32 targets"""
    import torch
    from odam_amd import multi_view
    z, tracks, args = optim_scene
    fit_args = []

    class FitSpy:
        def fit(self, params0, class_ids, view_counts, P, tgt, mask, **kw):
            fit_args.append((list(view_counts), np.asarray(P), np.asarray(tgt), np.asarray(mask)))
            p = np.asarray(params0, np.float32)
            return {"params": torch.from_numpy(p), "points": torch.from_numpy(np.stack([oracle.points(x) for x in p]))}
    op = multi_view.optim_process(tracks, *args, "super_quadric", True, 200, 1, fitter=FitSpy(), return_params=True)
    assert op["fitted"].all()
    quadrics = [multi_view.SuperQuadric(z["params"][i], q.obj_class, oracle.points(z["params"][i])) for i, q in enumerate(op["quadrics"])]
    rec = Recorder()
    out = multi_view.reprojection(tracks, quadrics, *args, fitter=rec)
    assert [s[0] for s in rec.sent] == ["reproject", "score"] and rec.calls == []      # one launch each, the cached points
    vc, P, tgt, mask = fit_args[0]
    _, pts, rvc, rP = rec.sent[0]
    assert rvc == vc and rP.dtype == np.float32 and np.array_equal(rP, P) and pts.shape == (len(tracks), 1000, 3)
    _, ext, svc, boxes, smask, w, h = rec.sent[1]
    assert svc == vc and np.array_equal(smask, mask) and (w, h) == (640.0, 480.0)
    assert boxes.dtype == np.float32 and np.array_equal(np.where(mask > 0, boxes, 0), tgt)
    assert out["n_views"].tolist() == vc and out["view_offsets"].tolist() == np.concatenate([[0], np.cumsum(vc)]).tolist()
    # the reference's fitted shapes explain their detections: every fitted object of the scene within a few pixels
    print("mean_abs_px", out["mean_abs_px"], "mean_iou", out["mean_iou"])
    assert np.isfinite(out["loss_2d"]).all() and (out["n_bad"] == 0).all() and (out["n_edges"] == [int(m.sum()) for m in np.split(mask, np.cumsum(vc)[:-1])]).all()
    want = R.reprojection_score(R.reproject(pts, vc, P)["ext"], None, vc, boxes, mask, 640, 480)
    for key in ("loss_2d", "mean_abs_px", "mean_iou", "min_iou"):
        assert np.array_equal(out[key], want[key].astype(np.float64)), key
    assert np.array_equal(out["residual"], want["residual"].astype(np.float64)) and np.array_equal(out["iou"], want["iou"].astype(np.float64))
    for i in range(len(tracks)):
        a = out["view_offsets"][i]
        assert out["worst_img"][i] == out["img_ids"][a + want["worst_view"][i]]
        assert out["iou"][a + want["worst_view"][i]] == out["min_iou"][i]


def test_reprojection_points_come_from_one_points_call(optim_scene, oracle):
    from odam_amd import multi_view
    z, tracks, args = optim_scene
    with_pts = [multi_view.SuperQuadric(z["params"][i], 0, oracle.points(z["params"][i])) for i in range(len(tracks))]
    without = [multi_view.SuperQuadric(z["params"][i], 0, None) for i in range(len(tracks))]
    without[2] = with_pts[2]
    a, b = Recorder(), Recorder()
    ra = multi_view.reprojection(tracks, with_pts, *args, fitter=a)
    rb = multi_view.reprojection(tracks, without, *args, fitter=b)
    assert a.calls == [] and b.calls == [("points", len(tracks) - 1)]
    for key in ra:
        assert np.array_equal(ra[key], rb[key], equal_nan=True), key


def test_reprojection_of_a_mixed_list(golden, oracle):
    """SuperQuadric, DualQuadric (float64 closed form and float32 fitted Q), None, and a track without a valid view"""
    from odam_amd import multi_view, sq
    z = golden("quadric_svd.npz")
    tracks = S.fixture_tracks(z)
    args = ([int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], S.IMG_H, S.IMG_W, z["K"])
    kind = z["kind"].astype(int)
    n = len(tracks)
    # the closed-form rows: what closed_form_quadrics sends
    svd_args = []

    class SvdSpy:
        @staticmethod
        def quadric_svd(view_counts, P, edges, mask):
            svd_args.append((list(view_counts), np.asarray(P), np.asarray(edges), np.asarray(mask)))
            return S.quadric_svd(view_counts, P, edges, mask)
    cf = multi_view.closed_form_quadrics(tracks, *args, n_views=1, fitter=SvdSpy())
    quadrics = list(cf["quadrics"])
    assert sum(q is None for q in quadrics) == 2      # the two-view object and the one that is not an ellipsoid
    rec = Recorder()
    out = multi_view.reprojection(tracks, quadrics, *args, fitter=rec)
    assert [s[0] for s in rec.sent] == ["reproject_dual", "score"]
    keep = [j for j, q in enumerate(quadrics) if q is not None]
    vc, P, edges, mask = svd_args[0]
    pick = np.concatenate([np.arange(sum(vc[:j]), sum(vc[:j + 1])) for j in keep])
    _, Q, rvc, rP = rec.sent[0]
    assert Q.dtype == np.float64 and rvc == [vc[j] for j in keep] and rP.dtype == np.float64 and np.array_equal(rP, P[pick])
    _, ext, svc, boxes, smask, w, h = rec.sent[1]
    assert ext.dtype == np.float64 and boxes.dtype == np.float64 and np.array_equal(boxes, edges[pick]) and np.array_equal(smask, mask[pick])
    for i in range(n):
        if quadrics[i] is None:
            assert np.isnan(out["loss_2d"][i]) and np.isnan(out["min_iou"][i]) and out["worst_img"][i] == -1
            assert out["n_views"][i] == 0 and out["n_edges"][i] == 0 and out["n_bad"][i] == 0
            assert out["view_offsets"][i] == out["view_offsets"][i + 1]
        elif kind[i] == S.KIND_EXACT:      # the closed form of exact edges reprojects onto them (measured: <= 1.7e-13 px)
            assert out["mean_abs_px"][i] <= EXACT_PX and out["min_iou"][i] >= 1 - 1e-12 and out["n_bad"][i] == 0
        elif kind[i] == S.KIND_NOISY:
            assert 0.1 <= out["mean_abs_px"][i] <= 3.0 and 0.8 <= out["mean_iou"][i] < 1.0
    # the mixed list: a super-quadric, a float32 dual quadric, None, a closed-form one; track 1 moved out of the image
    z2 = golden("dq_fits.npz")
    q32 = sq.DualQuadric(z2["c0_Q"])
    assert q32.Q.dtype == np.float32
    p9 = sq.init_params([0.0, 0.0, 0.5], 0.3, [0.8, 0.5, 1.0])
    sup = multi_view.SuperQuadric(p9, 0, None)
    gone = tracks[1].copy()
    gone[:, 2:6] = [5.0, 3.0, 635.0, 478.0]      # every edge inside the 20 px border: no constrained edge, no valid view
    mixed_tracks = [tracks[0], gone, tracks[4], tracks[6], tracks[8]]
    mixed = [sup, quadrics[0], None, q32, quadrics[8]]
    rec = Recorder()
    out = multi_view.reprojection(mixed_tracks, mixed, *args, fitter=rec)
    assert sorted(s[0] for s in rec.sent) == ["reproject", "reproject_dual", "score", "score"] and rec.calls == [("points", 1)]
    assert out["n_views"].tolist() == [3, 0, 0, 64, 65] and out["view_offsets"].tolist() == [0, 3, 3, 3, 67, 132]
    assert np.isnan(out["loss_2d"][[1, 2]]).all() and (out["worst_img"][[1, 2]] == -1).all()
    assert np.isfinite(out["loss_2d"][[0, 3, 4]]).all() and (out["worst_img"][[0, 3, 4]] >= 0).all()
    assert out["mean_abs_px"][4] <= EXACT_PX and out["mean_abs_px"][3] > 1.0 and out["mean_abs_px"][0] > 1.0
    assert out["pred"].shape == (132, 4) and out["residual"].shape == (132, 4) and out["iou"].shape == (132,)
    assert not np.isnan(out["iou"]).any() and (out["img_ids"] >= 0).all()
    # each object alone gives the same numbers: the groups do not interact
    for i in (0, 3, 4):
        solo = multi_view.reprojection([mixed_tracks[i]], [mixed[i]], *args, fitter=Recorder())
        a, b = out["view_offsets"][i], out["view_offsets"][i + 1]
        assert np.array_equal(solo["pred"], out["pred"][a:b], equal_nan=True) and solo["loss_2d"][0] == out["loss_2d"][i]
        assert solo["worst_img"][0] == out["worst_img"][i]
    with pytest.raises(TypeError):
        multi_view.reprojection([tracks[0]], [np.eye(4)], *args, fitter=Recorder())
    with pytest.raises(ValueError):
        multi_view.reprojection(tracks[:2], [None], *args, fitter=Recorder())
    empty = multi_view.reprojection([], [], *args, fitter=Recorder())
    assert empty["loss_2d"].shape == (0,) and empty["view_offsets"].tolist() == [0] and empty["pred"].shape == (0, 4)


def test_odam_process_reprojection_reaches_it(golden):
    from odam_amd import multi_view
    from odam_amd.processor import OdamProcess
    z = golden("quadric_svd.npz")
    tracks = [z[f"track{i}"].copy() for i in (0, 2, 4)]
    names = [int(x) for x in z["img_names"]]
    rec = Recorder()
    proc = OdamProcess(None, None, None, None, fitter=rec)
    proc.init_sequence(z["K"], S.IMG_H, S.IMG_W)
    proc.usable_frames, proc.T_wcs, proc.P_cws = names, list(z["T_wcs"]), list(z["P_cws"])
    proc.tracks = [t.copy() for t in tracks]
    from odam_amd import sq
    quadrics = [sq.DualQuadric(z["gt_Q"][0]), None, sq.DualQuadric(z["gt_Q"][4])]
    out = proc.reprojection(tracks, quadrics)
    ref = multi_view.reprojection(tracks, quadrics, names, z["T_wcs"], z["P_cws"], S.IMG_H, S.IMG_W, z["K"], fitter=Recorder())
    assert set(out) == set(ref) and all(np.array_equal(out[k], ref[k], equal_nan=True) for k in ref)
    assert out["mean_abs_px"][0] <= EXACT_PX and out["mean_abs_px"][2] <= EXACT_PX and np.isnan(out["mean_abs_px"][1])
    assert proc._refine_state is None and all(np.array_equal(a, b) for a, b in zip(proc.tracks, tracks))


# ---- the C declarations -------------------------------------------------------------------------------------------------------------
C_TO_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}
ARG_NAMES = {
    "odam_sq_reproject_batch": ["ctx", "n_obj", "points", "n_pts", "view_offsets", "P", "max_views", "out_ext", "out_nvalid", "stream"],
    "odam_dq_reproject_batch": ["ctx", "n_obj", "Q", "view_offsets", "P", "max_views", "out_ext", "out_status", "stream"],
    "odam_reproject_score_f32": ["ctx", "n_obj", "view_offsets", "ext", "bad", "boxes", "mask", "img_w", "img_h", "max_views", "out_res",
                                 "out_iou", "out_obj", "out_obj_i", "stream"],
}
ARG_NAMES["odam_reproject_score_f64"] = ARG_NAMES["odam_reproject_score_f32"]


@pytest.mark.parametrize("name", sorted(ARG_NAMES))
def test_ctypes_signatures_match_the_header(name):
    from odam_amd import _lib, sq
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_sq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/odam_sq.h" % name
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    assert names == ARG_NAMES[name] and sq.REPROJECT_ARGTYPES[name] == want
    assert hasattr(_lib.lib(), name)
    f = sq._reproject_entry(name)
    assert list(f.argtypes) == want and f.restype is ctypes.c_int


def test_argument_checks_come_before_any_device_work():
    """with every pointer given (never dereferenced on these paths): the codes of the neighbouring entry points"""
    from odam_amd import _lib, sq
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: _lib.lib().odam_last_error()
    f = sq._reproject_entry("odam_sq_reproject_batch")
    assert f(p, 1, None, 1000, p, p, 4, p, p, None) == 1 and b"odam_sq_reproject_batch" in err()      # ODAM_E_INVALID
    assert f(p, -1, p, 1000, p, p, 4, p, p, None) == 1
    assert f(p, 1, p, 4097, p, p, 4, p, p, None) == 3 and b"n_pts" in err()                            # ODAM_E_LIMIT
    assert f(p, 1, p, 0, p, p, 4, p, p, None) == 3
    assert f(p, 1, p, 1000, p, p, 0, p, p, None) == 3 and b"max_views" in err()
    assert f(p, 1, p, 1000, p, p, 16 * 1024 + 1, p, p, None) == 3
    assert f(p, 0, p, 1000, p, p, 4, p, p, None) == 0
    f = sq._reproject_entry("odam_dq_reproject_batch")
    assert f(p, 1, p, None, p, 4, p, p, None) == 1 and b"odam_dq_reproject_batch" in err()
    assert f(p, 1, p, p, p, 0, p, p, None) == 3 and f(p, 0, p, p, p, 4, p, p, None) == 0
    for name in ("odam_reproject_score_f32", "odam_reproject_score_f64"):
        f = sq._reproject_entry(name)
        assert f(p, 1, p, p, None, p, None, 640, 480, 4, p, p, p, p, None) == 1 and name.encode() in err()
        assert f(p, 1, p, p, None, p, p, 0, 480, 4, p, p, p, p, None) == 1                             # an image without width
        assert f(p, 1, p, p, None, p, p, 640, float("nan"), 4, p, p, p, p, None) == 1
        assert f(p, 1, p, p, None, p, p, 640, 480, 0, p, p, p, p, None) == 3
        assert f(p, 0, p, p, None, p, p, 640, 480, 4, p, p, p, p, None) == 0                            # `bad` is nullable
