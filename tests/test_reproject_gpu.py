"""gfx950 reprojection kernels (odam_amd/csrc/reproject.hip through sq.SqFitter.reproject / reproject_dual / reprojection_score and
the raw entry points) against their numpy restatement tests/reproject_ref.py, the reference's get_bbox, the exact box edges of
tests/golden/quadric_svd.npz and the fit's own loss log.

What is asked:
  float32 (reproject_sq, score_f32)  the restatement's bits on every output
  float64 boxes (reproject_dq)       1e-11 px against the restatement and against get_bbox, 8e-12 px against exact edges: the bounds
                                     of the CPU checks (tests/test_reproject_host.py); the device's binary64 sqrt and division are
                                     not taken to be bit-equal
  float64 scores                     fed the device's own ext, so only the score arithmetic differs: a sum of F non-negative terms
                                     in another order, then at most 8 more roundings: (F + 8) 2^-52 relative; an IoU is 17 operations
                                     of which the last 8 are not exact for integers' neighbours: 8 x 2^-52 relative; the residual is
                                     one subtraction: equal; integers equal
  loss_2d against the fit's log      the extents are the fit's own, the fit adds s_d * (1 / F) in its own order: (F + 8) 2^-24"""
import ctypes

import numpy as np
import pytest

import dq_ref
import quadric_svd_ref as S
import reproject_ref as R

pytestmark = pytest.mark.gpu

BBOX_PX = 1e-11
EXACT_PX = 8e-12
U64 = 2.0 ** -52


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter("cuda:0", 200)
    yield f
    f.close()


@pytest.fixture(scope="module")
def cams(golden):
    """the 300 cameras of quadric_svd.npz looking at a scene around (0, 0, 0.5)"""
    return golden("quadric_svd.npz")["P_cws"].reshape(-1, 12)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _cloud(rs, n_pts):
    return (rs.standard_normal((n_pts, 3)) * 0.25 + [0.0, 0.0, 0.5]).astype(np.float32)


SENT_F, SENT_I = np.float32(-1234.5), -77


def _raw_sq(fitter, pts, vc, P, max_views, tail=5):
    """odam_sq_reproject_batch on buffers that start as sentinels and are `tail` rows longer than the views"""
    import torch
    from odam_amd import _lib, sq
    offs = np.concatenate([[0], np.cumsum(vc)]).astype(np.int32)
    rows = int(offs[-1])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ext = torch.full((rows + tail, 4), float(SENT_F), device="cuda", dtype=torch.float32)
    nv = torch.full((rows + tail,), SENT_I, device="cuda", dtype=torch.int32)
    d_pts, d_off, d_P = d(np.asarray(pts, np.float32)), d(offs), d(np.asarray(P, np.float32).reshape(-1, 12))
    rc = sq._reproject_entry("odam_sq_reproject_batch")(fitter._h, len(vc), _lib.ptr(d_pts), int(d_pts.shape[1]), _lib.ptr(d_off), _lib.ptr(d_P),
                                                        int(max_views), _lib.ptr(ext), _lib.ptr(nv), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().odam_last_error()
    torch.cuda.synchronize()
    return ext.cpu().numpy(), nv.cpu().numpy()


# ---- 1. reproject_sq: the restatement's bits ------------------------------------------------------------------------------------
def test_reproject_sq_on_the_references_points(fitter, golden):
    z = golden("sq_steps.npz")
    pts, P, vc = [], [], []
    for c in range(int(z["n_cases"])):
        for k in (0, 100, 199):
            pts.append(z[f"c{c}_pts{k}"]); P.append(z[f"c{c}_P"]); vc.append(len(z[f"c{c}_P"]))
    got = _np(fitter.reproject(np.stack(pts), vc, np.concatenate(P)))
    want = R.reproject(np.stack(pts), vc, np.concatenate(P))
    R.assert_same_f32(got["ext"], want["ext"], "ext")
    assert got["n_valid"].dtype == np.int32 and np.array_equal(got["n_valid"], want["n_valid"]) and (got["n_valid"] == 1000).all()


@pytest.mark.parametrize("n_pts", [1, 63, 65, 1000])
def test_reproject_sq_view_counts_and_untouched_words(fitter, cams, n_pts):
    """view counts at the slice and wave boundaries, an object without views between two others, one entirely behind its cameras,
    a NaN point, a point whose pixel is Inf / Inf; rows that no view owns keep the sentinel"""
    rs = np.random.RandomState(100 + n_pts)
    vc = [1, 63, 0, 64, 65, 129, 7, 5]
    pts = np.stack([_cloud(rs, n_pts) for _ in vc])
    P = np.concatenate([cams[rs.choice(len(cams), F, replace=False)] for F in vc]).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(vc)])
    P[offs[6]:offs[7]] *= -1.0                 # object 6: every depth negated -> nothing in front of any camera
    pts[7, 0] = np.nan                         # object 7: a NaN point (its depth is NaN: not valid) ...
    if n_pts > 1:                              # ... and one whose depth and x overflow while y does not: u = Inf / Inf
        pts[7, 1] = [0.1, 0.1, 3e38]
        for j in range(vc[7]):
            P[offs[7] + j] = [500 + 10 * j, 0, 320, 0, 0, 500, 0, 0, 0, 0, 2, 0]
    ext, nv = _raw_sq(fitter, pts, vc, P, max(vc))
    want = R.reproject(pts, vc, P, fill=(SENT_F, SENT_I))
    rows = offs[-1]
    R.assert_same_f32(ext[:rows], want["ext"], "ext")
    assert np.array_equal(nv[:rows], want["n_valid"])
    assert (ext[rows:] == SENT_F).all() and (nv[rows:] == SENT_I).all()
    assert (nv[offs[6]:offs[7]] == 0).all() and (ext[offs[6]:offs[7]] == [1e6, -1e6, 1e6, -1e6]).all()
    assert (nv[:offs[6]] > 0).any()
    if n_pts > 1:
        last = ext[offs[7]:offs[8]]
        assert np.isnan(last[:, :2]).all() and not np.isnan(last[:, 2:]).any() and (nv[offs[7]:offs[8]] < n_pts).all()
    # through SqFitter (its own buffers): the same bits
    got = _np(fitter.reproject(pts, vc, P))
    R.assert_same_f32(got["ext"], want["ext"], "SqFitter.reproject")
    assert np.array_equal(got["n_valid"], want["n_valid"])
    # an object with more views than max_views owns none: its rows keep the sentinel, the others are as before
    ext64, nv64 = _raw_sq(fitter, pts, vc, P, 64)
    want64 = R.reproject(pts, vc, P, max_views=64, fill=(SENT_F, SENT_I))
    R.assert_same_f32(ext64[:rows], want64["ext"], "max_views 64")
    assert np.array_equal(nv64[:rows], want64["n_valid"]) and (nv64[offs[4]:offs[6]] == SENT_I).all() and (nv64[offs[3]:offs[4]] != SENT_I).all()


# ---- 2. reproject_dq ------------------------------------------------------------------------------------------------------------------
def test_reproject_dq_vs_restatement_get_bbox_and_exact_edges(fitter, golden, measured):
    z = golden("quadric_svd.npz")
    kind = z["kind"].astype(int)
    n = int(z["n_obj"])
    views = [R.svd_track_views(z, i) for i in range(n)]
    d = golden("dq_fits.npz")
    nd = int(d["n_cases"])
    Q = np.concatenate([z["gt_Q"], np.stack([d[f"c{c}_Q"] for c in range(nd)]).astype(np.float64)])
    Ps = [v[0] for v in views] + [d[f"c{c}_P"].astype(np.float64) for c in range(nd)]
    vc = [len(p) for p in Ps]
    assert {3, 64, 65, 129, 300} <= set(vc)
    out = fitter.reproject_dual(Q, vc, np.concatenate(Ps))
    assert out["ext"].dtype.is_floating_point and out["ext"].element_size() == 8
    got = _np(out)
    want = R.reproject_dual(Q, vc, np.concatenate(Ps))
    assert np.array_equal(got["status"], want["status"]) and (got["status"] == 0).all()
    offs = np.concatenate([[0], np.cumsum(vc)])
    w_ref = float(np.abs(got["ext"] - want["ext"]).max())
    w_bbox = max(float(np.abs(got["ext"][offs[i]:offs[i + 1]] - R.get_bbox_rows(Q[i], Ps[i])).max()) for i in range(len(vc)))
    w_exact = max(float(np.abs(got["ext"][offs[i]:offs[i + 1]] - views[i][1]).max()) for i in range(n) if kind[i] in (S.KIND_EXACT, S.KIND_TWO_VIEWS))
    print("reproject_dq: vs restatement %.3e px, vs get_bbox %.3e px, vs exact edges %.3e px" % (w_ref, w_bbox, w_exact))
    measured("reproject_dq_vs_restatement_px", w_ref)
    measured("reproject_dq_vs_get_bbox_px", w_bbox)
    measured("reproject_dq_vs_exact_edges_px", w_exact)
    assert w_ref <= BBOX_PX and w_bbox <= BBOX_PX and w_exact <= EXACT_PX


def test_reproject_dq_status(fitter, golden):
    """a camera inside the ellipsoid (dq_ref.discriminant_problem): status 1 and NaN for that view only; c22 == 0 likewise"""
    d = dq_ref.case(golden("dq_fits.npz"), 0)
    Q = dq_ref.make_obj(d["init5"], d["half_dims"])["Q"].reshape(4, 4)
    P = dq_ref.discriminant_problem(d, view=3).astype(np.float64)
    Pz = d["P"].astype(np.float64).copy()
    Pz[1, 8:12] = 0.0
    F = len(P)
    got = _np(fitter.reproject_dual(np.stack([Q, Q, Q]), [F, F, F], np.concatenate([d["P"].astype(np.float64), P, Pz])))
    st = got["status"].reshape(3, F)
    assert (st[0] == 0).all() and st[1].tolist() == [0, 0, 0, 1] + [0] * (F - 4) and st[2].tolist() == [0, 1] + [0] * (F - 2)
    ext = got["ext"].reshape(3, F, 4)
    assert np.isnan(ext[1, 3]).all() and np.isnan(ext[2, 1]).all() and np.isfinite(ext[0]).all()
    assert np.array_equal(np.delete(ext[1], 3, axis=0), np.delete(ext[0], 3, axis=0))      # the other views are unaffected
    assert np.array_equal(np.delete(ext[2], 1, axis=0), np.delete(ext[0], 1, axis=0))
    want = R.reproject_dual(np.stack([Q, Q, Q]), [F, F, F], np.concatenate([d["P"].astype(np.float64), P, Pz]))
    assert np.array_equal(got["status"], want["status"]) and np.allclose(got["ext"], want["ext"], rtol=0, atol=BBOX_PX, equal_nan=True)


# ---- 3. reprojection_score ------------------------------------------------------------------------------------------------------------
def test_score_f32_bit_for_bit(fitter, cams):
    """fed the device's own ext; view counts at the wave boundaries, an object without views, masked edges, bad views, ties"""
    rs = np.random.RandomState(7)
    vc = [1, 64, 0, 65, 129, 3]
    pts = np.stack([_cloud(rs, 200) for _ in vc])
    P = np.concatenate([cams[rs.choice(len(cams), F, replace=False)] for F in vc]).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(vc)])
    P[offs[3] + 64] *= -1.0                                     # a view with nothing in front of the camera
    r = fitter.reproject(pts, vc, P)
    ext = r["ext"].cpu().numpy()
    bad = (r["n_valid"] == 0)
    boxes = (ext + rs.uniform(-6, 6, ext.shape)).astype(np.float32)
    boxes[offs[4]:offs[4] + 129] = ext[offs[4]:offs[4] + 129]   # object 4: every IoU is 1 (or 0 where the box is off the image): ties
    boxes[offs[5]:offs[6]] = [700, 900, 500, 600]               # object 5: detections that miss the prediction: every IoU 0
    mask = (rs.uniform(size=ext.shape) > 0.25).astype(np.float32)
    mask[offs[1] + 5] = 0
    mask[offs[0]:offs[1]] = 0                                   # object 0: no constrained edge at all
    got = _np(fitter.reprojection_score(r["ext"], bad, vc, boxes, mask, 640, 480))
    want = R.reprojection_score(ext, bad.cpu().numpy(), vc, boxes, mask, 640, 480)
    assert got["loss_2d"].dtype == np.float32
    for key in ("residual", "iou", "loss_2d", "mean_abs_px", "mean_iou", "min_iou"):
        a, b = got[key], want[key]
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        R.assert_same_f32(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0), key)
    for key in ("worst_view", "n_edges", "n_bad"):
        assert np.array_equal(got[key], want[key]), key
    assert got["worst_view"].tolist()[2] == -1 and np.isnan(got["loss_2d"][2]) and got["n_bad"][3] == 1
    assert np.isnan(got["mean_abs_px"][0]) and got["loss_2d"][0] == 0 and got["worst_view"][5] == 0 and got["min_iou"][5] == 0
    assert got["iou"][offs[3] + 64] == 0


def test_score_f64_within_the_derived_bounds(fitter, golden, measured):
    z = golden("quadric_svd.npz")
    ids = [i for i in range(int(z["n_obj"])) if int(z["kind"][i]) in (S.KIND_NOISY, S.KIND_MASKED)]
    rows = [S.track_rows(z, i) for i in ids]      # P, edges, mask of the views with a constrained edge
    vc = [len(r[2]) for r in rows] + [0]
    assert {64, 65, 129, 300} <= set(vc)
    P, boxes, mask = (np.concatenate([r[k] for r in rows]) for k in range(3))
    r = fitter.reproject_dual(np.concatenate([z["gt_Q"][ids], np.eye(4)[None]]), vc, P)
    ext = r["ext"].cpu().numpy()
    got = _np(fitter.reprojection_score(r["ext"], r["status"], vc, boxes, mask, S.IMG_W, S.IMG_H))
    want = R.reprojection_score(ext, r["status"].cpu().numpy(), vc, boxes, mask, S.IMG_W, S.IMG_H)
    assert got["loss_2d"].dtype == np.float64 and np.array_equal(got["residual"], want["residual"])
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b))) if len(a) else 0.0
    e_iou = rel(got["iou"], want["iou"])
    print("score_f64: per-view IoU %.2f x 2^-52" % (e_iou / U64))
    measured("reproject_score_f64_iou_ulps", e_iou / U64)
    assert (want["iou"] > 0).all() and e_iou <= 8 * U64
    for j, F in enumerate(vc[:-1]):
        for key in ("loss_2d", "mean_abs_px", "mean_iou"):
            e = abs(got[key][j] - want[key][j]) / abs(want[key][j])
            measured("reproject_score_f64_sum_ulps", e / U64)
            assert e <= (F + 8) * U64, (key, j, e / U64)
        assert abs(got["min_iou"][j] - want["min_iou"][j]) <= 8 * U64 * want["min_iou"][j]
    for key in ("worst_view", "n_edges", "n_bad"):
        assert np.array_equal(got[key], want[key]), key
    noisy = [j for j, i in enumerate(ids) if int(z["kind"][i]) == S.KIND_NOISY]
    assert np.isnan(got["loss_2d"][-1]) and got["worst_view"][-1] == -1 and (got["mean_abs_px"][noisy] > 0.1).all()


# ---- 4. consistency with the fit ------------------------------------------------------------------------------------------------------
def test_loss_2d_of_the_fits_trajectory_is_the_fits_loss_log(fitter, golden):
    z = golden("sq_steps.npz")
    cases = [dq_ref.case(z, c) for c in (0, 1)]
    vc = [len(d["tgt"]) for d in cases]
    P, tgt, mask = (np.concatenate([d[k] for d in cases]) for k in ("P", "tgt", "mask"))
    fit = fitter.fit(np.stack([d["p0"] for d in cases]), [int(d["cls"]) for d in cases], vc, P, tgt, mask, n_iters=200,
                     want_loss=True, want_traj=True)
    loss = fit["loss"].cpu().numpy()
    for k in (1, 50, 199):
        r = fitter.reproject(fitter.points(fit["traj"][:, k - 1]), vc, P)
        s = _np(fitter.reprojection_score(r["ext"], r["n_valid"] == 0, vc, tgt, mask, 640, 480))
        for j, F in enumerate(vc):
            e = abs(float(s["loss_2d"][j]) - float(loss[j, k])) / abs(float(loss[j, k]))
            print("object %d step %3d: loss_2d %.9g, fit's log %.9g, rel %.2e (bound %.2e)" % (j, k, s["loss_2d"][j], loss[j, k], e, (F + 8) * 2.0 ** -24))
            assert e <= (F + 8) * 2.0 ** -24, (j, k, e)
        assert (s["n_bad"] == 0).all()


# ---- 5. the host path on the device ----------------------------------------------------------------------------------------------------
def _same(out, ref, px, rel_sum):
    """multi_view.reprojection on the device against the stand-in: integers and the layout equal, pixels within px, sums within
    px + rel_sum x F relative, IoU (boxes of at least 10 px a side: d iou <= 4 px / 10 per edge pair) within px + 8 x 2^-52"""
    for key in ("n_views", "n_edges", "n_bad", "view_offsets", "img_ids"):
        assert np.array_equal(out[key], ref[key]), key
    assert np.allclose(out["pred"], ref["pred"], rtol=0, atol=px, equal_nan=True)
    assert np.allclose(out["residual"], ref["residual"], rtol=0, atol=px)
    assert np.allclose(out["iou"], ref["iou"], rtol=8 * U64, atol=px)
    F = np.maximum(out["n_views"], 1)
    for key in ("loss_2d", "mean_abs_px", "mean_iou", "min_iou"):
        a, b = out[key], ref[key]
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        ok = ~np.isnan(a)
        assert (np.abs(a[ok] - b[ok]) <= 4 * px + rel_sum * (F[ok] + 8) * np.abs(b[ok])).all(), key


def test_multi_view_reprojection_of_optim_process_output(fitter, golden):
    from odam_amd import multi_view
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    args = ([int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], 480, 640, z["K"])
    op = multi_view.optim_process(tracks, *args, "super_quadric", True, 200, 10, fitter=fitter, return_params=True)
    assert op["fitted"].any() and not op["fitted"].all()      # the unfitted ones have no cached points: one points call
    out = multi_view.reprojection(tracks, op["quadrics"], *args, fitter=fitter)
    ref = multi_view.reprojection(tracks, op["quadrics"], *args, fitter=R.RefFitter())
    _same(out, ref, 0.0, 0.0)                                 # float32 throughout: the restatement's bits
    assert np.array_equal(out["worst_img"], ref["worst_img"])
    print("fitted", op["fitted"], "mean_abs_px", out["mean_abs_px"], "mean_iou", out["mean_iou"])
    assert (out["n_views"] > 0).all() and np.isfinite(out["loss_2d"]).all()


def test_multi_view_reprojection_of_closed_form_output(fitter, golden):
    from odam_amd import multi_view
    z = golden("quadric_svd.npz")
    tracks = S.fixture_tracks(z)
    args = ([int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], S.IMG_H, S.IMG_W, z["K"])
    kind = z["kind"].astype(int)
    cf = multi_view.closed_form_quadrics(tracks, *args, n_views=3, fitter=fitter)
    assert sum(q is None for q in cf["quadrics"]) == 2
    out = multi_view.reprojection(tracks, cf["quadrics"], *args, fitter=fitter)
    ref = multi_view.reprojection(tracks, cf["quadrics"], *args, fitter=R.RefFitter())
    edges = np.concatenate([S.track_rows(z, i)[1] for i in range(len(tracks)) if cf["quadrics"][i] is not None])
    assert (edges[:, 1] - edges[:, 0] >= 10).all() and (edges[:, 3] - edges[:, 2] >= 10).all()
    _same(out, ref, BBOX_PX, U64)
    for i in range(len(tracks)):
        if cf["quadrics"][i] is None:      # skipped
            assert np.isnan(out["loss_2d"][i]) and out["worst_img"][i] == -1 and out["n_views"][i] == 0
        elif kind[i] == S.KIND_EXACT:
            print("exact object %d: mean_abs_px %.3e" % (i, out["mean_abs_px"][i]))
            assert cf["status"][i] == 0 and out["mean_abs_px"][i] <= EXACT_PX and out["n_bad"][i] == 0
        elif kind[i] == S.KIND_NOISY:
            assert 0.1 <= out["mean_abs_px"][i] <= 3.0


def test_error_paths_with_a_live_context(fitter):
    import torch
    from odam_amd import _lib, sq
    t = torch.zeros(64, device="cuda", dtype=torch.float64)
    p, h = _lib.ptr(t), fitter._h
    f = sq._reproject_entry("odam_sq_reproject_batch")
    assert f(h, 1, None, 1000, p, p, 4, p, p, None) == 1
    assert f(h, 1, p, 4097, p, p, 4, p, p, None) == 3
    assert f(h, 1, p, 1000, p, p, 0, p, p, None) == 3
    assert f(h, 0, p, 1000, p, p, 4, p, p, None) == 0
    g = sq._reproject_entry("odam_dq_reproject_batch")
    assert g(h, 1, None, p, p, 4, p, p, None) == 1 and g(h, 1, p, p, p, 0, p, p, None) == 3 and g(h, 0, p, p, p, 4, p, p, None) == 0
    for name in ("odam_reproject_score_f32", "odam_reproject_score_f64"):
        s = sq._reproject_entry(name)
        assert s(h, 1, p, None, None, p, p, 640, 480, 4, p, p, p, p, None) == 1
        assert s(h, 1, p, p, None, p, p, 640, 480, 0, p, p, p, p, None) == 3
        assert s(h, 0, p, p, None, p, p, 640, 480, 4, p, p, p, p, None) == 0
    torch.cuda.synchronize()
    assert (t == 0).all()
    # the empty call and the host's own refusals
    e = fitter.reproject(np.zeros((0, 1000, 3), np.float32), [], np.zeros((0, 12), np.float32))
    assert e["ext"].shape == (0, 4) and fitter.reproject_dual(np.zeros((0, 4, 4)), [], np.zeros((0, 12)))["status"].shape == (0,)
    # objects, but none that owns a view
    assert fitter.reproject(np.zeros((2, 10, 3), np.float32), [0, 0], np.zeros((0, 12), np.float32))["n_valid"].shape == (0,)
    s = _np(fitter.reprojection_score(np.zeros((0, 4)), None, [0, 0], np.zeros((0, 4)), np.zeros((0, 4)), 640, 480))
    assert np.isnan(s["loss_2d"]).all() and s["worst_view"].tolist() == [-1, -1] and s["n_edges"].tolist() == [0, 0] and s["n_bad"].tolist() == [0, 0]
    with pytest.raises(_lib.OdamError):
        fitter.reproject(np.zeros((1, 4097, 3), np.float32), [1], np.zeros((1, 12), np.float32))
    with pytest.raises(_lib.OdamError):
        fitter.reproject_dual(np.eye(4)[None], [-1], np.zeros((0, 12)))
