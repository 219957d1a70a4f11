"""Host restatement of the reprojection kernels (odam_amd/csrc/reproject.hip, reproject_core.h; include/odam_sq.h): numpy, with the
kernels' operations in the kernels' order.

  * reproject_sq: float32; the projection rows are odam_sq::proj_row (two fmaf, restated by dq_ref.fma32), the division and the
    comparisons are numpy's float32 ones, min / max are exact -- the device's bits are asked for.
  * reproject_dq: float64; every entry of C = (P Q) P^T as ((a0 b0 + a1 b1) + a2 b2) + a3 b3, then get_bbox's formulas.  The
    device's binary64 sqrt and division are not taken to be bit-equal: tests hold it to a tolerance.
  * score: per view residuals and IoU, per object the sums in the order of dq_ref.wave_sums (lane partials, XOR butterfly), in
    float32 (bits asked for) or float64.
RefFitter stands in for sq.SqFitter where multi_view.reprojection is run on the CPU."""
import numpy as np

from dq_ref import fma32

f32 = np.float32
FILL = f32(1000000.0)
MAX_PTS = 4096


def _proj_row(w, m):
    """odam_sq::proj_row for points w [N, 3] and matrix rows m [F, 4] -> [F, N] float32"""
    w0, w1, w2 = (w[None, :, k] for k in range(3))
    m0, m1, m2, m3 = (m[:, k, None] for k in range(4))
    with np.errstate(all="ignore"):
        return (fma32(w2, m2, fma32(w1, m1, (w0 * m0).astype(f32))) + m3).astype(f32)


def reproject_sq_one(points, P):
    """points [N, 3], P [F, 12] float32 -> ext [F, 4] float32 (x_min, x_max, y_min, y_max), n_valid [F] int32"""
    w = np.ascontiguousarray(points, f32).reshape(-1, 3)
    M = np.ascontiguousarray(P, f32).reshape(-1, 3, 4)
    qx, qy, qz = (_proj_row(w, M[:, r]) for r in range(3))
    with np.errstate(all="ignore"):
        den = (np.abs(qz) + f32(1e-6)).astype(f32)
        u, v = (qx / den).astype(f32), (qy / den).astype(f32)
        valid = qz > f32(0.5)

    def extent(x, lo):
        fill = FILL if lo else -FILL
        nan = (valid & np.isnan(x)).any(axis=1)
        y = np.where(valid & ~np.isnan(x), x, fill)
        r = np.minimum(y.min(axis=1), fill) if lo else np.maximum(y.max(axis=1), fill)
        return np.where(nan, f32(np.nan), r.astype(f32) + f32(0.0)).astype(f32)      # -0 -> +0, as the kernel stores it
    ext = np.stack([extent(u, True), extent(u, False), extent(v, True), extent(v, False)], axis=1)
    return ext, valid.sum(axis=1).astype(np.int32)


def _dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def reproject_dq_one(Q, P):
    """Q [4, 4], P [F, 12] -> ext [F, 4] float64 (x_min, x_max, y_min, y_max; NaN where status is 1), status [F] int32"""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    M = np.asarray(P, np.float64).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        PQ = _dot4(M[:, :, None, :], Q.T[None, None, :, :])      # [F, 3, 4]: row i of P with column k of Q
        c00, c02 = _dot4(PQ[:, 0], M[:, 0]), _dot4(PQ[:, 0], M[:, 2])
        c11, c12 = _dot4(PQ[:, 1], M[:, 1]), _dot4(PQ[:, 1], M[:, 2])
        c22 = _dot4(PQ[:, 2], M[:, 2])

        def axis(cii, ci2):
            D = 4.0 * (ci2 * ci2) - (4.0 * cii) * c22
            ok = D >= 0.0
            b = np.sqrt(np.where(ok, D, 0.0))
            r = 0.5 / c22
            s2 = 2.0 * ci2
            x0, x1 = r * (s2 + b), r * (s2 - b)
            return np.where(x1 < x0, x1, x0), np.where(x1 > x0, x1, x0), ok
        x_lo, x_hi, okx = axis(c00, c02)
        y_lo, y_hi, oky = axis(c11, c12)
    good = okx & oky & (c22 != 0.0)
    ext = np.where(good[:, None], np.stack([x_lo, x_hi, y_lo, y_hi], axis=1), np.nan)
    return ext, (~good).astype(np.int32)


def wave_sums(rows):
    """dq_ref.wave_sums for any float type: rows [n][F] -> [n]"""
    rows = np.asarray(rows)
    n, F = rows.shape
    J = (F + 63) // 64
    pad = np.zeros((n, J * 64), rows.dtype)
    pad[:, :F] = rows
    pad = pad.reshape(n, J, 64)
    part = np.zeros((n, 64), rows.dtype)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for j in range(J):
            part = part + pad[:, j]
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[:, idx ^ off]
    return part[:, 0]


def view_scores(ext, bad, boxes, mask, img_w, img_h, dtype):
    """per view: residual [F, 4], iou [F] in `dtype` (reproject_core.h: edge_residual, box_iou)"""
    T = np.dtype(dtype).type
    e = np.asarray(ext, dtype).reshape(-1, 4)
    b = np.asarray(boxes, dtype).reshape(-1, 4)
    m = np.asarray(mask, f32).reshape(-1, 4) != 0
    bad = np.zeros(len(e), bool) if bad is None else (np.asarray(bad).reshape(-1) != 0)
    zero, w, h = T(0), T(img_w), T(img_h)
    with np.errstate(all="ignore"):
        d = e - b
        a = np.where(d < zero, -d, d)
        res = np.where(m & ~np.isnan(a), a, zero).astype(dtype)
        clip = lambda x, hi: np.where(x < zero, zero, np.where(x > hi, hi, x))
        pos = lambda x: np.where(x > zero, x, zero)
        px0, px1, py0, py1 = clip(e[:, 0], w), clip(e[:, 1], w), clip(e[:, 2], h), clip(e[:, 3], h)
        area_p = pos(px1 - px0) * pos(py1 - py0)
        area_d = pos(b[:, 1] - b[:, 0]) * pos(b[:, 3] - b[:, 2])
        ix0, ix1 = np.where(b[:, 0] > px0, b[:, 0], px0), np.where(b[:, 1] < px1, b[:, 1], px1)
        iy0, iy1 = np.where(b[:, 2] > py0, b[:, 2], py0), np.where(b[:, 3] < py1, b[:, 3], py1)
        inter = pos(ix1 - ix0) * pos(iy1 - iy0)
        uni = (area_p + area_d) - inter
        q = inter / uni
        iou = np.where(bad | ~(uni > zero) | np.isnan(q), zero, q).astype(dtype)
    return res, iou


def score_one(ext, bad, boxes, mask, img_w, img_h, dtype):
    """one object -> residual [F, 4], iou [F], obj [4] (loss_2d, mean_abs_px, mean_iou, min_iou), obj_i [3] (worst_view, n_edges,
    n_bad)"""
    T = np.dtype(dtype).type
    F = len(np.asarray(mask).reshape(-1, 4))
    if F == 0:
        return np.zeros((0, 4), dtype), np.zeros(0, dtype), np.full(4, np.nan, dtype), np.array([-1, 0, 0], np.int32)
    res, iou = view_scores(ext, bad, boxes, mask, img_w, img_h, dtype)
    s = wave_sums(np.concatenate([res.T, iou[None]]))
    n_edges = int((np.asarray(mask).reshape(-1, 4) != 0).sum())
    n_bad = 0 if bad is None else int((np.asarray(bad).reshape(-1) != 0).sum())
    Ff = T(F)
    with np.errstate(all="ignore"):
        loss = ((s[0] / Ff + s[1] / Ff) + s[2] / Ff) + s[3] / Ff
        mean_abs = (((s[0] + s[1]) + s[2]) + s[3]) / T(n_edges) if n_edges else T(np.nan)
        mean_iou = s[4] / Ff
    worst = int(np.argmin(iou))      # the first of equal minima
    return res, iou, np.array([loss, mean_abs, mean_iou, iou[worst]], dtype), np.array([worst, n_edges, n_bad], np.int32)


def _offsets(view_counts, max_views):
    vc = np.asarray(view_counts, np.int64).reshape(-1)
    offs = np.zeros(len(vc) + 1, np.int64)
    offs[1:] = np.cumsum(vc)
    owned = (vc >= 1) & (vc <= (max_views if max_views is not None else max(int(vc.max()) if len(vc) else 1, 1)))
    return offs, owned


def reproject(points, view_counts, P, max_views=None, fill=None):
    """odam_sq_reproject_batch: rows that no view owns keep `fill` = (ext row, n_valid word)"""
    pts = np.asarray(points, f32)
    P = np.asarray(P, f32).reshape(-1, 12)
    offs, owned = _offsets(view_counts, max_views)
    ext = np.zeros((offs[-1], 4), f32)
    nv = np.zeros(offs[-1], np.int32)
    if fill is not None:
        ext[:], nv[:] = fill
    for i in np.flatnonzero(owned):
        ext[offs[i]:offs[i + 1]], nv[offs[i]:offs[i + 1]] = reproject_sq_one(pts[i], P[offs[i]:offs[i + 1]])
    return {"ext": ext, "n_valid": nv}


def reproject_dual(Q, view_counts, P, max_views=None):
    Q = np.asarray(Q, np.float64).reshape(-1, 4, 4)
    P = np.asarray(P, np.float64).reshape(-1, 12)
    offs, owned = _offsets(view_counts, max_views)
    ext = np.zeros((offs[-1], 4))
    st = np.zeros(offs[-1], np.int32)
    for i in np.flatnonzero(owned):
        ext[offs[i]:offs[i + 1]], st[offs[i]:offs[i + 1]] = reproject_dq_one(Q[i], P[offs[i]:offs[i + 1]])
    return {"ext": ext, "status": st}


def reprojection_score(ext, bad, view_counts, boxes, mask, img_w, img_h, max_views=None):
    ext = np.asarray(ext)
    dtype = np.float64 if ext.dtype == np.float64 else np.float32
    ext = ext.reshape(-1, 4)
    boxes = np.asarray(boxes).reshape(-1, 4)
    mask = np.asarray(mask).reshape(-1, 4)
    bad = None if bad is None else np.asarray(bad).reshape(-1)
    offs, owned = _offsets(view_counts, max_views)
    n = len(owned)
    res, iou = np.zeros((offs[-1], 4), dtype), np.zeros(offs[-1], dtype)
    obj, obj_i = np.empty((n, 4), dtype), np.empty((n, 3), np.int32)
    for i in range(n):
        a, b = (offs[i], offs[i + 1]) if owned[i] else (0, 0)
        r = score_one(ext[a:b], None if bad is None else bad[a:b], boxes[a:b], mask[a:b], img_w, img_h, dtype)
        res[a:b], iou[a:b], obj[i], obj_i[i] = r
    return {"residual": res, "iou": iou, "loss_2d": obj[:, 0], "mean_abs_px": obj[:, 1], "mean_iou": obj[:, 2], "min_iou": obj[:, 3],
            "worst_view": obj_i[:, 0], "n_edges": obj_i[:, 1], "n_bad": obj_i[:, 2]}


class RefFitter:
    """stands in for sq.SqFitter where multi_view.reprojection is all that is called; points() is the CPU oracle's surface sampler
    (oracle/sq_oracle.c), which the device equals bit for bit (tests/test_sq_gpu.py)"""
    reproject = staticmethod(reproject)
    reproject_dual = staticmethod(reproject_dual)
    reprojection_score = staticmethod(reprojection_score)

    def __init__(self):
        self.calls = []
        self._oracle = None

    def points(self, params):
        from conftest import Oracle
        self._oracle = self._oracle or Oracle()
        self.calls.append(("points", len(params)))
        return np.stack([self._oracle.points(p) for p in np.asarray(params, f32).reshape(-1, 9)])


def assert_same_f32(a, b, what=""):
    """bit for bit"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, a, b)


# ---- fixture helpers shared by tests/test_reproject_host.py, tests/test_reproject_gpu.py and tests/golden/make_reproject_figures.py
def get_bbox_rows(Q, P):
    """sq.DualQuadric(Q).get_bbox(P) per view, reordered to x_min, x_max, y_min, y_max"""
    from odam_amd import sq
    q = sq.DualQuadric(np.asarray(Q, np.float64))
    return np.stack([q.get_bbox(M)[[0, 2, 1, 3]] for M in np.asarray(P, np.float64).reshape(-1, 3, 4)])


def svd_track_views(z, i):
    """every row of track i of quadric_svd.npz: P [F, 12] and the edge columns x_min, x_max, y_min, y_max"""
    tr = z[f"track{i}"]
    ids = {int(f): k for k, f in enumerate(z["img_names"])}
    img = np.array([ids[int(f)] for f in tr[:, 0]])
    return z["P_cws"][img].reshape(-1, 12), tr[:, [2, 4, 3, 5]]
