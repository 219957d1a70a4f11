"""numpy restatement of odam_amd/csrc/box_iou.hip (arithmetic of box_iou_core.h) in the kernels' own order, per scene, with the same
gates and limits.  Not product code: the checker of tests/test_evaluate_host.py and tests/test_evaluate_gpu.py.

The IoU mirrors odam_amd/merge.py::box3d_iou_pairs with every sum written out in index order (numpy's own reductions add four
terms as t0 + ((t1 + t2) + t3)); the matching is the reference's match_sequence (eval_scan2cad.py:249-267) as a plain loop."""
import numpy as np

MAX_GT = 4096
MAX_CLASS = 64


def _sum_in_order(terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


def _signed_area(x, y):
    """x, y: [n, 4]"""
    return 0.5 * _sum_in_order([x[:, k] * y[:, (k + 1) & 3] - y[:, k] * x[:, (k + 1) & 3] for k in range(4)])


def _boundary_inside(px, py, qx, qy, closed):
    contrib = []
    with np.errstate(all="ignore"):
        for j in range(4):
            j1 = (j + 1) & 3
            dx = px[:, j1] - px[:, j]; dy = py[:, j1] - py[:, j]
            enter = np.full(len(px), -np.inf); leave = np.full(len(px), np.inf)
            out_par = np.zeros(len(px), bool)
            for k in range(4):
                k1 = (k + 1) & 3
                ex = qx[:, k1] - qx[:, k]; ey = qy[:, k1] - qy[:, k]
                dist = ex * (py[:, j] - qy[:, k]) - ey * (px[:, j] - qx[:, k])
                rate = ex * dy - ey * dx
                t = -dist / rate
                par = rate == 0
                out_par |= par & ((dist < 0) if closed else (dist <= 0))
                enter = np.maximum(enter, np.where(rate > 0, t, -np.inf))
                leave = np.minimum(leave, np.where(rate < 0, t, np.inf))
            t0 = np.minimum(np.maximum(enter, 0.0), 1.0); t1 = np.minimum(np.maximum(leave, 0.0), 1.0)
            ok = (t1 > t0) & ~out_par
            sx = px[:, j] + t0 * dx; sy = py[:, j] + t0 * dy
            ex = px[:, j] + t1 * dx; ey = py[:, j] + t1 * dy
            contrib.append(np.where(ok, sx * ey - sy * ex, 0.0))
    return _sum_in_order(contrib) * 0.5


def _norm(a, b):
    d = a - b
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _volume(c):
    return (_norm(c[:, 0], c[:, 1]) * _norm(c[:, 1], c[:, 2])) * _norm(c[:, 0], c[:, 4])


def iou_pairs(C1, C2):
    """box_iou_core.h::box3d_iou for the pairs (C1[i], C2[i]), [n, 8, 3] each -> (iou3d [n], iou_bev [n])"""
    C1 = np.asarray(C1, np.float64).reshape(-1, 8, 3); C2 = np.asarray(C2, np.float64).reshape(-1, 8, 3)
    x1, y1 = C1[:, 3::-1, 0], C1[:, 3::-1, 1]
    x2, y2 = C2[:, 3::-1, 0], C2[:, 3::-1, 1]
    with np.errstate(all="ignore"):
        s1 = _signed_area(x1, y1); s2 = _signed_area(x2, y2)
        a1 = np.abs(s1); a2 = np.abs(s2)
        f1 = (s1 < 0)[:, None]; f2 = (s2 < 0)[:, None]
        ax = np.where(f1, x1[:, ::-1], x1); ay = np.where(f1, y1[:, ::-1], y1)
        bx = np.where(f2, x2[:, ::-1], x2); by = np.where(f2, y2[:, ::-1], y2)
        raw = np.maximum(_boundary_inside(ax, ay, bx, by, True) + _boundary_inside(bx, by, ax, ay, False), 0.0)
        inter = np.where(s2 > 0, raw, 0.0)
        bev = inter / ((a1 + a2) - inter)
        dz = np.maximum(0.0, np.minimum(C1[:, 0, 2], C2[:, 0, 2]) - np.maximum(C1[:, 4, 2], C2[:, 4, 2]))
        iv = inter * dz
        return iv / ((_volume(C1) + _volume(C2)) - iv), bev


def gate_open(gate, ca, cb):
    """[n, m] bool: the pairs a launch evaluates (0 all, 1 equal class, 2 the merge rule of run_merge.py:105-110)"""
    ca = np.asarray(ca).reshape(-1, 1); cb = np.asarray(cb).reshape(1, -1)
    same = ca == cb
    if gate == 0:
        return np.ones(same.shape, bool)
    if gate == 1:
        return same
    sc = lambda c: (c == 4) | (c == 5)
    return same | (sc(ca) & sc(cb))


def iou_scene(A, B, cls_a=None, cls_b=None, gate=0):
    """one scene: ([n, m] iou3d, [n, m] iou_bev); a gated-off pair is exactly 0 in both"""
    A = np.asarray(A, np.float64).reshape(-1, 8, 3); B = np.asarray(B, np.float64).reshape(-1, 8, 3)
    n, m = len(A), len(B)
    if gate not in (0, 1, 2) or (gate and (cls_a is None or cls_b is None)):
        raise ValueError("gate")
    i3 = np.zeros((n, m)); i2 = np.zeros((n, m))
    if n and m:
        op = gate_open(gate, cls_a if gate else np.zeros(n), cls_b if gate else np.zeros(m))
        i, j = np.nonzero(op)
        if len(i):
            i3[i, j], i2[i, j] = iou_pairs(A[i], B[j])
    return i3, i2


def iou_batch(scenes_a, scenes_b, cls_a=None, cls_b=None, gate=0):
    """all scenes: the flat pair arrays as the kernel lays them out, and pair_off"""
    outs = [iou_scene(a, b, None if cls_a is None else cls_a[s], None if cls_b is None else cls_b[s], gate)
            for s, (a, b) in enumerate(zip(scenes_a, scenes_b))]
    pair_off = np.concatenate([[0], np.cumsum([o[0].size for o in outs])]).astype(np.int64)
    flat = lambda k: np.concatenate([o[k].reshape(-1) for o in outs]) if outs else np.zeros(0)
    return flat(0), flat(1), pair_off


def match_scene(iou, cls_pred, cls_gt, threshold, n_class=8):
    """match_sequence on one scene.  iou [n, m] (rows = predictions); returns counts [3, n_class] (gts, preds, tps), claimed [n],
    gt_match [m]"""
    cls_pred = np.asarray(cls_pred, np.int64).reshape(-1); cls_gt = np.asarray(cls_gt, np.int64).reshape(-1)
    n, m = len(cls_pred), len(cls_gt)
    if not 1 <= n_class <= MAX_CLASS:
        raise ValueError("n_class")
    if m > MAX_GT:
        raise OverflowError("more than %d ground-truth boxes in a scene" % MAX_GT)
    iou = np.asarray(iou, np.float64).reshape(n, m)
    counts = np.zeros((3, n_class), np.int32); claimed = np.zeros(n, np.int32); gt_match = np.full(m, -1, np.int32)
    for c in cls_gt:
        if 0 <= c < n_class:
            counts[0, c] += 1
    used = set()
    for p in range(n):
        cp = cls_pred[p]
        if not 0 <= cp < n_class:
            continue
        counts[1, cp] += 1
        for i in range(m):
            if cls_gt[i] == cp and iou[p, i] > threshold and i not in used:      # no break: as the reference
                used.add(i)
                counts[2, cp] += 1
                claimed[p] += 1
                gt_match[i] = p
    return counts, claimed, gt_match


def match_batch(ious, cls_preds, cls_gts, threshold, n_class=8):
    outs = [match_scene(i, p, g, threshold, n_class) for i, p, g in zip(ious, cls_preds, cls_gts)]
    cat = lambda k, dt: np.concatenate([o[k] for o in outs]) if outs else np.zeros(0, dt)
    return (np.stack([o[0] for o in outs]) if outs else np.zeros((0, 3, n_class), np.int32)), cat(1, np.int32), cat(2, np.int32)


def degenerate_pairs(a, b):
    """from one overlapping pair (a, b): identical boxes, a box without volume (0 / 0) against itself and on either side, a NaN corner
    on either side, a NaN height, a clockwise clipper -> (A, B) [8, 8, 3]"""
    flat = a.copy(); flat[:] = a[0]
    nan_a = a.copy(); nan_a[2, 0] = np.nan
    nan_z = b.copy(); nan_z[4, 2] = np.nan
    cw = b[[3, 2, 1, 0, 7, 6, 5, 4]]
    return np.stack([a, flat, flat, a, nan_a, a, a, a]), np.stack([a, flat, a, flat, b, nan_a, nan_z, cw])
