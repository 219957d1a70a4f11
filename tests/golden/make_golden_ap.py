"""Golden for the average precision: the reference's own eval_det_cls, voc_ap and eval_det (src/utils/eval_utils.py, imported
here) on 10 synthetic images of 0-15 ground-truth boxes over the eight classes, with perturbed, duplicated (two or three predictions
on one box), wrong-class and spurious predictions in shuffled order, at thresholds 0.25 and 0.5 and in both AP forms.  Stores the
inputs and, observed on the reference's own run: every IoU it evaluated (folded into ovmax / jmax per prediction by its own
`iou > ovmax`), the tp / fp flags per ranked prediction (the arrays it hands to np.cumsum), rec, prec and AP per class.
eval_det's print raises for class 3 (its CARE_CLASSES has no entry): eval_det runs on the other seven classes, eval_det_cls on all.
Arrays only.  Run: python tests/golden/make_golden_ap.py"""
import contextlib
import io
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

THRESHOLDS = (0.25, 0.5)
N_GT = (7, 0, 15, 4, 11, 1, 9, 13, 6, 10)      # image 1 has no ground truth; image 3's predictions are all dropped
MARGIN = 1e-6
SEED = 11


def make_images(bu):
    rs = np.random.RandomState(SEED)
    images = []
    for s, n_gt in enumerate(N_GT):
        gts, preds = [], []

        def add_pred(c, ctr, dims, yaw, sigma):
            preds.append((c, bu.get_3d_box(dims * rs.uniform(1 - sigma, 1 + sigma, 3), bu.rotz(yaw + rs.normal(0, sigma)),
                                           ctr + rs.normal(0, sigma * 0.5, 3)), float(rs.uniform(0.05, 1.0))))
        if s == 0:                        # class 7 once: one box, one prediction
            ctr = rs.uniform(-4, 4, 3) * [1, 1, 0.2]; dims = rs.uniform(0.4, 1.8, 3); yaw = rs.uniform(-np.pi, np.pi)
            gts.append((7, bu.get_3d_box(dims, bu.rotz(yaw), ctr)))
            add_pred(7, ctr, dims, yaw, 0.05)
        for g in range(n_gt - len(gts)):
            c = int(rs.randint(0, 7))
            ctr = rs.uniform(-4, 4, 3) * [1, 1, 0.2]; dims = rs.uniform(0.4, 1.8, 3); yaw = rs.uniform(-np.pi, np.pi)
            gts.append((c, bu.get_3d_box(dims, bu.rotz(yaw), ctr)))
            kind = rs.randint(0, 7)
            if kind == 0:                 # missed
                pass
            elif kind == 1:               # found twice
                add_pred(c, ctr, dims, yaw, 0.05); add_pred(c, ctr, dims, yaw, 0.08)
            elif kind == 2:               # found three times: a box contested by three predictions
                add_pred(c, ctr, dims, yaw, 0.04); add_pred(c, ctr, dims, yaw, 0.06); add_pred(c, ctr, dims, yaw, 0.08)
            elif kind == 3:               # found, under another class
                add_pred((c + 1 + int(rs.randint(0, 6))) % 7, ctr, dims, yaw, 0.05)
            elif kind == 4 and len(gts) < n_gt:      # a second box of the class nearly on top: two candidates for one prediction
                gts.append((c, bu.get_3d_box(dims * 0.8, bu.rotz(yaw + 0.05), ctr + [0.05, -0.04, 0.0])))
                add_pred(c, ctr, dims, yaw, 0.03)
            else:                         # found, well or badly
                add_pred(c, ctr, dims, yaw, [0.05, 0.15, 0.3][int(rs.randint(0, 3))])
        for _ in range(max(int(rs.randint(0, 4)), 2 if n_gt == 0 else 0)):      # spurious
            add_pred(int(rs.randint(0, 7)), rs.uniform(-4, 4, 3) * [1, 1, 0.2], rs.uniform(0.4, 1.8, 3), rs.uniform(-np.pi, np.pi), 0.0)
        if s == 3:
            preds = []
        gts = gts[:n_gt]
        preds = [preds[k] for k in rs.permutation(len(preds))]
        images.append((gts, preds))
    return images


def import_reference():
    import refenv
    refenv.setup()
    import matplotlib
    matplotlib.use("Agg")
    for name in ("dom", "dom.libs"):
        sys.modules.setdefault(name, types.ModuleType(name))
    helper = types.ModuleType("dom.libs.o3d_helper")
    helper.load_scene_mesh = helper.lineset_from_pc = None      # imported by name, never called here
    sys.modules.setdefault("dom.libs.o3d_helper", helper)
    import src.utils.eval_utils as eu
    import src.utils.box_utils as bu
    return eu, bu


def main():
    eu, bu = import_reference()
    images = make_images(bu)
    n_image = len(images)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g, _ in images])]).astype(np.int32)
    pred_off = np.concatenate([[0], np.cumsum([len(p) for _, p in images])]).astype(np.int32)
    n_gt, n_pred = int(gt_off[-1]), int(pred_off[-1])
    gt_cls = np.asarray([c for g, _ in images for c, _ in g], np.int32)
    pred_cls = np.asarray([c for _, p in images for c, _, _ in p], np.int32)
    pred_score = np.asarray([s for _, p in images for _, _, s in p], np.float64)
    pred_img = np.repeat(np.arange(n_image), np.diff(pred_off))
    npos = np.bincount(gt_cls, minlength=8).astype(np.int32); npred = np.bincount(pred_cls, minlength=8).astype(np.int32)
    cls_off = np.concatenate([[0], np.cumsum(npred)]).astype(np.int32)
    assert (npos > 0).all() and (npred > 0).all(), "eval_det needs every class on both sides"

    T = len(THRESHOLDS)
    rank = np.full(n_pred, -1, np.int32)
    ovmax = np.full(n_pred, np.nan); jmax = np.full(n_pred, -2, np.int32); second = np.full(n_pred, -np.inf)
    is_tp = np.zeros((T, n_pred), np.int32)
    tp = np.zeros((T, n_pred), np.int32); fp = np.zeros((T, n_pred), np.int32)
    rec = np.zeros((T, n_pred)); prec = np.zeros((T, n_pred)); ap = np.zeros((T, 2, 8))
    all_iou = []
    real_iou, real_cumsum = bu.iou_3d, np.cumsum
    for c in range(8):
        # the reference's per-class dicts, as eval_det builds them (:198-217); img ids are the image numbers
        pred_c, gt_c, idx_c, gidx_c = {}, {}, [], {}
        for s, (gts, preds) in enumerate(images):
            for p, (pc, box, score) in enumerate(preds):
                if pc == c:
                    pred_c.setdefault(s, []).append((box, score)); gt_c.setdefault(s, [])
                    idx_c.append(int(pred_off[s]) + p)
        for s, (gts, preds) in enumerate(images):
            for j, (gc, box) in enumerate(gts):
                if gc == c:
                    gt_c.setdefault(s, []).append(box); gidx_c.setdefault(s, []).append(j)
        idx_c = np.asarray(idx_c)
        order = idx_c[np.argsort(-pred_score[idx_c])]      # eval_det_cls:126 on the same confidences in the same order
        rank[order] = np.arange(len(order))
        for t, thr in enumerate(THRESHOLDS):
            for m, use07 in enumerate((False, True)):
                ious, sums = [], []
                bu.iou_3d = lambda a, b: (ious.append(real_iou(a, b)), ious[-1])[1]
                np.cumsum = lambda x, *a, **k: (sums.append(np.array(x)), real_cumsum(x, *a, **k))[1]
                try:
                    r, p, a = eu.eval_det_cls(pred_c, gt_c, thr, use07)
                finally:
                    bu.iou_3d, np.cumsum = real_iou, real_cumsum
                fp_flags, tp_flags = sums      # :167-168
                assert len(r) == len(order) and np.array_equal(tp_flags + fp_flags, np.ones(len(order)))
                o = int(cls_off[c])
                ap[t, m, c] = a
                if m == 0:
                    is_tp[t, order] = tp_flags.astype(np.int32)
                    tp[t, o:o + len(order)] = np.cumsum(tp_flags); fp[t, o:o + len(order)] = np.cumsum(fp_flags)
                    rec[t, o:o + len(order)] = r; prec[t, o:o + len(order)] = p
                else:
                    assert np.array_equal(rec[t, o:o + len(order)], r) and np.array_equal(prec[t, o:o + len(order)], p)
                if t == 0 and m == 0:      # fold the IoUs the reference evaluated, in its order, by its own rule
                    k = 0
                    for d in order:
                        s = int(pred_img[d])
                        ov, jm, sec = -np.inf, -1, -np.inf
                        for j in gidx_c.get(s, []):
                            v = ious[k]; k += 1
                            all_iou.append(v)
                            if v > ov:
                                sec = ov; ov = v; jm = j
                            elif v > sec:
                                sec = v
                        ovmax[d], jmax[d], second[d] = ov, jm, sec
                    assert k == len(ious)
    # eval_det itself on the classes it can print (class 3 has no name there): the same three dicts
    pred_all = {s: [(c, b, sc) for c, b, sc in preds if c != 3] for s, (gts, preds) in enumerate(images)}
    gt_all = {s: [(c, b) for c, b in gts if c != 3] for s, (gts, preds) in enumerate(images)}
    for t, thr in enumerate(THRESHOLDS):
        for m, use07 in enumerate((False, True)):
            with contextlib.redirect_stdout(io.StringIO()):
                r, p, a = eu.eval_det(pred_all, gt_all, thr, use07)
            assert sorted(a) == [0, 1, 2, 4, 5, 6, 7]
            for c in a:
                o, n = int(cls_off[c]), int(npred[c])
                assert a[c] == ap[t, m, c] and np.array_equal(r[c], rec[t, o:o + n]) and np.array_equal(p[c], prec[t, o:o + n])
    # what the fixture must contain
    n_g, n_p = np.diff(gt_off), np.diff(pred_off)
    assert ((n_g == 0) & (n_p > 0)).any(), "an image without ground truth"
    assert ((n_p == 0) & (n_g > 0)).any(), "an image without predictions"
    assert n_g.max() <= 15 and (npred == 1).any(), "a class with a single prediction"
    for c in range(8):
        sc = pred_score[pred_cls == c]
        assert len(np.unique(sc)) == len(sc), "two equal scores in a class"
    all_iou = np.asarray(all_iou)
    assert ((all_iou >= 0) & (all_iou <= 1)).all()
    for t, thr in enumerate(THRESHOLDS):
        reach = (ovmax > thr) & (jmax >= 0)
        key = pred_img[reach].astype(np.int64) * 100 + jmax[reach]
        contested = np.bincount(np.unique(key, return_inverse=True)[1])
        assert contested.max() >= 3, "a box contested by three predictions"
        assert np.abs(all_iou - thr).min() > MARGIN
        assert is_tp[t].sum() < reach.sum(), "a duplicate that is a false positive"
        print("threshold %.2f: %d true positives of %d predictions, %d reach a box, most contested box %d; AP %s | 11-point %s"
              % (thr, is_tp[t].sum(), n_pred, reach.sum(), contested.max(), np.round(ap[t, 0], 3), np.round(ap[t, 1], 3)))
    two = second > -np.inf
    assert two.any() and (ovmax[two] - second[two] > MARGIN)[ovmax[two] > 0].all(), "two candidates within the margin of a maximum"
    assert (second[two][ovmax[two] > 0] > 0).any(), "a prediction with two overlapping candidates"
    # (where ovmax is 0 every candidate is an exact 0 -- no intersection -- in any rounding: the first wins here and there)
    np.savez_compressed(os.path.join(HERE, "eval_ap.npz"),
                        gt_boxes=np.asarray([b for g, _ in images for _, b in g]).reshape(-1, 8, 3), gt_cls=gt_cls, gt_off=gt_off,
                        pred_boxes=np.asarray([b for _, p in images for _, b, _ in p]).reshape(-1, 8, 3), pred_cls=pred_cls,
                        pred_score=pred_score, pred_off=pred_off, thresholds=np.asarray(THRESHOLDS), npos=npos, npred=npred,
                        cls_off=cls_off, rank=rank, ovmax=ovmax, jmax=jmax, is_tp=is_tp, tp=tp, fp=fp, rec=rec, prec=prec, ap=ap,
                        ap11_thresholds=np.arange(0., 1.1, 0.1), eval_det_classes=np.asarray([0, 1, 2, 4, 5, 6, 7], np.int32))
    print("ap golden: %d images, %d ground-truth boxes, %d predictions, %d IoUs evaluated" % (n_image, n_gt, n_pred, len(all_iou)))


if __name__ == "__main__":
    main()
