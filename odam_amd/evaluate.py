"""Evaluation of a finished map: which predicted boxes are found among the ground-truth boxes, at what 3D IoU.

Keeps the behaviour of the reference's src/scripts/eval_scan2cad.py (likojack/ODAM): `load_prediction_ours` (:191-215) reads the
dict `optim_process` returns, `match_sequence` (:249-267) matches predictions to ground truth by `box_utils.box3d_iou`, `get_f1`
(:270-295) turns the counts into precision / recall / F1 per class.  The IoU of every pair of every scene is ONE launch
(odam_box3d_iou_batch) and the matching of every scene a second (odam_box3d_match_batch): include/odam_eval.h, csrc/box_iou.hip.
With another run's map in place of the ground truth the same computation compares two runs (`compare_maps`).

Classes are the detector's integer ids 0..7 (eval_scan2cad.py:36-45 maps them onto the eight CARE_CLASSES, in this order).
Parsing Scan2CAD annotation files is not here: ground truth arrives as corner arrays [k, 8, 3] and class ids [k].

One difference of argument order: the reference calls box3d_iou(gt, prediction); the launches take the predictions as box 1 (rows) and
the ground truth as box 2 (columns).  The two orders differ by rounding, and for a box whose top face winds clockwise: such a
ground-truth box matches nothing here, such a prediction matches nothing in the reference.  Boxes of `get_3d_box` and
`compute_oriented_bbox` wind the same way.
"""
import ctypes

import numpy as np
import torch

from . import _lib

N_CLASS = 8            # eval_scan2cad.py:25-45
MAX_GT = 4096          # ground-truth boxes per scene (the matching kernel's flag bits)

_VP, _CI, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
EVAL_ARGTYPES = {
    "odam_box3d_iou_batch": [_VP, _CI, _VP, _VP, _VP, _LL, _VP, _VP, _VP, _VP, _CI, _VP, _VP, _VP],
    "odam_box3d_match_batch": [_VP, _CI, _VP, _VP, _VP, _VP, _VP, _VP, ctypes.c_double, _CI, _CI, _VP, _VP, _VP, _VP],
    "odam_det_ap": [_VP, _CI, _CI, _CI, _CI, _CI, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _LL, ctypes.c_double, _CI, _VP,
                    _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
}


def _entry(name):
    f = getattr(_lib.lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = EVAL_ARGTYPES[name], ctypes.c_int
    return f


def _default_fitter(fitter):
    if fitter is not None:
        return fitter
    from . import multi_view
    return multi_view.default_fitter()


def _boxes(x, dev):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=torch.float64)
    return t.reshape(-1, 8, 3).contiguous()


def _classes(x, dev):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=dev, dtype=torch.int32)
    return t.reshape(-1).contiguous()


def _cat(parts, empty_shape, dtype, dev):
    return torch.cat(parts) if parts else torch.empty(empty_shape, device=dev, dtype=dtype)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    if off[-1] >= 2 ** 31:
        raise _lib.OdamError(f"{off[-1]} boxes in one call: the offsets are 32-bit")
    return off


def _iou_launch(boxes_a, boxes_b, cls_a, cls_b, gate, fitter, want_bev):
    """iou_scenes, plus "_dev": the device offsets, classes and the unsliced IoU buffer, which match_scenes hands to its second launch"""
    fitter = _default_fitter(fitter)
    dev = fitter.device
    if len(boxes_a) != len(boxes_b):
        raise ValueError("one entry per scene in both lists")
    if gate not in (0, 1, 2):
        raise ValueError(f"gate must be 0, 1 or 2, got {gate}")
    if gate and (cls_a is None or cls_b is None):
        raise ValueError("gate != 0 needs the classes of both sides")
    A = [_boxes(x, dev) for x in boxes_a]; B = [_boxes(x, dev) for x in boxes_b]
    a_off = _offsets([len(x) for x in A]); b_off = _offsets([len(x) for x in B])
    pair_off = np.zeros(len(A) + 1, np.int64)
    pair_off[1:] = np.cumsum(np.diff(a_off) * np.diff(b_off))
    n_scene, n_pairs = len(A), int(pair_off[-1])
    d_A = _cat(A, (0, 8, 3), torch.float64, dev); d_B = _cat(B, (0, 8, 3), torch.float64, dev)
    d_ca = d_cb = None
    if cls_a is not None and cls_b is not None:
        d_ca = _cat([_classes(x, dev) for x in cls_a], (0,), torch.int32, dev)
        d_cb = _cat([_classes(x, dev) for x in cls_b], (0,), torch.int32, dev)
        if d_ca.shape[0] != a_off[-1] or d_cb.shape[0] != b_off[-1]:
            raise ValueError("one class per box")
    iou3d = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.float64)      # (never a null pointer: one spare word when empty)
    bev = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.float64) if want_bev else None
    d_aoff = torch.from_numpy(a_off.astype(np.int32)).to(dev); d_boff = torch.from_numpy(b_off.astype(np.int32)).to(dev)
    d_poff = torch.from_numpy(pair_off).to(dev)
    if n_pairs:
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_entry("odam_box3d_iou_batch")(
                fitter._h, n_scene, _lib.ptr(d_aoff), _lib.ptr(d_boff), _lib.ptr(d_poff), n_pairs, _lib.ptr(d_A), _lib.ptr(d_B),
                _lib.ptr(d_ca), _lib.ptr(d_cb), int(gate), _lib.ptr(iou3d), _lib.ptr(bev), ctypes.c_void_p(stream)),
                "odam_box3d_iou_batch")
    return {"iou3d": iou3d[:n_pairs], "iou_bev": None if bev is None else bev[:n_pairs], "a_off": a_off, "b_off": b_off,
            "pair_off": pair_off, "_dev": (d_aoff, d_boff, d_poff, d_ca, d_cb, iou3d)}


def iou_scenes(boxes_a, boxes_b, cls_a=None, cls_b=None, gate=0, fitter=None, want_bev=True):
    """3D IoU (and bird's-eye IoU) of every pair inside every scene, ONE launch.  boxes_a / boxes_b: lists, one [k, 8, 3] array per
    scene (numpy or torch); cls_a / cls_b: lists of [k] class ids, needed when gate != 0 (1 = equal class only, 2 = the merge rule).
    Returns device tensors "iou3d" / "iou_bev" [n_pairs] (scene s row-major [n_s][m_s] from pair_off[s]) and the host offsets
    "a_off", "b_off", "pair_off"."""
    r = _iou_launch(boxes_a, boxes_b, cls_a, cls_b, gate, fitter, want_bev)
    del r["_dev"]
    return r


def box3d_iou_matrix(A, B, cls_a=None, cls_b=None, gate=0, fitter=None):
    """One scene: the IoU of every box of A [n, 8, 3] (the clipped box, box_utils.box3d_iou's corners1) with every box of B
    [m, 8, 3] (the clipper).  Returns device tensors {"iou3d": [n, m], "iou_bev": [n, m]}, float64."""
    r = iou_scenes([A], [B], None if cls_a is None else [cls_a], None if cls_b is None else [cls_b], gate, fitter)
    n, m = int(r["a_off"][1]), int(r["b_off"][1])
    return {"iou3d": r["iou3d"].reshape(n, m), "iou_bev": r["iou_bev"].reshape(n, m)}


def match_scenes(preds, gts, threshold=0.25, fitter=None, n_class=N_CLASS):
    """match_sequence (eval_scan2cad.py:249-267) for many scenes in two launches.  preds / gts: lists, one entry per scene, each
    (boxes [k, 8, 3], classes [k], ...).  Predictions are tried in their given order; a prediction claims EVERY free ground-truth box
    of its class whose IoU is above the threshold (the reference has no `break`), and every claim is a true positive.

    Returns device tensors: counts [n_scene, 3, n_class] int32 (ground truth, predictions, true positives per class), claimed
    [sumN] (boxes each prediction claimed), gt_match [sumM] (index inside the scene of the claiming prediction, else -1), iou3d
    [n_pairs]; "iou" is the list of per-scene [n_s, m_s] views of it; pred_off / gt_off / pair_off are host arrays."""
    fitter = _default_fitter(fitter)
    dev = fitter.device
    if len(preds) != len(gts):
        raise ValueError("one entry per scene in both lists")
    n_scene = len(preds)
    max_gt = max([len(g[1]) for g in gts], default=0)
    if max_gt > MAX_GT:      # before any launch; the entry point answers the same (ODAM_E_LIMIT)
        raise _lib.OdamError(f"match_scenes: {max_gt} ground-truth boxes in a scene, more than {MAX_GT} (ODAM_E_LIMIT)")
    r = _iou_launch([p[0] for p in preds], [g[0] for g in gts], [p[1] for p in preds], [g[1] for g in gts], 1, fitter, False)
    d_aoff, d_boff, d_poff, d_cp, d_cg, iou_buf = r["_dev"]
    sum_n, sum_m = int(r["a_off"][-1]), int(r["b_off"][-1])
    counts = torch.empty(max(n_scene, 1), 3, n_class, device=dev, dtype=torch.int32)
    claimed = torch.empty(max(sum_n, 1), device=dev, dtype=torch.int32)
    gt_match = torch.empty(max(sum_m, 1), device=dev, dtype=torch.int32)
    pad = lambda t: t if t.shape[0] else torch.zeros(1, device=dev, dtype=torch.int32)
    d_cp, d_cg = pad(d_cp), pad(d_cg)
    if n_scene:
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_entry("odam_box3d_match_batch")(
                fitter._h, n_scene, _lib.ptr(d_aoff), _lib.ptr(d_boff), _lib.ptr(d_poff), _lib.ptr(iou_buf), _lib.ptr(d_cp),
                _lib.ptr(d_cg), float(threshold), int(n_class), max_gt, _lib.ptr(counts), _lib.ptr(claimed), _lib.ptr(gt_match),
                ctypes.c_void_p(stream)), "odam_box3d_match_batch")
    po, ao, bo = r["pair_off"], r["a_off"], r["b_off"]
    iou = [r["iou3d"][po[s]:po[s + 1]].reshape(int(ao[s + 1] - ao[s]), int(bo[s + 1] - bo[s])) for s in range(n_scene)]
    return {"counts": counts[:n_scene], "claimed": claimed[:sum_n], "gt_match": gt_match[:sum_m], "iou3d": r["iou3d"], "iou": iou,
            "pred_off": ao, "gt_off": bo, "pair_off": po}


def predictions_from_result(out, min_views=1):
    """What load_prediction_ours (eval_scan2cad.py:203-214) does with a result dict of optim_process / refine / merge: objects whose
    track has fewer than min_views rows are dropped, class = int(median(track[:, 1])), box = bboxes_qc[obj].  An object whose class
    is not one of the eight is dropped (the reference's DETECTOR_CLASS_MAPPER would raise).
    Returns (boxes [k, 8, 3] float64, classes [k] int32, object ids [k])."""
    boxes, classes, ids = [], [], []
    for obj_id, track in enumerate(out["tracks"]):
        if len(track) < min_views:
            continue
        c = int(np.median(np.asarray(track)[:, 1]))
        if not 0 <= c < N_CLASS:
            continue
        boxes.append(np.asarray(out["bboxes_qc"][obj_id], np.float64).reshape(8, 3)); classes.append(c); ids.append(obj_id)
    return (np.asarray(boxes, np.float64).reshape(-1, 8, 3), np.asarray(classes, np.int32), np.asarray(ids, np.int64))


def _ratio(a, b):
    return a / b if b != 0 else 0


def f1_table(counts):
    """get_f1 (eval_scan2cad.py:270-295) on counts [..., 3, n_class] (ground truth, predictions, true positives; leading axes are
    summed).  Per class precision ("accuracy" there) and recall are 0 when the class has no ground truth, F1 is 0 when both are 0; the
    averages come from the summed counts.  One deviation: where the reference would raise ZeroDivisionError (a class with ground
    truth and no prediction, empty totals) the value is 0.
    Returns {"precision", "recall", "f1": [n_class] float64, "avg_precision", "avg_recall", "avg_f1", "gts", "preds", "tps"}."""
    c = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, np.int64)
    c = c.reshape(-1, 3, c.shape[-1]).sum(axis=0)
    n_class = c.shape[-1]
    prec, rec, f1 = np.zeros(n_class), np.zeros(n_class), np.zeros(n_class)
    for k in range(n_class):
        g, p, t = (int(x) for x in c[:, k])
        prec[k] = 0 if g == 0 else _ratio(t, p)
        rec[k] = 0 if g == 0 else t / g
        f1[k] = 2 * prec[k] * rec[k] / (prec[k] + rec[k]) if prec[k] + rec[k] != 0 else 0
    G, P, T = (int(x) for x in c.sum(axis=1))
    ap, ar = _ratio(T, P), _ratio(T, G)
    return {"precision": prec, "recall": rec, "f1": f1, "avg_precision": ap, "avg_recall": ar,
            "avg_f1": _ratio(2 * ap * ar, ap + ar), "gts": c[0], "preds": c[1], "tps": c[2]}


def evaluate(results, gts, threshold=0.25, min_views=1, fitter=None):
    """The three steps over many scenes: results = list of result dicts (optim_process's output), gts = list of (boxes [k, 8, 3],
    classes [k]).  Returns f1_table's dict plus "counts" [n_scene, 3, 8], and per scene "claimed", "gt_match", "iou" (numpy) and
    "pred_ids" (the object ids of the predictions that were kept)."""
    preds = [predictions_from_result(r, min_views) for r in results]
    m = match_scenes(preds, gts, threshold, fitter)
    counts = m["counts"].cpu().numpy()
    claimed = m["claimed"].cpu().numpy(); gt_match = m["gt_match"].cpu().numpy()
    ao, bo = m["pred_off"], m["gt_off"]
    out = f1_table(counts)
    out.update(counts=counts, threshold=threshold,
               claimed=[claimed[ao[s]:ao[s + 1]] for s in range(len(preds))],
               gt_match=[gt_match[bo[s]:bo[s + 1]] for s in range(len(preds))],
               iou=[x.cpu().numpy() for x in m["iou"]], pred_ids=[p[2] for p in preds])
    return out


def compare_maps(out_a, out_b, threshold=0.25, min_views=1, fitter=None):
    """Map A against map B as the ground truth (two result dicts of the same scene, e.g. the fp32 and the bf16 run): evaluate()'s
    dict for the one scene, plus "matched" [k, 2] (object id in A, object id in B) and "matched_iou" [k], the IoU of every pair the
    matching made, in B's order."""
    gt = predictions_from_result(out_b, min_views)
    out = evaluate([out_a], [gt], threshold, min_views, fitter)
    gm, iou, ids_a = out["gt_match"][0], out["iou"][0], out["pred_ids"][0]
    hit = np.nonzero(gm >= 0)[0]
    out["matched"] = np.stack([ids_a[gm[hit]], gt[2][hit]], axis=1) if len(hit) else np.zeros((0, 2), np.int64)
    out["matched_iou"] = iou[gm[hit], hit] if len(hit) else np.zeros(0)
    out["gt_ids"] = gt[2]
    return out


# ---- average precision: the reference's src/utils/eval_utils.py eval_det / eval_det_cls / voc_ap ------------------------------------
# Score-ranked precision / recall curves and AP per class, every class and every image (scene or frame) in one call of six launches
# (odam_det_ap: include/odam_eval.h, csrc/det_ap.hip).  Where this departs from the reference, and why, is in DESIGN 6k:
#   - equal scores keep their input order and a NaN score ranks last (np.argsort leaves ties open);
#   - a class with ground truth and no prediction has AP 0 and empty curves (the reference raises KeyError);
#   - a class with predictions and no ground truth has AP NaN in both forms and is left out of the mean;
#   - a class id outside 0 .. n_class-1 is counted nowhere; its per-prediction words are NaN / -1.
MAX_AP_PRED = 32768    # prediction slots per call (ODAM_AP_MAX_PRED: the ranking counts pairs)
ROW_SLOTS = 30         # detection rows per frame of a packed block (ODAM_AP_ROW_SLOTS)
_AP_KINDS = {"aabb": 0, "obb": 1, "aabb3d": 2, "box2d": 3}
_AP_OUT = (("ovmax", "p", torch.float64), ("jmax", "p", torch.int32), ("rank", "p", torch.int32), ("is_tp", "p", torch.int32),
           ("gt_claim", "g", torch.int32), ("order", "p", torch.int32), ("npos", "c", torch.int32), ("npred", "c", torch.int32),
           ("cls_off", "c1", torch.int32), ("ap", "c", torch.float64), ("tp", "p", torch.int32), ("fp", "p", torch.int32),
           ("rec", "p", torch.float64), ("prec", "p", torch.float64))


def _ap_launch(kind, n_image, n_pred, n_gt, n_class, d_poff, d_goff, pred_box, gt_box, cls_p, cls_g, score, d_pair_off, iou, n_pairs,
               ovthresh, use_07_metric, fitter, dev):
    """odam_det_ap on device inputs -> its fourteen outputs as device tensors (the ragged ones are [n_pred] long; class c owns the
    words cls_off[c] .. cls_off[c+1]-1, the rest is not written)"""
    if n_pred > MAX_AP_PRED:      # before any launch; the entry point answers the same (ODAM_E_LIMIT)
        raise _lib.OdamError(f"average precision: {n_pred} prediction slots in one call, more than {MAX_AP_PRED} (ODAM_E_LIMIT)")
    size = {"p": max(n_pred, 1), "g": max(n_gt, 1), "c": n_class, "c1": n_class + 1}
    out = {name: torch.empty(size[s], device=dev, dtype=dt) for name, s, dt in _AP_OUT}
    scratch = torch.empty(max(2 * n_pred + 2 * n_gt, 1), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_entry("odam_det_ap")(
            fitter._h, int(kind), int(n_image), int(n_pred), int(n_gt), int(n_class), _lib.ptr(d_poff), _lib.ptr(d_goff),
            _lib.ptr(pred_box), _lib.ptr(gt_box), _lib.ptr(cls_p), _lib.ptr(cls_g), _lib.ptr(score), _lib.ptr(d_pair_off),
            _lib.ptr(iou), int(n_pairs), float(ovthresh), int(bool(use_07_metric)), _lib.ptr(scratch),
            *[_lib.ptr(out[name]) for name, _, _ in _AP_OUT], ctypes.c_void_p(stream)), "odam_det_ap")
    keep = {"p": n_pred, "g": n_gt, "c": n_class, "c1": n_class + 1}
    return {name: out[name][:keep[s]] for name, s, _ in _AP_OUT}


def average_precision(preds, gts, ovthresh=0.25, use_07_metric=False, iou="aabb", fitter=None, n_class=N_CLASS):
    """eval_det_cls (eval_utils.py:86-176) for every class over many images at once.  preds: list, one entry per image, of
    (boxes [k, 8, 3], classes [k], scores [k]); gts: list of (boxes [k, 8, 3], classes [k]).  iou = "aabb": the axis-aligned boxes
    of the corners, which is what the reference computes whatever get_iou_func says; "obb": the oriented-box IoU its default
    argument names (odam_box3d_iou_batch, gate 1, one more launch).

    Returns device tensors -- per prediction "ovmax", "jmax" (index among all ground truth of its image), "rank" (inside its class),
    "is_tp"; per ground-truth box "gt_claim" (the true positive on it, an index into the concatenated predictions, or -1); per class
    "npos", "npred", "ap", "cls_off" and, in rank order from cls_off[c], "order", "tp", "fp", "rec", "prec" -- and the host offsets
    "pred_off", "gt_off"."""
    fitter = _default_fitter(fitter)
    dev = fitter.device
    if len(preds) != len(gts):
        raise ValueError("one entry per image in both lists")
    if iou not in ("aabb", "obb"):
        raise ValueError(f'iou must be "aabb" or "obb", got {iou!r}')
    pad = lambda t, dt: t if t.shape[0] else torch.zeros(1, device=dev, dtype=dt)
    sc = _cat([torch.as_tensor(np.asarray(p[2]) if not torch.is_tensor(p[2]) else p[2]).to(device=dev, dtype=torch.float64).reshape(-1)
               for p in preds], (0,), torch.float64, dev)
    if iou == "obb":
        r = _iou_launch([p[0] for p in preds], [g[0] for g in gts], [p[1] for p in preds], [g[1] for g in gts], 1, fitter, False)
        d_poff, d_goff, d_pair, d_cp, d_cg, iou_buf = r["_dev"]
        po, go, n_pairs, A, B = r["a_off"], r["b_off"], int(r["pair_off"][-1]), None, None
    else:
        A = [_boxes(p[0], dev) for p in preds]; B = [_boxes(g[0], dev) for g in gts]
        po = _offsets([len(x) for x in A]); go = _offsets([len(x) for x in B])
        d_cp = _cat([_classes(p[1], dev) for p in preds], (0,), torch.int32, dev)
        d_cg = _cat([_classes(g[1], dev) for g in gts], (0,), torch.int32, dev)
        A = pad(_cat(A, (0, 8, 3), torch.float64, dev), torch.float64); B = pad(_cat(B, (0, 8, 3), torch.float64, dev), torch.float64)
        d_poff = torch.from_numpy(po.astype(np.int32)).to(dev); d_goff = torch.from_numpy(go.astype(np.int32)).to(dev)
        d_pair = iou_buf = None
        n_pairs = 0
    n_pred, n_gt = int(po[-1]), int(go[-1])
    if d_cp.shape[0] != n_pred or d_cg.shape[0] != n_gt or sc.shape[0] != n_pred:
        raise ValueError("one class per box and one score per prediction")
    out = _ap_launch(_AP_KINDS[iou], len(preds), n_pred, n_gt, n_class, d_poff, d_goff, A, B, pad(d_cp, torch.int32),
                     pad(d_cg, torch.int32), pad(sc, torch.float64), d_pair, iou_buf, n_pairs, ovthresh, use_07_metric, fitter, dev)
    out.update(pred_off=po, gt_off=go)
    return out


def ap_table(r):
    """The host summary of average_precision's / detections_ap's device tensors: {"ap": [n_class] (NaN where the class has no ground
    truth), "mAP": the mean over the classes with ground truth (NaN when there is none), "npos", "npred"}."""
    ap = r["ap"].cpu().numpy(); npos = r["npos"].cpu().numpy(); npred = r["npred"].cpu().numpy()
    have = npos > 0
    return {"ap": ap, "mAP": float(ap[have].mean()) if have.any() else float("nan"), "npos": npos, "npred": npred}


def eval_det(pred_all, gt_all, ovthresh=0.25, use_07_metric=False, iou="aabb", fitter=None):
    """The reference's eval_det (eval_utils.py:185-235) without its prints and plots: pred_all {img_id: [(class, box [8, 3], score)]},
    gt_all {img_id: [(class, box [8, 3])]} -> (rec, prec, ap), dicts keyed by class, rec / prec numpy arrays in rank order.  Classes
    are any hashable names (at most 64).  A class with ground truth and no prediction has AP 0 and empty curves (the reference
    raises KeyError); one with predictions and no ground truth has AP NaN."""
    names, imgs = [], list(pred_all.keys()) + [k for k in gt_all.keys() if k not in pred_all]
    for src in (pred_all, gt_all):      # the order in which the reference's `gt` dict meets the classes (:200-217)
        for img in src.keys():
            for item in src[img]:
                if item[0] not in names:
                    names.append(item[0])
    if len(names) > 64:
        raise ValueError(f"{len(names)} classes, more than 64")
    if not names:
        return {}, {}, {}
    cid = {n: i for i, n in enumerate(names)}
    preds = [(np.asarray([b for _, b, _ in pred_all.get(i, [])], np.float64).reshape(-1, 8, 3),
              np.asarray([cid[c] for c, _, _ in pred_all.get(i, [])], np.int32),
              np.asarray([s for _, _, s in pred_all.get(i, [])], np.float64)) for i in imgs]
    gts = [(np.asarray([b for _, b in gt_all.get(i, [])], np.float64).reshape(-1, 8, 3),
            np.asarray([cid[c] for c, _ in gt_all.get(i, [])], np.int32)) for i in imgs]
    r = average_precision(preds, gts, ovthresh, use_07_metric, iou, fitter, n_class=len(names))
    off = r["cls_off"].cpu().numpy(); rec = r["rec"].cpu().numpy(); prec = r["prec"].cpu().numpy(); ap = r["ap"].cpu().numpy()
    return ({n: rec[off[i]:off[i + 1]] for i, n in enumerate(names)}, {n: prec[off[i]:off[i + 1]] for i, n in enumerate(names)},
            {n: float(ap[i]) for i, n in enumerate(names)})


def prediction_scores(out, min_views=1):
    """A confidence for every object predictions_from_result keeps, in its order: the mean of the scores of the object's detections
    (track column 13).  The reference defines no score for a fitted object; this definition is the project's own."""
    boxes, classes, ids = predictions_from_result(out, min_views)
    return np.asarray([float(np.mean(np.asarray(out["tracks"][i], np.float64)[:, 13])) for i in ids], np.float64)


def evaluate_ap(results, gts, ovthresh=0.25, use_07_metric=False, iou="aabb", min_views=1, fitter=None):
    """average_precision over many scenes: results = list of result dicts (optim_process's output), scored by prediction_scores;
    gts = list of (boxes [k, 8, 3], classes [k]).  Returns ap_table's dict plus, per scene, "is_tp", "ovmax", "gt_claim" (index inside
    the scene's kept predictions, or -1) and "pred_ids", and per class "rec" / "prec" (lists of numpy arrays in rank order)."""
    preds = [predictions_from_result(r, min_views)[:2] + (prediction_scores(r, min_views),) for r in results]
    ids = [predictions_from_result(r, min_views)[2] for r in results]
    r = average_precision(preds, [g[:2] for g in gts], ovthresh, use_07_metric, iou, fitter)
    out = ap_table(r)
    po, go = r["pred_off"], r["gt_off"]
    is_tp, ovmax, claim = r["is_tp"].cpu().numpy(), r["ovmax"].cpu().numpy(), r["gt_claim"].cpu().numpy()
    off, rec, prec = r["cls_off"].cpu().numpy(), r["rec"].cpu().numpy(), r["prec"].cpu().numpy()
    n = len(preds)
    out.update(ovthresh=ovthresh, pred_ids=ids, is_tp=[is_tp[po[s]:po[s + 1]] for s in range(n)],
               ovmax=[ovmax[po[s]:po[s + 1]] for s in range(n)],
               gt_claim=[np.where(claim[go[s]:go[s + 1]] >= 0, claim[go[s]:go[s + 1]] - po[s], -1) for s in range(n)],
               rec=[rec[off[c]:off[c + 1]] for c in range(N_CLASS)], prec=[prec[off[c]:off[c + 1]] for c in range(N_CLASS)])
    return out


def compare_maps_ap(out_a, out_b, ovthresh=0.25, use_07_metric=False, iou="aabb", min_views=1, fitter=None):
    """Map A, ranked by prediction_scores, against map B as the ground truth (two result dicts of the same scene): evaluate_ap's dict
    for the one scene, plus "gt_ids", the object ids of B that were kept."""
    gt = predictions_from_result(out_b, min_views)
    out = evaluate_ap([out_a], [gt[:2]], ovthresh, use_07_metric, iou, min_views, fitter)
    out["gt_ids"] = gt[2]
    return out


def detections_ap(blk_pred, cnt_pred, blk_gt, cnt_gt, iou="aabb3d", ovthresh=0.25, use_07_metric=False, fitter=None, n_class=N_CLASS):
    """One detector run against another, frame by frame, without the detections leaving the device: two blocks of equal frame count
    as OdamProcess.detect_frames_packed returns them (float32 [F, 30, 15] and int32 [F] on the device), the second taken as the
    ground truth.  Images are frames; class = column 1, score = column 14; iou = "aabb3d": the box t_co -+ dims / 2 of DETR.nms_3d
    (columns 9-11, 6-8); "box2d": the image box (columns 2-5).  Slots past a frame's count are ignored, whatever they hold.
    Returns ap_table's dict (the only copy to the host) plus "device": the call's outputs as device tensors over the F * 30 slots."""
    fitter = _default_fitter(fitter)
    if iou not in ("aabb3d", "box2d"):
        raise ValueError(f'iou must be "aabb3d" or "box2d", got {iou!r}')
    for b, c in ((blk_pred, cnt_pred), (blk_gt, cnt_gt)):
        if not (torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and b.dim() == 3 and tuple(b.shape[1:]) == (ROW_SLOTS, 15)
                and b.is_contiguous() and torch.is_tensor(c) and c.is_cuda and c.dtype == torch.int32 and c.is_contiguous()
                and tuple(c.shape) == (b.shape[0],)):
            raise ValueError("detections_ap: contiguous device tensors float32 [F, 30, 15] and int32 [F]")
    if blk_pred.shape[0] != blk_gt.shape[0]:
        raise ValueError("detections_ap: two blocks of equal frame count")
    F = int(blk_pred.shape[0])
    dev = blk_pred.device
    one = torch.zeros(1, device=dev, dtype=torch.int32)
    one_f = torch.zeros(ROW_SLOTS * 15, device=dev, dtype=torch.float32)
    r = _ap_launch(_AP_KINDS[iou], F, F * ROW_SLOTS, F * ROW_SLOTS, n_class, cnt_pred if F else one, cnt_gt if F else one,
                   blk_pred if F else one_f, blk_gt if F else one_f, None, None, None, None, None, 0, ovthresh, use_07_metric, fitter, dev)
    out = ap_table(r)
    out["device"] = r
    return out
