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
