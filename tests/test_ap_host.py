"""Average precision without a GPU: the numpy restatement of the kernels (tests/det_ap_ref.py) against the reference's own
eval_det_cls / voc_ap / eval_det run (tests/golden/eval_ap.npz, written by tests/golden/make_golden_ap.py), the host functions of
odam_amd/evaluate.py around a stand-in for the launches, the arithmetic header as a stand-alone host program, and the built library's
new entry point.

What is asked of the restatement on the fixture:
  ranks, tp / fp flags, prefix sums, jmax   integers: equal
  ovmax                                     1e-12, the bound the project holds its IoU forms to
  rec, prec                                 2^-52 relative: one division of exact integers
  AP                                        n 2^-52 with the class's n: every term is non-negative and the sum is at most 1, so two
                                            summation orders of n terms differ by at most that"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import det_ap_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52
IOU_TOL = 1e-12


def _fixture_args(z):
    return dict(n_image=len(z["pred_off"]) - 1, n_pred=len(z["pred_cls"]), n_gt=len(z["gt_cls"]), pred_off=z["pred_off"],
                gt_off=z["gt_off"], pred_box=z["pred_boxes"], gt_box=z["gt_boxes"], cls_pred=z["pred_cls"], cls_gt=z["gt_cls"],
                score=z["pred_score"])


_RESTATED = {}


def restated(z, t, use07):
    """the restatement on the fixture, computed once per (threshold, form) and shared"""
    if (t, use07) not in _RESTATED:
        _RESTATED[t, use07] = R.det_ap(0, n_class=8, ovthresh=float(z["thresholds"][t]), use_07_metric=use07, **_fixture_args(z))
    return _RESTATED[t, use07]


@pytest.mark.parametrize("use07", [False, True])
@pytest.mark.parametrize("t", [0, 1])
def test_restatement_equals_the_reference_run(golden, t, use07):
    z = golden("eval_ap.npz")
    r = restated(z, t, use07)
    assert np.array_equal(r["npos"], z["npos"]) and np.array_equal(r["npred"], z["npred"]) and np.array_equal(r["cls_off"], z["cls_off"])
    assert np.array_equal(np.asarray(r["rank"]), z["rank"]) and np.array_equal(np.asarray(r["jmax"]), z["jmax"])
    assert np.array_equal(np.asarray(r["is_tp"]), z["is_tp"][t])
    assert np.array_equal(r["tp"], z["tp"][t]) and np.array_equal(r["fp"], z["fp"][t])
    ov = np.asarray(r["ovmax"])
    fin = np.isfinite(z["ovmax"])
    assert np.array_equal(ov[~fin], z["ovmax"][~fin]) and np.abs(ov[fin] - z["ovmax"][fin]).max() <= IOU_TOL
    assert np.abs(r["rec"] - z["rec"][t]).max() <= U * np.abs(z["rec"][t]).max() and (np.abs(r["rec"] - z["rec"][t]) <= U * np.abs(z["rec"][t])).all()
    assert (np.abs(r["prec"] - z["prec"][t]) <= U * np.abs(z["prec"][t])).all()
    want = z["ap"][t, int(use07)]
    err = np.abs(r["ap"] - want)
    print("AP, restatement - reference, per class:", err)
    assert (err <= z["npred"] * U).all(), (err, z["npred"] * U)
    # the box a true positive sits on names it, and nobody else
    claim = np.asarray(r["gt_claim"])
    tps = np.nonzero(np.asarray(r["is_tp"]) == 1)[0]
    assert sorted(claim[claim >= 0].tolist()) == tps.tolist()
    img = np.repeat(np.arange(len(z["pred_off"]) - 1), np.diff(z["pred_off"]))
    for d in tps:
        assert claim[z["gt_off"][img[d]] + r["jmax"][d]] == d
    assert [R.ap11_threshold(i) for i in range(11)] == z["ap11_thresholds"].tolist()


def _as_lists(z):
    po, go = z["pred_off"], z["gt_off"]
    n = len(po) - 1
    preds = [(z["pred_boxes"][po[s]:po[s + 1]], z["pred_cls"][po[s]:po[s + 1]], z["pred_score"][po[s]:po[s + 1]]) for s in range(n)]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(n)]
    return preds, gts


def _stand_in(preds, gts, ovthresh=0.25, use_07_metric=False, iou="aabb", fitter=None, n_class=8):
    """evaluate.average_precision with the restatement in place of the launches: the same dict, tensors on the host"""
    import torch
    a = R.from_lists(preds, gts)
    r = R.det_ap(0, n_class=n_class, ovthresh=ovthresh, use_07_metric=use_07_metric, **a)
    out = {k: torch.from_numpy(np.asarray(r[k])) for k in ("npos", "npred", "cls_off", "ap", "order", "tp", "fp", "rec", "prec")}
    out.update(ovmax=torch.from_numpy(R.filled(r["ovmax"], np.nan, np.float64)), jmax=torch.from_numpy(R.filled(r["jmax"], -9, np.int32)),
               rank=torch.from_numpy(R.filled(r["rank"], -9, np.int32)), is_tp=torch.from_numpy(R.filled(r["is_tp"], -9, np.int32)),
               gt_claim=torch.from_numpy(R.filled(r["gt_claim"], -9, np.int32)), pred_off=a["pred_off"].astype(np.int64),
               gt_off=a["gt_off"].astype(np.int64))
    return out


def test_eval_det_takes_and_gives_the_references_dicts(golden, monkeypatch):
    from odam_amd import evaluate
    monkeypatch.setattr(evaluate, "average_precision", _stand_in)
    z = golden("eval_ap.npz")
    preds, gts = _as_lists(z)
    names = {c: "class%d" % c for c in range(8)}      # any hashable name
    ids = ["img%d" % s for s in range(len(preds))]
    pred_all = {i: [(names[int(c)], b, float(s)) for b, c, s in zip(*p)] for i, p in zip(ids, preds)}
    gt_all = {i: [(names[int(c)], b) for b, c in zip(*g)] for i, g in zip(ids, gts)}
    for t in (0, 1):
        for use07 in (False, True):
            rec, prec, ap = evaluate.eval_det(pred_all, gt_all, float(z["thresholds"][t]), use07)
            assert sorted(rec) == sorted(prec) == sorted(ap) == sorted(names.values())
            for c in range(8):
                o, n = int(z["cls_off"][c]), int(z["npred"][c])
                assert rec[names[c]].shape == (n,) and np.allclose(rec[names[c]], z["rec"][t, o:o + n], rtol=U, atol=0)
                assert np.allclose(prec[names[c]], z["prec"][t, o:o + n], rtol=U, atol=0)
                assert abs(ap[names[c]] - z["ap"][t, int(use07), c]) <= n * U
    # an image that only the ground truth knows, a class without predictions: AP 0 and empty curves where the reference raises
    gt_all["extra"] = [("unseen", z["gt_boxes"][0])]
    rec, prec, ap = evaluate.eval_det(pred_all, gt_all, 0.25)
    assert ap["unseen"] == 0.0 and rec["unseen"].shape == (0,) and prec["unseen"].shape == (0,)
    assert abs(ap["class0"] - z["ap"][0, 0, 0]) <= z["npred"][0] * U
    assert evaluate.eval_det({}, {}) == ({}, {}, {})


def test_deviations_from_the_reference():
    box = lambda ctr: np.asarray(ctr) + np.asarray([[x, y, z] for z in (0.5, -0.5) for x, y in ((1, 1), (1, -1), (-1, -1), (-1, 1))]) * 0.5
    gts = [(np.stack([box([0, 0, 0]), box([5, 0, 0]), box([9, 9, 9])]), [0, 1, 9])]      # class 0: box and predictions; 1: box only; 9: outside
    preds = [(np.stack([box([0.1, 0, 0]), box([0, 0.1, 0]), box([3, 3, 3]), box([0, 0, 0]), box([0, 0, 0])]), [0, 0, 2, -1, 8],
              [0.9, 0.8, 0.7, 0.95, 0.99])]                                                 # class 2: predictions only
    for use07 in (False, True):
        r = R.det_ap(0, n_class=8, ovthresh=0.25, use_07_metric=use07, **R.from_lists(preds, gts))
        assert r["npos"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and r["npred"].tolist() == [2, 0, 1, 0, 0, 0, 0, 0]
        assert r["ap"][1] == 0.0 and r["cls_off"][1] == r["cls_off"][2]                    # ground truth, no prediction: 0, empty curves
        o = r["cls_off"][2]
        assert np.isnan(r["ap"][2]) and np.isnan(r["rec"][o]) and r["prec"][o] == 0.0      # predictions, no ground truth
        assert r["tp"][o] == 0 and r["fp"][o] == 1 and r["ovmax"][2] == -np.inf and r["jmax"][2] == -1
        assert np.isnan(r["ap"][3:]).all()                                                 # neither
        assert abs(r["ap"][0] - 1.0) <= 11 * U and r["is_tp"][:2] == [1, 0] and r["gt_claim"] == [0, -1, -1]
        for d in (3, 4):                                                                   # ids -1 and 8: counted nowhere, NaN / -1
            assert np.isnan(r["ovmax"][d]) and (r["jmax"][d], r["rank"][d], r["is_tp"][d]) == (-1, -1, -1)
        assert r["rank"][:3] == [0, 1, 0]
    # the mean is over the classes with ground truth, on the host
    import torch
    from odam_amd import evaluate
    t = evaluate.ap_table({k: torch.from_numpy(np.asarray(r[k])) for k in ("ap", "npos", "npred")})
    assert abs(t["mAP"] - 0.5) <= 11 * U and np.isnan(t["ap"][2]) and t["npos"].tolist() == r["npos"].tolist()
    t = evaluate.ap_table({"ap": torch.full((8,), float("nan")), "npos": torch.zeros(8, dtype=torch.int32), "npred": torch.zeros(8, dtype=torch.int32)})
    assert np.isnan(t["mAP"])
    # equal scores keep their input order; a NaN score ranks after every number, two NaN by input order
    sc = [0.5, np.nan, 0.5, 0.7, np.nan, -np.inf]
    r = R.det_ap(0, n_class=1, **R.from_lists([(np.stack([box([i, 0, 0]) for i in range(6)]), [0] * 6, sc)], [(np.zeros((0, 8, 3)), [])]))
    assert r["rank"] == [1, 4, 2, 0, 5, 3] and r["order"].tolist() == [3, 0, 2, 5, 1, 4]


def test_prediction_scores_and_evaluate_ap(monkeypatch):
    from odam_amd import evaluate
    monkeypatch.setattr(evaluate, "average_precision", _stand_in)
    rs = np.random.RandomState(4)
    box = lambda ctr: np.asarray(ctr) + np.asarray([[x, y, z] for z in (0.5, -0.5) for x, y in ((1, 1), (1, -1), (-1, -1), (-1, 1))]) * 0.5

    def track(n, c, scores):
        t = np.zeros((n, 82)); t[:, 1] = c; t[:, 13] = scores
        return t
    tracks = [track(3, 0, [0.9, 0.8, 0.7]), track(1, 1, [0.6]), track(4, 11, [0.5] * 4), track(5, 0, rs.uniform(0.1, 0.2, 5))]
    out = {"tracks": tracks, "bboxes_qc": [box([0, 0, 0]), box([4, 0, 0]), box([8, 0, 0]), box([0.2, 0, 0])]}
    s = evaluate.prediction_scores(out)
    assert s.dtype == np.float64 and s.shape == (3,)                        # the object of class 11 is dropped, as predictions_from_result does
    assert s[0] == np.mean([0.9, 0.8, 0.7]) and s[1] == 0.6 and s[2] == np.mean(tracks[3][:, 13])
    assert evaluate.prediction_scores(out, min_views=3).shape == (2,)
    gt = (np.stack([box([0, 0, 0]), box([4.1, 0, 0])]), [0, 1])
    e = evaluate.evaluate_ap([out], [gt], 0.25)
    assert e["pred_ids"][0].tolist() == [0, 1, 3] and e["is_tp"][0].tolist() == [1, 1, 0] and e["gt_claim"][0].tolist() == [0, 1]
    assert e["ap"][0] == 1.0 and e["ap"][1] == 1.0 and e["mAP"] == 1.0 and e["npred"].tolist()[:2] == [2, 1]
    assert e["rec"][0].tolist() == [1.0, 1.0] and e["prec"][0].tolist() == [1.0, 0.5]
    c = evaluate.compare_maps_ap(out, out, 0.25)
    assert c["gt_ids"].tolist() == [0, 1, 3] and c["mAP"] == 1.0 and c["gt_claim"][0].tolist() == [0, 1, 2]


def _hex64(x):
    return " ".join("%016x" % v for v in np.asarray(x, np.float64).reshape(-1).view(np.uint64))


def _hex32(x):
    return " ".join("%08x" % v for v in np.asarray(x, np.float32).reshape(-1).view(np.uint32))


def write_cases(path, z):
    """the fixture's same-class pairs and the degenerate ones, with the restatement's answers (tests/native/det_ap_check.cpp)"""
    rs = np.random.RandomState(7)
    lines = []
    po, go = z["pred_off"], z["gt_off"]
    pairs = [(z["pred_boxes"][d], z["gt_boxes"][g]) for s in range(len(po) - 1) for d in range(po[s], po[s + 1])
             for g in range(go[s], go[s + 1]) if z["pred_cls"][d] == z["gt_cls"][g]]
    a0, b0 = pairs[0]
    flat = a0.copy(); flat[:, 2] = 0.0
    nan_a = a0.copy(); nan_a[3, 1] = np.nan
    pairs += [(a0, a0), (flat, flat), (flat, b0), (nan_a, b0), (b0, nan_a), (a0, a0 + 100.0), (np.zeros((8, 3)), np.zeros((8, 3)))]
    for a, b in pairs:
        lines.append("C %s %s %s" % (_hex64(a), _hex64(b), _hex64(R.iou_aabb_corners(a, b))))
    rows = rs.uniform(0.1, 1.0, (40, 15)).astype(np.float32)
    rows[:, 4:6] += rows[:, 2:4]
    rows[5] = rows[4]; rows[7, 6] = 0.0; rows[9, 9] = np.nan; rows[11, 4] = rows[11, 2]; rows[13, 2] = np.nan
    for a, b in zip(rows[:-1], rows[1:]):
        i3 = R.iou_3d(*R.aabb_of_row(a), *R.aabb_of_row(b))
        lines.append("R %s %s %s %s" % (_hex32(a), _hex32(b), _hex64(i3), _hex64(R.iou_2d_rows(a, b))))
    sc = [0.5, 0.5, 0.7, np.nan, -np.inf, np.inf, 0.0, -0.0]
    for e, se in enumerate(sc):
        for d, sd in enumerate(sc):
            lines.append("K %s %d %s %d %d" % (_hex64(se), e, _hex64(sd), d, int(R.ranks_before(se, e, sd, d))))
    for tp, fp, npos in [(0, 0, 0), (0, 1, 0), (0, 0, 5), (0, 3, 5), (3, 4, 7), (7, 0, 7), (1, 2, 3), (1000, 31000, 1234)]:
        lines.append("V %d %d %d %s %s" % (tp, fp, npos, _hex64(R.curve_rec(tp, npos)), _hex64(R.curve_prec(tp, fp))))
    for i in range(11):
        lines.append("T %d %s" % (i, _hex64(z["ap11_thresholds"][i])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


def test_arithmetic_header_as_a_host_program(golden, tmp_path):
    """det_ap_core.h compiled by the host compiler, on the fixture's pairs and the degenerate ones: the restatement's bits"""
    n = write_cases(str(tmp_path / "cases.txt"), golden("eval_ap.npz"))
    exe = str(tmp_path / "det_ap_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(REPO, "tests", "native", "det_ap_check.cpp"), "-o", exe])
    p = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and ("%d cases, 0 differ" % n) in p.stdout


def test_library_exports_the_entry_point_with_the_headers_signature():
    from odam_amd import _lib, evaluate
    L = _lib.lib()
    assert hasattr(L, "odam_det_ap"), "the built library has no odam_det_ap"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_eval.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+odam_det_ap\s*\(([^)]*)\)\s*;", txt)
    assert m, "odam_det_ap is not declared in include/odam_eval.h"
    c_types = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else c_types[arg.replace("const ", "").rsplit(" ", 1)[0]])
    assert evaluate.EVAL_ARGTYPES["odam_det_ap"] == want and len(want) == 34
    f = evaluate._entry("odam_det_ap")
    assert f.restype is ctypes.c_int
    assert "#define ODAM_AP_MAX_PRED %d\n" % evaluate.MAX_AP_PRED in txt and "#define ODAM_AP_ROW_SLOTS %d\n" % evaluate.ROW_SLOTS in txt
    assert evaluate.MAX_AP_PRED == R.MAX_PRED and evaluate.ROW_SLOTS == R.ROW_SLOTS
    # the argument checks come before any device work (the pointers below are never followed)
    P = 64
    ok = dict(ctx=P, kind=0, n_image=1, n_pred=2, n_gt=2, n_class=8, pred_off=P, gt_off=P, pred_box=P, gt_box=P, cls_pred=P, cls_gt=P,
              score=P, pair_off=None, iou=None, n_pairs=0, ovthresh=0.25, use07=0, scratch=P)
    outs = [P] * 14

    def call(outs=outs, **kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok], *outs, None)
    bad = [dict(ctx=None), dict(kind=-1), dict(kind=4), dict(n_class=0), dict(n_class=65), dict(n_image=-1), dict(n_pred=-1), dict(n_gt=-1),
           dict(n_pairs=-1), dict(pred_off=None), dict(gt_off=None), dict(scratch=None), dict(pred_box=None), dict(gt_box=None),
           dict(cls_pred=None), dict(cls_gt=None), dict(score=None), dict(kind=1), dict(kind=1, pair_off=P), dict(kind=1, iou=P),
           dict(kind=2, n_pred=30, n_gt=29), dict(kind=3, n_pred=31, n_gt=30), dict(kind=2, pred_box=None)]
    for kw in bad:
        assert call(**kw) == 1 and b"odam_det_ap" in L.odam_last_error(), kw      # ODAM_E_INVALID
    for k in range(14):
        assert call(outs=[None if i == k else P for i in range(14)]) == 1
    assert call(n_pred=evaluate.MAX_AP_PRED + 1) == 3 and b"32768" in L.odam_last_error()      # ODAM_E_LIMIT
    assert call(kind=2, n_image=1093, n_pred=32790, n_gt=32790) == 3
    with pytest.raises(_lib.OdamError, match="32769"):
        evaluate._ap_launch(0, 1, evaluate.MAX_AP_PRED + 1, 0, 8, *[None] * 9, 0, 0.25, False, None, "cpu")
