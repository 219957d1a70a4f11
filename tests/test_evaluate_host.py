"""The numpy restatement of the evaluation kernels (tests/box_iou_ref.py) and the host half of odam_amd/evaluate.py against the
reference-run fixtures: box_iou.npz (box_utils.box3d_iou on 512 pairs), eval_match.npz (eval_scan2cad.py's match_sequence and get_f1
on 8 scenes at two thresholds, tests/golden/make_golden_eval.py) and the tracks of sq_merge.npz.  No device."""
import numpy as np
import pytest

import box_iou_ref as R

IOU_TOL = 1e-12      # the bound tests/test_merge.py holds the host closed form to


def _scenes(z):
    go, po = z["gt_off"], z["pred_off"]
    n = len(go) - 1
    preds = [(z["pred_boxes"][po[s]:po[s + 1]], z["pred_cls"][po[s]:po[s + 1]]) for s in range(n)]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(n)]
    return preds, gts


def test_restated_iou_matches_the_reference(golden):
    z = golden("box_iou.npz")
    i3, i2 = R.iou_pairs(z["A"], z["B"])
    print("restatement vs box3d_iou: 3D %.3g, bev %.3g" % (np.abs(i3 - z["iou3d"]).max(), np.abs(i2 - z["iou_bev"]).max()))
    assert np.abs(i3 - z["iou3d"]).max() <= IOU_TOL and np.abs(i2 - z["iou_bev"]).max() <= IOU_TOL
    assert np.array_equal(i3 == 0, z["iou3d"] == 0) and np.array_equal(i2 == 0, z["iou_bev"] == 0)
    assert (z["iou3d"] == 0).sum() > 50 and (z["iou3d"] > 0.3).sum() > 50


def test_restated_iou_agrees_with_the_host_closed_form(golden):
    """the product's merge.box3d_iou_pairs lets numpy add four terms as t0 + ((t1 + t2) + t3); the kernels add in index order"""
    from odam_amd import merge
    z = golden("box_iou.npz")
    i3, i2 = R.iou_pairs(z["A"], z["B"])
    h3, h2 = merge.box3d_iou_pairs(z["A"], z["B"])
    assert np.abs(i3 - h3).max() <= IOU_TOL and np.abs(i2 - h2).max() <= IOU_TOL and np.array_equal(i3 == 0, h3 == 0)


def test_restated_iou_of_a_scene_gates_and_shapes():
    rs = np.random.RandomState(3)
    from odam_amd.multi_view import get_3d_box
    box = lambda: get_3d_box(rs.uniform(.5, 2, 3), np.eye(3), rs.uniform(-1, 1, 3))
    A = np.stack([box() for _ in range(5)]); B = np.stack([box() for _ in range(7)])
    ca = np.array([0, 4, 5, 4, 2]); cb = np.array([4, 5, 0, 2, 2, 7, 4])
    full, _ = R.iou_scene(A, B)
    assert full.shape == (5, 7) and (full > 0).sum() > 10
    for gate in (1, 2):
        g3, g2 = R.iou_scene(A, B, ca, cb, gate)
        op = R.gate_open(gate, ca, cb)
        assert np.array_equal(g3[op], full[op]) and (g3[~op] == 0).all() and (g2[~op] == 0).all()
    assert R.gate_open(2, ca, cb)[1, 1] and not R.gate_open(1, ca, cb)[1, 1] and not R.gate_open(2, ca, cb)[0, 0]
    assert R.iou_scene(A[:0], B)[0].shape == (0, 7) and R.iou_scene(A, B[:0])[0].shape == (5, 0)
    with pytest.raises(ValueError):
        R.iou_scene(A, B, None, cb, 1)


@pytest.mark.parametrize("t", [0, 1])
def test_restated_matching_equals_the_reference_run(golden, t):
    z = golden("eval_match.npz")
    thr = float(z["thresholds"][t])
    preds, gts = _scenes(z)
    assert any(len(g[1]) == 0 and len(p[1]) > 0 for p, g in zip(preds, gts))          # what the fixture must contain
    assert any(len(p[1]) == 0 and len(g[1]) > 0 for p, g in zip(preds, gts))
    assert (z["claimed"][t] >= 2).any()
    ious = [R.iou_scene(p[0], g[0], p[1], g[1], gate=1)[0] for p, g in zip(preds, gts)]
    # the reference evaluated box3d_iou(gt, prediction) on the same-class pairs; the kernels' order is (prediction, gt)
    flat = np.concatenate([i.reshape(-1) for i in ious])
    ev = z["ref_iou3d"] >= 0
    print("restatement vs the reference's IoU of the same-class pairs: %.3g" % np.abs(flat[ev] - z["ref_iou3d"][ev]).max())
    assert np.abs(flat[ev] - z["ref_iou3d"][ev]).max() <= IOU_TOL and ev.sum() > 100
    assert np.abs(z["ref_iou3d"][ev] - thr).min() > 1e-6                               # no count can flip on rounding
    counts, claimed, gt_match = R.match_batch(ious, [p[1] for p in preds], [g[1] for g in gts], thr)
    assert np.array_equal(counts, z["counts"][t]) and counts.dtype == np.int32
    assert np.array_equal(claimed, z["claimed"][t]) and np.array_equal(gt_match, z["gt_match"][t])
    from odam_amd import evaluate
    f = evaluate.f1_table(counts)
    got = np.stack([f["precision"], f["recall"], f["f1"]], axis=1)
    assert np.allclose(got, z["f1"][t], rtol=1e-15, atol=0)
    avg = np.array([f["avg_precision"], f["avg_recall"], f["avg_f1"]])
    assert np.allclose(avg, z["f1_avg"][t], rtol=1e-15, atol=0)


def test_matching_rules():
    """no break: one prediction claims every free box of its class; a used box is not claimed twice; a class id outside
    0..n_class-1 is counted nowhere; a NaN IoU never matches; more than 4096 ground-truth boxes is refused"""
    iou = np.array([[0.9, 0.8, 0.1, 0.7], [0.95, 0.1, 0.6, np.nan], [0.9, 0.9, 0.9, 0.9], [0.9, 0.9, 0.9, 0.9]])
    counts, claimed, gt_match = R.match_scene(iou, [1, 1, -1, 8], [1, 1, 1, 1], 0.5, n_class=8)
    assert claimed.tolist() == [3, 1, 0, 0] and gt_match.tolist() == [0, 0, 1, 0]
    assert counts[:, 1].tolist() == [4, 2, 4] and counts.sum() == 10
    counts, claimed, gt_match = R.match_scene(iou[:, :2], [1, 1, 1, 1], [-1, 8], 0.5)
    assert counts.sum() == 4 and claimed.sum() == 0 and (gt_match == -1).all()
    with pytest.raises(OverflowError):
        R.match_scene(np.zeros((1, 4097)), [0], np.zeros(4097, int), 0.5)


def test_f1_table_where_the_reference_would_divide_by_zero():
    from odam_amd import evaluate
    c = np.zeros((2, 3, 8), np.int64)
    c[0, :, 0] = [4, 2, 1]; c[1, :, 0] = [0, 2, 1]       # class 0: 4 gts, 4 preds, 2 tps over two scenes
    c[0, 0, 1] = 3                                        # class 1: ground truth and no prediction (ZeroDivisionError there)
    c[0, 1, 2] = 5                                        # class 2: predictions and no ground truth: 0 by the reference's rule
    f = evaluate.f1_table(c)
    assert f["precision"][0] == 0.5 and f["recall"][0] == 0.5 and f["f1"][0] == 0.5
    assert f["precision"][1] == 0 and f["recall"][1] == 0 and f["f1"][1] == 0 and f["f1"][2] == 0 and f["precision"][2] == 0
    assert f["avg_precision"] == 2 / 9 and f["avg_recall"] == 2 / 7
    e = evaluate.f1_table(np.zeros((3, 8), int))
    assert e["avg_f1"] == 0 and e["avg_precision"] == 0 and not e["f1"].any()


def test_predictions_from_result(golden):
    from odam_amd import evaluate
    z = golden("sq_merge.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    out = {"tracks": tracks, "bboxes_qc": list(z["bboxes_qc"])}
    boxes, cls, ids = evaluate.predictions_from_result(out)
    assert boxes.shape == (9, 8, 3) and boxes.dtype == np.float64 and np.array_equal(boxes, z["bboxes_qc"])
    assert cls.dtype == np.int32 and cls.tolist() == [int(np.median(t[:, 1])) for t in tracks] and ids.tolist() == list(range(9))
    keep = [i for i, t in enumerate(tracks) if len(t) >= 30]
    boxes, cls, ids = evaluate.predictions_from_result(out, min_views=30)
    assert 0 < len(keep) < 9 and ids.tolist() == keep and np.array_equal(boxes, z["bboxes_qc"][keep])
    boxes, cls, ids = evaluate.predictions_from_result(out, min_views=1000)
    assert boxes.shape == (0, 8, 3) and cls.shape == (0,)


def degenerate_pairs(golden):
    z = golden("box_iou.npz")
    return R.degenerate_pairs(z["A"][0], z["B"][0])


def test_degenerate_pairs_in_the_restatement(golden):
    A, B = degenerate_pairs(golden)
    with np.errstate(all="ignore"):
        i3, i2 = R.iou_pairs(A, B)
        h3, h2 = __import__("odam_amd.merge", fromlist=["x"]).box3d_iou_pairs(A, B)
    assert abs(i3[0] - 1) <= IOU_TOL and abs(i2[0] - 1) <= IOU_TOL
    assert np.isnan(i3[1]) and i3[7] == 0 and i2[7] == 0 and np.isnan(i3[6])
    assert np.array_equal(np.isnan(i3), np.isnan(h3)) and np.array_equal(np.isnan(i2), np.isnan(h2))
    ok = ~np.isnan(i3)
    assert np.abs(i3[ok] - h3[ok]).max() <= IOU_TOL


def test_leaf_header_on_the_host_equals_the_restatement_bit_for_bit(golden, tmp_path):
    """odam_amd/csrc/box_iou_core.h compiled by the host compiler (tests/native/box_iou_check.cpp, a stand-alone program) on the
    512 fixture pairs and the degenerate ones: every bit of both outputs, NaN for NaN"""
    import os
    import subprocess
    from conftest import REPO
    exe = str(tmp_path / "box_iou_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(REPO, "tests", "native", "box_iou_check.cpp")])
    z = golden("box_iou.npz")
    dA, dB = degenerate_pairs(golden)
    A = np.concatenate([z["A"], dA]); B = np.concatenate([z["B"], dB])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int64(len(A)).tobytes()); f.write(np.ascontiguousarray(A).tobytes()); f.write(np.ascontiguousarray(B).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        i3, i2 = R.iou_pairs(A, B)
    for g, w in ((got[:, 0], i3), (got[:, 1], i2)):
        assert np.array_equal(np.isnan(g), np.isnan(w))
        ok = ~np.isnan(w)
        assert np.array_equal(g[ok].view(np.uint64), w[ok].view(np.uint64))
