"""Golden for the evaluation: the reference's own match_sequence and get_f1 (src/scripts/eval_scan2cad.py:249-295, imported here)
on 8 synthetic scenes of 0-15 ground-truth boxes with perturbed, duplicated, wrong-class and spurious predictions in shuffled
order, at thresholds 0.25 and 0.5.  Stores the inputs, the counts per scene, which prediction claimed which box (observed on the
reference's own run: every `total_tps[c] += 1` follows the box3d_iou call that caused it) and the numbers get_f1 printed.
Run: python tests/golden/make_golden_eval.py"""
import contextlib
import io
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

THRESHOLDS = (0.25, 0.5)
N_GT = (7, 0, 15, 4, 11, 1, 9, 13)      # scene 1 has no ground truth; scene 3's predictions are all dropped below
MARGIN = 1e-6


def make_scenes(bu):
    rs = np.random.RandomState(5)
    scenes = []
    for s, n_gt in enumerate(N_GT):
        gts, preds = [], []

        def add_pred(c, ctr, dims, yaw, sigma):
            preds.append((c, bu.get_3d_box(dims * rs.uniform(1 - sigma, 1 + sigma, 3), bu.rotz(yaw + rs.normal(0, sigma)),
                                           ctr + rs.normal(0, sigma * 0.5, 3))))
        for g in range(n_gt):
            c = int(rs.randint(0, 8))
            ctr = rs.uniform(-4, 4, 3) * [1, 1, 0.2]; dims = rs.uniform(0.4, 1.8, 3); yaw = rs.uniform(-np.pi, np.pi)
            gts.append((c, bu.get_3d_box(dims, bu.rotz(yaw), ctr)))
            kind = rs.randint(0, 6)
            if kind == 0:                 # missed
                pass
            elif kind == 1:               # found twice: the box is contested by two predictions
                add_pred(c, ctr, dims, yaw, 0.05); add_pred(c, ctr, dims, yaw, 0.08)
            elif kind == 2:               # found, under another class
                add_pred((c + 1 + int(rs.randint(0, 7))) % 8, ctr, dims, yaw, 0.05)
            elif kind == 3:               # a second ground-truth box of the class nearly on top: one prediction claims both
                gts.append((c, bu.get_3d_box(dims * 0.9, bu.rotz(yaw + 0.05), ctr + [0.03, -0.02, 0.0])))
                add_pred(c, ctr, dims, yaw, 0.03)
            else:                         # found, well or badly
                add_pred(c, ctr, dims, yaw, [0.05, 0.15, 0.3][int(rs.randint(0, 3))])
        for _ in range(max(int(rs.randint(0, 4)), 2 if n_gt == 0 else 0)):      # spurious
            add_pred(int(rs.randint(0, 8)), rs.uniform(-4, 4, 3) * [1, 1, 0.2], rs.uniform(0.4, 1.8, 3), rs.uniform(-np.pi, np.pi), 0.0)
        if s == 3:
            preds = []
        gts = gts[:15]
        preds = [preds[k] for k in rs.permutation(len(preds))]
        scenes.append((gts, preds))
    return scenes


def main():
    import refenv
    refenv.setup()
    import src.scripts.eval_scan2cad as ev
    import src.utils.box_utils as bu
    names = [ev.DETECTOR_CLASS_MAPPER[c] for c in range(8)]
    assert list(ev.CARE_CLASSES) == names          # get_f1 walks CARE_CLASSES in the detector's class order
    scenes = make_scenes(bu)
    n_scene = len(scenes)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g, _ in scenes])]).astype(np.int32)
    pred_off = np.concatenate([[0], np.cumsum([len(p) for _, p in scenes])]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum([len(p) * len(g) for g, p in scenes])]).astype(np.int64)
    ref_iou = np.full(pair_off[-1], -1.0)          # what the reference evaluated (same-class pairs), -1 elsewhere
    real_iou = bu.box3d_iou
    last = {}

    class Claims(dict):                            # total_tps: `total_tps[c] += 1` is the claim of the pair just evaluated
        def __setitem__(self, k, v):
            if k in self and v == self[k] + 1:
                last["claims"].append(last["pair"])
            super().__setitem__(k, v)

    counts = np.zeros((len(THRESHOLDS), n_scene, 3, 8), np.int32)
    claimed = np.zeros((len(THRESHOLDS), pred_off[-1]), np.int32)
    gt_match = np.full((len(THRESHOLDS), gt_off[-1]), -1, np.int32)
    f1 = np.zeros((len(THRESHOLDS), 8, 3)); f1_avg = np.zeros((len(THRESHOLDS), 3))
    for t, thr in enumerate(THRESHOLDS):
        tot = [{k: 0 for k in names}, {k: 0 for k in names}, Claims({k: 0 for k in names})]
        for s, (gts, preds) in enumerate(scenes):
            ids_g = {id(b): i for i, (_, b) in enumerate(gts)}; ids_p = {id(b): p for p, (_, b) in enumerate(preds)}

            def spy(gt_bbx, pred_bbx):
                p, i = ids_p[id(pred_bbx)], ids_g[id(gt_bbx)]
                out = real_iou(gt_bbx, pred_bbx)
                last["pair"] = (p, i)
                ref_iou[pair_off[s] + p * len(gts) + i] = out[0]
                return out
            bu.box3d_iou = spy
            before = [{k: d[k] for k in names} for d in tot]
            last["claims"] = []
            with np.errstate(all="raise"):         # a pair on which the reference's clipper divides by zero is not a case
                ev.match_sequence(tot[0], tot[1], tot[2], [{"class": names[c], "bbox": b} for c, b in preds],
                                  [(names[c], b) for c, b in gts], None, thr, "scene%d" % s)
            bu.box3d_iou = real_iou
            for k in range(3):
                counts[t, s, k] = [tot[k][c] - before[k][c] for c in names]
            for p, i in last["claims"]:
                claimed[t, pred_off[s] + p] += 1
                assert gt_match[t, gt_off[s] + i] == -1
                gt_match[t, gt_off[s] + i] = p
            assert claimed[t, pred_off[s]:pred_off[s + 1]].sum() == counts[t, s, 2].sum()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ev.get_f1(*tot)
        nums = [float(x) for x in re.findall(r"(?:accuracy|recall|F1): ([-+0-9.e]+|nan|inf)", buf.getvalue())]
        assert len(nums) == 27, buf.getvalue()
        f1[t] = np.asarray(nums[:24]).reshape(8, 3); f1_avg[t] = nums[24:]
    # what the fixture must contain
    n_g = np.diff(gt_off); n_p = np.diff(pred_off)
    assert ((n_g == 0) & (n_p > 0)).any(), "a scene with no ground truth"
    assert ((n_p == 0) & (n_g > 0)).any(), "a scene with no predictions"
    assert n_g.max() <= 15 and len(n_g) == 8
    assert (claimed >= 2).any(axis=1).all(), "a prediction that claims two ground-truth boxes"
    evaluated = ref_iou >= 0
    for t, thr in enumerate(THRESHOLDS):
        contested = 0
        for s, (gts, preds) in enumerate(scenes):
            blk = ref_iou[pair_off[s]:pair_off[s + 1]].reshape(len(preds), len(gts))
            contested += int(((blk > thr).sum(axis=0) >= 2).sum())
        assert contested >= 1, "a ground-truth box contested by two predictions"
        margin = np.abs(ref_iou[evaluated] - thr).min()
        assert margin > MARGIN, margin
        print("threshold %.2f: counts gts %d preds %d tps %d; contested boxes %d; smallest margin %.3g over %d same-class pairs"
              % (thr, counts[t, :, 0].sum(), counts[t, :, 1].sum(), counts[t, :, 2].sum(), contested, margin, evaluated.sum()))
    np.savez_compressed(os.path.join(HERE, "eval_match.npz"),
                        gt_boxes=np.asarray([b for g, _ in scenes for _, b in g]).reshape(-1, 8, 3),
                        gt_cls=np.asarray([c for g, _ in scenes for c, _ in g], np.int32), gt_off=gt_off,
                        pred_boxes=np.asarray([b for _, p in scenes for _, b in p]).reshape(-1, 8, 3),
                        pred_cls=np.asarray([c for _, p in scenes for c, _ in p], np.int32), pred_off=pred_off, pair_off=pair_off,
                        thresholds=np.asarray(THRESHOLDS), counts=counts, claimed=claimed, gt_match=gt_match, f1=f1, f1_avg=f1_avg,
                        ref_iou3d=ref_iou)
    print("eval golden: %d scenes, %d ground-truth boxes, %d predictions" % (n_scene, gt_off[-1], pred_off[-1]))


if __name__ == "__main__":
    main()
