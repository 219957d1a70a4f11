#!/usr/bin/env python3
"""Time of the average-precision call (odam_amd/evaluate.py over csrc/det_ap.hip, six launches), next to the numpy restatement
tests/det_ap_ref.py on the same inputs:
  - 312 scenes of 20 predictions x 15 ground-truth boxes (the size of the reference's val list): average_precision with the
    axis-aligned overlap (six launches) and with the oriented one (odam_box3d_iou_batch first: seven);
  - one pair of 1000-frame detection blocks [1000, 30, 15] as detect_frames_packed returns them: detections_ap, both box kinds;
  - the ranking at its cap: 32768 predictions of one class in one image.
Median of the calls with [min .. max] after a warm-up call, inputs resident on the device; there is no pass mark.
   python tools/det_ap_timing.py [--calls 20] [--host-calls 1]
"call" is the host time of the function -- concatenation, uploads of the offsets and enqueues: it does not wait for the kernels;
"device" is the time between two events around it on the stream.
   python tools/det_ap_timing.py --reference      needs no GPU: the reference's own eval_det_cls over the eight classes on the 312
scenes, where a checkout of it is at hand (tests/golden/refenv.py), for the figure DESIGN 6k quotes beside the device's."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * float(np.median(xs)), 1e3 * xs[0], 1e3 * xs[-1])


def timed(fn, calls):
    import torch
    wall, devt = [], []
    for _ in range(calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        wall.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        devt.append(e0.elapsed_time(e1) * 1e-3)
    return out, wall, devt


def host_timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def boxes(rs, k, spread):
    from odam_amd.multi_view import get_3d_box

    def rotz(t):
        c, s = np.cos(t), np.sin(t)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return np.asarray([get_3d_box(rs.uniform(.3, 2, 3), rotz(rs.uniform(-3, 3)), rs.uniform(-spread, spread, 3)) for _ in range(k)]).reshape(k, 8, 3)


def scenes(S=312, n_p=20, n_g=15):
    rs = np.random.RandomState(0)
    gts, preds = [], []
    for _ in range(S):
        g = boxes(rs, n_g, 3.0); gc = rs.randint(0, 8, n_g)
        p = np.concatenate([g + rs.normal(0, 0.03, g.shape), boxes(rs, n_p - n_g, 3.0)]); pc = np.concatenate([gc, rs.randint(0, 8, n_p - n_g)])
        k = rs.permutation(n_p)
        gts.append((g, gc)); preds.append((p[k], pc[k], rs.uniform(0, 1, n_p)))
    return preds, gts


def blocks(F, seed=1):
    rs = np.random.RandomState(seed)
    a = np.zeros((F, 30, 15), np.float32)
    a[:, :, 1] = rs.randint(0, 8, (F, 30))
    a[:, :, 2:4] = rs.uniform(0, 0.6, (F, 30, 2)); a[:, :, 4:6] = a[:, :, 2:4] + rs.uniform(0.1, 0.4, (F, 30, 2))
    a[:, :, 6:9] = rs.uniform(0.3, 1.5, (F, 30, 3)); a[:, :, 9:12] = rs.uniform(-3, 3, (F, 30, 3)); a[:, :, 14] = rs.uniform(0.3, 1, (F, 30))
    b = a.copy()
    b[:, :, 2:6] += rs.normal(0, 0.02, (F, 30, 4)).astype(np.float32); b[:, :, 6:12] += rs.normal(0, 0.05, (F, 30, 6)).astype(np.float32)
    b[:, :, 14] = rs.uniform(0.3, 1, (F, 30))
    return a, rs.randint(0, 31, F).astype(np.int32), b, rs.randint(0, 31, F).astype(np.int32)


def reference_time(calls):
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import contextlib
    import io
    import make_golden_ap
    eu, _ = make_golden_ap.import_reference()
    preds, gts = scenes()

    def run():
        out = {}
        for c in range(8):
            pred_c = {s: [(b, sc) for b, k, sc in zip(*p) if k == c] for s, p in enumerate(preds)}
            pred_c = {s: v for s, v in pred_c.items() if v}
            gt_c = {s: [b for b, k in zip(*g) if k == c] for s, g in enumerate(gts)}
            gt_c = {s: v for s, v in gt_c.items() if v or s in pred_c}
            with contextlib.redirect_stdout(io.StringIO()):
                out[c] = eu.eval_det_cls(pred_c, gt_c, 0.25, False)[2]
        return out
    ap, ts = host_timed(run, calls)
    print("312 scenes of 20 predictions x 15 ground-truth boxes, the reference's eval_det_cls over 8 classes on the CPU: %s   mAP %.4f"
          % (stats(ts), float(np.mean(list(ap.values())))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.reference:
        return reference_time(max(a.host_calls, 1))
    import torch
    import det_ap_ref as R
    from odam_amd import evaluate, sq
    fitter = sq.SqFitter("cuda:0", 10)
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).cuda()
    # ---- 312 scenes of 20 predictions x 15 ground-truth boxes
    preds, gts = scenes()
    dp = [(d(p, np.float64), d(c, np.int32), d(s, np.float64)) for p, c, s in preds]; dg = [(d(g, np.float64), d(c, np.int32)) for g, c in gts]
    print("312 scenes of 20 predictions x 15 ground-truth boxes (%d calls on the device, %d on the host)" % (a.calls, a.host_calls))
    for iou in ("aabb", "obb"):
        evaluate.average_precision(dp, dg, 0.25, iou=iou, fitter=fitter)      # warm-up: code object load
        r, wall, devt = timed(lambda: evaluate.average_precision(dp, dg, 0.25, iou=iou, fitter=fitter), a.calls)
        print("  average_precision(%-4s)   call %s   device %s   mAP %.4f" % (iou, stats(wall), stats(devt), evaluate.ap_table(r)["mAP"]))
        if iou == "aabb":
            args = R.from_lists(preds, gts)
            ref, th = host_timed(lambda: R.det_ap(0, n_class=8, ovthresh=0.25, **args), a.host_calls)
            same = np.array_equal(r["is_tp"].cpu().numpy(), np.asarray(ref["is_tp"])) and np.array_equal(r["rank"].cpu().numpy(), np.asarray(ref["rank"]))
            print("  numpy restatement         host %s   flags and ranks equal: %s   largest |AP difference| %.3g"
                  % (stats(th), same, np.nanmax(np.abs(r["ap"].cpu().numpy() - ref["ap"]))))
    # ---- one pair of 1000-frame detection blocks
    A, ca, B, cb = blocks(1000)
    dA, dB, dca, dcb = d(A, np.float32), d(B, np.float32), d(ca, np.int32), d(cb, np.int32)
    print("1000 frames, two blocks [1000, 30, 15] (%d and %d detections)" % (ca.sum(), cb.sum()))
    for iou in ("aabb3d", "box2d"):
        evaluate.detections_ap(dA, dca, dB, dcb, iou=iou, fitter=fitter)
        t, wall, devt = timed(lambda: evaluate.detections_ap(dA, dca, dB, dcb, iou=iou, fitter=fitter)["device"]["ap"], a.calls)
        print("  detections_ap(%-6s)     call %s   device %s   mAP %.4f" % (iou, stats(wall), stats(devt), float(np.nanmean(t.cpu().numpy()))))
    # ---- the ranking at its cap: one class, one image
    n = evaluate.MAX_AP_PRED
    rs = np.random.RandomState(2)
    g = boxes(rs, 15, 3.0)
    p = g[rs.randint(0, 15, n)] + rs.normal(0, 0.05, (n, 8, 3))
    one_p = [(d(p, np.float64), torch.zeros(n, dtype=torch.int32, device="cuda"), d(rs.uniform(0, 1, n), np.float64))]
    one_g = [(d(g, np.float64), torch.zeros(15, dtype=torch.int32, device="cuda"))]
    evaluate.average_precision(one_p, one_g, 0.25, fitter=fitter)
    r, wall, devt = timed(lambda: evaluate.average_precision(one_p, one_g, 0.25, fitter=fitter), a.calls)
    rk = r["rank"].cpu().numpy()
    print("%d predictions of one class in one image (the cap of the ranking), 15 ground-truth boxes" % n)
    print("  average_precision(aabb)   call %s   device %s   ranks are a permutation: %s   AP %.4f"
          % (stats(wall), stats(devt), np.array_equal(np.sort(rk), np.arange(n)), float(r["ap"][0])))
    fitter.close()


if __name__ == "__main__":
    main()
