#!/usr/bin/env python3
"""Time of the two evaluation launches (odam_amd/evaluate.py over csrc/box_iou.hip), next to the host closed form
merge.box3d_iou_pairs and the numpy restatement tests/box_iou_ref.py on the same inputs:
  - the merge cost of 500 objects: one 500 x 500 launch with gate 2 (box3d_iou_matrix), against merge.cost_matrix on the host;
  - an evaluation of 312 scenes of 20 predictions x 15 ground-truth boxes (the size of the reference's val list): match_scenes,
    two launches, against the restatement's IoU and matching loop.
Median of the calls with [min .. max] after a warm-up call; there is no pass mark and this is not a throughput item.
   python tools/box_iou_timing.py [--calls 20] [--host-calls 3]
"call" is the host time of the function -- uploads and enqueues: it does not wait for the kernels; "device" is the time between two
events around it on the stream."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    a = ap.parse_args()
    import torch
    import box_iou_ref as R
    from odam_amd import evaluate, merge, sq
    fitter = sq.SqFitter("cuda:0", 10)
    rs = np.random.RandomState(0)
    # ---- the merge cost of 500 objects
    n = 500
    B = boxes(rs, n, 4.0); cls = rs.randint(0, 8, n)
    tracks = [np.tile(np.r_[0., c, np.zeros(80)], (3, 1)) for c in cls]
    dB, dc = torch.from_numpy(B).cuda(), torch.from_numpy(cls.astype(np.int32)).cuda()
    evaluate.box3d_iou_matrix(dB, dB, dc, dc, gate=2, fitter=fitter)      # warm-up: code object load
    r, wall, devt = timed(lambda: evaluate.box3d_iou_matrix(dB, dB, dc, dc, gate=2, fitter=fitter), a.calls)
    host, th = host_timed(lambda: merge.cost_matrix(tracks, B), a.host_calls)
    dev_cost, td = host_timed(lambda: merge.cost_matrix(tracks, B, fitter=fitter), a.host_calls)
    print("500 x 500, gate 2 (%d open pairs of 250000; %d calls on the device, %d on the host)" % (int(R.gate_open(2, cls, cls).sum()), a.calls, a.host_calls))
    print("  box3d_iou_matrix          call %s   device %s" % (stats(wall), stats(devt)))
    print("  merge.cost_matrix         host %s   with fitter (upload, launch, copy back, mirror) %s   worst |device - host| %.2e"
          % (stats(th), stats(td), np.abs(dev_cost - host).max()))
    # ---- 312 scenes of 20 predictions x 15 ground-truth boxes
    S, n_p, n_g = 312, 20, 15
    gts, preds = [], []
    for _ in range(S):
        g = boxes(rs, n_g, 3.0); gc = rs.randint(0, 8, n_g)
        p = np.concatenate([g + rs.normal(0, 0.03, g.shape), boxes(rs, n_p - n_g, 3.0)]); pc = np.concatenate([gc, rs.randint(0, 8, n_p - n_g)])
        k = rs.permutation(n_p)
        gts.append((g, gc)); preds.append((p[k], pc[k]))
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).cuda()
    dg = [(d(g, np.float64), d(c, np.int32)) for g, c in gts]; dp = [(d(p, np.float64), d(c, np.int32)) for p, c in preds]
    evaluate.match_scenes(dp, dg, 0.25, fitter=fitter)
    m, wall, devt = timed(lambda: evaluate.match_scenes(dp, dg, 0.25, fitter=fitter), a.calls)

    def restated():
        ious = [R.iou_scene(p[0], g[0], p[1], g[1], gate=1)[0] for p, g in zip(preds, gts)]
        return R.match_batch(ious, [p[1] for p in preds], [g[1] for g in gts], 0.25)
    ref, th = host_timed(restated, a.host_calls)
    same = np.array_equal(m["counts"].cpu().numpy(), ref[0]) and np.array_equal(m["gt_match"].cpu().numpy(), ref[2])
    f = evaluate.f1_table(m["counts"])
    print("%d scenes of %d predictions x %d ground-truth boxes (%d pairs)" % (S, n_p, n_g, S * n_p * n_g))
    print("  match_scenes (2 launches) call %s   device %s   numpy restatement %s   counts and matches equal: %s   F1 %.3f"
          % (stats(wall), stats(devt), stats(th), same, f["avg_f1"]))
    fitter.close()


if __name__ == "__main__":
    main()
