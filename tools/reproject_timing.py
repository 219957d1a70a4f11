#!/usr/bin/env python3
"""Time of the three reprojection launches (SqFitter.reproject, reproject_dual, reprojection_score), inputs resident on the device,
next to the numpy restatement (tests/reproject_ref.py) and, for the dual quadric, next to the Python loop over
sq.DualQuadric.get_bbox that the launch replaces: 30 objects x 40 views and 500 objects x 256 views.  Median of the calls with
[min .. max]; there is no pass mark and this is not a throughput item.
   python tools/reproject_timing.py [--calls 20] [--host-calls 1]
"call" is the host time of the method -- the upload of the view offsets and the enqueue: it does not wait for the kernel; "device"
is the time between two events around it on the stream."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=1, help="calls of the host versions at the large shape (5 at the small one)")
    a = ap.parse_args()
    import torch
    import quadric_svd_ref as S
    import reproject_ref as R
    from odam_amd import sq
    P_cws = np.load(os.path.join(REPO, "tests", "golden", "quadric_svd.npz"))["P_cws"]
    fitter = sq.SqFitter("cuda:0", 10)
    for n_obj, views, host_calls in ((30, 40, 5), (500, 256, a.host_calls)):
        probs = [S.exact_problem(P_cws, views, 5000 + i) for i in range(n_obj)]
        vc = [len(p[2]) for p in probs]
        P64, edges = (np.concatenate([p[k] for p in probs]) for k in (0, 1))
        Q = np.stack([p[3] for p in probs])
        rs = np.random.RandomState(0)
        boxes = edges + rs.uniform(-2, 2, edges.shape)
        mask = np.ones_like(edges, dtype=np.float32)
        # super-quadrics at the same places: translate from Q, scales of the ellipsoid's size
        p9 = np.stack([sq.init_params(q[:3, 3] / q[3, 3], 0.1 * i, [0.5, 0.4, 0.6]) for i, q in enumerate(Q)])
        pts = fitter.points(p9)
        P32 = P64.astype(np.float32)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        dP32, dP64, dQ, dm = d(P32), d(P64), d(Q), d(mask)
        dB32, dB64 = d(boxes.astype(np.float32)), d(boxes)
        head = "%4d objects x %3d views" % (n_obj, views)
        print("%s (%d calls on the device, %d on the host)" % (head, a.calls, host_calls))
        fitter.reproject(pts, vc, dP32)      # warm-up: code object load
        r32, wall, devt = timed(lambda: fitter.reproject(pts, vc, dP32), a.calls)
        ref, host = host_timed(lambda: R.reproject(pts.cpu().numpy(), vc, P32), host_calls)
        same = np.array_equal(r32["ext"].cpu().numpy().view(np.uint32), ref["ext"].view(np.uint32))
        print("  reproject (1000 points)   call %s   device %s   numpy restatement %s   bits equal: %s" % (stats(wall), stats(devt), stats(host), same))
        fitter.reproject_dual(dQ, vc, dP64)
        r64, wall, devt = timed(lambda: fitter.reproject_dual(dQ, vc, dP64), a.calls)
        ref, host = host_timed(lambda: R.reproject_dual(Q, vc, P64), host_calls)
        offs = np.concatenate([[0], np.cumsum(vc)])
        loop, host2 = host_timed(lambda: np.concatenate([R.get_bbox_rows(Q[i], P64[offs[i]:offs[i + 1]]) for i in range(n_obj)]), host_calls)
        got = r64["ext"].cpu().numpy()
        print("  reproject_dual            call %s   device %s   numpy restatement %s   get_bbox loop %s   worst vs restatement %.2e px, vs get_bbox %.2e px"
              % (stats(wall), stats(devt), stats(host), stats(host2), np.abs(got - ref["ext"]).max(), np.abs(got - loop).max()))
        for name, ext, bad, bx, href in (("float32", r32["ext"], r32["n_valid"] == 0, dB32, boxes.astype(np.float32)), ("float64", r64["ext"], r64["status"], dB64, boxes)):
            fitter.reprojection_score(ext, bad, vc, bx, dm, 640, 480)
            s, wall, devt = timed(lambda: fitter.reprojection_score(ext, bad, vc, bx, dm, 640, 480), a.calls)
            e, b = ext.cpu().numpy(), bad.cpu().numpy()
            ref, host = host_timed(lambda: R.reprojection_score(e, b, vc, href, mask, 640, 480), host_calls)
            dev = np.nanmax(np.abs(s["loss_2d"].cpu().numpy().astype(np.float64) - ref["loss_2d"]) / np.abs(ref["loss_2d"]))
            print("  reprojection_score %s  call %s   device %s   numpy restatement %s   worst loss_2d vs restatement %.2e relative"
                  % (name, stats(wall), stats(devt), stats(host), dev))
    fitter.close()


if __name__ == "__main__":
    main()
