#!/usr/bin/env python3
"""Time of one closed-form dual-quadric call (SqFitter.quadric_svd -> odam_dq_svd_batch), inputs resident on the device, next to
the float64 numpy restatement (tests/quadric_svd_ref.py: numpy products, LAPACK eigh, one object after the other) on the same
inputs: 30 objects x 40 views and 500 objects x 256 views.  Median of the calls with [min .. max]; there is no pass mark.
   python tools/quadric_svd_timing.py [--calls 20] [--host-calls 5]
"call" is the wall time of quadric_svd including the upload of the view offsets and the download of the status words (which ends
the launch); "device" is the time between two events around it on the stream."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5, help="calls of the numpy restatement at the large shape (20 at the small one)")
    a = ap.parse_args()
    import torch
    import quadric_svd_ref as R
    from odam_amd import sq
    P_cws = np.load(os.path.join(REPO, "tests", "golden", "quadric_svd.npz"))["P_cws"]
    fitter = sq.SqFitter("cuda:0", 10)
    for n_obj, views, host_calls in ((30, 40, a.calls), (500, 256, a.host_calls)):
        probs = [R.exact_problem(P_cws, views, 5000 + i) for i in range(n_obj)]
        vc = [len(p[2]) for p in probs]
        P, e, m = (np.concatenate([p[k] for p in probs]) for k in range(3))
        dP, de, dm = (torch.from_numpy(x).cuda() for x in (P, e, m))
        out = fitter.quadric_svd(vc, dP, de, dm)      # warm-up: code object load
        assert (out["status"] == 0).all()
        wall, devt = [], []
        for _ in range(a.calls):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = fitter.quadric_svd(vc, dP, de, dm)
            e1.record()
            wall.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            devt.append(e0.elapsed_time(e1) * 1e-3)
        host = []
        for _ in range(host_calls):
            t0 = time.perf_counter()
            ref = R.quadric_svd(vc, P, e, m)
            host.append(time.perf_counter() - t0)
        Q = out["Q"].cpu().numpy()
        worst = max(R.q_err(Q[i], ref["Q"][i]) / R.scale_u(ref["eig"][i]) for i in range(n_obj))
        print("%4d objects x %3d views: call %s   device %s   (%d calls)" % (n_obj, views, stats(wall), stats(devt), a.calls))
        print("%25s numpy restatement %s   (%d calls); worst device-vs-restatement err %.3f u" % ("", stats(host), host_calls, worst))
    fitter.close()


if __name__ == "__main__":
    main()
