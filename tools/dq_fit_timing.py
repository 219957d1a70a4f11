#!/usr/bin/env python3
"""Wall time of ONE dual-quadric fit call (odam_dq_fit_batch through SqFitter.fit_dual): N objects x F views x 500 Adam steps,
inputs resident on the device, median of repeated calls (each call ends with the read-back of the [N, 2] status, as
fit_dual does):
   python tools/dq_fit_timing.py [objects = 30,500] [views = 256] [calls = 20]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from odam_amd import sq, synth  # noqa: E402

objects = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "30,500").split(",")]
views = int(sys.argv[2]) if len(sys.argv) > 2 else 256
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
fitter = sq.SqFitter("cuda:0", 200)
probs = [synth.make_sq_problem(views, 900 + i) for i in range(12)]
for n in objects:
    use = [probs[i % len(probs)] for i in range(n)]
    ih = [sq.init_dual(p["translate"], p["angle"], p["dims"]) for p in use]
    tm = [sq.lines_to_targets(p["bbox_lines"]) for p in use]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    args = (dev(np.stack([a for a, _ in ih])), dev(np.stack([b for _, b in ih])), [views] * n,
            dev(np.concatenate([p["P"].astype(np.float32).reshape(-1, 12) for p in use])),
            dev(np.concatenate([t for t, _ in tm])), dev(np.concatenate([m for _, m in tm])))
    times = []
    for i in range(calls + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fitter.fit_dual(*args, n_iters=500)
        torch.cuda.synchronize()
        if i >= 3:
            times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    print("%d objects x %d views x 500 steps: median %.3f ms per call over %d calls (min %.3f, max %.3f) = %.0f objects/s; status ok: %s" % (
        n, views, 1e3 * med, calls, 1e3 * min(times), 1e3 * max(times), n / med, bool((out["status"][:, 0] == 0).all())))
fitter.close()
