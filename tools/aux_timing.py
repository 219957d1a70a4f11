#!/usr/bin/env python3
"""Time of one call with the outputs of every decoder layer off and on, on one device:
  forward    Detector(x) against Detector(x, aux=True) -- odam_detr_forward against odam_detr_forward_aux, which adds the decoder's
             final norm and the six heads after each of the first dec_layers - 1 decoder layers -- at --frames x 3 x --height x --width,
             ResNet-50, --dtype
  criterion  SetCriterion over the dec_layers layers in ONE layered call (one cost launch, one assignment launch, two launches of the
             losses, one read-back) against dec_layers single-layer calls, at --crit-frames frames, 100 queries, 0 .. 32 targets per frame
Median of --calls calls with [min .. max] after --warmup calls; "call" is the host time up to the return (the criterion's return waits
for its read-back; the forward is followed by a synchronize).  There is no pass mark.
   python tools/aux_timing.py [--calls 20] [--warmup 3] [--frames 8] [--height 800] [--width 1066] [--dtype fp32] [--crit-frames 32]"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * float(np.median(xs)), 1e3 * xs[0], 1e3 * xs[-1])


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1066)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--crit-frames", type=int, default=32)
    a = ap.parse_args()
    import torch
    from criterion_timing import COSTS, WEIGHTS, inputs
    from odam_amd import criterion, detector, weights

    det = detector.Detector(max_batch=a.frames, device="cuda:0", dtype=a.dtype)
    det.load_state_dict(weights.make_state_dict(seed=0))
    L = det.arch["dec_layers"]
    torch.manual_seed(0)
    x = torch.randn(a.frames, 3, a.height, a.width).cuda()
    off = timed(lambda: det(x), a.calls, a.warmup)
    on = timed(lambda: det(x, aux=True), a.calls, a.warmup)
    same = all(torch.equal(det(x)[k], det(x, aux=True)[k]) for k in detector.AUX_KEYS + ("pred_obj_features",))
    det.close()
    print("forward, %d x 3 x %d x %d, ResNet-50, %s, %d decoder layers (%d calls after %d)" % (a.frames, a.height, a.width, a.dtype, L, a.calls, a.warmup))
    print("  aux off   call   %s" % stats(off))
    print("  aux on    call   %s" % stats(on))
    print("  medians on / off = %.4f   last slot equals the plain forward bit for bit: %s" % (np.median(on) / np.median(off), same))

    B = a.crit_frames
    layers = [inputs(B, 100, seed=s) for s in range(L)]
    targets = [{"objects": torch.from_numpy(t["objects"]).cuda()} for t in layers[0][1]]
    dev = [{k: torch.from_numpy(v).cuda() for k, v in out.items()} for out, _ in layers]
    outputs = dict(dev[-1], aux_outputs=dev[:-1])
    wd = dict(WEIGHTS)
    wd.update({f"{k}_{i}": v for i in range(L - 1) for k, v in WEIGHTS.items()})
    crit = criterion.SetCriterion(18, criterion.HungarianMatcher(**COSTS), wd, 0.1, list(criterion.LOSS_NAMES))
    got = {}

    def layered():
        got["layered"] = crit(outputs, targets)

    def one_by_one():
        got["single"] = [crit(d, targets) for d in dev]
    t_l = timed(layered, a.calls, a.warmup)
    t_s = timed(one_by_one, a.calls, a.warmup)
    same = all(float(got["single"][l][k]) == float(got["layered"][k if l == L - 1 else f"{k}_{l}"])
               for l in range(L) for k in got["single"][l] if not (k == "class_error" and l < L - 1))
    print("criterion, %d frames x 100 queries, %d targets, %d layers" % (B, sum(int(t["objects"].shape[0]) for t in targets), L))
    print("  one layered call          call   %s" % stats(t_l))
    print("  %d single-layer calls      call   %s" % (L, stats(t_s)))
    print("  medians layered / single = %.4f   every entry equal bit for bit: %s" % (np.median(t_l) / np.median(t_s), same))


if __name__ == "__main__":
    main()
