#!/usr/bin/env python3
"""Time of one validation-loss call (odam_amd/criterion.py over csrc/det_loss.hip: the cost launch, the assignment launch and the
two launches of the losses) at B = 32 frames, Q = 100 queries, 19 logits, 30 angle bins and 0 .. 32 targets per frame, next to the
numpy restatement tests/criterion_ref.py (cost, solver and losses in float64) on the same inputs on the host.
Median of the calls with [min .. max] after a warm-up call, outputs and targets resident on the device; there is no pass mark.
   python tools/criterion_timing.py [--calls 20] [--host-calls 1] [--frames 32] [--queries 100]
"call" is the host time of criterion(outputs, targets) up to its return -- staging of the targets, four enqueues and the read-back
of the table, which waits for the kernels; "events" is the time between two events around the cost entry point and around the
assignment entry point (with the upload of its shapes and offsets), on a batch staged beforehand.  It also prints the largest |x - x64| / (2^-24 A) of the table against the restatement."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

COSTS = dict(cost_class=1.0, cost_bbox=5.0, cost_giou=2.0)
WEIGHTS = {"loss_ce": 1, "loss_bbox": 5, "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1, "loss_giou": 2}


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * float(np.median(xs)), 1e3 * xs[0], 1e3 * xs[-1])


def inputs(B, Q, seed=0, n_logit=19, W=12, n_angle=30):
    rs = np.random.RandomState(seed)
    f = lambda x: np.ascontiguousarray(x, np.float32)
    boxes = lambda n: np.concatenate([rs.uniform(0.15, 0.85, (n, 2)), rs.uniform(0.04, 0.45, (n, 2))], 1)
    out = {"pred_logits": f(rs.normal(0, 2.5, (B, Q, n_logit))), "pred_boxes": f(boxes(B * Q).reshape(B, Q, 4)),
           "pred_angle": f(rs.normal(0, 2, (B, Q, n_angle))), "pred_offset": f(rs.normal(0, 0.1, (B, Q, 2))),
           "pred_size": f(rs.uniform(0.2, 2.0, (B, Q, 3))), "pred_depth": f(rs.uniform(0.5, 5.0, (B, Q, 1)))}
    targets = []
    for n in rs.randint(0, 33, B):
        o = rs.uniform(-1, 1, (n, W))
        o[:, 0] = rs.randint(0, n_logit - 1, n); o[:, 1:5] = boxes(n); o[:, 5:8] = rs.uniform(0.2, 2.0, (n, 3))
        o[:, 8:10] = rs.normal(0, 0.1, (n, 2)); o[:, W - 2] = rs.uniform(0.5, 5.0, n); o[:, W - 1] = rs.randint(0, n_angle, n)
        targets.append({"objects": f(o)})
    return out, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--queries", type=int, default=100)
    a = ap.parse_args()
    import torch
    import criterion_ref as R
    from odam_amd import criterion
    B, Q = a.frames, a.queries
    out, targets = inputs(B, Q)
    d_out = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
    d_tgt = [{"objects": torch.from_numpy(t["objects"]).cuda()} for t in targets]
    crit = criterion.SetCriterion(18, criterion.HungarianMatcher(**COSTS), WEIGHTS, 0.1, list(criterion.LOSS_NAMES))
    got = crit(d_out, d_tgt)      # warm-up: code object load
    wall = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = crit(d_out, d_tgt)
        wall.append(time.perf_counter() - t0)
    # the three entry points alone, between two events
    S = criterion._Staged(d_out, d_tgt)
    devt = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cost, _ = criterion.match_cost(S, **COSTS)
        e1.record()
        torch.cuda.synchronize()
        devt.append(("cost", e0.elapsed_time(e1) * 1e-3))
        shapes, off = [(S.Q, g) for g in S.sizes], S.Q * S.off[:-1]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        criterion.lsap_batch(cost, shapes, cost_off=off, device=S.dev)
        e1.record()
        torch.cuda.synchronize()
        devt.append(("assign", e0.elapsed_time(e1) * 1e-3))
    print("%d frames x %d queries, %d targets in all (%d calls on the device, %d on the host)" % (B, Q, S.n_obj, a.calls, a.host_calls))
    print("  criterion(outputs, targets)        call     %s" % stats(wall))
    for name in ("cost", "assign"):
        print("  %-6s entry point (upload + launch) events   %s" % (name, stats([t for n, t in devt if n == name])))
    # the restatement on the host
    ts = []
    for _ in range(max(a.host_calls, 1)):
        t0 = time.perf_counter()
        idx = R.matcher(out, targets, **COSTS)
        ref = R.criterion(out, targets, idx, 18, 0.1, WEIGHTS)
        ts.append(time.perf_counter() - t0)
    print("  numpy restatement (float64)        host     %s" % stats(ts))
    dev_idx = crit.matcher(d_out, d_tgt)
    same = all(np.array_equal(i.numpy(), ri) and np.array_equal(j.numpy(), rj) for (i, j), (ri, rj) in zip(dev_idx, idx))
    worst = max(R.within(float(v), *ref["table"][k])[1] for k, v in got.items())
    print("  indices equal: %s   largest |x - x64| / (2^-24 A) over the table: %.3f" % (same, worst))


if __name__ == "__main__":
    main()
