#!/usr/bin/env python3
"""Time of ONE batched association forward (odam_assoc_forward_batch: B samples, padded block, transport and loss in one launch) next to
the two ways of getting B assignments without it: B calls of Associator.assignment(..., sequence=True) (the launch sequence per frame)
and B calls of the default path (the persistent matching kernel per frame).  Neither of the two gives the padding semantics or the loss;
they are what the parent of this feature could do for B samples.
   python tools/assoc_batch_timing.py [--batch 16] [--tracks 42] [--spread 6] [--dets 12] [--calls 30] [--rounds 5]
Track counts are drawn in tracks +- spread (the README quotes 42 live tracks), detections in 1 .. 2 dets - 1.  After a warm-up of every
path the three are timed in alternation, `rounds` times `calls` calls each; a figure is the host time of `calls` calls ending in a
stream synchronise, per call.  Median of the rounds with [min .. max]; no pass mark.  The results of the batch are checked against the
per-sample calls only for being finite: they are different functions of the input wherever a sample has padding rows."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * float(np.median(xs)), 1e3 * xs[0], 1e3 * xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=42)
    ap.add_argument("--spread", type=int, default=6)
    ap.add_argument("--dets", type=int, default=12)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("assoc_batch_timing: no GPU; a CPU run says nothing about these times")
    from make_golden_assoc import make_inputs
    from odam_amd import associator, weights
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    valid = [(int(rs.randint(max(1, a.tracks - a.spread), a.tracks + a.spread + 1)), int(rs.randint(1, min(30, 2 * a.dets - 1) + 1))) for _ in range(a.batch)]
    ins = [make_inputs(T, n, 7000 + i) for i, (T, n) in enumerate(valid)]
    tracks = [torch.from_numpy(tr).to(dev) for tr, _ in ins]
    dets = [torch.from_numpy(de).to(dev) for _, de in ins]
    all_tracks, all_dets = torch.cat(tracks), torch.cat(dets)
    net = associator.Associator({"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                max_tracks=max(256, sum(T for T, _ in valid)), device=dev)
    net.load_state_dict(weights.make_associator_state_dict(2, 8, seed=0))
    sync = lambda: torch.cuda.current_stream(torch.device(dev)).synchronize()

    def batched():
        return net.forward_batch(all_tracks, all_dets, valid)[0]

    def per_sample(sequence):
        return [net.assignment(tracks[i], dets[i], T, n, sequence=sequence) for i, (T, n) in enumerate(valid)]
    paths = [("one batched call", batched), ("B calls, launch sequence", lambda: per_sample(True)), ("B calls, default path", lambda: per_sample(False))]
    for _, fn in paths:      # warm-up: every shape of the timed window, twice
        for _ in range(2):
            out = fn()
        sync()
        outs = [out] if torch.is_tensor(out) else out
        assert all(bool(torch.isfinite(o).all()) for o in outs)
    times = {name: [] for name, _ in paths}
    for _ in range(a.rounds):
        for name, fn in paths:
            sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / a.calls)
    print("B = %d samples, tracks %s, detections %s; padded block %d rows, %d track rows in all" %
          (a.batch, [T for T, _ in valid], [n for _, n in valid], a.batch * (max(T for T, _ in valid) + 30), sum(T for T, _ in valid)))
    for name, _ in paths:
        print("%-28s %s per %d assignments" % (name, stats(times[name]), a.batch))
    b = float(np.median(times[paths[0][0]]))
    for name, _ in paths[1:]:
        print("%-28s %.2f x the batched call" % (name, float(np.median(times[name])) / b))
    net.close()


if __name__ == "__main__":
    main()
