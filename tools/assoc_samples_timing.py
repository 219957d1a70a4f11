#!/usr/bin/env python3
"""Time of cutting validation samples on the device (assoc_samples.SceneTable.cut: the plan on the host, one launch) next to the host path
of the same run (SceneTable.cut_host: the same plan, numpy arithmetic, then the upload of the two tensors), and of a whole scene scored
through each (associator.validate_scene against associator.validate fed by cut_host).
   python tools/assoc_samples_timing.py [--objects 44] [--frames 300] [--batch 16] [--calls 20] [--rounds 5]
(a) one batch of `batch` late frames of a synthetic scene (tests/assoc_samples_ref.py: make_table; every object born in the first 30 frames,
    so a late frame has about `objects` tracks): host time of `calls` calls ending in a stream synchronise, per call;
(b) every usable frame of the scene in batches of `batch`: host time of one pass ending in a stream synchronise.
The paths are timed in alternation after a warm-up, `rounds` times; a figure is the median with [min .. max]; no pass mark.  The planning
step (plan(): pure numpy, part of BOTH paths) is timed on its own: it is the part of cut() that does not go away."""
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
    ap.add_argument("--objects", type=int, default=44)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("assoc_samples_timing: no GPU; a CPU run says nothing about these times")
    import assoc_samples_ref as ref
    from odam_amd import assoc_samples, associator, weights
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    table, unmatched = ref.make_table(rs, a.objects, a.frames, p_obs=0.15, last_birth=30)
    scene = assoc_samples.SceneTable(table, unmatched, ref.make_poses(rs, a.frames), (1296, 968), device=dev)
    sync = lambda: torch.cuda.current_stream(torch.device(dev)).synchronize()
    frames = [int(f) for f in np.linspace(a.frames // 2, a.frames - 1, a.batch).astype(int)]
    valid = [p["valid"] for p in scene.plan(frames)]

    def host():
        b = scene.cut_host(frames)
        return b["tracks"].to(dev), b["detections"].to(dev)

    def device():
        b = scene.cut(frames)
        return b["tracks"], b["detections"]
    paths = [("cut_host + upload", host), ("cut (device)", device), ("plan alone", lambda: scene.plan(frames))]
    for _, fn in paths:
        for _ in range(2):
            fn()
        sync()
    h, d = host(), device()
    exact = [c for c in range(79) if c not in (12, 13)]
    assert torch.equal(h[0][:, exact], d[0][:, exact]) and torch.equal(h[1][:, exact], d[1][:, exact])
    times = {name: [] for name, _ in paths}
    for _ in range(a.rounds):
        for name, fn in paths:
            sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / a.calls)
    print("(a) B = %d samples, tracks %s, detections %s; %d track rows, %.2f MB of tracks" %
          (a.batch, [t for t, _ in valid], [n for _, n in valid], sum(t for t, _ in valid), sum(t for t, _ in valid) * 79 * 100 * 4 / 1e6))
    for name, _ in paths:
        print("    %-22s %s per batch" % (name, stats(times[name])))
    print("    cut_host + upload is %.2f x cut; the plan is %.0f %% of cut" %
          (float(np.median(times[paths[0][0]])) / float(np.median(times[paths[1][0]])),
           100 * float(np.median(times[paths[2][0]])) / float(np.median(times[paths[1][0]]))))

    net = associator.Associator({"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                max_tracks=1024, device=dev)
    net.load_state_dict(weights.make_associator_state_dict(2, 8, seed=0))
    usable = scene.usable_frames()

    def validate_host():
        terms = []
        for chunk in scene.batches(usable, a.batch):
            b = scene.cut_host(chunk)
            samples, t0 = [], 0
            for i, (t, n) in enumerate(b["valid_list"]):
                samples.append({"tracks": b["tracks"][t0:t0 + t], "detections": b["detections"][i, :, :n], "match": b["gt_matches"][i]})
                t0 += t
            terms += associator.validate(net, samples, 0.1, len(samples))["loss_terms"]
        return terms

    def validate_device():
        return associator.validate_scene(net, scene, 0.1, batch_size=a.batch, frames=usable)["loss_terms"]
    paths = [("validate <- cut_host", validate_host), ("validate_scene", validate_device)]
    res = {}
    for name, fn in paths:
        res[name] = fn()
        sync()
    print("(b) %d usable frames of %d, %d objects, batches of %d; largest |difference| of a loss term between the paths %.3g" %
          (len(usable), a.frames, a.objects, a.batch, float(np.abs(np.asarray(res[paths[0][0]]) - np.asarray(res[paths[1][0]])).max())))
    times = {name: [] for name, _ in paths}
    scene.plan_seconds = 0.0
    for _ in range(a.rounds):
        for name, fn in paths:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append(time.perf_counter() - t0)
    for name, _ in paths:
        print("    %-22s %s per scene" % (name, stats(times[name])))
    print("    validate <- cut_host is %.2f x validate_scene; planning inside validate_scene: %.3f ms per scene" %
          (float(np.median(times[paths[0][0]])) / float(np.median(times[paths[1][0]])), 1e3 * scene.plan_seconds / a.rounds))
    net.close()
    scene.close()


if __name__ == "__main__":
    main()
