#!/usr/bin/env python3
"""Time of the IoU tracker (odam_amd/tracker.py over csrc/track_iou.hip): ONE launch over a synthetic posed scene of 1000 frames, next to the
numpy restatement tests/track_iou_ref.py on the same inputs (and equal to it, bit for bit, or this tool says so), and -- for context only --
next to the network path's association time per frame from the latest bench record under profiles/ (with_association.ms_per_frame).
Median of the calls with [min .. max] after a warm-up call; there is no pass mark and this is not a throughput item.
   python tools/track_iou_timing.py [--frames 1000] [--objects 40] [--dets 8] [--calls 10] [--chunk 0]
"call" is the host time of IouTracker.step on device-resident inputs, the 12-byte read-back of the state header included (so it waits for
the kernel); "device" is the time between two events around it on the stream.  --chunk K feeds the scene K frames per call on one state."""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

IMG_W, IMG_H = 1296, 968


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * float(np.median(xs)), 1e3 * xs[0], 1e3 * xs[-1])


def scene(rs, n_frames, n_obj, n_det):
    """objects on a grid, a wandering camera, every object seen in bursts: float32 rows in parallel.pack_detections' layout"""
    side = int(np.ceil(np.sqrt(n_obj)))
    centre = np.stack([(np.arange(n_obj) % side) * 1.5, (np.arange(n_obj) // side) * 1.5, np.zeros(n_obj)], axis=1) + rs.uniform(-0.2, 0.2, (n_obj, 3))
    dims = rs.uniform(0.45, 1.1, (n_obj, 3)); cls = rs.randint(0, 8, n_obj)
    bc = rs.uniform(0.15, 0.85, (n_obj, 2)); bh = rs.uniform(0.05, 0.15, (n_obj, 2)); phase = rs.uniform(0, 6.28, n_obj)
    T = np.tile(np.eye(4), (n_frames, 1, 1))
    t = np.cumsum(rs.normal(0, 0.02, (n_frames, 3)), axis=0) + [3.0, 3.0, 1.5]
    yaw = np.cumsum(rs.normal(0, 0.02, n_frames))
    blk = np.full((n_frames, 30, 15), -1.0, np.float32); cnt = np.zeros(n_frames, np.int32)
    for f in range(n_frames):
        c, s = np.cos(yaw[f]), np.sin(yaw[f])
        T[f, :3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, 0.36, 0.93], [0, -0.93, 0.36]])
        T[f, :3, 3] = t[f]
        vis = rs.permutation(n_obj)[:min(30, rs.poisson(n_det))]
        cnt[f] = len(vis)
        for k, o in enumerate(vis):
            c2 = bc[o] + 0.05 * np.sin(f / 40.0 + phase[o]) + rs.normal(0, 0.006, 2)
            t_co = T[f, :3, :3].T @ (centre[o] + rs.normal(0, 0.02, 3) - T[f, :3, 3])
            blk[f, k] = np.r_[f, cls[o], c2 - bh[o], c2 + bh[o], dims[o] * (1 + rs.normal(0, 0.02, 3)), t_co, 0.0, 1.0, rs.uniform(0.6, 1.0)]
    return blk, cnt, np.arange(n_frames, dtype=np.int32), T


def bench_record():
    best = None
    for p in glob.glob(os.path.join(REPO, "profiles", "r*_bench_line.json")):
        m = re.match(r"r(\d+)_bench_line\.json$", os.path.basename(p))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), p)
    if best is None:
        return None
    try:
        with open(best[1]) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return None

    def find(o):
        if isinstance(o, dict):
            if isinstance(o.get("with_association"), dict) and "ms_per_frame" in o["with_association"]:
                return o["with_association"]
            for v in o.values():
                r = find(v)
                if r is not None:
                    return r
        return None
    w = find(rec)
    return None if w is None else (os.path.relpath(best[1], REPO), w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--dets", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=0)
    a = ap.parse_args()
    import torch
    import track_iou_ref as R
    from odam_amd import sq, tracker
    blk, cnt, fid, T = scene(np.random.RandomState(0), a.frames, a.objects, a.dets)
    t0 = time.perf_counter()
    want = R.run(blk, cnt, fid, T, IMG_W, IMG_H)
    t_ref = time.perf_counter() - t0
    fitter = sq.SqFitter("cuda:0", 10)
    trk = tracker.IouTracker(device="cuda:0", fitter=fitter)
    d = [torch.from_numpy(x).cuda() for x in (blk, cnt, fid, T)]
    step = a.chunk or a.frames

    def run():
        trk.reset()
        parts = [trk.step(d[0][i:i + step], d[1][i:i + step], d[2][i:i + step], d[3][i:i + step], IMG_W, IMG_H) for i in range(0, a.frames, step)]
        return [torch.cat([p[k] for p in parts]) for k in range(3)]
    got = run()      # warm-up: code object load
    same = all(got[k].cpu().numpy().tobytes() == want[k].tobytes() for k in range(3))
    wall, devt = [], []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0 = time.perf_counter()
        e0.record()
        run()
        e1.record()
        wall.append(time.perf_counter() - s0)
        torch.cuda.synchronize()
        devt.append(e0.elapsed_time(e1) * 1e-3)
    print("%d frames, %d detections (%.1f per frame, most %d), %d objects -> %d tracks; %d frames per call; %d calls"
          % (a.frames, int(cnt.sum()), cnt.mean(), int(cnt.max()), a.objects, trk.n_tracks[0], step, a.calls))
    print("  IouTracker.step            call %s   device %s" % (stats(wall), stats(devt)))
    print("  per frame                  call %9.4f ms   device %9.4f ms" % (1e3 * np.median(wall) / a.frames, 1e3 * np.median(devt) / a.frames))
    print("  numpy restatement          %9.3f ms (%9.4f ms per frame)   ids and both IoU outputs equal, bit for bit: %s" % (1e3 * t_ref, 1e3 * t_ref / a.frames, same))
    rec = bench_record()
    if rec is None:
        print("  network path               no bench record with with_association.ms_per_frame under profiles/")
    else:
        print("  network path, for context  %9.4f ms per frame (with_association.ms_per_frame of %s, %s live tracks at its end; another scene, "
              "another rule: not a like-for-like comparison)" % (rec[1]["ms_per_frame"], rec[0], rec[1].get("live_tracks_at_end", "?")))
    fitter.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
