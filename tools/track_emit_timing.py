#!/usr/bin/env python3
"""What it costs to get the IoU tracker's result into the resident row store, on a synthetic posed scene of 1000 frames
(tools/track_iou_timing.py's generator; the tracker's one launch is made once, before the clock, and is not part of either number):

    python tools/track_emit_timing.py [--frames 1000] [--objects 40] [--dets 8] [--rounds 12]

  (a) host      what OdamProcess._track_frames_iou does after the tracker call -- the detection block and the ids copied back,
                _track_rows per frame, the one-row slices grouped by id and concatenated -- plus TrackRows.load of the result
  (b) device    TrackRows.append_tracked on the block and the ids as they lie on the device (the poses' azimuths are made on the host
                inside the clock), one small copy back
each into an empty store and up to a synchronisation, alternating inside every round; medians with [min .. max] after 2 warm-up
rounds.  The two stores are compared in every round: the same rows per track, every column but 9-12 bit for bit.  There is no pass
mark."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WARM = 2
K = np.array([[1170.0, 0, 648.0], [0, 1170.0, 484.0], [0, 0, 1.0]])


def stats(xs):
    xs = sorted(xs)
    return "%9.3f ms [%9.3f .. %9.3f]" % (float(np.median(xs)), xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--dets", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    import torch
    from track_iou_timing import IMG_H, IMG_W, scene
    from odam_amd import parallel, processor, sq, tracker
    from odam_amd.track_store import TrackRows
    dev = "cuda:0"
    blk, cnt, fid, T = scene(np.random.RandomState(0), a.frames, a.objects, a.dets)
    f = sq.SqFitter(dev, 1)
    trk = tracker.IouTracker(device=dev, fitter=f, max_tracks=4096)
    trk.reset()
    d_blk, d_cnt = torch.from_numpy(blk).to(dev), torch.from_numpy(cnt).to(dev)
    d_ids = trk.step(d_blk, d_cnt, fid, T, IMG_W, IMG_H)[0]
    n_tracks = trk.n_tracks[0]
    proc = processor.OdamProcess(None, None, None, None, fitter=f)
    proc.init_sequence(K, IMG_H, IMG_W)
    host_store, dev_store = TrackRows(f), TrackRows(f)
    wall = {"host": [], "device": []}
    for i in range(a.rounds):
        host_store.reset(); dev_store.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, h_blk, h_cnt = d_ids.cpu().numpy(), d_blk.cpu().numpy(), d_cnt.cpu().numpy()
        add = {}
        for k in range(a.frames):
            nk = int(min(max(int(h_cnt[k]), 0), parallel.MAX_DETS))
            if nk == 0:
                continue
            rows = proc._track_rows(h_blk[k, :nk].astype(np.float64), T[k], with_code=False)
            for d in range(nk):
                if ids[k, d] >= 0:
                    add.setdefault(int(ids[k, d]), []).append(rows[d:d + 1])
        tracks = [np.concatenate(add[t], axis=0) for t in sorted(add)]
        host_store.load(tracks)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        azi = np.array([processor.get_cam_azi(t) for t in T])
        added = dev_store.append_tracked(d_blk, d_cnt, d_ids, T, azi, IMG_W, IMG_H, n_tracks)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert len(tracks) == n_tracks and added == host_store.n_rows and dev_store.lengths == host_store.lengths
        x, y = host_store.packed()["rows14"].cpu().numpy(), dev_store.packed()["rows14"].cpu().numpy()
        cols = [0, 1, 2, 3, 4, 5, 6, 7, 8, 13]
        assert x[:, cols].tobytes() == y[:, cols].tobytes() and np.allclose(x, y, rtol=1e-12, atol=1e-12)
        if i >= WARM:
            wall["host"].append((t1 - t0) * 1e3)
            wall["device"].append((t2 - t1) * 1e3)
    f.close()
    print("%d frames, %d detections, %d rows of %d tracks" % (a.frames, int(np.clip(cnt, 0, 30).sum()), added, n_tracks))
    print("  (a) host rows + TrackRows.load      %s" % stats(wall["host"]))
    print("  (b) TrackRows.append_tracked        %s" % stats(wall["device"]))
    print("  (b) / (a) = %.4f" % (np.median(wall["device"]) / np.median(wall["host"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
