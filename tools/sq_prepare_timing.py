#!/usr/bin/env python3
"""What the prelude of a fit pass costs on the host and on the device -- one command for the whole table:

    python tools/sq_prepare_timing.py [--out sq_prepare_timing.json]

At every size (30 tracks x 40 views; 500 tracks x 256 views; 16 tracks x 8192 views, where one thread writes eight views and the
ordered sums of a track walk 8192 rows in one lane) it times, as medians of 10 calls after 2 warm-ups each, from the SAME host
list of [n, 82] float64 tracks:
  host     multi_view._host_prelude: _object_constraints per track, averaging_T_wos_batch, init_params, get_3d_box, and the packing
           of the constraint rows in numpy -- what optim_process does before it calls fit
  device   multi_view._device_prelude: one concatenate, the upload, odam_sq_prepare_batch, the read-back of class / counts / status,
           and the gather of the packed rows on the device, up to a synchronisation (a fit would be enqueued behind it instead)
  kernel   the launch alone, between device events
Every size is a process of its own under its own `timeout`, started only if the one before it ended well.  The wall clock is the host's
around the call; nothing is excluded from the device path."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"30x40": (30, 40), "500x256": (500, 256), "16x8192": (16, 8192)}
IMG_H, IMG_W = 480, 640


def make_tracks(n, F, seed=0):
    """n tracks of F rows over F + 16 images (ids unsorted), rows in frame order as association leaves them"""
    import numpy as np
    rs = np.random.RandomState(seed)
    n_img = F + 16
    img_names = rs.permutation(np.arange(100, 100 + n_img)).tolist()
    P_cws = rs.standard_normal((n_img, 3, 4))
    tracks = []
    for _ in range(n):
        t = np.zeros((F, 82))
        t[:, 0] = np.sort(rs.choice(img_names, F, replace=False))
        t[:, 1] = rs.randint(0, 8)
        x0, y0 = rs.uniform(0, 300, F), rs.uniform(0, 200, F)
        t[:, 2:6] = np.stack([x0, y0, x0 + rs.uniform(30, 330, F), y0 + rs.uniform(30, 270, F)], 1)
        t[:, 6:9] = rs.uniform(0.3, 1.5, 3) * rs.uniform(0.9, 1.1, (F, 3))
        t[:, 9:12] = rs.uniform(-3, 3, 3) + 0.1 * rs.standard_normal((F, 3))
        t[:, 12] = rs.uniform(-3, 3) + rs.uniform(-0.5, 0.5, F)
        t[:, 13:] = rs.uniform(size=(F, 69))
        tracks.append(t)
    return tracks, img_names, P_cws


def one_size(size):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import multi_view, sq
    n, F = SIZES[size]
    tracks, img_names, P_cws = make_tracks(n, F)
    f = sq.SqFitter("cuda:0", 200)
    args = (tracks, img_names, P_cws, IMG_H, IMG_W, "super_quadric", True, 10)
    wall = {"host": [], "device": []}
    for i in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = multi_view._host_prelude(*args)
        t1 = time.perf_counter()
        d = multi_view._device_prelude(*args, f)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            wall["host"].append((t1 - t0) * 1e3)
            wall["device"].append((t2 - t1) * 1e3)
    assert d is not None and h["fit_ids"] == d["fit_ids"] and h["fit_counts"] == d["fit_counts"] and h["classes"] == d["classes"]
    for k in ("P", "tgt", "mask"):
        assert np.array_equal(h[k], d[k].cpu().numpy()), k
    # the launch alone
    rows = np.concatenate([t[:, :14] for t in tracks])
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tracks])])
    d_rows, evt = torch.from_numpy(rows).to("cuda:0"), []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f.prepare(d_rows, offs, img_names, P_cws, IMG_H, IMG_W)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            evt.append(e0.elapsed_time(e1))
    f.close()
    print("RESULT " + json.dumps({"size": size, "host_ms": wall["host"], "device_ms": wall["device"], "prepare_event_ms": evt,
                                  "median_host_ms": float(np.median(wall["host"])), "median_device_ms": float(np.median(wall["device"])),
                                  "median_prepare_event_ms": float(np.median(evt)), "fitted": len(h["fit_ids"]), "packed_rows": int(sum(h["fit_counts"]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", choices=list(SIZES))
    ap.add_argument("--step-timeout", type=int, default=150)
    a = ap.parse_args()
    if a.size:
        return one_size(a.size)
    rows = []
    for size in SIZES:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--size", size]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:      # nothing more is started on the device after a step that did not end well
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            print(f"size {size} ended with status {r.returncode}: stopping", file=sys.stderr)
            return r.returncode or 1
        row = json.loads(line[0][len("RESULT "):])
        rows.append(row)
        n = SIZES[size][0]
        for k in ("host", "device"):
            print("%-7s %-8s wall median %8.3f ms  [%8.3f .. %8.3f]   %7.1f us per track" % (
                k, size, row[f"median_{k}_ms"], min(row[f"{k}_ms"]), max(row[f"{k}_ms"]), 1e3 * row[f"median_{k}_ms"] / n), flush=True)
        print("kernel  %-8s events median %7.3f ms  [%8.3f .. %8.3f]   (prepare: uploads of the image tables, launch, read-back)" % (
            size, row["median_prepare_event_ms"], min(row["prepare_event_ms"]), max(row["prepare_event_ms"])), flush=True)
        print("%s: device prelude x %.2f of the host prelude" % (size, row["median_host_ms"] / row["median_device_ms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
