#!/usr/bin/env python3
"""What the track merge between the two fit passes costs on the host and on the device -- one command for the table:

    python tools/track_merge_timing.py [--out track_merge_timing.json]

At both sizes (30 tracks x 100 rows over 1,000 images; 500 tracks x 256 rows over 10,000 images, the config-5 scene) it times, as
medians of 5 calls after 1 warm-up each, from the SAME optim_process-like dict of [n, 82] float64 tracks and fitted boxes:
  host      merge.merge_process(data, img_names): the pair costs in numpy, sklearn's clustering, the assembly loops
  host+iou  merge.merge_process(data, img_names, fitter=f): the pair costs from the device, the rest on the host
  device    merge.merge_process(data, img_names, fitter=f, on_device=True): uploads, the IoU launch, the clustering launch, the
            assembly pass, the read-back of offsets / source rows / classes, and the gather of the [n, 82] rows on the host
  packed    merge.merge_packed: the same without the read-back and the host gather (the 14-column rows stay on the device, ready
            for SqFitter.prepare), up to a synchronisation
  cluster / assemble   the launches alone, between device events
and checks that the device's merged tracks equal the host's.  Every size is a process of its own under its own `timeout`, started only
if the one before it ended well.  The wall clock is the host's around the call; nothing is excluded from the device paths."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"30x100": (30, 100, 1000), "500x256": (500, 256, 10000)}


def make_scene(n, F, n_img, seed=0):
    """n tracks of F rows over n_img images; tracks 2 i and 2 i + 1 are fragments of one object (their boxes overlap)"""
    import numpy as np
    sys.path.insert(0, REPO)
    from odam_amd.multi_view import get_3d_box
    rs = np.random.RandomState(seed)

    def rotz(t):
        c, s = np.cos(t), np.sin(t)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    cen = rs.uniform(-4, 4, (n // 2 + 1, 3))
    boxes = [get_3d_box(np.array([1., 1, 1]) + rs.uniform(0, .05, 3), rotz(rs.uniform(-.05, .05)), cen[i // 2] + rs.uniform(-.03, .03, 3))
             for i in range(n)]
    tracks = []
    for i in range(n):
        t = rs.uniform(size=(F, 82))
        t[:, 0] = np.sort(rs.choice(n_img, F, replace=False))
        t[:, 1] = (i // 2) % 8
        tracks.append(t)
    return {"tracks": tracks, "bboxes_qc": boxes}, list(range(n_img))


def one_size(size):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import evaluate, merge, sq
    n, F, n_img = SIZES[size]
    data, names = make_scene(n, F, n_img)
    f = sq.SqFitter("cuda:0", 10)
    paths = {"host": lambda: merge.merge_process(data, names),
             "host+iou": lambda: merge.merge_process(data, names, fitter=f),
             "device": lambda: merge.merge_process(data, names, fitter=f, on_device=True),
             "packed": lambda: merge.merge_packed(data, names, f)}
    wall, last = {k: [] for k in paths}, {}
    for k, fn in paths.items():
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if i >= 1:
                wall[k].append((time.perf_counter() - t0) * 1e3)
    assert last["packed"] is not None
    for k in ("host+iou", "device"):
        assert len(last[k]) == len(last["host"]) and all(np.array_equal(a, b) for a, b in zip(last[k], last["host"])), k
    # the launches alone
    boxes = np.asarray(data["bboxes_qc"], np.float64).reshape(n, 8, 3)
    cls = np.array([int(np.median(t[:, 1])) for t in data["tracks"]], np.int32)
    r = evaluate.iou_scenes([boxes], [boxes], [cls], [cls], gate=2, fitter=f, want_bev=False)
    rows = torch.from_numpy(np.concatenate([t[:, :14] for t in data["tracks"]])).to("cuda:0")
    offs = np.concatenate([[0], np.cumsum([len(t) for t in data["tracks"]])])
    evt = {"cluster": [], "assemble": []}
    for i in range(6):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        cl = f.merge_cluster(r["iou3d"], r["a_off"], r["pair_off"])
        e[1].record()
        f.merge_assemble(cl, r["a_off"], rows, offs, [names])
        e[2].record()
        torch.cuda.synchronize()
        if i >= 1:
            evt["cluster"].append(e[0].elapsed_time(e[1]))
            evt["assemble"].append(e[1].elapsed_time(e[2]))
    f.close()
    out = {"size": size, "tracks": n, "rows_per_track": F, "images": n_img, "merged_tracks": len(last["host"])}
    for k, v in wall.items():
        out[f"{k}_ms"] = v
        out[f"median_{k}_ms"] = float(np.median(v))
    for k, v in evt.items():
        out[f"{k}_event_ms"] = v
        out[f"median_{k}_event_ms"] = float(np.median(v))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", choices=list(SIZES))
    ap.add_argument("--step-timeout", type=int, default=200)
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
        print("%s: %d tracks x %d rows over %d images -> %d merged tracks" % (size, row["tracks"], row["rows_per_track"], row["images"],
                                                                              row["merged_tracks"]), flush=True)
        for k in ("host", "host+iou", "device", "packed"):
            print("  %-9s wall median %9.3f ms  [%9.3f .. %9.3f]" % (k, row[f"median_{k}_ms"], min(row[f"{k}_ms"]), max(row[f"{k}_ms"])), flush=True)
        for k in ("cluster", "assemble"):
            print("  %-9s events median %7.3f ms  [%9.3f .. %9.3f]" % (k, row[f"median_{k}_event_ms"], min(row[f"{k}_event_ms"]),
                                                                       max(row[f"{k}_event_ms"])), flush=True)
        print("  device x %.2f, packed x %.2f of the host path of this run" % (row["median_host_ms"] / row["median_device_ms"],
                                                                             row["median_host_ms"] / row["median_packed_ms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
