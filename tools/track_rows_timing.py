#!/usr/bin/env python3
"""What a fit pass costs before its launch when the tracks' rows stay on the device -- one command for the whole table:

    python tools/track_rows_timing.py [--out track_rows_timing.json]

At both sizes (30 tracks x 40 views; 500 tracks x 256 views: synth.make_scene, so that the fits and the merge have something to do) it
times, in ONE process and alternating inside every round, from the same host list of [n, 82] float64 tracks:
  (a) device     multi_view._device_prelude: the concatenate, the upload, odam_sq_prepare_batch, the read-back, the gather of the packed
                 rows -- optim_process(prelude="device")'s prelude, the baseline: this path is the parent commit's, untouched
  (b) resident   TrackRows.sync of a list that grew by 30 rows (one frame's worth) since the round before, packed() -- the sort and the
                 gather on the device -- and the same prelude from the block
  (c) loaded     a full TrackRows.load of the list, packed() (no kernel), the prelude from the block
  (d) map_scene  pipeline.map_scene (fit -> merge -> fit) with device_prelude and the device merge, without and with resident_rows
each up to a synchronisation, and in processes of its own
  (e) group + gather alone, between device events: N = 128k rows of 500 tracks (one pass), N = 2M rows of 4096 tracks (two passes).
Medians of 10 after 2 warm-ups, with min and max.  What (a) and (b) hand to the fit is asserted equal bit for bit in every round, and the
merged tracks and parameters of the two map_scene runs likewise.  Every step is a process under its own `timeout`, started only if the
one before it ended well."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"30x40": (30, 40), "500x256": (500, 256)}
SORTS = {"128kx500": (128 * 1024, 500), "2Mx4096": (2 * 1024 * 1024, 4096)}
ROUNDS, WARM = 12, 2
NEW_ROWS = 30


def _bits_equal(a, b):
    import numpy as np
    import torch
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def one_size(size):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import multi_view, pipeline, sq, synth
    from odam_amd.processor import OdamProcess
    from odam_amd.track_store import TrackRows
    n, F = SIZES[size]
    sc = synth.make_scene(F + 16, n, seed=1, min_views=F, max_views=F)
    tracks, img_names, P_cws = sc["tracks"], sc["img_names"], sc["P_cws"]
    assert len(tracks) == n and min(len(t) for t in tracks) > ROUNDS + 1
    f = sq.SqFitter("cuda:0", 200)
    grown = lambda i: [t[:len(t) - (ROUNDS - 1) + i] for t in tracks[:NEW_ROWS]] + tracks[NEW_ROWS:]      # round i: 30 rows more than round i - 1
    tail = (img_names, P_cws, sc["img_h"], sc["img_w"], "super_quadric", True, 10)
    from_block = lambda blk: multi_view._prelude_from_rows(blk["rows14"], blk["row_offsets"], *tail, f, check=blk["check"])
    store, other = TrackRows(f), TrackRows(f)
    store.load(grown(-1))
    wall = {"device": [], "resident": [], "loaded": []}
    for i in range(ROUNDS):
        tr = grown(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = multi_view._device_prelude(tr, *tail, f)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        added = store.sync(tr)
        b = from_block(store.packed())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        other.load(tr)
        c = from_block(other.packed())
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert added == NEW_ROWS and store.loads == 1 and store.groupings == i + 1
        for x in (b, c):      # what reaches the fit
            assert a["fit_ids"] == x["fit_ids"] and a["fit_counts"] == x["fit_counts"] and a["classes"] == x["classes"]
            assert all(_bits_equal(a[k], x[k]) for k in ("P", "tgt", "mask", "fit_init"))
        if i >= WARM:
            wall["device"].append((t1 - t0) * 1e3)
            wall["resident"].append((t2 - t1) * 1e3)
            wall["loaded"].append((t3 - t2) * 1e3)
    # (d) the whole back end
    outs = {}
    for key in ("map_scene", "map_scene_resident"):
        wall[key] = []
    for i in range(ROUNDS):
        for key, resident in (("map_scene", False), ("map_scene_resident", True)):
            proc = OdamProcess(None, None, None, None, fitter=f)
            proc.init_sequence(sc["K"], sc["img_h"], sc["img_w"])
            proc.usable_frames, proc.T_wcs, proc.P_cws = img_names, sc["T_wcs"], P_cws
            proc.device_prelude = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[key] = pipeline.map_scene(proc, tracks, resident_rows=resident, device_merge=True)
            torch.cuda.synchronize()
            if i >= WARM:
                wall[key].append((time.perf_counter() - t0) * 1e3)
            if resident:
                assert proc._rows.loads == 1
    x, y = outs["map_scene"], outs["map_scene_resident"]
    assert _bits_equal(x["params"], y["params"]) and len(x["tracks"]) == len(y["tracks"]) and all(_bits_equal(p, q) for p, q in zip(x["tracks"], y["tracks"]))
    f.close()
    out = {"size": size, "tracks": n, "rows": int(sum(len(t) for t in tracks)), "fitted": len(a["fit_ids"]), "merged_tracks": len(x["tracks"])}
    for k, v in wall.items():
        out[f"{k}_ms"] = v
        out[f"median_{k}_ms"] = float(np.median(v))
    print("RESULT " + json.dumps(out), flush=True)


def one_sort(size):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import track_store as ts
    N, T = SORTS[size]
    rs = np.random.RandomState(0)
    tid = rs.randint(0, T, N).astype(np.int32)
    off = np.zeros(T + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(tid, minlength=T))
    d_tid, d_off = torch.from_numpy(tid).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    log = torch.from_numpy(rs.standard_normal((N, 14))).to("cuda:0")
    src = torch.empty(N, device="cuda:0", dtype=torch.int32)
    status = torch.zeros(1, device="cuda:0", dtype=torch.int32)
    out = torch.empty(N, 14, device="cuda:0", dtype=torch.float64)
    evt = {"group": [], "gather": []}
    for i in range(ROUNDS):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        ts.group(d_tid, T, d_off, src_out=src, status=status)
        e[1].record()
        ts.gather14(log, src, out=out)
        e[2].record()
        torch.cuda.synchronize()
        if i >= WARM:
            evt["group"].append(e[0].elapsed_time(e[1]))
            evt["gather"].append(e[1].elapsed_time(e[2]))
    assert int(status.item()) == 0 and np.array_equal(src.cpu().numpy(), np.argsort(tid, kind="stable"))
    res = {"size": size, "rows": N, "tracks": T}
    for k, v in evt.items():
        res[f"{k}_event_ms"] = v
        res[f"median_{k}_event_ms"] = float(np.median(v))
    print("RESULT " + json.dumps(res), flush=True)


def _step(flag, size, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), flag, size]
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:      # nothing more is started on the device after a step that did not end well
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        print(f"step {size} ended with status {r.returncode}: stopping", file=sys.stderr)
        return None, r.returncode or 1
    return json.loads(line[0][len("RESULT "):]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", choices=list(SIZES))
    ap.add_argument("--sort", choices=list(SORTS))
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.size:
        return one_size(a.size)
    if a.sort:
        return one_sort(a.sort)
    rows = []
    span = lambda v: "median %9.3f ms  [%9.3f .. %9.3f]" % (sorted(v)[len(v) // 2] if len(v) % 2 else (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2]) / 2, min(v), max(v))
    for size in SIZES:
        row, rc = _step("--size", size, a.step_timeout)
        if row is None:
            return rc
        rows.append(row)
        print("%s: %d tracks, %d rows, %d fitted, %d merged tracks" % (size, row["tracks"], row["rows"], row["fitted"], row["merged_tracks"]), flush=True)
        for key, text in (("device", "(a) device prelude (concatenate + upload)"), ("resident", "(b) resident, sync of %d new rows" % NEW_ROWS),
                          ("loaded", "(c) resident, full load"), ("map_scene", "(d) map_scene"), ("map_scene_resident", "(d) map_scene, resident rows")):
            print("  %-42s wall %s" % (text, span(row[f"{key}_ms"])), flush=True)
        ok = row["median_resident_ms"] <= max(row["device_ms"])
        print("  (b) / (a) = %.3f, (c) / (a) = %.3f, map_scene resident / default = %.3f; (b) within (a)'s min-max spread or faster: %s" % (
            row["median_resident_ms"] / row["median_device_ms"], row["median_loaded_ms"] / row["median_device_ms"],
            row["median_map_scene_resident_ms"] / row["median_map_scene_ms"], "yes" if ok else "NO"), flush=True)
    for size in SORTS:
        row, rc = _step("--sort", size, a.step_timeout)
        if row is None:
            return rc
        rows.append(row)
        print("(e) %s: %d rows of %d tracks" % (size, row["rows"], row["tracks"]), flush=True)
        for k in ("group", "gather"):
            print("  %-42s events %s" % ("odam_rows_" + ("group" if k == "group" else "gather14"), span(row[f"{k}_event_ms"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
