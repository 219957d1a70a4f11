#!/usr/bin/env python3
"""What mapping S scenes in the launches of one buys -- one command for the whole table:

    python tools/map_scenes_timing.py [--out map_scenes_timing.json]

For S in 1, 4, 8 synthetic scenes (synth.make_scene: about 30 objects of 40 views each, different seeds) it times, in ONE process and
alternating inside every round, on process objects made fresh from the same host track lists:
  sequential   S calls of pipeline.map_scene(proc, resident_rows=True), one after the other -- the baseline, the parent commit's path
  again        the same S calls once more in the same round: the spread of the baseline against itself
  batched      ONE pipeline.map_scenes(procs)
each between two synchronisations of the device, host clock.  Medians of 10 after 2 warm-up rounds, with min and max, the per-stage
seconds map_scenes reports (fit1 / merge / fit2), and the launch shape of the batched fit from SqFitter.last_launch.  The parameters
and merged tracks of the two paths are asserted equal bit for bit in every round.  Every S is a process under its own `timeout`,
started only if the one before it ended well."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = (1, 4, 8)
OBJECTS, VIEWS = 30, 40
ROUNDS, WARM = 12, 2


def _bits_equal(a, b):
    import numpy as np
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def one(S):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import pipeline, sq, synth
    from odam_amd.processor import OdamProcess
    scenes = [synth.make_scene(VIEWS + 16, OBJECTS, seed=100 + s, min_views=VIEWS, max_views=VIEWS) for s in range(S)]
    f = sq.SqFitter("cuda:0", 200)

    def procs():
        out = []
        for sc in scenes:
            p = OdamProcess(None, None, None, None, fitter=f)
            p.init_sequence(sc["K"], sc["img_h"], sc["img_w"])
            p.usable_frames, p.T_wcs, p.P_cws = sc["img_names"], sc["T_wcs"], sc["P_cws"]
            p.tracks = sc["tracks"]      # (neither path writes to the rows)
            out.append(p)
        return out

    def sequential():
        ps = procs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [pipeline.map_scene(p, resident_rows=True) for p in ps]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, outs

    wall = {"sequential": [], "again": [], "batched": []}
    stage = {"fit1": [], "merge": [], "fit2": []}
    launch = None
    for i in range(ROUNDS):
        ta, a = sequential()
        ps = procs()
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = pipeline.map_scenes(ps, stages=st)
        torch.cuda.synchronize()
        tb = (time.perf_counter() - t0) * 1e3
        launch = f.last_launch()      # the newest fit: pass 2 of the batch
        tc, _ = sequential()
        assert st["batched"] == list(range(S)), st["single"]
        for x, y in zip(a, b):
            assert _bits_equal(x["params"], y["params"]) and np.array_equal(x["fitted"], y["fitted"]) and len(x["tracks"]) == len(y["tracks"])
            assert all(_bits_equal(p, q) for p, q in zip(x["tracks"], y["tracks"]))
            assert _bits_equal(np.asarray(x["bboxes_qc"]), np.asarray(y["bboxes_qc"]))
        if i >= WARM:
            wall["sequential"].append(ta)
            wall["batched"].append(tb)
            wall["again"].append(tc)
            for k in stage:
                stage[k].append(st[k] * 1e3)
    f.close()
    res = {"scenes": S, "tracks": int(sum(len(sc["tracks"]) for sc in scenes)), "merged_tracks": int(sum(len(x["tracks"]) for x in b)),
           "fitted_pass2": int(sum(int(x["fitted"].sum()) for x in b)), "launch": launch}
    for k, v in list(wall.items()) + [("stage_" + k, v) for k, v in stage.items()]:
        res[f"{k}_ms"] = v
        res[f"median_{k}_ms"] = float(np.median(v))
    print("RESULT " + json.dumps(res), flush=True)


def _step(S, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--scenes", str(S)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:      # nothing more is started on the device after a step that did not end well
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        print(f"S = {S} ended with status {r.returncode}: stopping", file=sys.stderr)
        return None, r.returncode or 1
    return json.loads(line[0][len("RESULT "):]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", type=int, choices=list(SCENES))
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.scenes:
        return one(a.scenes)
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2]) / 2
    span = lambda v: "median %9.3f ms  [%9.3f .. %9.3f]" % (med(v), min(v), max(v))
    rows = []
    for S in SCENES:
        row, rc = _step(S, a.step_timeout)
        if row is None:
            return rc
        rows.append(row)
        print("S = %d: %d tracks -> %d merged, %d fitted in pass 2" % (S, row["tracks"], row["merged_tracks"], row["fitted_pass2"]), flush=True)
        print("  %-34s wall %s" % ("%d x map_scene(resident_rows=True)" % S, span(row["sequential_ms"])), flush=True)
        print("  %-34s wall %s" % ("the same again", span(row["again_ms"])), flush=True)
        print("  %-34s wall %s" % ("map_scenes", span(row["batched_ms"])), flush=True)
        print("  %-34s fit1 %.3f  merge %.3f  fit2 %.3f ms (medians)" % ("  of which", row["median_stage_fit1_ms"], row["median_stage_merge_ms"],
                                                                      row["median_stage_fit2_ms"]), flush=True)
        spread = abs(row["median_again_ms"] - row["median_sequential_ms"])
        diff = row["median_sequential_ms"] - row["median_batched_ms"]
        print("  sequential / batched = %.2f; sequential - batched = %.3f ms against a spread of the baseline against itself of %.3f ms "
              "(medians), %.3f ms (min to max)" % (row["median_sequential_ms"] / row["median_batched_ms"], diff, spread,
                                                  max(row["sequential_ms"] + row["again_ms"]) - min(row["sequential_ms"] + row["again_ms"])), flush=True)
        L = row["launch"]
        print("  batched fit, pass 2: grid %d x %d threads, %d workgroup(s) per object, longest first: %s" % (L["grid"], L["threads"], L["split"],
                                                                                                             L["ordered"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
