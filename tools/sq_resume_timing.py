#!/usr/bin/env python3
"""What the resumable fit costs the cold path, and what resuming buys -- one command for the whole table:

    python tools/sq_resume_timing.py --parent-lib /path/to/the/parent/commit's/libodam_amd.so [--out sq_resume_timing.json]

At both sizes (30 objects x 40 views; 500 objects x 256 views) it times, as medians of 10 launches after 2 warm-ups each:
  parent      the cold 200-step launch, odam_sq_fit_batch of the PARENT commit's library (ODAM_AMD_LIB, odam_amd/_lib.py)
  cold        the same launch of this tree's library
  parent2     the parent once more (how far the machine drifts between two runs of the same code)
  null_state  the 200 steps through odam_sq_fit_resume with a null state_in
  resumed50   a resumed 50-step launch (state of a 150-step fit)
Every step is a process of its own (one library per process) under its own `timeout`, started only if the one before it ended well --
the two libraries alternate.  A launch is timed with the host clock around fit() between two synchronisations (what a refresh costs
its caller, the read-back of the view counts at 500 objects included) and with device events.
Acceptance (issue "resumable fits", section 4): `cold`'s median lies inside [min, max] of `parent`'s own ten runs, at both sizes."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"30x40": (30, 40), "500x256": (500, 256)}
STEPS = ["parent", "cold", "parent2", "null_state", "resumed50"]


def one_step(step, size):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from odam_amd import sq, synth
    n, F = SIZES[size]
    base = [synth.make_sq_problem(F, 1000 + s) for s in range(10)]
    probs = [base[i % 10] for i in range(n)]
    p0 = np.stack([sq.init_params(p["translate"], p["angle"], p["dims"]) for p in probs])
    tm = [sq.lines_to_targets(p["bbox_lines"]) for p in base]
    dev = "cuda:0"
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    P = up(np.concatenate([base[i % 10]["P"].astype(np.float32).reshape(-1, 12) for i in range(n)]))
    tgt = up(np.concatenate([tm[i % 10][0] for i in range(n)]))
    mask = up(np.concatenate([tm[i % 10][1] for i in range(n)]))
    cls, vc = [p["class_id"] for p in probs], [F] * n
    f = sq.SqFitter(dev, 200)
    kw = dict(n_iters=200, want_points=True)
    if step == "null_state":
        kw["want_state"] = True
    elif step == "resumed50":
        st = f.fit(up(p0), cls, vc, P, tgt, mask, n_iters=150, want_state=True)["state"]
        kw = dict(n_iters=50, want_points=True, want_state=True, state=st)
    d_p0 = up(p0)
    wall, evt = [], []
    for i in range(12):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = f.fit(d_p0, cls, vc, P, tgt, mask, **kw)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= 2:
            wall.append((t1 - t0) * 1e3)
            evt.append(e0.elapsed_time(e1))
    digest = int(out["params"].view(torch.int32).to(torch.int64).sum().item())
    shape = f.last_launch() if hasattr(f, "last_launch") and step not in ("parent", "parent2") else None
    f.close()
    print("RESULT " + json.dumps({"step": step, "size": size, "lib": os.environ.get("ODAM_AMD_LIB", "in-tree"), "wall_ms": wall, "event_ms": evt,
                                  "median_wall_ms": float(np.median(wall)), "median_event_ms": float(np.median(evt)),
                                  "params_digest": digest, "launch": shape}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libodam_amd.so built from the parent commit (without it the parent steps are left out)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--size", choices=list(SIZES))
    ap.add_argument("--step-timeout", type=int, default=150)
    a = ap.parse_args()
    if a.step:
        return one_step(a.step, a.size)
    rows = []
    for size in SIZES:
        for step in STEPS:
            parent = step.startswith("parent")
            if parent and not a.parent_lib:
                continue
            env = dict(os.environ)
            env.pop("ODAM_AMD_LIB", None)
            if parent:
                env["ODAM_AMD_LIB"] = os.path.abspath(a.parent_lib)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--size", size]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:      # nothing more is started on the device after a step that did not end well
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                print(f"step {step} at {size} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode or 1
            rows.append(json.loads(line[0][len("RESULT "):]))
            print("%-10s %-8s wall median %8.3f ms  [%8.3f .. %8.3f]   events median %8.3f ms" % (
                step, size, rows[-1]["median_wall_ms"], min(rows[-1]["wall_ms"]), max(rows[-1]["wall_ms"]), rows[-1]["median_event_ms"]), flush=True)
    by = {(r["step"], r["size"]): r for r in rows}
    verdict = {}
    for size in SIZES:
        c = by[("cold", size)]
        assert c["params_digest"] == by[("null_state", size)]["params_digest"], "the resumable entry with a null state changed the fit"
        if ("parent", size) in by:
            p = by[("parent", size)]
            assert c["params_digest"] == p["params_digest"], "the cold path's results moved"
            verdict[size] = {"cold_median_wall_ms": c["median_wall_ms"], "parent_min_wall_ms": min(p["wall_ms"]), "parent_max_wall_ms": max(p["wall_ms"]),
                             "inside_parent_spread": min(p["wall_ms"]) <= c["median_wall_ms"] <= max(p["wall_ms"]),
                             "not_slower_than_parent_spread": c["median_wall_ms"] <= max(p["wall_ms"])}
        print("%s: resumed 50 steps %.3f ms against cold 200 steps %.3f ms per refresh (x %.2f)" % (
            size, by[("resumed50", size)]["median_wall_ms"], c["median_wall_ms"], c["median_wall_ms"] / by[("resumed50", size)]["median_wall_ms"]))
    print("acceptance:", json.dumps(verdict))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows, "acceptance": verdict}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
