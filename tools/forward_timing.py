#!/usr/bin/env python3
"""Forward wall time of the detector per arithmetic mode, with the per-stage totals of its contraction launches.

   python tools/forward_timing.py --backbone resnet101 --batch 32 --size 800 1066 --dtypes fp32 bf16 mxfp8 [--steps 10 --warmup 3]
                                  [--hidden-dim 512 --nheads 8]

One JSON line per dtype: the median wall time of --steps forwards after --warmup (the stream synchronised around each), then one
profiled forward's totals (Detector.profile_read_stages: stem, layer1 .. layer4, rest = input_proj + transformer projections /
FFN + heads; attention from profile_read_attention).  The profiled forward brackets every launch with events, so its sums are
slightly above the unprofiled wall time's share."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=(800, 1066), metavar=("H", "W"))
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "mxfp8"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden-dim", type=int, default=256, help="transformer width (a multiple of 64 in 128 .. 1024)")
    ap.add_argument("--nheads", type=int, default=8, help="attention heads (head dim hidden_dim / nheads: 32 or 64)")
    a = ap.parse_args()
    import torch
    from odam_amd import detector, weights
    H, W = a.size
    sd = weights.make_state_dict(backbone=a.backbone, hidden=a.hidden_dim, seed=0)
    img = torch.randn(a.batch, 3, H, W, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    for dt in a.dtypes:
        det = detector.Detector(backbone=a.backbone, hidden_dim=a.hidden_dim, nheads=a.nheads, max_batch=a.batch, device="cuda:0",
                                n_streams=1, dtype=dt)
        det.load_state_dict(sd)
        for _ in range(a.warmup):
            det(img)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            det(img)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        det.profile(H, W, True)
        det(img)
        torch.cuda.synchronize()
        stages = det.profile_read_stages(H, W)
        na, ams, afl = det.profile_read_attention(H, W)
        det.profile(H, W, False)
        det.close()
        print(json.dumps({
            "backbone": a.backbone, "hidden_dim": a.hidden_dim, "nheads": a.nheads, "batch": a.batch, "size": [H, W], "dtype": dt,
            "forward_ms_median": round(statistics.median(times), 3), "forward_ms_min": round(min(times), 3),
            "frames_per_s": round(a.batch * 1e3 / statistics.median(times), 1), "steps": a.steps, "warmup": a.warmup,
            "stages": {k: {"launches": n, "ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1) if ms > 0 else 0.0}
                       for k, (n, ms, fl) in stages.items()},
            "attention": {"launches": na, "ms": round(ams, 3), "tflops": round(afl / ams / 1e9, 1) if ams > 0 else 0.0},
        }), flush=True)


if __name__ == "__main__":
    main()
