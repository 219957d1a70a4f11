#!/usr/bin/env python3
"""Time of one encoder self-attention launch (odam_op_attention_hd, the detector's launcher and kernel choice) per head width:

   python tools/attention_timing.py [--batch 32 --tokens 850 --configs 256:8 256:4 512:8 --dtypes fp32 bf16 --iters 50]

Q and K sit in one [B L, 2E] buffer and V in [B L, E], as the encoder has them.  One JSON line per (E, heads, dtype): the median
over 5 repeats of the mean time of --iters back-to-back launches (events around each repeat), the repeats' [min, max], and TFLOP/s = 4 B H L^2 d / t
(QK^T and PV, 2 flop per multiply-add)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=850)
    ap.add_argument("--configs", nargs="+", default=["256:8", "256:4", "512:8"], help="hidden_dim:nheads")
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import torch
    from odam_amd import _lib
    L, B = a.tokens, a.batch
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    g = torch.Generator().manual_seed(0)
    for cfg in a.configs:
        E, H = (int(x) for x in cfg.split(":"))
        D = E // H
        for dt in a.dtypes:
            tdt = torch.bfloat16 if dt == "bf16" else torch.float32
            qk = torch.randn(B * L, 2 * E, generator=g).to(tdt).to("cuda:0")
            v = torch.randn(B * L, E, generator=g).to(tdt).to("cuda:0")
            o = torch.empty(B * L, E, dtype=tdt, device="cuda:0")
            launch = lambda: _lib.check(_lib.lib().odam_op_attention_hd(p(qk), 2 * E, p(qk, E), 2 * E, p(v), E, p(o), E, B, H, L, L, D,
                                                                        int(dt == "bf16"), None, st), "attention_hd")
            for _ in range(3):
                launch()
            reps = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                reps.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            us = statistics.median(reps)
            print(json.dumps({"hidden_dim": E, "nheads": H, "head_dim": D, "dtype": dt, "batch": B, "tokens": L,
                              "us_per_launch": round(us, 1), "us_range": [round(min(reps), 1), round(max(reps), 1)],
                              "tflops": round(4.0 * B * H * L * L * D / us / 1e6, 1),
                              "config": _lib.config().get("att.x3" if dt == "fp32" else "att.bf16_mfma")}), flush=True)


if __name__ == "__main__":
    main()
