"""Detector-forward throughput per backbone at the bench frame (3 x 800 x 1066), and the per-layer table of one ResNet-18/34
forward from a rocprofv3 kernel trace.

  python3 tests/native/perf_backbones.py                       frames/s, batch 32: resnet18 / 34 / 50 x fp32 / bf16
  python3 tests/native/perf_backbones.py --only resnet34 fp32  one configuration (what a profiler run wraps: 2 warm-up + 3 timed forwards)
  python3 tests/native/perf_backbones.py --layers <kernel_trace.csv> resnet34 [B] [nforwards]
                                                               per-launch TFLOP/s of the last forward's backbone (BasicBlock plan:
                                                               stem, then per block conv1, [downsample], conv2 + residual; input_proj)"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W = 800, 1066


def co(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def throughput(backbone, dtype, B=32, warm=2, n=3):
    import torch
    from odam_amd import detector, weights
    det = detector.Detector(backbone=backbone, max_batch=B, dtype=dtype, n_streams=1)
    det.load_state_dict(weights.make_state_dict(backbone=backbone, seed=0))
    img = torch.randn(B, 3, H, W, device="cuda:0")
    for _ in range(warm):
        det(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        det(img)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    det.close()
    return dt


def basic_plan(blocks, B):
    """(name, flops) of the backbone's contraction launches in launch order, then input_proj"""
    H1, W1 = co(H, 7, 2, 3), co(W, 7, 2, 3)
    h, w = co(H1, 3, 2, 1), co(W1, 3, 2, 1)
    seq = [("stem 7x7/2 3->64 (+max-pool)", 2.0 * B * H1 * W1 * 64 * 147)]
    cin = 64
    for l, nb in enumerate(blocks):
        p = 64 << l
        for i in range(nb):
            s = 2 if (i == 0 and l > 0) else 1
            ho, wo = co(h, 3, s, 1), co(w, 3, s, 1)
            M = B * ho * wo
            seq.append((f"layer{l + 1}.{i}.conv1 3x3/{s} {cin}->{p}", 2.0 * M * p * 9 * cin))
            if s != 1 or cin != p:
                seq.append((f"layer{l + 1}.{i}.downsample 1x1/{s} {cin}->{p}", 2.0 * M * p * cin))
            seq.append((f"layer{l + 1}.{i}.conv2 3x3 {p}->{p} +res", 2.0 * M * p * 9 * p))
            cin, h, w = p, ho, wo
    seq.append((f"input_proj 1x1 {cin}->256", 2.0 * B * h * w * 256 * cin))
    return seq


def layers(path, backbone, B, nfwd):
    from odam_amd.weights import RESNET_BLOCKS
    rows = [r for r in csv.DictReader(open(path)) if "conv_gemm" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // nfwd
    last = rows[(nfwd - 1) * per:]
    plan = basic_plan(RESNET_BLOCKS[backbone], B)
    tot_t = tot_f = 0.0
    print(f"{'launch':44s} {'us':>9s} {'TFLOP/s':>8s}  kernel")
    for (name, fl), r in zip(plan, last):
        t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        tot_t += t
        tot_f += fl
        k = r["Kernel_Name"].replace("void odam_cg::", "").replace("(odam_cg::ConvGemmArgs)", "")
        print(f"{name:44s} {t * 1e6:9.1f} {fl / t / 1e12:8.1f}  {k}")
    print(f"{'backbone + input_proj':44s} {tot_t * 1e6:9.1f} {tot_f / tot_t / 1e12:8.1f}  ({len(last)} contraction launches per forward)")


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--layers":
        layers(a[1], a[2], int(a[3]) if len(a) > 3 else 32, int(a[4]) if len(a) > 4 else 5)
    elif a and a[0] == "--only":
        dt = throughput(a[1], a[2])
        print(f"{a[1]} {a[2]} B=32: {dt * 1e3:.2f} ms/forward = {32 / dt:.1f} frames/s", flush=True)
    else:
        for dtype in ("fp32", "bf16"):
            for bb in ("resnet18", "resnet34", "resnet50"):
                dt = throughput(bb, dtype)
                print(f"{bb} {dtype} B=32: {dt * 1e3:.2f} ms/forward = {32 / dt:.1f} frames/s", flush=True)
