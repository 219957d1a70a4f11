#!/usr/bin/env python3
"""Wall time of the step between odam_detr_postprocess and the association, host path against device path, for N frames
whose post-processed rows [N, Q, 16] are resident on the device (R50, 640 x 480 frames -> 800 x 1066 network input, scene weights):

  host     download of [N, Q, 16], then per frame Detector.select (odam_detr_select) + processor.detection_array, then
           parallel.pack_detections -- ends with the packed block on the host
  device   Detector.select_pack (odam_detr_select_pack, one launch) -- timed to the end of the kernel, and to the packed block's
           arrival on the host (what a world of one downloads; the sharded chain hands the device block to the all-gather)

and the whole detection call around them: detect_resident + the host step against detect_resident_packed + the block's download.
Medians of repeated calls, every timed region ends in a device synchronise.
   python tools/detect_select_timing.py [frames = 256] [calls = 20] [whole-call repeats = 3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from odam_amd import detector, parallel, synth, weights  # noqa: E402
from odam_amd.processor import detection_array  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
whole = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DEV, THR, SIZE = "cuda:0", 0.6, (synth.IMG_W, synth.IMG_H)
K = synth.K_SCANNET
fids = list(range(N))

det = detector.Detector(backbone="resnet50", max_batch=32, device=DEV, n_streams=2)
det.load_state_dict(weights.make_state_dict(seed=0, scene=True))
frames = torch.from_numpy(np.stack(list(synth.make_frames(N, seed=3, sweep=0.5, noise=4)))).to(DEV)      # raw uint8 [N, 480, 640, 3]


def host_step(rows_dev):
    rows = rows_dev.cpu().numpy()
    per = []
    for b in range(rows.shape[0]):
        s = det.select(rows[b], THR, True, det.arch["angle_bins"])
        per.append(detection_array({k: [v] for k, v in s.items()}, 0, fids[b], *SIZE))
    return parallel.pack_detections(per)


def median_ms(fn, n):
    t = []
    for i in range(n + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 2:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), min(t), max(t)


rows_dev = torch.from_numpy(det.detect_resident(frames, SIZE, K)).to(DEV)
hb, hc = host_step(rows_dev)
blk, cnt = det.select_pack(rows_dev, fids, SIZE, THR)
same = np.array_equal(blk.cpu().numpy().view(np.uint32), hb.view(np.uint32)) and np.array_equal(cnt.cpu().numpy(), hc)
print("%d frames, Q = %d; %.1f detections kept per frame; device block == host block: %s" % (N, det.num_queries, float(hc.mean()), same))
fid_dev = det._frame_ids_dev(fids)
out = (blk, cnt)
fmt = "%-58s median %8.3f ms  (min %.3f, max %.3f)  = %.2f us per frame"
for name, fn, n in (
        ("host: download + select + detection_array + pack", lambda: host_step(rows_dev), calls),
        ("device: select_pack, to the end of the kernel", lambda: det.select_pack(rows_dev, fid_dev, SIZE, THR, out=out), calls),
        ("device: select_pack + download of the packed block", lambda: [t.cpu() for t in det.select_pack(rows_dev, fid_dev, SIZE, THR, out=out)], calls),
        ("whole call: detect_resident + host step", lambda: host_step(torch.from_numpy(det.detect_resident(frames, SIZE, K))), whole),
        ("whole call: detect_resident_packed + download of the block", lambda: [t.cpu() for t in det.detect_resident_packed(frames, SIZE, K, fids, SIZE, THR)], whole)):
    if n < 1:
        continue
    med, lo, hi = median_ms(fn, n)
    print(fmt % (name, med, lo, hi, 1e3 * med / N))
det.close()
sys.exit(0 if same else 1)
