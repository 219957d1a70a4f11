"""Host side of the device threshold / NMS / row-packing path (odam_detr_select_pack): the angle table the kernel looks up,
torch tensors through parallel.allgather_detections, and the entry's ctypes signature against the header.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO


def _frame_with_bins(bins, n_bins):
    """[n,16] rows, one per angle bin in `bins`: far apart, distinct classes, descending scores -- select keeps all, in order"""
    n = len(bins)
    rows = np.zeros((n, 16), np.float32)
    rows[:, 0] = np.linspace(0.99, 0.7, n, dtype=np.float32)
    rows[:, 1] = np.arange(n)
    rows[:, 2], rows[:, 3] = 200.0 * np.arange(n), 10.0
    rows[:, 4], rows[:, 5] = rows[:, 2] + 50.0, 60.0
    rows[:, 6] = 10.0 * np.arange(n)
    rows[:, 8] = 3.0
    rows[:, 9] = bins
    rows[:, 10:13] = 0.5
    return rows


@pytest.mark.parametrize("n_bins", [30, 12])
def test_sincos_table_is_the_host_paths_columns(n_bins):
    """detector.sincos_table(n_bins)[bin] == columns 12, 13 of processor.detection_array after pack_detections' float32 cast, for
    every bin -- with all bins in one frame and with one detection per frame (numpy's float32 sine must not depend on the length)"""
    from odam_amd import parallel
    from odam_amd.detector import Detector, sincos_table
    from odam_amd.processor import detection_array
    table = sincos_table(n_bins)
    assert table.shape == (n_bins, 2) and table.dtype == np.float32

    def host(bins):
        s = Detector.select(_frame_with_bins(bins, n_bins), 0.6, True, n_bins)
        assert len(s["scores"]) == len(bins)
        blk, cnt = parallel.pack_detections([detection_array({k: [v] for k, v in s.items()}, 0, 5, 640, 480)])
        assert cnt[0] == len(bins)
        return blk[0, :len(bins), 12:14]
    assert np.array_equal(host(np.arange(n_bins)).view(np.uint32), table.view(np.uint32))
    for b in range(n_bins):
        assert np.array_equal(host(np.array([b])).view(np.uint32), table[b:b + 1].view(np.uint32)), b
    assert np.array_equal(host(np.array([3, 3, 0, n_bins - 1])).view(np.uint32), table[[3, 3, 0, n_bins - 1]].view(np.uint32))


def _blocks(n_frames):
    """per-frame rows with 0 .. 3 detections, as tests/test_parallel.py builds them"""
    return [[[float(f), float(k)] + [0.5 * f + k] * 13 + [-1.0] * 64 for k in range(f % 4)] for f in range(n_frames)]


def test_allgather_detections_takes_torch_tensors_world_of_one():
    from odam_amd import parallel
    blk, cnt = parallel.pack_detections(_blocks(7))
    gb, gc = parallel.allgather_detections(torch.from_numpy(blk.copy()), torch.from_numpy(cnt.copy()), 7, "cpu")
    wb, wc = parallel.allgather_detections(blk, cnt, 7, "cpu")
    assert isinstance(gb, np.ndarray) and isinstance(gc, np.ndarray) and gb.dtype == wb.dtype and gc.dtype == wc.dtype
    assert np.array_equal(gb.view(np.uint32), wb.view(np.uint32)) and np.array_equal(gc, wc)


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    from odam_amd import parallel
    n_frames = 11
    s, e = parallel.frame_shard(n_frames, rank, ws)
    blk, cnt = parallel.pack_detections(_blocks(n_frames)[s:e])
    wb, wc = parallel.allgather_detections(blk, cnt, n_frames, "cpu")
    gb, gc = parallel.allgather_detections(torch.from_numpy(blk.copy()), torch.from_numpy(cnt.copy()), n_frames, "cpu")
    full = parallel.pack_detections(_blocks(n_frames))
    ok = isinstance(gb, np.ndarray) and gb.dtype == wb.dtype and gc.dtype == wc.dtype and \
        np.array_equal(gb.view(np.uint32), wb.view(np.uint32)) and np.array_equal(gc, wc) and \
        np.array_equal(gb.view(np.uint32), full[0].view(np.uint32)) and np.array_equal(gc, full[1])
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_allgather_detections_takes_torch_tensors_gloo_world_of_two():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 311) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)], res


C_TO_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float}


def test_select_pack_ctypes_signature_matches_the_header():
    """the argument list detector.py gives ctypes for odam_detr_select_pack is the header's, argument by argument"""
    from odam_amd import _lib, detector
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_detr.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+odam_detr_select_pack\s*\(([^)]*)\)\s*;", txt)
    assert m, "odam_detr_select_pack is not declared in include/odam_detr.h"
    want, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    assert names == ["rows16", "B", "Q", "threshold", "nms_2d", "frame_ids", "seq_w", "seq_h", "sincos", "n_bins", "det_block",
                     "det_count", "keep_idx", "stream"]
    assert detector.SELECT_PACK_ARGTYPES == want
    f = detector._select_pack_entry()
    assert list(f.argtypes) == want and f.restype is ctypes.c_int
    # argument checks come before any device work: a null pointer is code 1, more than 256 queries code 3, each with a message
    assert f(None, 1, 100, 0.6, 1, None, 640.0, 480.0, None, 30, None, None, None, None) == 1
    assert b"odam_detr_select_pack" in _lib.lib().odam_last_error()
    assert f(64, 1, 257, 0.6, 1, 64, 640.0, 480.0, 64, 30, 64, 64, None, None) == 3
    assert b"256" in _lib.lib().odam_last_error()
