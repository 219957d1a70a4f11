"""Threshold, greedy NMS and detection-row packing on the device (odam_detr_select_pack, odam_amd/csrc/det_select.hip) against
the host chain it replaces -- Detector.select (odam_detr_select), processor.detection_array, parallel.pack_detections -- which
is the yardstick everywhere here and not the code under test.  Every comparison is np.array_equal on the float32 block, the
counts and the kept query indices."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEQ_W, SEQ_H = 1296, 968
THR = 0.6


def host_chain(rows, frame_ids, threshold=THR, nms_2d=True, n_bins=30, seq=(SEQ_W, SEQ_H)):
    """[B,Q,16] rows -> (block [B,30,15], count [B], keep [B,30], kept per frame before truncation) through the host path"""
    from odam_amd import _lib, parallel
    from odam_amd.detector import Detector
    from odam_amd.processor import detection_array
    rows = np.ascontiguousarray(rows, np.float32)
    B, Q = rows.shape[:2]
    per_frame, keep, n_all = [], np.full((B, 30), -1, np.int32), []
    for b in range(B):
        s = Detector.select(rows[b], threshold, nms_2d, n_bins)
        per_frame.append(detection_array({k: [v] for k, v in s.items()}, 0, frame_ids[b], *seq))
        idx = np.zeros(max(Q, 1), np.int32)
        n = ctypes.c_int()
        _lib.check(_lib.lib().odam_detr_select(rows[b].ctypes.data_as(_lib.c_float_p), ctypes.c_int(Q), ctypes.c_float(threshold),
                                               ctypes.c_int(int(nms_2d)), idx.ctypes.data_as(_lib.c_int_p), ctypes.byref(n)), "odam_detr_select")
        assert n.value == len(s["scores"])
        keep[b, :min(n.value, 30)] = idx[:min(n.value, 30)]
        n_all.append(n.value)
    blk, cnt = parallel.pack_detections(per_frame)
    return blk, cnt, keep, n_all


def device_chain(det, rows, frame_ids, threshold=THR, nms_2d=True, seq=(SEQ_W, SEQ_H)):
    d = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(DEV)
    blk, cnt, keep = det.select_pack(d, frame_ids, seq, threshold, nms_2d, return_keep=True)
    torch.cuda.synchronize()
    return blk.cpu().numpy(), cnt.cpu().numpy(), keep.cpu().numpy()


def assert_same(got, want, what):
    assert got[0].dtype == np.float32 and got[0].shape == want[0].shape, what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what      # NaN-proof: the bits
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


def clustered(rs, Q, ties=False, all_above=False):
    """one frame as tests/test_detr_oracle.py::test_select_nms_random_clusters_vs_oracle draws them: a few clusters of heavily
    overlapping boxes, near-threshold scores, identical sizes, three classes"""
    n_clu = int(rs.randint(1, 6))
    centres = rs.uniform(-2, 2, (n_clu, 3)).astype(np.float32) + np.array([0, 0, 3], np.float32)
    rows = np.zeros((Q, 16), np.float32)
    which = rs.randint(0, n_clu, Q)
    if ties:
        rows[:, 0] = rs.choice(np.array([0.5, 0.65, 0.7, 0.8, 0.9], np.float32), Q)
    else:
        rows[:, 0] = rs.uniform(0.61 if all_above else 0.3, 1.0, Q).astype(np.float32)
        if not all_above:
            rows[rs.rand(Q) < 0.2, 0] = np.float32(0.6) - np.float32(2e-5)
        rows[:, 0] += np.arange(Q, dtype=np.float32) * np.float32(1e-6)
    rows[:, 1] = rs.randint(0, 3, Q)
    jit = rs.choice([0.0, 0.02, 0.3], Q)[:, None].astype(np.float32)
    t = centres[which] + rs.normal(0, 1, (Q, 3)).astype(np.float32) * jit
    dims = np.abs(rs.normal(0.8, 0.3, (Q, 3))).astype(np.float32) + np.float32(0.05)
    dims[rs.rand(Q) < 0.3] = np.float32(0.7)
    cx, cy = 320 + 100 * t[:, 0], 240 + 100 * t[:, 1]
    hw = 40 + 30 * rs.rand(Q, 2)
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = cx - hw[:, 0], cy - hw[:, 1], cx + hw[:, 0], cy + hw[:, 1]
    rows[:, 6:9] = t
    rows[:, 9] = rs.randint(0, 30, Q)
    rows[:, 10:13] = dims
    return rows


def separated(Q, n_over, score_lo=0.61):
    """`n_over` boxes over the threshold that touch nothing (distinct classes, far apart in space and in the image), the rest below"""
    rows = np.zeros((Q, 16), np.float32)
    rows[:, 0] = 0.2
    rows[:n_over, 0] = np.linspace(0.99, score_lo, n_over, dtype=np.float32)
    rows[:, 1] = np.arange(Q)
    rows[:, 2], rows[:, 3] = 30.0 * np.arange(Q), 5.0
    rows[:, 4], rows[:, 5] = rows[:, 2] + 20.0, 45.0
    rows[:, 6], rows[:, 8] = 4.0 * np.arange(Q), 3.0
    rows[:, 9] = np.arange(Q) % 30
    rows[:, 10:13] = 0.6
    return rows


def _pair_kept(pair):
    """does the host keep the second (lower-scored) row of a two-row frame?"""
    from odam_amd.detector import Detector
    return len(Detector.select(pair, THR, True, 30)["scores"]) == 2


def edge_pairs(kind, where, want_kept):
    """two rows whose IoU sits within a few ulps of the limit -- IoU3D of same-class boxes at 0.25 (`kind` "3d": unit cubes 0.6
    apart, the image boxes disjoint) or IoU2D of different-class boxes at 0.5 ("2d": 100-pixel squares a third apart, the 3-D
    boxes disjoint): the second box's position is moved ulp by ulp (np.nextafter) around the crossing and the first position
    the HOST path decides the wanted way is taken."""
    pair = np.zeros((2, 16), np.float32)
    pair[:, 0] = [0.9, 0.8]
    pair[:, 8] = 3.0
    pair[:, 9] = [4, 17]
    pair[:, 10:13] = 1.0
    if kind == "3d":
        pair[:, 1] = 2
        pair[:, 6] = where
        pair[0, 2:6] = [100 * where, 500, 100 * where + 50, 550]
        pair[1, 2:6] = [100 * where, 700, 100 * where + 50, 750]
        col, start = 6, np.float32(where) + np.float32(0.6)
    else:
        pair[:, 1] = [1, 2]
        pair[:, 6] = [where, where + 50.0]
        pair[:, 2:6] = [where, 10, where + 100, 110]
        col, start = 2, np.float32(where) + np.float32(100.0 / 3.0)
    decisions = {}
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        v = start
        for _ in range(12):
            p = pair.copy()
            p[1, col] = v
            if kind == "2d":
                p[1, 4] = v + np.float32(100.0)
            decisions.setdefault(_pair_kept(p), p)
            v = np.nextafter(v, direction)
    assert set(decisions) == {True, False}, (kind, where, "no decision change within 12 ulps of the crossing")
    return decisions[want_kept]


@pytest.fixture(scope="module")
def det():
    from odam_amd import detector
    return detector.Detector(device=DEV)      # select_pack needs no weights


def test_synthetic_frames_equal_the_host_chain(det):
    """B = 5, Q = 100: a clustered frame, an empty one, one truncated at 30, one with tied scores, one with NaN scores and pairs on
    both sides of the IoU limits -- both nms_2d values."""
    rs = np.random.RandomState(7)
    Q = 100
    # frame 4: rows below the threshold, far from everything; four edge pairs at rows (3, 8), (13, 18), (23, 28), (33, 38) --
    # 3-D kept / suppressed at x = 10 / 20 m, 2-D kept / suppressed at x = 1000 / 2000 px -- and NaN scores: ten on top of a kept
    # box (they would be suppressed, were they candidates) and three on their own (they would be kept)
    f_nan = separated(Q, 0)
    f_nan[:, 6] = -50.0 - f_nan[:, 6]
    f_nan[:, 2], f_nan[:, 4] = -5000.0 - f_nan[:, 2], -5000.0 - f_nan[:, 2] + 20.0
    edge = [edge_pairs("3d", 10.0, True), edge_pairs("3d", 20.0, False), edge_pairs("2d", 1000.0, True), edge_pairs("2d", 2000.0, False)]
    for k, p in enumerate(edge):
        f_nan[10 * k + 3], f_nan[10 * k + 8] = p[0], p[1]
    f_nan[50:60] = f_nan[3]
    f_nan[50:63, 0] = np.nan
    empty = clustered(rs, Q)
    empty[:, 0] = rs.uniform(0.05, 0.6, Q).astype(np.float32)
    empty[0, 0] = np.float32(THR)                              # the threshold itself is not over it
    frames = np.stack([clustered(rs, Q), empty, separated(Q, 40), clustered(rs, Q, ties=True), f_nan])
    fids = [7, 8, 2 ** 24 + 1, 10, 11]
    want = {n2: host_chain(frames, fids, nms_2d=n2) for n2 in (True, False)}
    # preconditions, on the host result
    n_cand = [(frames[b, :, 0] > np.float32(THR)).sum() for b in range(5)]
    assert any(n < c for n, c in zip(want[False][3], n_cand)), "no suppression by the 3-D test"
    assert any(a < b for a, b in zip(want[True][3], want[False][3])), "no suppression by the 2-D test alone"
    assert want[True][3][2] == 40 and want[True][1][2] == 30, "no frame truncated at exactly 30"
    assert want[True][1][1] == 0 and n_cand[1] == 0, "no empty frame"
    assert len(np.unique(frames[3, frames[3, :, 0] > THR, 0])) < n_cand[3] and want[True][1][3] >= 2, "no tied scores"
    kept4 = set(want[True][2][4].tolist())
    assert {3, 8, 13, 23, 28, 33} <= kept4 and not ({18, 38} & kept4) and not (set(range(50, 60)) & kept4), sorted(kept4)
    for n2 in (True, False):
        assert_same(device_chain(det, frames, fids, nms_2d=n2), want[n2], f"nms_2d={n2}")


@pytest.mark.parametrize("Q", [1, 7, 64, 65, 100, 256])
def test_query_counts(det, Q):
    """every lane / slot boundary of the one-wavefront layout: frame 0 as the clustered generator draws it, frame 1 with every
    query over the threshold (Q = 256: all four candidates of every lane in use)"""
    rs = np.random.RandomState(100 + Q)
    frames = np.stack([clustered(rs, Q), clustered(rs, Q, all_above=True)])
    want = host_chain(frames, [3, 4])
    assert (frames[1, :, 0] > THR).all() and want[1][1] >= 1
    assert_same(device_chain(det, frames, [3, 4]), want, Q)
    if Q >= 64:      # and a frame that keeps 30 of Q
        frames = np.stack([separated(Q, min(Q, 250)), separated(Q, 30)])
        want = host_chain(frames, [5, 6])
        assert want[1].tolist() == [30, 30]
        assert_same(device_chain(det, frames, [5, 6]), want, Q)


def test_more_than_256_queries_is_refused(det):
    from odam_amd import _lib
    rows = torch.zeros(1, 257, 16, device=DEV)
    with pytest.raises(_lib.OdamError, match=r"code 3: .*256 queries"):
        det.select_pack(rows, [0], (SEQ_W, SEQ_H), THR)


def test_reference_postprocess_fixture(det, golden):
    """the reference-run postprocess fixture of tests/test_detr_oracle.py::test_select_nms_matches_reference_postprocess through the
    kernel: the host chain's block, and the reference's own keeps (classes and scores in its order)"""
    from test_detr_oracle import KEYS, _rows16
    z = golden("detr_post.npz")
    rows = _rows16({k: z[k] for k in KEYS}, 640, 480)
    B = rows.shape[0]
    want = host_chain(rows, list(range(B)), seq=(640, 480))
    got = device_chain(det, rows, list(range(B)), seq=(640, 480))
    assert_same(got, want, "detr_post.npz")
    for b in range(B):
        n = len(z[f"post{b}_scores"])
        assert 5 < n <= 30 and got[1][b] == n
        assert np.array_equal(got[0][b, :n, 1].astype(np.int64), z[f"post{b}_classes"])
        assert np.allclose(got[0][b, :n, 14], z[f"post{b}_scores"], rtol=1e-6, atol=1e-4)


# ---- the whole path ------------------------------------------------------------------------------------------------------------
SEQ = dict(n=8, h=256, w=320, seed=11)


@pytest.fixture(scope="module")
def scene():
    from odam_amd import detector, synth, weights
    seq = synth.make_sequence(**SEQ)
    d = detector.Detector(backbone="resnet50", max_batch=2, device=DEV, n_streams=2)
    d.load_state_dict(weights.make_state_dict(seed=0, scene=True))
    yield d, seq
    d.close()


def test_detect_resident_packed_and_detect_frames_packed(scene):
    """B = 3 frames at 256 x 320 through the R50 detector in batches of 2 on two streams: detect_resident_packed equals
    pack_detections of the host chain over detect_resident's rows, OdamProcess.detect_frames_packed equals
    pack_detections(detect_frames(...))"""
    from PIL import Image
    from odam_amd import parallel, transforms
    from odam_amd.processor import OdamProcess
    d, seq = scene
    tf = transforms.Transforms(size=SEQ["h"])
    imgs = [Image.fromarray(f) for f in seq["frames"][:3]]
    x = torch.stack([tf(im, None)[0] for im in imgs]).to(DEV)
    assert x.shape == (3, 3, 256, 320)
    fids, size = seq["img_names"][:3], (SEQ["w"], SEQ["h"])
    rows = d.detect_resident(x, size, seq["K"])
    for thr in (0.6, 0.5, 0.4, 0.3, 0.7, 0.8):      # the first threshold at which the host path does real work on these rows
        want = host_chain(rows, fids, threshold=thr, seq=size)
        n_cand = (rows[:, :, 0] > np.float32(thr)).sum(1)
        if any(1 <= n <= 30 for n in want[3]) and any(n < c for n, c in zip(want[3], n_cand)):
            break
    else:
        pytest.fail("no threshold at which the host path keeps 1 .. 30 detections in a frame and suppresses a candidate")
    blk, cnt = d.detect_resident_packed(x, size, seq["K"], fids, size, thr)
    torch.cuda.synchronize()
    assert blk.is_cuda and cnt.is_cuda and blk.shape == (3, 30, 15) and cnt.dtype == torch.int32
    assert np.array_equal(blk.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(cnt.cpu().numpy(), want[1])

    proc = OdamProcess(d, None, tf, None, detect_threshold=thr)
    proc.init_sequence(seq["K"], SEQ["h"], SEQ["w"])
    hb, hc = parallel.pack_detections(proc.detect_frames(imgs, fids))
    assert hc.sum() >= 1
    pb, pc = proc.detect_frames_packed(imgs, fids)
    torch.cuda.synchronize()
    assert pb.is_cuda and np.array_equal(pb.cpu().numpy().view(np.uint32), hb.view(np.uint32)) and np.array_equal(pc.cpu().numpy(), hc)
    with pytest.raises(ValueError, match="one size"):
        proc.detect_frames_packed([imgs[0], imgs[1].resize((300, 200))], fids[:2])


def test_run_scene_with_device_select_is_the_same_chain(scene):
    """pipeline.run_scene over 8 frames, world of one: device_select=True returns the tracks and the fitted parameters and boxes
    of device_select=False, bit for bit"""
    from PIL import Image
    from odam_amd import associator, pipeline, transforms
    from odam_amd.processor import OdamProcess
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import scene_weights
    d, seq = scene
    net = associator.Associator({"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                max_tracks=64, device=DEV)
    net.load_state_dict(scene_weights.make_scene_associator_state_dict(2, 8, seed=0))
    imgs = [Image.fromarray(f) for f in seq["frames"]]
    res = {}
    for flag in (False, True):
        proc = OdamProcess(d, net, transforms.Transforms(size=SEQ["h"]), None)
        proc.init_sequence(seq["K"], SEQ["h"], SEQ["w"])
        out = pipeline.run_scene(proc, SEQ["n"], seq["img_names"], seq["T_wcs"], frames=imgs, device_select=flag)
        res[flag] = {"tracks": [np.asarray(t) for t in proc.tracks], "merged": [np.asarray(t) for t in out["tracks"]],
                     "params": np.asarray(out["params"]), "fitted": np.asarray(out["fitted"]),
                     "qc": np.asarray(out["bboxes_qc"]), "dl": np.asarray(out["bboxes_dl"])}
    a, b = res[False], res[True]
    assert len(a["tracks"]) >= 3 and sum(len(t) for t in a["tracks"]) >= 8 and len(a["params"]) >= 1
    same = lambda u, v: u.shape == v.shape and np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
    for k in ("tracks", "merged"):
        assert len(a[k]) == len(b[k]) and all(same(u, v) for u, v in zip(a[k], b[k])), k
    for k in ("params", "fitted", "qc", "dl"):
        assert same(a[k], b[k]), k
    net.close()
