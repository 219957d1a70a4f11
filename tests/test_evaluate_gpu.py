"""gfx950 evaluation kernels (odam_amd/csrc/box_iou.hip through odam_amd/evaluate.py, merge.cost_matrix(fitter=...) and the raw entry
points of include/odam_eval.h) against their numpy restatement tests/box_iou_ref.py and the reference-run fixtures box_iou.npz,
eval_match.npz and sq_merge.npz.

What is asked:
  IoU (binary64)   |device - restatement| <= 1e-12 on both outputs -- the bound tests/test_merge.py and tests/test_evaluate_host.py
                   hold the host closed form and the restatement to against the reference; exact zeros where the restatement (and the
                   golden) is zero; NaN for NaN.  The device's binary64 sqrt and division are not taken to be bit-equal, hence a bound.
                   Gated pairs: exactly 0; open pairs: the bits of the gate = 0 launch.
  matching         integers: equal.  The F1 table: 1e-15 relative against the numbers get_f1 printed.
  untouched words  buffers start as sentinels and are 5 rows longer than needed: every word no pair / box / scene owns keeps its sentinel."""
import ctypes

import numpy as np
import pytest

import box_iou_ref as R

pytestmark = pytest.mark.gpu

IOU_TOL = 1e-12
SENT_D, SENT_I = -1234.5, -77


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter("cuda:0", 10)
    yield f
    f.close()


def _d(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offs(scenes_a, scenes_b):
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in scenes_a])]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum([len(x) for x in scenes_b])]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum(np.diff(a_off).astype(np.int64) * np.diff(b_off))]).astype(np.int64)
    return a_off, b_off, pair_off


def _cat(parts, shape, dt):
    parts = [np.asarray(p, dt).reshape((-1,) + shape) for p in parts]
    return np.concatenate(parts + [np.zeros((1,) + shape, dt)])      # one spare row: never an empty tensor's null pointer


def _raw_iou(fitter, scenes_a, scenes_b, cls_a=None, cls_b=None, gate=0, tail=5, bev=True, null_cls=False):
    """odam_box3d_iou_batch on buffers that start as sentinels and are `tail` words longer than the pairs -> rc, iou3d, iou_bev"""
    import torch
    from odam_amd import _lib, evaluate
    a_off, b_off, pair_off = _offs(scenes_a, scenes_b)
    n_pairs = int(pair_off[-1])
    d_A, d_B = _d(_cat(scenes_a, (8, 3), np.float64)), _d(_cat(scenes_b, (8, 3), np.float64))
    d_ca = None if cls_a is None or null_cls else _d(_cat(cls_a, (), np.int32))
    d_cb = None if cls_b is None else _d(_cat(cls_b, (), np.int32))
    o3 = torch.full((n_pairs + tail,), SENT_D, device="cuda", dtype=torch.float64)
    o2 = torch.full((n_pairs + tail,), SENT_D, device="cuda", dtype=torch.float64) if bev else None
    d_ao, d_bo, d_po = _d(a_off), _d(b_off), _d(pair_off)
    rc = evaluate._entry("odam_box3d_iou_batch")(fitter._h, len(scenes_a), _lib.ptr(d_ao), _lib.ptr(d_bo), _lib.ptr(d_po), n_pairs, _lib.ptr(d_A),
                                                 _lib.ptr(d_B), _lib.ptr(d_ca), _lib.ptr(d_cb), gate, _lib.ptr(o3), _lib.ptr(o2), _stream())
    torch.cuda.synchronize()
    return rc, o3.cpu().numpy(), (o2.cpu().numpy() if bev else None)


def _raw_match(fitter, ious, cls_pred, cls_gt, threshold, n_class=8, max_gt=None, tail=5):
    """odam_box3d_match_batch on given IoU blocks ([n_s, m_s] each) -> rc, counts, claimed, gt_match (sentinel tails included)"""
    import torch
    from odam_amd import _lib, evaluate
    a_off, b_off, pair_off = _offs(cls_pred, cls_gt)
    d_iou = _d(_cat([np.asarray(i, np.float64).reshape(-1) for i in ious], (), np.float64))
    d_cp, d_cg = _d(_cat(cls_pred, (), np.int32)), _d(_cat(cls_gt, (), np.int32))
    n_scene = len(ious)
    counts = torch.full((n_scene + tail, 3, n_class), SENT_I, device="cuda", dtype=torch.int32)
    claimed = torch.full((int(a_off[-1]) + tail,), SENT_I, device="cuda", dtype=torch.int32)
    gt_match = torch.full((int(b_off[-1]) + tail,), SENT_I, device="cuda", dtype=torch.int32)
    d_ao, d_bo, d_po = _d(a_off), _d(b_off), _d(pair_off)
    mg = int(np.diff(b_off).max(initial=0)) if max_gt is None else max_gt
    rc = evaluate._entry("odam_box3d_match_batch")(fitter._h, n_scene, _lib.ptr(d_ao), _lib.ptr(d_bo), _lib.ptr(d_po), _lib.ptr(d_iou), _lib.ptr(d_cp),
                                                   _lib.ptr(d_cg), float(threshold), n_class, mg, _lib.ptr(counts), _lib.ptr(claimed),
                                                   _lib.ptr(gt_match), _stream())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), claimed.cpu().numpy(), gt_match.cpu().numpy()


def _close(got, want, what, measured=None, name=None):
    """NaN for NaN, exact zeros where the restatement has them, the bound elsewhere; returns the largest difference"""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok] == 0, want[ok] == 0), what
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print("%s: largest |device - restatement| %.3g over %d values" % (what, err, ok.sum()))
    if measured is not None:
        measured(name, err)
    assert err <= IOU_TOL, (what, err)
    return err


def _random_boxes(rs, k, spread=1.5):
    from odam_amd.multi_view import get_3d_box

    def rotz(t):
        c, s = np.cos(t), np.sin(t)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return np.asarray([get_3d_box(rs.uniform(.4, 2, 3), rotz(rs.uniform(-3, 3)), rs.uniform(-spread, spread, 3) * [1, 1, 0.3])
                       for _ in range(k)]).reshape(k, 8, 3)


# ---- 1. IoU against the restatement and the reference's values ---------------------------------------------------------------------
def test_iou_of_the_512_reference_pairs_in_three_layouts(fitter, golden, measured):
    from odam_amd import evaluate
    z = golden("box_iou.npz")
    A, B = z["A"], z["B"]
    # a row: one box against 512; a column: 512 against one (through the host wrapper: [n, m] device tensors)
    for a, b, what in ((A[:1], B, "1 x 512"), (A, B[:1], "512 x 1")):
        got = evaluate.box3d_iou_matrix(a, b, fitter=fitter)
        w3, w2 = R.iou_scene(a, b)
        assert got["iou3d"].shape == w3.shape and got["iou3d"].is_cuda and got["iou3d"].dtype.is_floating_point
        _close(got["iou3d"].cpu().numpy(), w3, what + " iou3d", measured, "box_iou_vs_restatement")
        _close(got["iou_bev"].cpu().numpy(), w2, what + " iou_bev", measured, "box_iou_vs_restatement")
    # the 512 pairs themselves: the diagonals of 23 x 23 blocks (the last is 6 x 6), all blocks in one launch
    cuts = list(range(0, 512, 23)) + [512]
    sa = [A[i:j] for i, j in zip(cuts[:-1], cuts[1:])]; sb = [B[i:j] for i, j in zip(cuts[:-1], cuts[1:])]
    rc, o3, o2 = _raw_iou(fitter, sa, sb)
    assert rc == 0
    w3, w2, pair_off = R.iou_batch(sa, sb)
    _close(o3[:pair_off[-1]], w3, "23 x 23 blocks iou3d", measured, "box_iou_vs_restatement")
    _close(o2[:pair_off[-1]], w2, "23 x 23 blocks iou_bev", measured, "box_iou_vs_restatement")
    assert (o3[pair_off[-1]:] == SENT_D).all() and (o2[pair_off[-1]:] == SENT_D).all()
    d3 = np.concatenate([np.diag(o3[pair_off[s]:pair_off[s + 1]].reshape(len(sa[s]), -1)) for s in range(len(sa))])
    d2 = np.concatenate([np.diag(o2[pair_off[s]:pair_off[s + 1]].reshape(len(sa[s]), -1)) for s in range(len(sa))])
    e3, e2 = np.abs(d3 - z["iou3d"]).max(), np.abs(d2 - z["iou_bev"]).max()
    print("device vs the reference's box3d_iou on the 512 pairs: 3D %.3g, bev %.3g" % (e3, e2))
    measured("box_iou_vs_reference", max(e3, e2))
    assert e3 <= IOU_TOL and e2 <= IOU_TOL
    assert np.array_equal(d3 == 0, z["iou3d"] == 0) and np.array_equal(d2 == 0, z["iou_bev"] == 0)
    # and each pair as a scene of its own: 512 scenes of 1 x 1
    rc, p3, p2 = _raw_iou(fitter, [a[None] for a in A], [b[None] for b in B])
    assert rc == 0 and np.array_equal(p3[:512], d3) and np.array_equal(p2[:512], d2) and (p3[512:] == SENT_D).all()


# ---- 2. ragged scenes, untouched words ---------------------------------------------------------------------------------------------
def test_ragged_scenes_and_untouched_words(fitter, measured):
    rs = np.random.RandomState(21)
    shapes = [(0, 5), (3, 0), (1, 1), (0, 0), (1, 63), (1, 64), (1, 65), (65, 2), (7, 130)]
    sa = [_random_boxes(rs, n) for n, _ in shapes]; sb = [_random_boxes(rs, m) for _, m in shapes]
    rc, o3, o2 = _raw_iou(fitter, sa, sb)
    assert rc == 0
    w3, w2, pair_off = R.iou_batch(sa, sb)
    n_pairs = int(pair_off[-1])
    assert n_pairs == 1 + 63 + 64 + 65 + 130 + 910 and (w3 > 0.05).sum() > 50
    _close(o3[:n_pairs], w3, "ragged iou3d", measured, "box_iou_vs_restatement")
    _close(o2[:n_pairs], w2, "ragged iou_bev", measured, "box_iou_vs_restatement")
    assert len(o3) == n_pairs + 5 and (o3[n_pairs:] == SENT_D).all() and (o2[n_pairs:] == SENT_D).all()
    # without the bird's-eye output; and one scene alone
    rc, q3, _ = _raw_iou(fitter, sa, sb, bev=False)
    assert rc == 0 and np.array_equal(q3, o3)
    rc, s3, s2 = _raw_iou(fitter, sa[-1:], sb[-1:])
    assert rc == 0 and np.array_equal(s3[:910], o3[n_pairs - 910:n_pairs]) and (s3[910:] == SENT_D).all() and (s2[910:] == SENT_D).all()
    # scenes without a pair, and no scene: ODAM_OK and nothing written
    rc, e3, _ = _raw_iou(fitter, sa[:2], sb[:2])
    assert rc == 0 and (e3 == SENT_D).all()
    rc, e3, _ = _raw_iou(fitter, [], [])
    assert rc == 0 and (e3 == SENT_D).all()


# ---- 3. gates ----------------------------------------------------------------------------------------------------------------------
def test_gates(fitter):
    from odam_amd import _lib
    rs = np.random.RandomState(22)
    shapes = [(9, 70), (0, 3), (40, 5)]
    sa = [_random_boxes(rs, n) for n, _ in shapes]; sb = [_random_boxes(rs, m) for _, m in shapes]
    ca = [rs.randint(0, 8, n) for n, _ in shapes]; cb = [rs.randint(0, 8, m) for _, m in shapes]
    rc, f3, f2 = _raw_iou(fitter, sa, sb, ca, cb, 0)
    assert rc == 0
    n_pairs = 9 * 70 + 40 * 5
    for gate in (1, 2):
        rc, g3, g2 = _raw_iou(fitter, sa, sb, ca, cb, gate)
        assert rc == 0
        op = np.concatenate([R.gate_open(gate, a, b).reshape(-1) for a, b in zip(ca, cb)])
        assert 0 < op.sum() < n_pairs and (f3[:n_pairs][~op] > 0).any()
        assert (g3[:n_pairs][~op] == 0).all() and (g2[:n_pairs][~op] == 0).all() and not np.signbit(g3[:n_pairs][~op]).any()
        assert np.array_equal(g3[:n_pairs][op].view(np.uint64), f3[:n_pairs][op].view(np.uint64))
        assert np.array_equal(g2[:n_pairs][op].view(np.uint64), f2[:n_pairs][op].view(np.uint64))
        assert (g3[n_pairs:] == SENT_D).all()
        w3, _, _ = R.iou_batch(sa, sb, ca, cb, gate)
        assert np.array_equal(w3 == 0, g3[:n_pairs] == 0)
    op1 = np.concatenate([R.gate_open(1, a, b).reshape(-1) for a, b in zip(ca, cb)])
    op2 = np.concatenate([R.gate_open(2, a, b).reshape(-1) for a, b in zip(ca, cb)])
    assert (op2 & ~op1).any()                                # a sofa / chair pair: open under the merge rule only
    # a gate without classes, a gate that does not exist
    for kw in (dict(cls_a=ca, cls_b=cb, gate=1, null_cls=True), dict(gate=2), dict(cls_a=ca, cls_b=cb, gate=3)):
        rc, n3, _ = _raw_iou(fitter, sa, sb, **kw)
        assert rc == 1 and b"odam_box3d_iou_batch" in _lib.lib().odam_last_error() and (n3 == SENT_D).all()


# ---- 4. degenerate inputs ----------------------------------------------------------------------------------------------------------
def test_degenerate_boxes(fitter, golden):
    from odam_amd import evaluate
    z = golden("box_iou.npz")
    A, B = R.degenerate_pairs(z["A"][0], z["B"][0])
    rc, o3, o2 = _raw_iou(fitter, [a[None] for a in A], [b[None] for b in B])
    assert rc == 0
    with np.errstate(all="ignore"):
        w3, w2 = R.iou_pairs(A, B)
    _close(o3[:8], w3, "degenerate iou3d")
    _close(o2[:8], w2, "degenerate iou_bev")
    assert abs(o3[0] - 1) <= IOU_TOL and abs(o2[0] - 1) <= IOU_TOL       # identical boxes
    assert o3[7] == 0 and o2[7] == 0                                     # the clipper wound clockwise: 0, as the reference
    assert np.isnan(w3[[1, 4, 5, 6]]).any()                              # (the cases do contain NaN results)
    # a NaN IoU never matches: the NaN pairs as predictions of the class of their ground truth
    m = evaluate.match_scenes([(A, np.zeros(8, int))], [(B, np.zeros(8, int))], threshold=0.25, fitter=fitter)
    iou = m["iou"][0].cpu().numpy()
    counts, claimed, gt_match = R.match_scene(iou, np.zeros(8, int), np.zeros(8, int), 0.25)
    assert np.array_equal(m["counts"].cpu().numpy()[0], counts) and np.array_equal(m["claimed"].cpu().numpy(), claimed)
    assert np.array_equal(m["gt_match"].cpu().numpy(), gt_match)
    nan_rows = np.isnan(iou).all(axis=1)
    assert nan_rows.any() and (claimed[nan_rows] == 0).all() and claimed[0] >= 1


# ---- 5. matching -------------------------------------------------------------------------------------------------------------------
def _fixture_scenes(z):
    go, po = z["gt_off"], z["pred_off"]
    n = len(go) - 1
    preds = [(z["pred_boxes"][po[s]:po[s + 1]], z["pred_cls"][po[s]:po[s + 1]]) for s in range(n)]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(n)]
    return preds, gts


@pytest.mark.parametrize("t", [0, 1])
def test_matching_equals_the_reference_run(fitter, golden, t):
    from odam_amd import evaluate
    z = golden("eval_match.npz")
    thr = float(z["thresholds"][t])
    preds, gts = _fixture_scenes(z)
    m = evaluate.match_scenes(preds, gts, threshold=thr, fitter=fitter)
    assert m["counts"].dtype.is_floating_point is False and tuple(m["counts"].shape) == (8, 3, 8)
    assert np.array_equal(m["counts"].cpu().numpy(), z["counts"][t])
    assert np.array_equal(m["claimed"].cpu().numpy(), z["claimed"][t]) and np.array_equal(m["gt_match"].cpu().numpy(), z["gt_match"][t])
    ev = z["ref_iou3d"] >= 0
    dev_iou = m["iou3d"].cpu().numpy()
    assert np.abs(dev_iou[ev] - z["ref_iou3d"][ev]).max() <= IOU_TOL and (dev_iou[~ev] == 0).all()
    # the same through evaluate(): result dicts as optim_process returns them
    results = [{"tracks": [np.tile(np.r_[0.0, float(c), np.zeros(80)], (3, 1)) for c in p[1]], "bboxes_qc": list(p[0])} for p in preds]
    e = evaluate.evaluate(results, gts, threshold=thr, fitter=fitter)
    assert np.array_equal(e["counts"], z["counts"][t])
    assert np.array_equal(np.concatenate(e["claimed"]), z["claimed"][t]) and np.array_equal(np.concatenate(e["gt_match"]), z["gt_match"][t])
    got = np.stack([e["precision"], e["recall"], e["f1"]], axis=1)
    assert np.allclose(got, z["f1"][t], rtol=1e-15, atol=0)
    assert np.allclose([e["avg_precision"], e["avg_recall"], e["avg_f1"]], z["f1_avg"][t], rtol=1e-15, atol=0)


def test_matching_lane_stride_classes_and_untouched_words(fitter):
    """65 and 130 same-class ground-truth boxes (the lanes stride), class ids -1 and n_class on both sides, NaN IoUs, scenes without
    predictions or ground truth, random IoU blocks: against the restatement; the tails keep their sentinels"""
    rs = np.random.RandomState(23)
    shapes = [(3, 65), (70, 130), (0, 5), (4, 0), (0, 0), (1, 64), (6, 63)]
    ious = [rs.uniform(0, 1, (n, m)) for n, m in shapes]
    ious[1][rs.uniform(size=ious[1].shape) < 0.05] = np.nan
    cp = [np.zeros(n, int) for n, _ in shapes]; cg = [np.zeros(m, int) for _, m in shapes]
    cp[1] = rs.choice([0, 0, 0, 1, -1, 8], 70); cg[1] = rs.choice([0, 0, 0, 1, -1, 8], 130)
    cp[6] = rs.randint(0, 8, 6); cg[6] = rs.randint(0, 8, 63)
    for thr in (0.7, 0.97):
        rc, counts, claimed, gt_match = _raw_match(fitter, ious, cp, cg, thr)
        assert rc == 0
        wc, wcl, wgm = R.match_batch(ious, cp, cg, thr)
        assert np.array_equal(counts[:len(shapes)], wc) and (counts[len(shapes):] == SENT_I).all()
        assert np.array_equal(claimed[:len(wcl)], wcl) and (claimed[len(wcl):] == SENT_I).all()
        assert np.array_equal(gt_match[:len(wgm)], wgm) and (gt_match[len(wgm):] == SENT_I).all()
    assert wcl.max() >= 2 and (wgm >= 64).any() and (wgm == -1).any()        # several claims by one prediction; predictions past lane 63
    assert wc[1, 0, 0] + wc[1, 0, 1] < 130 and wc[1, 1, 0] + wc[1, 1, 1] < 70      # the ids -1 and 8 are counted nowhere
    # n_class = 1: class 1 is now outside too
    rc, counts, claimed, gt_match = _raw_match(fitter, ious, cp, cg, 0.7, n_class=1)
    wc, wcl, wgm = R.match_batch(ious, cp, cg, 0.7, n_class=1)
    assert rc == 0 and np.array_equal(counts[:len(shapes)], wc) and np.array_equal(claimed[:len(wcl)], wcl) and np.array_equal(gt_match[:len(wgm)], wgm)
    rc, counts, _, _ = _raw_match(fitter, [], [], [], 0.5)
    assert rc == 0 and (counts == SENT_I).all()


def test_matching_limits(fitter):
    from odam_amd import _lib, evaluate
    one = np.zeros((1, 8, 3))
    with pytest.raises(_lib.OdamError, match="4097"):
        evaluate.match_scenes([(one, [0])], [(np.zeros((4097, 8, 3)), np.zeros(4097, int))], fitter=fitter)
    # the entry point's own check, before any launch: nothing is written
    rc, counts, claimed, gt_match = _raw_match(fitter, [np.zeros((1, 2))], [[0]], [[0, 0]], 0.5, max_gt=4097)
    assert rc == 3 and b"4096" in _lib.lib().odam_last_error()      # ODAM_E_LIMIT
    assert (counts == SENT_I).all() and (claimed == SENT_I).all() and (gt_match == SENT_I).all()
    for n_class in (0, 65):
        rc, counts, _, _ = _raw_match(fitter, [np.zeros((1, 2))], [[0]], [[0, 0]], 0.5, n_class=n_class)
        assert rc == 1 and b"n_class" in _lib.lib().odam_last_error() and (counts == SENT_I).all()
    # 4096 boxes of one class is inside the limit: one prediction with IoU above the threshold everywhere claims them all
    iou = np.full((2, 4096), 0.9)
    rc, counts, claimed, gt_match = _raw_match(fitter, [iou], [[0, 0]], [np.zeros(4096, int)], 0.5)
    assert rc == 0 and claimed[:2].tolist() == [4096, 0] and (gt_match[:4096] == 0).all() and counts[0, :, 0].tolist() == [4096, 2, 4096]


# ---- 6. map against map, merge on the device ---------------------------------------------------------------------------------------
def _merge_fixture(golden):
    z = golden("sq_merge.npz")
    tracks = [z[f"track{i}"].copy() for i in range(int(z["n_tracks"]))]
    return z, tracks, {"tracks": tracks, "bboxes_qc": list(z["bboxes_qc"])}


def test_compare_a_map_with_itself(fitter, golden):
    from odam_amd import evaluate
    z, tracks, out = _merge_fixture(golden)
    c = evaluate.compare_maps(out, out, threshold=0.25, fitter=fitter)
    k = len(tracks)
    # every object finds itself; a fragment of the same class that overlaps it may be claimed too (no break), by an earlier object
    iou = c["iou"][0]
    assert iou.shape == (k, k) and np.abs(np.diag(iou) - 1).max() <= IOU_TOL
    assert (c["gt_match"][0] >= 0).all() and c["tps"].sum() == k and c["gts"].sum() == k and c["preds"].sum() == k
    assert c["avg_precision"] == 1 and c["avg_recall"] == 1 and c["avg_f1"] == 1
    assert len(c["matched"]) == k and np.array_equal(c["matched"][:, 1], np.arange(k)) and (c["matched_iou"] > 0.25).all()
    cls = np.array([int(np.median(t[:, 1])) for t in tracks])
    assert np.array_equal(cls[c["matched"][:, 0]], cls)
    # at a threshold no fragment pair reaches, the matching is the identity
    c = evaluate.compare_maps(out, out, threshold=0.999, fitter=fitter)
    assert np.array_equal(c["matched"][:, 0], np.arange(k)) and np.abs(c["matched_iou"] - 1).max() <= IOU_TOL and c["avg_f1"] == 1
    # dropping short tracks from both maps
    c = evaluate.compare_maps(out, out, threshold=0.999, min_views=30, fitter=fitter)
    keep = [i for i, t in enumerate(tracks) if len(t) >= 30]
    assert c["gt_ids"].tolist() == keep and c["matched"][:, 0].tolist() == keep


def test_merge_on_the_device(fitter, golden):
    from odam_amd import merge
    z, tracks, out = _merge_fixture(golden)
    ref = [z[f"merged{i}"] for i in range(int(z["n_merged"]))]
    host = merge.cost_matrix(tracks, out["bboxes_qc"])
    dev = merge.cost_matrix(tracks, out["bboxes_qc"], fitter=fitter)
    print("merge cost, device vs host: %.3g" % np.abs(dev - host).max())
    assert np.abs(dev - host).max() <= IOU_TOL and np.array_equal(dev, dev.T) and (np.diag(dev) == 0).all()
    assert np.array_equal(dev == 1, host == 1) and (host < 1).sum() >= 8
    got = merge.merge_process(out, [int(x) for x in z["img_names"]], fitter=fitter)
    assert len(got) == len(ref) == 5
    for a, b in zip(got, ref):
        assert a.shape == b.shape and np.array_equal(a, b)
