"""gfx950 average-precision kernels (odam_amd/csrc/det_ap.hip through the raw entry point odam_det_ap and odam_amd/evaluate.py)
against their numpy restatement tests/det_ap_ref.py and the reference's own eval_det_cls / voc_ap run tests/golden/eval_ap.npz.

What is asked, against the restatement and against the reference alike:
  ranks, jmax, flags, claims, counts, offsets, tp / fp   integers: equal
  ovmax                 1e-12 (the bound the project holds its IoU forms to); -inf for -inf, NaN for NaN
  rec, prec             2^-52 relative: one division of exact integers
  AP                    n 2^-52 with the class's n: non-negative terms, a sum of at most 1
  untouched words       every buffer starts as a sentinel and is 5 words longer than needed: the words nobody owns keep it, scratch
                        past 2 n_pred + 2 n_gt included"""
import ctypes

import numpy as np
import pytest

import det_ap_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
IOU_TOL = 1e-12
SENT_D, SENT_I = -1234.5, -77
TAIL = 5
OUTS = (("ovmax", "p", np.float64), ("jmax", "p", np.int32), ("rank", "p", np.int32), ("is_tp", "p", np.int32), ("gt_claim", "g", np.int32),
        ("order", "p", np.int32), ("npos", "c", np.int32), ("npred", "c", np.int32), ("cls_off", "c1", np.int32), ("ap", "c", np.float64),
        ("tp", "p", np.int32), ("fp", "p", np.int32), ("rec", "p", np.float64), ("prec", "p", np.float64))


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter("cuda:0", 10)
    yield f
    f.close()


def _d(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.size == 0:      # never an empty tensor's null pointer
        x = np.zeros(1, x.dtype)
    return torch.from_numpy(x).cuda()


def raw(fitter, kind, a, n_class=8, ovthresh=0.25, use07=False, null=()):
    """odam_det_ap on buffers that start as sentinels and are TAIL words longer than owned -> rc, {name: numpy array, "scratch"}.
    `a`: det_ap_ref.det_ap's keyword arguments (numpy); `null`: names passed as null pointers"""
    import torch
    from odam_amd import _lib, evaluate
    n_pred, n_gt = a["n_pred"], a["n_gt"]
    size = {"p": n_pred, "g": n_gt, "c": n_class, "c1": n_class + 1}
    out = {name: torch.full((size[s] + TAIL,), SENT_D if dt is np.float64 else SENT_I, device="cuda",
                            dtype=torch.float64 if dt is np.float64 else torch.int32) for name, s, dt in OUTS}
    scratch = torch.full((2 * n_pred + 2 * n_gt + TAIL,), SENT_I, device="cuda", dtype=torch.int32)
    dt = {"pred_off": np.int32, "gt_off": np.int32, "cls_pred": np.int32, "cls_gt": np.int32, "score": np.float64, "pair_off": np.int64,
          "iou": np.float64, "pred_box": np.float32 if kind >= 2 else np.float64, "gt_box": np.float32 if kind >= 2 else np.float64}
    dev = {k: (None if a.get(k) is None or k in null else _d(np.asarray(a[k], t))) for k, t in dt.items()}
    outs = [None if name in null else out[name] for name, _, _ in OUTS]
    rc = evaluate._entry("odam_det_ap")(
        fitter._h, kind, a["n_image"], n_pred, n_gt, n_class, _lib.ptr(dev["pred_off"]), _lib.ptr(dev["gt_off"]), _lib.ptr(dev["pred_box"]),
        _lib.ptr(dev["gt_box"]), _lib.ptr(dev["cls_pred"]), _lib.ptr(dev["cls_gt"]), _lib.ptr(dev["score"]), _lib.ptr(dev["pair_off"]),
        _lib.ptr(dev["iou"]), int(a.get("n_pairs", 0)), float(ovthresh), int(use07), _lib.ptr(None if "scratch" in null else scratch),
        *[_lib.ptr(o) for o in outs], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = {name: out[name].cpu().numpy() for name, _, _ in OUTS}
    got["scratch"] = scratch.cpu().numpy()
    return rc, got


def untouched(got):
    return all((v == (SENT_D if v.dtype == np.float64 else SENT_I)).all() for v in got.values())


def same_floats(got, want, tol_rel=None, tol_abs=None):
    """NaN for NaN, infinities equal, the bound on the rest; returns the largest difference"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    err = np.abs(got[fin] - want[fin])
    bound = tol_abs if tol_rel is None else tol_rel * np.abs(want[fin])
    assert (err <= bound).all(), (float(err.max()), bound)
    return float(err.max()) if err.size else 0.0


def check(got, r, a, n_class=8, record=None):
    """every output of one call against the restatement's dict `r` (same bounds as against the reference), and the words nobody owns"""
    n_pred, n_gt, tot = a["n_pred"], a["n_gt"], int(r["cls_off"][-1])
    for name in ("jmax", "rank", "is_tp"):
        assert np.array_equal(got[name][:n_pred], R.filled(r[name], SENT_I, np.int32)), name
    assert np.array_equal(got["gt_claim"][:n_gt], R.filled(r["gt_claim"], SENT_I, np.int32))
    e_ov = same_floats(got["ovmax"][:n_pred], R.filled(r["ovmax"], SENT_D, np.float64), tol_abs=IOU_TOL)
    for name in ("npos", "npred"):
        assert np.array_equal(got[name][:n_class], r[name]), name
    assert np.array_equal(got["cls_off"][:n_class + 1], r["cls_off"])
    for name in ("order", "tp", "fp"):
        assert np.array_equal(got[name][:tot], r[name]), name
    e_rec = same_floats(got["rec"][:tot], r["rec"], tol_rel=U)
    e_prec = same_floats(got["prec"][:tot], r["prec"], tol_rel=U)
    assert np.array_equal(np.isnan(got["ap"][:n_class]), np.isnan(r["ap"]))
    ok = ~np.isnan(r["ap"])
    e_ap = np.abs(got["ap"][:n_class][ok] - r["ap"][ok])
    assert (e_ap <= r["npred"][ok] * U).all(), (e_ap, r["npred"][ok] * U)
    # the words nobody owns: past the buffers' owned length, past the last class's curve, and scratch past 2 n_pred + 2 n_gt
    size = {"p": n_pred, "g": n_gt, "c": n_class, "c1": n_class + 1}
    for name, s, dt in OUTS:
        sent = SENT_D if dt is np.float64 else SENT_I
        assert len(got[name]) == size[s] + TAIL and (got[name][size[s]:] == sent).all(), name
        if name in ("order", "tp", "fp", "rec", "prec"):
            assert (got[name][tot:] == sent).all(), name
    assert (got["scratch"][2 * n_pred + 2 * n_gt:] == SENT_I).all()
    worst = max([e_ov, e_rec, e_prec] + e_ap.tolist())
    print("largest |device - restatement|: ovmax %.3g rec %.3g prec %.3g ap %.3g" % (e_ov, e_rec, e_prec, e_ap.max() if e_ap.size else 0))
    if record is not None:
        record("ap_vs_restatement", worst)
    return worst


def cube(ctr, size=1.0):
    """8 corners of an axis-aligned box in the get_3d_box layout (top face 0-3, bottom 4-7)"""
    s = np.asarray(size, np.float64) * np.ones(3)
    return np.asarray(ctr, np.float64) + np.asarray([[x, y, z] for z in (0.5, -0.5) for x, y in ((0.5, 0.5), (0.5, -0.5), (-0.5, -0.5), (-0.5, 0.5))]) * s


def fixture_args(z):
    return dict(n_image=len(z["pred_off"]) - 1, n_pred=len(z["pred_cls"]), n_gt=len(z["gt_cls"]), pred_off=z["pred_off"], gt_off=z["gt_off"],
                pred_box=z["pred_boxes"], gt_box=z["gt_boxes"], cls_pred=z["pred_cls"], cls_gt=z["gt_cls"], score=z["pred_score"])


# ---- 1. the reference's run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use07", [False, True])
@pytest.mark.parametrize("t", [0, 1])
def test_fixture_against_the_reference_and_the_restatement(fitter, golden, measured, t, use07):
    from odam_amd import evaluate
    z = golden("eval_ap.npz")
    a, thr = fixture_args(z), float(z["thresholds"][t])
    rc, got = raw(fitter, 0, a, ovthresh=thr, use07=use07)
    assert rc == 0
    check(got, R.det_ap(0, n_class=8, ovthresh=thr, use_07_metric=use07, **a), a, record=measured)
    # the reference's own numbers
    n, tot = a["n_pred"], int(z["cls_off"][-1])
    assert np.array_equal(got["rank"][:n], z["rank"]) and np.array_equal(got["jmax"][:n], z["jmax"]) and np.array_equal(got["is_tp"][:n], z["is_tp"][t])
    assert np.array_equal(got["tp"][:tot], z["tp"][t]) and np.array_equal(got["fp"][:tot], z["fp"][t])
    assert np.array_equal(got["npos"][:8], z["npos"]) and np.array_equal(got["npred"][:8], z["npred"])
    e = [same_floats(got["ovmax"][:n], z["ovmax"], tol_abs=IOU_TOL), same_floats(got["rec"][:tot], z["rec"][t], tol_rel=U),
         same_floats(got["prec"][:tot], z["prec"][t], tol_rel=U)]
    e_ap = np.abs(got["ap"][:8] - z["ap"][t, int(use07)])
    print("device vs the reference: ovmax %.3g rec %.3g prec %.3g ap %s" % (e[0], e[1], e[2], e_ap))
    measured("ap_vs_reference", max(e + e_ap.tolist()))
    assert (e_ap <= z["npred"] * U).all(), (e_ap, z["npred"] * U)
    # the same through the host functions: lists of arrays, and the reference's dicts
    po, go = z["pred_off"], z["gt_off"]
    preds = [(z["pred_boxes"][po[s]:po[s + 1]], z["pred_cls"][po[s]:po[s + 1]], z["pred_score"][po[s]:po[s + 1]]) for s in range(a["n_image"])]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(a["n_image"])]
    r = evaluate.average_precision(preds, gts, thr, use07, fitter=fitter)
    assert r["ap"].is_cuda and np.array_equal(r["pred_off"], po) and tuple(r["is_tp"].shape) == (n,)
    for name, _, _ in OUTS:
        k = len(r[name])
        assert np.array_equal(r[name].cpu().numpy()[:tot if name in ("order", "tp", "fp", "rec", "prec") else k],
                              got[name][:tot if name in ("order", "tp", "fp", "rec", "prec") else k], equal_nan=True), name
    table = evaluate.ap_table(r)
    assert table["mAP"] == got["ap"][:8].mean() and np.array_equal(table["npos"], z["npos"])
    pred_all = {s: [(int(c), b, float(sc)) for b, c, sc in zip(*p)] for s, p in enumerate(preds)}
    gt_all = {s: [(int(c), b) for b, c in zip(*g)] for s, g in enumerate(gts)}
    rec, prec, ap = evaluate.eval_det(pred_all, gt_all, thr, use07, fitter=fitter)
    for c in range(8):
        o, k = int(z["cls_off"][c]), int(z["npred"][c])
        assert np.array_equal(rec[c], got["rec"][o:o + k]) and np.array_equal(prec[c], got["prec"][o:o + k]) and ap[c] == got["ap"][c]


# ---- 2. wave and chunk edges -----------------------------------------------------------------------------------------------------
def test_wave_and_chunk_edges(fitter, measured):
    """images with 0, 1, 63, 64, 65 predictions of one class; 1 x 130 and 65 x 2 ground truth; empty images between full ones; classes
    of 255, 256, 257 and 513 predictions (the rank tiles and the curve chunks are 256: every carry is crossed); a class without
    predictions (5), one without ground truth (6), none of either (7), ids outside the range (-1, 8, 64)"""
    rs = np.random.RandomState(31)
    preds, gts = [], []

    def image(n_pred, n_gt, c, extra_gt_cls=None):
        g = np.stack([cube([3.0 * j, 0, 0]) for j in range(n_gt)]) if n_gt else np.zeros((0, 8, 3))
        p = np.stack([cube([3.0 * (k % max(n_gt, 1)) + rs.uniform(-0.6, 0.6), rs.uniform(-0.3, 0.3), 0], rs.uniform(0.8, 1.2))
                      for k in range(n_pred)]) if n_pred else np.zeros((0, 8, 3))
        gc = np.full(n_gt, c) if extra_gt_cls is None else np.asarray(extra_gt_cls)
        preds.append((p, np.full(n_pred, c), rs.uniform(0, 1, n_pred))); gts.append((g, gc))
    for n in (0, 1, 63, 64, 65):
        image(n, 3, 0)
        image(0, 0, 0)                           # an empty image between full ones
    image(1, 130, 0); image(65, 2, 0)
    for c, n in ((1, 255), (2, 256), (3, 257), (4, 513)):
        image(n, 4, c)
    image(0, 2, 5)                               # class 5: ground truth only
    image(6, 0, 6)                               # class 6: predictions only
    image(4, 4, 0, extra_gt_cls=[-1, 8, 64, 0])  # ground truth outside the range
    preds[-1] = (preds[-1][0], np.asarray([-1, 8, 0, 64]), preds[-1][2])
    a = R.from_lists(preds, gts)
    assert a["n_pred"] == 0 + 1 + 63 + 64 + 65 + 1 + 65 + 255 + 256 + 257 + 513 + 6 + 4
    r = R.det_ap(0, n_class=8, ovthresh=0.25, **a)
    for use07 in (False, True):
        rc, got = raw(fitter, 0, a, ovthresh=0.25, use07=use07)
        assert rc == 0
        if use07:      # the restatement's curves are the same; only the AP form differs
            r = dict(r, ap=np.asarray([np.nan if r["npos"][c] == 0 else 0.0 if r["npred"][c] == 0 else
                                       R.ap_11point(r["rec"][r["cls_off"][c]:r["cls_off"][c + 1]], r["prec"][r["cls_off"][c]:r["cls_off"][c + 1]])
                                       for c in range(8)]))
        check(got, r, a, record=measured)
    assert r["npred"].tolist() == [260, 255, 256, 257, 513, 0, 6, 0] and r["npos"].tolist() == [3 * 5 + 130 + 2 + 1, 4, 4, 4, 4, 2, 0, 0]
    assert r["ap"][5] == 0 and np.isnan(r["ap"][6]) and np.isnan(r["ap"][7]) and 0 < r["ap"][4] < 1
    assert (np.asarray(r["is_tp"]) == 1).sum() > 20 and (np.asarray(r["is_tp"]) == -1).sum() == 3


# ---- 3. ties and NaN ---------------------------------------------------------------------------------------------------------------
def test_ties_and_nan(fitter):
    nan_box = cube([0, 0, 0]); nan_box[2, 1] = np.nan
    gts = [(np.stack([cube([0, 0, 0]), cube([0, 0, 0]), cube([5, 0, 0])]), [0, 0, 0]),      # two equal boxes: the first wins
           (np.stack([nan_box, cube([0.2, 0, 0])]), [0, 0]),                                  # a NaN IoU never wins
           (np.stack([cube([0, 0, 0]), cube([1, 0, 0])]), [1, 2])]                            # ground truth of other classes only
    preds = [(np.stack([cube([0.1, 0, 0]), cube([0.1, 0, 0]), cube([5.1, 0, 0]), cube([5.1, 0, 0])]), [0, 0, 0, 0], [0.5, 0.5, np.nan, 0.5]),
             (np.stack([cube([0, 0, 0]), cube([0, 0, 0])]), [0, 0], [np.nan, 0.9]),
             (np.stack([cube([0, 0, 0])]), [0], [0.7])]
    a = R.from_lists(preds, gts)
    r = R.det_ap(0, n_class=8, ovthresh=0.25, **a)
    rc, got = raw(fitter, 0, a)
    assert rc == 0
    check(got, r, a)
    # ranks: 0.9 (5), 0.7 (6), then the three 0.5 in input order (0, 1, 3), then the NaN scores in input order (2, 4)
    assert got["order"][:7].tolist() == [5, 6, 0, 1, 3, 2, 4] and got["rank"][:7].tolist() == [2, 3, 5, 4, 6, 0, 1]
    assert got["jmax"][:7].tolist() == [0, 0, 2, 2, 1, 1, -1]             # equal maxima: box 0, not 1; the NaN box never
    assert got["is_tp"][:7].tolist() == [1, 0, 0, 1, 0, 1, 0]             # prediction 3 (0.5) ranks before 2 (NaN) on box 2
    assert got["gt_claim"][:7].tolist() == [0, -1, 3, -1, 5, -1, -1]
    assert got["ovmax"][6] == -np.inf and got["ovmax"][0] > 0.8
    rc2, again = raw(fitter, 0, a)                                        # the same input, the same words
    assert rc2 == 0 and all(np.array_equal(got[k], again[k], equal_nan=True) for k in got if k != "scratch")


# ---- 4. contested boxes ------------------------------------------------------------------------------------------------------------
def test_ten_predictions_on_one_box(fitter):
    rs = np.random.RandomState(33)
    sc = rs.permutation(10) / 10.0 + 0.05
    preds = [(np.stack([cube([0.02 * k, 0, 0]) for k in range(10)]), [3] * 10, sc)]
    gts = [(np.stack([cube([0, 0, 0]), cube([4, 0, 0])]), [3, 3])]
    a = R.from_lists(preds, gts)
    rc, got = raw(fitter, 0, a, ovthresh=0.5)
    assert rc == 0
    check(got, R.det_ap(0, n_class=8, ovthresh=0.5, **a), a)
    first = int(np.argmax(sc))
    assert (got["jmax"][:10] == 0).all() and (got["ovmax"][:10] > 0.5).all()
    assert got["is_tp"][:10].tolist() == [int(k == first) for k in range(10)] and got["gt_claim"][:2].tolist() == [first, -1]
    assert got["tp"][:10].tolist() == [1] * 10 and got["fp"][:10].tolist() == list(range(10)) and got["ap"][3] == 0.5


# ---- 5. kind 1: the oriented-box IoU ------------------------------------------------------------------------------------------------
def test_overlap_read_from_the_oriented_iou_launch(fitter, golden):
    from odam_amd import evaluate
    z = golden("eval_ap.npz")
    a = fixture_args(z)
    po, go = z["pred_off"], z["gt_off"]
    n_image = a["n_image"]
    preds = [(z["pred_boxes"][po[s]:po[s + 1]], z["pred_cls"][po[s]:po[s + 1]], z["pred_score"][po[s]:po[s + 1]]) for s in range(n_image)]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(n_image)]
    ious = evaluate.iou_scenes([p[0] for p in preds], [g[0] for g in gts], [p[1] for p in preds], [g[1] for g in gts], gate=1, fitter=fitter, want_bev=False)
    b = dict(a, pred_box=None, gt_box=None, pair_off=ious["pair_off"], iou=ious["iou3d"].cpu().numpy(), n_pairs=int(ious["pair_off"][-1]))
    want = R.det_ap(1, n_class=8, ovthresh=0.25, **b)
    rc, got = raw(fitter, 1, b)
    assert rc == 0
    check(got, want, b)
    assert np.array_equal(got["ovmax"][:a["n_pred"]], R.filled(want["ovmax"], SENT_D, np.float64))      # read, not computed: the same bits
    r = evaluate.average_precision(preds, gts, 0.25, iou="obb", fitter=fitter)
    for name in ("ovmax", "jmax", "rank", "is_tp", "gt_claim", "ap", "npos", "npred"):
        assert np.array_equal(r[name].cpu().numpy(), got[name][:len(r[name])], equal_nan=True), name
    # axis-aligned boxes: the oriented IoU is the axis-aligned one, so both kinds give the same answers
    rs = np.random.RandomState(35)
    gts = [(np.stack([cube([2.5 * j, 0, 0], [1, 1.5, 0.8]) for j in range(m)]) if m else np.zeros((0, 8, 3)), rs.randint(0, 3, m)) for m in (4, 0, 7)]
    preds = []
    for g, gc in gts:
        k = len(gc) + 2
        ctr = [[2.5 * (j % max(len(gc), 1)) + rs.choice([-0.45, -0.1, 0.1, 0.45]), 0, 0] for j in range(k)]
        pc = np.asarray([gc[j % len(gc)] if len(gc) and j != 1 else rs.randint(0, 3) for j in range(k)])      # its box's class, but for one
        preds.append((np.stack([cube(c, [1, 1.5, 0.8]) for c in ctr]), pc, rs.uniform(0, 1, k)))
    r0 = evaluate.average_precision(preds, gts, 0.4, fitter=fitter)
    r1 = evaluate.average_precision(preds, gts, 0.4, iou="obb", fitter=fitter)
    for name in ("jmax", "rank", "is_tp", "gt_claim", "tp", "fp", "npos", "npred", "cls_off"):
        assert np.array_equal(r0[name].cpu().numpy()[:int(r0["cls_off"][-1]) if name in ("tp", "fp") else None],
                              r1[name].cpu().numpy()[:int(r0["cls_off"][-1]) if name in ("tp", "fp") else None]), name
    same_floats(r1["ovmax"].cpu().numpy(), r0["ovmax"].cpu().numpy(), tol_abs=IOU_TOL)
    assert np.array_equal(r0["ap"].cpu().numpy(), r1["ap"].cpu().numpy(), equal_nan=True) and (r0["is_tp"] == 1).sum() >= 3


# ---- 6. kinds 2, 3: detection rows ---------------------------------------------------------------------------------------------------
def synthetic_blocks(seed=37, F=5, counts_a=(30, 0, 7, 12, 1), counts_b=(30, 5, 0, 12, 3)):
    """two [F, 30, 15] blocks as odam_detr_select_pack writes them: run B is run A perturbed, with rows dropped, added and relabelled;
    the slots past a frame's count hold garbage that is not -1: rows that look valid, huge numbers, NaN"""
    rs = np.random.RandomState(seed)

    def rows(n):
        x = np.zeros((n, 15), np.float32)
        x[:, 1] = rs.randint(0, 8, n)
        x[:, 2:4] = rs.uniform(0, 0.6, (n, 2)); x[:, 4:6] = x[:, 2:4] + rs.uniform(0.1, 0.4, (n, 2))
        x[:, 6:9] = rs.uniform(0.3, 1.5, (n, 3)); x[:, 9:12] = rs.uniform(-3, 3, (n, 3))
        x[:, 12:14] = rs.uniform(-1, 1, (n, 2)); x[:, 14] = rs.uniform(0.3, 1.0, n)
        return x
    A = np.zeros((F, 30, 15), np.float32); B = np.zeros((F, 30, 15), np.float32)
    for f in range(F):
        a = rows(30); a[:, 0] = f
        b = a.copy()
        b[:, 2:6] += rs.normal(0, 0.02, (30, 4)).astype(np.float32); b[:, 6:12] += rs.normal(0, 0.05, (30, 6)).astype(np.float32)
        b[:, 14] = rs.uniform(0.3, 1.0, 30)
        b[rs.uniform(size=30) < 0.15, 1] = 7                      # relabelled
        b = b[rs.permutation(30)]
        A[f], B[f] = a, b
        for blk, cnt in ((A, counts_a[f]), (B, counts_b[f])):      # garbage past the count
            tail = blk[f, cnt:]
            tail[0::3] = rows(len(tail[0::3])); tail[1::3] = 1e30; tail[2::3] = np.nan
    return A, np.asarray(counts_a, np.int32), B, np.asarray(counts_b, np.int32)


@pytest.mark.parametrize("iou,kind", [("aabb3d", 2), ("box2d", 3)])
def test_detection_blocks(fitter, measured, iou, kind):
    import torch
    from odam_amd import evaluate
    A, ca, B, cb = synthetic_blocks()
    F = len(ca)
    a = dict(n_image=F, n_pred=30 * F, n_gt=30 * F, pred_off=ca, gt_off=cb, pred_box=A, gt_box=B)
    want = R.det_ap(kind, n_class=8, ovthresh=0.25, **a)
    rc, got = raw(fitter, kind, a)
    assert rc == 0
    check(got, want, a, record=measured)
    owned = np.concatenate([np.arange(30) < c for c in ca])
    assert (got["rank"][:30 * F][~owned] == SENT_I).all() and (got["ovmax"][:30 * F][~owned] == SENT_D).all()      # slots past the counts: nothing
    assert (got["rank"][:30 * F][owned] >= 0).all() and (got["gt_claim"][:30 * F][np.concatenate([np.arange(30) < c for c in cb])] >= -1).all()
    assert (np.asarray(want["is_tp"])[owned] == 1).sum() >= 10 and int(want["npred"].sum()) == int(ca.sum()) and int(want["npos"].sum()) == int(cb.sum())
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    dca, dcb = torch.from_numpy(ca).cuda(), torch.from_numpy(cb).cuda()
    t = evaluate.detections_ap(dA, dca, dB, dcb, iou=iou, fitter=fitter)
    assert np.array_equal(t["ap"], got["ap"][:8], equal_nan=True) and np.array_equal(t["npos"], want["npos"]) and np.array_equal(t["npred"], want["npred"])
    assert t["device"]["is_tp"].is_cuda and np.array_equal(t["device"]["is_tp"].cpu().numpy()[owned], got["is_tp"][:30 * F][owned])
    # a run against itself: every class with detections has AP exactly 1, in either metric of the box
    t = evaluate.detections_ap(dA, dca, dA, dca, iou=iou, fitter=fitter)
    assert (t["ap"][t["npred"] > 0] == 1.0).all() and np.isnan(t["ap"][t["npred"] == 0]).all() and t["mAP"] == 1.0
    # a count the block cannot have owns no slot; no frames at all
    bad = ca.copy(); bad[0] = 31; bad[2] = -1
    a2 = dict(a, pred_off=bad)
    rc, got2 = raw(fitter, kind, a2)
    assert rc == 0
    check(got2, R.det_ap(kind, n_class=8, ovthresh=0.25, **a2), a2)
    assert (got2["rank"][:30] == SENT_I).all() and (got2["rank"][60:90] == SENT_I).all()
    t = evaluate.detections_ap(dA[:0], dca[:0], dB[:0], dcb[:0], iou=iou, fitter=fitter)
    assert np.isnan(t["ap"]).all() and (t["npred"] == 0).all() and np.isnan(t["mAP"])


def test_a_detector_run_against_itself():
    """OdamProcess.detections_ap with a block from detect_frames_packed against itself: every class with detections has AP exactly 1"""
    import torch
    from PIL import Image
    from odam_amd import detector, synth, transforms, weights
    from odam_amd.processor import OdamProcess
    seq = synth.make_sequence(n=8, h=256, w=320, seed=11)      # the sequence tests/test_select_pack_gpu.py detects on
    d = detector.Detector(backbone="resnet50", max_batch=2, device="cuda:0", n_streams=1)
    try:
        d.load_state_dict(weights.make_state_dict(seed=0, scene=True))
        proc = OdamProcess(d, None, transforms.Transforms(size=256), None, detect_threshold=0.3)
        proc.init_sequence(seq["K"], 256, 320)
        blk, cnt = proc.detect_frames_packed([Image.fromarray(f) for f in seq["frames"][:3]], seq["img_names"][:3])
        for iou in ("aabb3d", "box2d"):
            t = proc.detections_ap(blk, cnt, blk, cnt, iou=iou)
            n = int(cnt.sum().item())
            assert n >= 1 and int(t["npred"].sum()) == n and np.array_equal(t["npred"], t["npos"])
            assert (t["ap"][t["npred"] > 0] == 1.0).all() and t["mAP"] == 1.0, t
            assert int((t["device"]["is_tp"] == 1).sum().item()) == n
    finally:
        d.close()


def test_maps_through_the_host_functions(fitter, golden):
    """evaluate_ap / compare_maps_ap / OdamProcess.evaluate_ap on result dicts as optim_process returns them: the fixture's scenes with
    the scores in track column 13, and the merge fixture's map against itself"""
    from odam_amd import evaluate
    from odam_amd.processor import OdamProcess
    z = golden("eval_ap.npz")
    po, go = z["pred_off"], z["gt_off"]
    n_image = len(po) - 1

    def track(c, score):
        t = np.zeros((1, 82)); t[:, 1] = c; t[:, 13] = score      # one view: the mean of its scores is the score itself, bit for bit
        return t
    results = [{"tracks": [track(z["pred_cls"][d], z["pred_score"][d]) for d in range(po[s], po[s + 1])],
                "bboxes_qc": list(z["pred_boxes"][po[s]:po[s + 1]])} for s in range(n_image)]
    gts = [(z["gt_boxes"][go[s]:go[s + 1]], z["gt_cls"][go[s]:go[s + 1]]) for s in range(n_image)]
    assert np.array_equal(np.concatenate([evaluate.prediction_scores(r) for r in results]), z["pred_score"])
    e = evaluate.evaluate_ap(results, gts, 0.25, fitter=fitter)
    assert (np.abs(e["ap"] - z["ap"][0, 0]) <= z["npred"] * U).all() and np.array_equal(e["npos"], z["npos"]) and np.array_equal(e["npred"], z["npred"])
    assert np.array_equal(np.concatenate(e["is_tp"]), z["is_tp"][0]) and abs(e["mAP"] - z["ap"][0, 0].mean()) <= 116 * U
    for s in range(n_image):      # a claimed box names a true positive of its own scene
        c = e["gt_claim"][s]
        assert len(c) == go[s + 1] - go[s] and (e["is_tp"][s][c[c >= 0]] == 1).all()
    for c in range(8):
        o, k = int(z["cls_off"][c]), int(z["npred"][c])
        assert np.allclose(e["rec"][c], z["rec"][0, o:o + k], rtol=U, atol=0) and np.allclose(e["prec"][c], z["prec"][0, o:o + k], rtol=U, atol=0)
    # one scene through the processor
    proc = OdamProcess(None, None, None, None, fitter=fitter)
    one = proc.evaluate_ap(results[2], gts[2][0], gts[2][1], ovthresh=0.5, use_07_metric=True)
    want = R.det_ap(0, n_class=8, ovthresh=0.5, use_07_metric=True,
                    **R.from_lists([(z["pred_boxes"][po[2]:po[3]], z["pred_cls"][po[2]:po[3]], z["pred_score"][po[2]:po[3]])], [gts[2]]))
    assert np.array_equal(one["is_tp"][0], np.asarray(want["is_tp"])) and np.array_equal(np.isnan(one["ap"]), np.isnan(want["ap"]))
    assert (np.abs(one["ap"] - want["ap"])[~np.isnan(want["ap"])] <= 11 * U).all()
    # a map against itself: every object finds itself, so every class it has scores exactly 1
    m = golden("sq_merge.npz")
    out = {"tracks": [m[f"track{i}"].copy() for i in range(int(m["n_tracks"]))], "bboxes_qc": list(m["bboxes_qc"])}
    for iou in ("aabb", "obb"):
        c = evaluate.compare_maps_ap(out, out, 0.25, iou=iou, fitter=fitter)
        k = len(c["gt_ids"])
        assert k == len(out["tracks"]) and (c["is_tp"][0] == 1).all() and sorted(c["gt_claim"][0].tolist()) == list(range(k))
        assert (c["ap"][c["npred"] > 0] == 1.0).all() and c["mAP"] == 1.0


# ---- 7. offsets that contradict the sizes, status rules, nothing to do ----------------------------------------------------------------
def test_untrusted_offsets_status_rules_and_empty_calls(fitter, golden):
    from odam_amd import _lib
    z = golden("eval_ap.npz")
    a = fixture_args(z)
    # an image whose ground-truth range leaves [0, n_gt], one whose prediction range runs backwards: their predictions count nowhere
    bad = dict(a, gt_off=a["gt_off"].copy(), pred_off=a["pred_off"].copy())
    bad["gt_off"][3] = a["n_gt"] + 7
    bad["pred_off"][6] = bad["pred_off"][5] - 1
    want = R.det_ap(0, n_class=8, ovthresh=0.25, **bad)
    rc, got = raw(fitter, 0, bad)
    assert rc == 0
    check(got, want, bad)
    assert (np.asarray(want["rank"]) == -1).sum() >= 5 and (got["is_tp"][:a["n_pred"]] == -1).sum() == (np.asarray(want["rank"]) == -1).sum()
    # status rules: every refusal comes before any launch -- nothing is written
    P = dict(a, pair_off=np.zeros(a["n_image"] + 1, np.int64), iou=np.zeros(4), n_pairs=0)
    for kw in (dict(kind=-1), dict(kind=4), dict(n_class=0), dict(n_class=65), dict(null=("pred_off",)), dict(null=("scratch",)),
               dict(null=("ap",)), dict(null=("gt_claim",)), dict(null=("score",)), dict(null=("pred_box",)), dict(kind=1, null=("iou",)),
               dict(kind=1, null=("pair_off",))):
        kind = kw.pop("kind", 0)
        rc, g = raw(fitter, kind, P, **kw)
        assert rc == 1 and b"odam_det_ap" in _lib.lib().odam_last_error() and untouched(g), kw      # ODAM_E_INVALID
    for neg in ("n_image", "n_pred", "n_gt"):
        rc = raw_sizes(fitter, dict(a, **{neg: -1}))
        assert rc == 1
    rc = raw_sizes(fitter, dict(a, n_pred=R.MAX_PRED + 1))
    assert rc == 3 and b"32768" in _lib.lib().odam_last_error()      # ODAM_E_LIMIT
    rc = raw_sizes(fitter, dict(a, n_image=2, n_pred=60, n_gt=59), kind=2)
    assert rc == 1
    # nothing to rank: ODAM_OK, the per-class words are written, nothing else
    for n_image in (0, 3):
        e = R.from_lists([(np.zeros((0, 8, 3)), [], [])] * n_image, [(np.zeros((0, 8, 3)), [])] * n_image)
        rc, g = raw(fitter, 0, e)
        assert rc == 0 and (g["npos"][:8] == 0).all() and (g["npred"][:8] == 0).all() and (g["cls_off"][:9] == 0).all() and np.isnan(g["ap"][:8]).all()
        assert untouched({k: g[k] for k in ("ovmax", "jmax", "rank", "is_tp", "gt_claim", "order", "tp", "fp", "rec", "prec", "scratch")})
    e = R.from_lists([(np.zeros((0, 8, 3)), [], [])], [(np.stack([cube([0, 0, 0])] * 3), [1, 1, 4])])      # ground truth, no prediction at all
    rc, g = raw(fitter, 0, e)
    assert rc == 0 and g["npos"][:8].tolist() == [0, 2, 0, 0, 1, 0, 0, 0] and g["ap"][1] == 0 and g["ap"][4] == 0 and np.isnan(g["ap"][0])
    assert g["gt_claim"][:3].tolist() == [-1, -1, -1] and (g["gt_claim"][3:] == SENT_I).all()


def raw_sizes(fitter, a, kind=0):
    """the entry point with sizes that no buffer has to match: it must refuse before it reads or writes anything"""
    import torch
    from odam_amd import _lib, evaluate
    w = torch.full((64,), SENT_I, device="cuda", dtype=torch.int32)
    p = _lib.ptr(w)
    rc = evaluate._entry("odam_det_ap")(fitter._h, kind, a["n_image"], a["n_pred"], a["n_gt"], 8, p, p, p, p, p, p, p, p, p, 0, 0.25, 0, p,
                                        *[p] * 14, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (w == SENT_I).all()
    return rc
