"""The validation loss without a device: tests/criterion_ref.py (the numpy restatement of csrc/det_loss.hip) against the
reference's own HungarianMatcher and SetCriterion (tests/golden/criterion.npz, written by make_golden_criterion.py), the restated
solver against scipy, the Python surface's refusals (odam_amd/criterion.py) and the argument checks of the three entry points of
include/odam_loss.h, which come before any device work."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import criterion_ref as R
from conftest import REPO

OUT_KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")


def fixture_cases(z):
    """[(outputs, targets, indices, cost blocks, {loss: value})] of criterion.npz"""
    keys = [str(k) for k in z["loss_keys"]]
    for n, (Q, B, W) in enumerate(z["cases"].tolist()):
        out = {k: z[f"c{n}_{k}"] for k in OUT_KEYS}
        sizes = z[f"c{n}_sizes"].tolist()
        assert len(sizes) == B and out["pred_logits"].shape[:2] == (B, Q) and z[f"c{n}_objects"].shape[1] == W
        o_off = np.concatenate([[0], np.cumsum(sizes)])
        i_off = np.concatenate([[0], np.cumsum([min(Q, g) for g in sizes])])
        targets = [{"objects": z[f"c{n}_objects"][o_off[b]:o_off[b + 1]]} for b in range(B)]
        idx = [(z[f"c{n}_index_i"][i_off[b]:i_off[b + 1]], z[f"c{n}_index_j"][i_off[b]:i_off[b + 1]]) for b in range(B)]
        cost = [z[f"c{n}_cost"][Q * o_off[b]:Q * o_off[b + 1]].reshape(Q, sizes[b]) for b in range(B)]
        yield out, targets, idx, cost, dict(zip(keys, z[f"c{n}_losses"].tolist()))


def fixture_setup(z):
    costs = dict(zip(("cost_class", "cost_bbox", "cost_giou"), z["costs"].tolist()))
    weights = dict(zip([str(k) for k in z["weight_keys"]], z["weight_values"].tolist()))
    return int(z["num_classes"]), float(z["eos_coef"]), costs, weights


def test_fixture_holds_the_cases_the_issue_names(golden):
    z = golden("criterion.npz")
    cases = {(Q, tuple(z[f"c{n}_sizes"].tolist())): W for n, (Q, B, W) in enumerate(z["cases"].tolist())}
    for Q in (100, 2):
        for sizes in ((5, 0, 17), (0, 0), (32, 31, 1), (3,)):
            assert (Q, sizes) in cases
    assert 12 in cases.values() and any(W > 12 for W in cases.values())
    for out, targets, idx, cost, losses in fixture_cases(z):
        assert np.isfinite(list(losses.values())).all()
        if sum(len(t["objects"]) for t in targets) == 0:
            assert losses["class_error"] == 100.0
        for (i, j), t in zip(idx, targets):
            assert len(i) == len(j) == min(out["pred_logits"].shape[1], len(t["objects"]))


def test_restatement_against_the_reference(golden):
    """indices exactly the reference's on every frame; cost entries and every loss of the reference (float32, sums included) within
    K 2^-24 A of the float64 restatement"""
    z = golden("criterion.npz")
    num_classes, eos, costs, weights = fixture_setup(z)
    worst = {}
    for out, targets, idx, cost, losses in fixture_cases(z):
        got = R.matcher(out, targets, **costs)
        for b, ((gi, gj), (ri, rj)) in enumerate(zip(got, idx)):
            assert np.array_equal(gi, ri) and np.array_equal(gj, rj), b
            assert gi.dtype == np.int64 and gj.dtype == np.int64
        for (c64, A, K), c32 in zip(R.match_cost(out["pred_logits"], out["pred_boxes"], [t["objects"] for t in targets], **costs), cost):
            ok, ratio = R.within(c32, c64, A, K)
            assert ok, ("cost", ratio, K)
            assert K == max(out["pred_logits"].shape[2] + 9, 17) + 1      # the count written out in criterion_ref's docstring
            worst["cost"] = max(worst.get("cost", 0), ratio)
        ref = R.criterion(out, targets, idx, num_classes, eos, weights, f32_sums=True)
        assert ref["card_margin"] > 0
        for k, v in losses.items():
            x64, A, K = ref["table"][k]
            ok, ratio = R.within(v, x64, A, K)
            assert ok, (k, v, x64, ratio, K)
            worst[k] = max(worst.get(k, 0), ratio)
    print("reference float32 vs restatement, largest |x - x64| / (2^-24 A):", {k: round(v, 3) for k, v in worst.items()})


def test_kernel_counts_of_the_restatement(golden):
    """K of the kernel's own arithmetic (binary64 sums): the counts of criterion_ref's docstring, + 1"""
    z = golden("criterion.npz")
    num_classes, eos, costs, weights = fixture_setup(z)
    out, targets, idx, _, _ = next(fixture_cases(z))
    T = R.criterion(out, targets, idx, num_classes, eos, weights)["table"]
    C, n_a = num_classes + 1, out["pred_angle"].shape[2]
    assert T["loss_ce"][2] == C + 6 + 1 and T["loss_angle"][2] == n_a + 5 + 1 and T["loss_giou"][2] == 16 + 1
    assert T["loss_bbox"][2] == T["loss_size"][2] == T["loss_offset"][2] == T["loss_depth"][2] == 1 + 1
    assert T["class_error"][2] == T["cardinality_error"][2] == 1
    assert T["total"][2] == max(C + 6, n_a + 5, 16) + 1


LSAP_SHAPES = [(1, 1), (100, 1), (100, 2), (100, 31), (100, 32), (63, 5), (64, 5), (65, 5), (128, 32), (2, 32), (5, 17), (32, 32), (100, 0),
               (100, 33), (129, 4)]


def test_restated_solver_against_scipy():
    from scipy.optimize import linear_sum_assignment
    rs = np.random.RandomState(5)
    for r, c in LSAP_SHAPES:
        for kind in ("float", "ties"):
            cost = (rs.normal(0, 1, (r, c)) if kind == "float" else rs.randint(0, 4, (r, c))).astype(np.float32)
            si, sj = linear_sum_assignment(cost)
            gi, gj = R.lsap(cost)
            assert np.array_equal(gi, si) and np.array_equal(gj, sj), (r, c, kind)
    bad = rs.normal(0, 1, (6, 4)).astype(np.float32)
    for v in (np.nan, -np.inf):
        x = bad.copy(); x[2, 1] = v
        with pytest.raises(ValueError):
            R.lsap(x)
    x = bad.T.copy(); x[1, :] = np.inf      # a row of the 4 x 6 problem that can go nowhere
    with pytest.raises(ValueError):
        linear_sum_assignment(x)
    with pytest.raises(ValueError):
        R.lsap(x)


def test_build_reads_the_reference_keys():
    from odam_amd import criterion
    cfg = dict(set_cost_class=1.5, set_cost_bbox=5, set_cost_giou=2, bbox_loss_coef=4, giou_loss_coef=3, eos_coef=0.2, dataset_file="scan_net")
    for args in (cfg, types.SimpleNamespace(**cfg)):
        c = criterion.build(args)
        assert isinstance(c, criterion.SetCriterion) and isinstance(c.matcher, criterion.HungarianMatcher)
        assert (c.matcher.cost_class, c.matcher.cost_bbox, c.matcher.cost_giou) == (1.5, 5, 2)
        assert c.num_classes == 18 and c.eos_coef == 0.2
        assert c.weight_dict == {"loss_ce": 1, "loss_bbox": 4, "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1, "loss_giou": 3}
        assert c.losses == ["labels", "boxes", "cardinality", "size", "angle", "offset", "depth"]
    assert criterion.build(dict(cfg, dataset_file="coco")).num_classes == 91
    assert criterion.build(dict(cfg, dataset_file="other")).num_classes == 20
    for k in ("set_cost_class", "set_cost_bbox", "set_cost_giou", "bbox_loss_coef", "giou_loss_coef", "eos_coef"):
        with pytest.raises(KeyError):
            criterion.build({a: b for a, b in cfg.items() if a != k})
    m = criterion.HungarianMatcher()
    assert (m.cost_class, m.cost_bbox, m.cost_giou) == (1, 1, 1)
    with pytest.raises(AssertionError):
        criterion.HungarianMatcher(0, 0, 0)
    total = c.total({"loss_ce": 2.0, "loss_bbox": 0.5, "class_error": 7.0})
    assert float(total) == 1 * 2.0 + 4 * 0.5


def test_refusals(golden):
    from odam_amd import _lib, criterion
    m = criterion.HungarianMatcher(1, 5, 2)
    with pytest.raises(_lib.OdamError, match="masks"):
        criterion.SetCriterion(18, m, {}, 0.1, ["labels", "masks"])
    with pytest.raises(_lib.OdamError, match="masks"):
        criterion.build(dict(set_cost_class=1, set_cost_bbox=5, set_cost_giou=2, bbox_loss_coef=5, giou_loss_coef=2, eos_coef=0.1, masks=True))
    with pytest.raises(ValueError, match="keypoints"):
        criterion.SetCriterion(18, m, {}, 0.1, ["labels", "keypoints"])
    # W < 12: refused by the Python layer before anything is moved to a device, by the restatement and by the entry points
    z = golden("criterion.npz")
    num_classes, eos, costs, weights = fixture_setup(z)
    out, targets, idx, _, _ = next(fixture_cases(z))
    narrow = [{"objects": t["objects"][:, :11]} for t in targets]
    c = criterion.SetCriterion(num_classes, m, weights, eos, list(R.LOSS_NAMES))
    with pytest.raises(ValueError, match="W >= 12"):
        c(out, narrow)
    with pytest.raises(ValueError, match="W >= 12"):
        m(out, narrow)
    with pytest.raises(ValueError, match="W >= 12"):
        R.criterion(out, narrow, idx, num_classes, eos, weights)
    # a degenerate box: generalized_box_iou's AssertionError
    neg = {k: v.copy() for k, v in out.items()}
    neg["pred_boxes"][1, 7, 2] = -0.01
    with pytest.raises(AssertionError):
        R.match_cost(neg["pred_logits"], neg["pred_boxes"], [t["objects"] for t in targets], **costs)
    bad_t = [{"objects": t["objects"].copy()} for t in targets]
    bad_t[0]["objects"][idx[0][1][0], 4] = -0.2
    with pytest.raises(AssertionError):
        R.criterion(out, bad_t, idx, num_classes, eos, weights)
    with pytest.raises(AssertionError, match="degenerate"):
        criterion._raise_for_status([0, criterion.ST_DEGENERATE], "criterion")
    with pytest.raises(IndexError):
        criterion._raise_for_status([criterion.ST_CLASS], "criterion")
    criterion._raise_for_status([0, 0], "criterion")


def _declared(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_loss.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/odam_loss.h"
    c_types = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "float": ctypes.c_float}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else c_types[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return want, txt


def test_entry_points_check_their_arguments_before_any_device_work():
    """ODAM_E_INVALID = 1, ODAM_E_LIMIT = 3 (odam_sq.h), as the neighbours answer; the pointers below are never followed"""
    from odam_amd import _lib, criterion
    L = _lib.lib()
    for name in criterion.LOSS_ARGTYPES:
        assert hasattr(L, name), f"the built library has no {name}"
        want, txt = _declared(name)
        assert criterion.LOSS_ARGTYPES[name] == want, name
        assert criterion._entry(name).restype is ctypes.c_int
    for macro, v in (("ODAM_LSAP_MAX_SMALL", criterion.LSAP_MAX_SMALL), ("ODAM_LSAP_MAX_LARGE", criterion.LSAP_MAX_LARGE),
                     ("ODAM_LOSS_N_PARTIAL", len(criterion.PARTIAL_KEYS)), ("ODAM_LOSS_N_ENTRIES", len(criterion.TABLE_KEYS)),
                     ("ODAM_LOSS_N_WEIGHTS", len(criterion.WEIGHT_KEYS)), ("ODAM_LOSS_ST_DEGENERATE", criterion.ST_DEGENERATE),
                     ("ODAM_LOSS_ST_CLASS", criterion.ST_CLASS), ("ODAM_LOSS_ST_OFFSETS", criterion.ST_OFFSETS)):
        assert "#define %s %d\n" % (macro, v) in txt
    assert criterion.TABLE_KEYS == R.TABLE_KEYS and criterion.PARTIAL_KEYS == R.PARTIAL_KEYS and criterion.WEIGHT_KEYS == R.WEIGHT_KEYS
    assert criterion.KEYS_OF_LOSS == R.KEYS_OF_LOSS and criterion.LOSS_NAMES == R.LOSS_NAMES
    buf = np.zeros(64, np.float64)
    P = ctypes.c_void_p(buf.ctypes.data)

    # ---- odam_detr_match_cost(logits, boxes, B, Q, n_logit, objects, obj_off, n_obj, W, 3 weights, cost_out, status, stream)
    def cost(**kw):
        a = dict(logits=P, boxes=P, B=2, Q=100, n_logit=19, objects=P, obj_off=P, n_obj=5, W=12, out=P, status=P)
        a.update(kw)
        return criterion._entry("odam_detr_match_cost")(a["logits"], a["boxes"], a["B"], a["Q"], a["n_logit"], a["objects"], a["obj_off"],
                                                        a["n_obj"], a["W"], 1.0, 5.0, 2.0, a["out"], a["status"], None)
    for kw in [dict(B=-1), dict(Q=-1), dict(n_obj=-1), dict(n_logit=1), dict(W=11), dict(logits=None), dict(boxes=None), dict(objects=None),
               dict(obj_off=None), dict(out=None), dict(status=None)]:
        assert cost(**kw) == 1 and b"odam_detr_match_cost" in L.odam_last_error(), kw
    assert cost(B=0) == 0      # nothing to do, nothing launched

    # ---- odam_lsap_batch(cost, n_cost, cost_off, rows, cols, n_prob, max_small, max_large, match_off, n_match, col_of_row, n_pairs, status, stream)
    def lsap(**kw):
        a = dict(cost=P, n_cost=400, cost_off=P, rows=P, cols=P, n_prob=1, small=4, large=100, match_off=P, n_match=100, col=P, npairs=P, status=P)
        a.update(kw)
        return criterion._entry("odam_lsap_batch")(a["cost"], a["n_cost"], a["cost_off"], a["rows"], a["cols"], a["n_prob"], a["small"],
                                                   a["large"], a["match_off"], a["n_match"], a["col"], a["npairs"], a["status"], None)
    for kw in [dict(n_prob=-1), dict(small=-1), dict(small=5, large=4), dict(n_cost=-1), dict(n_match=-1), dict(cost=None), dict(cost_off=None),
               dict(rows=None), dict(cols=None), dict(match_off=None), dict(col=None), dict(npairs=None), dict(status=None)]:
        assert lsap(**kw) == 1 and b"odam_lsap_batch" in L.odam_last_error(), kw
    assert lsap(small=33, large=100) == 3 and b"32 x 128" in L.odam_last_error()      # ODAM_E_LIMIT, before any launch
    assert lsap(small=4, large=129) == 3
    assert lsap(n_prob=0) == 0

    # ---- odam_detr_criterion(6 outputs, B, Q, n_logit, n_angle, objects, obj_off, n_obj, W, match, num_boxes, eos, weights, partial, table, status, stream)
    w = (ctypes.c_double * 7)(1, 5, 2, 1, 3, 1, 1)

    def crit(**kw):
        a = dict(outs=[P] * 6, B=2, Q=100, n_logit=19, n_angle=30, objects=P, obj_off=P, n_obj=5, W=12, match=P, num_boxes=5.0,
                 weights=ctypes.cast(w, ctypes.c_void_p), partial=P, table=P, status=P)
        a.update(kw)
        return criterion._entry("odam_detr_criterion")(*a["outs"], a["B"], a["Q"], a["n_logit"], a["n_angle"], a["objects"], a["obj_off"],
                                                       a["n_obj"], a["W"], a["match"], a["num_boxes"], 0.1, a["weights"], a["partial"],
                                                       a["table"], a["status"], None)
    for kw in [dict(B=0), dict(B=-1), dict(Q=-1), dict(n_obj=-1), dict(n_logit=1), dict(n_angle=0), dict(W=11), dict(num_boxes=0.0),
               dict(num_boxes=float("nan")), dict(objects=None), dict(obj_off=None), dict(match=None), dict(weights=None), dict(partial=None),
               dict(table=None), dict(status=None)]:
        assert crit(**kw) == 1 and b"odam_detr_criterion" in L.odam_last_error(), kw
    for k in range(6):
        assert crit(outs=[None if i == k else P for i in range(6)]) == 1
