"""The validation loss on the device (odam_amd/csrc/det_loss.hip through the raw entry points of include/odam_loss.h and through
odam_amd/criterion.py): the batched assignment solver against scipy itself, exactly; the cost kernel and the criterion against the
float64 restatement (tests/criterion_ref.py) under |x - x64| <= K 2^-24 A, K counted there; the criterion against the reference's own
run (tests/golden/criterion.npz); bit identity of repeated calls and of a frame alone against the frame inside a batch; a small
detector end to end."""
import functools

import numpy as np
import pytest
import torch

import criterion_ref as R
from test_criterion_host import LSAP_SHAPES, OUT_KEYS, fixture_cases, fixture_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEVICE_SHAPES = [s for s in LSAP_SHAPES if min(s) <= 32 and max(s) <= 128]
BEYOND = [s for s in LSAP_SHAPES if not (min(s) <= 32 and max(s) <= 128)]


def _problem(rs, r, c, kind):
    return (rs.normal(0, 1, (r, c)) if kind == "float" else rs.randint(0, 4, (r, c))).astype(np.float32)


def _solve(blocks):
    """odam_lsap_batch on a list of host blocks in ONE launch -> ([(row_ind, col_ind)], n_pairs, status)"""
    from odam_amd import criterion
    flat = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks] + [np.zeros(1, np.float32)])).to(DEV)
    col, npairs, status, m_off = criterion.lsap_batch(flat, [b.shape for b in blocks])
    col = col.cpu().numpy()
    return [criterion._lists(col[m_off[k]:m_off[k + 1]]) for k in range(len(blocks))], npairs.cpu().numpy(), status.cpu().numpy(), col


def test_shapes_cover_the_limits():
    assert len(DEVICE_SHAPES) == 13 and sorted(BEYOND) == [(100, 33), (129, 4)]


@pytest.mark.parametrize("kind", ["float", "ties"])
def test_lsap_batch_is_scipy_on_every_shape(kind):
    """each shape alone and all of them in one launch; small-integer costs give many exact ties: scipy's tie order"""
    from scipy.optimize import linear_sum_assignment
    rs = np.random.RandomState(7 if kind == "float" else 8)
    blocks = [_problem(rs, r, c, kind) for r, c in DEVICE_SHAPES] + [_problem(rs, 32, 128, kind), _problem(rs, 17, 17, kind)]
    want = [linear_sum_assignment(b) for b in blocks]
    got, npairs, status, _ = _solve(blocks)
    assert not status.any()
    for b, (gi, gj), (si, sj), n in zip(blocks, got, want, npairs):
        assert np.array_equal(gi, si) and np.array_equal(gj, sj), b.shape
        assert n == min(b.shape) == len(gi)
    for b, (si, sj) in zip(blocks, want):
        (one,), npairs, status, _ = _solve([b])
        assert status[0] == 0 and np.array_equal(one[0], si) and np.array_equal(one[1], sj), b.shape


def test_lsap_batch_refuses_what_scipy_refuses():
    from scipy.optimize import linear_sum_assignment
    rs = np.random.RandomState(9)
    good = _problem(rs, 40, 6, "float")
    inf_row = _problem(rs, 4, 6, "float"); inf_row[1, :] = np.inf          # 4 rows must all be matched: infeasible
    nan = _problem(rs, 50, 7, "float"); nan[31, 2] = np.nan
    ninf = _problem(rs, 5, 9, "float"); ninf[4, 8] = -np.inf
    ok_inf = _problem(rs, 30, 5, "float"); ok_inf[3, :] = np.inf           # a tall block: the row stays unmatched, as in scipy
    for bad in (inf_row, nan, ninf):
        with pytest.raises(ValueError):
            linear_sum_assignment(bad)
    got, npairs, status, col = _solve([good, inf_row, nan, ninf, ok_inf])
    assert status.tolist() == [0, 1, 1, 1, 0] and npairs.tolist() == [6, 0, 0, 0, 5]
    assert (col[40:40 + 4 + 50 + 5] == -1).all()
    for k, b in ((0, good), (4, ok_inf)):
        si, sj = linear_sum_assignment(b)
        assert np.array_equal(got[k][0], si) and np.array_equal(got[k][1], sj)


def test_lsap_beyond_the_limits():
    """100 x 33 and 129 x 4: ODAM_E_LIMIT for the call before anything is launched; the Python layer solves them with scipy"""
    from scipy.optimize import linear_sum_assignment
    from odam_amd import _lib, criterion
    rs = np.random.RandomState(10)
    small = _problem(rs, 20, 5, "ties")
    for r, c in BEYOND:
        b = _problem(rs, r, c, "ties")
        flat = torch.from_numpy(np.concatenate([small.reshape(-1), b.reshape(-1)])).to(DEV)
        with pytest.raises(_lib.OdamError, match="code 3"):
            criterion.lsap_batch(flat, [small.shape, b.shape])
        got = criterion.linear_sum_assignment_batch([torch.from_numpy(small).to(DEV), torch.from_numpy(b).to(DEV)])
        for (gi, gj), blk in zip(got, (small, b)):
            si, sj = linear_sum_assignment(blk)
            assert np.array_equal(gi, si) and np.array_equal(gj, sj), blk.shape


def make_inputs(rs, B, Q, sizes, n_logit=19, W=12, n_angle=30):
    f = lambda x: np.ascontiguousarray(x, np.float32)
    boxes = lambda n: np.concatenate([rs.uniform(0.15, 0.85, (n, 2)), rs.uniform(0.04, 0.45, (n, 2))], 1)
    out = {"pred_logits": f(rs.normal(0, 2.5, (B, Q, n_logit))), "pred_boxes": f(boxes(B * Q).reshape(B, Q, 4)),
           "pred_angle": f(rs.normal(0, 2, (B, Q, n_angle))), "pred_offset": f(rs.normal(0, 0.1, (B, Q, 2))),
           "pred_size": f(rs.uniform(0.2, 2.0, (B, Q, 3))), "pred_depth": f(rs.uniform(0.5, 5.0, (B, Q, 1)))}
    targets = []
    for n in sizes:
        o = rs.uniform(-1, 1, (n, W))
        o[:, 0] = rs.randint(0, n_logit - 1, n); o[:, 1:5] = boxes(n); o[:, 5:8] = rs.uniform(0.2, 2.0, (n, 3))
        o[:, 8:10] = rs.normal(0, 0.1, (n, 2)); o[:, W - 2] = rs.uniform(0.5, 5.0, n); o[:, W - 1] = rs.randint(0, n_angle, n)
        targets.append({"objects": f(o)})
    return out, targets


def _device_cost(out, targets, costs):
    from odam_amd import criterion
    S = criterion._Staged(out, targets, keys=("pred_logits", "pred_boxes"), device=DEV)
    cost, status = criterion.match_cost(S, costs["cost_class"], costs["cost_bbox"], costs["cost_giou"])
    cost, status = cost.cpu().numpy(), status.cpu().numpy()
    return [cost[S.Q * S.off[b]:S.Q * S.off[b + 1]].reshape(S.Q, S.sizes[b]) for b in range(S.B)], status


COSTS = dict(cost_class=1.0, cost_bbox=5.0, cost_giou=2.0)
WEIGHTS = {"loss_ce": 1, "loss_bbox": 5, "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1, "loss_giou": 2}


@pytest.mark.parametrize("B", [1, 3])
def test_cost_kernel_against_the_restatement(B, measured):
    """Q on both sides of a wavefront and of the 128-lane workgroup, target counts 0 .. 32 and past the 32 rows staged at a time,
    19 logits and 7, W = 12 and 14"""
    rs = np.random.RandomState(20 + B)
    size_sets = [(0,), (1,), (2,), (31,), (32,), (33,), (70,)] if B == 1 else [(0, 31, 2), (32, 1, 0), (2, 32, 31), (40, 0, 65)]
    worst = 0.0
    for Q in (1, 63, 64, 65, 100, 130):
        for n, sizes in enumerate(size_sets):
            n_logit, W = ((19, 12), (7, 14), (19, 14), (7, 12))[(n + Q) % 4]
            out, targets = make_inputs(rs, B, Q, sizes, n_logit, W)
            got, status = _device_cost(out, targets, COSTS)
            assert not status.any()
            ref = R.match_cost(out["pred_logits"], out["pred_boxes"], [t["objects"] for t in targets], **COSTS)
            for c32, (c64, A, K) in zip(got, ref):
                assert c32.shape == c64.shape
                ok, ratio = R.within(c32, c64, A, K)
                worst = max(worst, ratio)
                assert ok, (Q, sizes, n_logit, W, ratio, K)
    print("cost kernel: largest |x - x64| / (2^-24 A) = %.3f" % worst)
    measured("criterion_cost_ratio", worst)


@functools.lru_cache(maxsize=None)
def _fixture():
    import os
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "criterion.npz"), allow_pickle=False)
    return fixture_setup(z), list(fixture_cases(z))


def _criterion(num_classes, eos, costs, weights, losses=R.LOSS_NAMES):
    from odam_amd import criterion
    return criterion.SetCriterion(num_classes, criterion.HungarianMatcher(**costs), weights, eos, list(losses))


def _check_table(got, ref, measured, tag):
    worst = {}
    for k, v in got.items():
        x64, A, K = ref["table"][k]
        ok, ratio = R.within(float(v), x64, A, K)
        print("  %-18s device %.9g   float64 %.9g   |x - x64| / (2^-24 A) = %.3f   K = %d" % (k, float(v), x64, ratio, K))
        worst[k] = ratio
        measured(f"criterion_{k}_ratio", ratio)
        assert ok, (tag, k, float(v), x64, ratio, K)
    return worst


def test_criterion_against_the_reference_run(measured):
    """every fixture case: the matcher's indices are the reference's, exactly; every loss within the bound of the float64
    restatement, and within the sum of both bounds of the reference's own float32 value"""
    (num_classes, eos, costs, weights), cases = _fixture()
    crit = _criterion(num_classes, eos, costs, weights)
    for n, (out, targets, idx, cost, losses) in enumerate(cases):
        d_out = {k: torch.from_numpy(v).to(DEV) for k, v in out.items()}
        d_out["pred_obj_features"] = torch.zeros(3, device=DEV); d_out["_hw"] = (6, 8)      # extra keys of Detector.__call__: ignored
        d_tgt = [{"objects": torch.from_numpy(t["objects"]).to(DEV)} for t in targets]
        got_idx = crit.matcher(d_out, d_tgt)
        for (gi, gj), (ri, rj) in zip(got_idx, idx):
            assert gi.dtype == torch.int64 and gj.dtype == torch.int64 and not gi.is_cuda
            assert np.array_equal(gi.numpy(), ri) and np.array_equal(gj.numpy(), rj), n
        got = crit(d_out, d_tgt)
        assert sorted(got) == sorted(losses) and all(v.dim() == 0 for v in got.values())
        ref = R.criterion(out, targets, idx, num_classes, eos, weights)
        ref32 = R.criterion(out, targets, idx, num_classes, eos, weights, f32_sums=True)
        assert ref["card_margin"] > 0
        print("case %d" % n)
        _check_table(got, ref, measured, n)
        for k, v in losses.items():
            x64, A, K = ref["table"][k]
            assert abs(float(got[k]) - v) <= (K + ref32["table"][k][2]) * R.U * A or float(got[k]) == v, (n, k, float(got[k]), v)
        table = crit.last_table.cpu().numpy()
        assert np.array_equal(table[:9], np.asarray([float(got[k]) for k in R.TABLE_KEYS[:9]]))
        assert table[9] == float(crit.total(got))      # the same products added in the same order
        ok, _ = R.within(table[9], *ref["table"]["total"])
        assert ok
        part = crit.last_partial.cpu().numpy()
        for k in range(len(R.PARTIAL_KEYS)):
            ok, ratio = R.within(part[:, k], ref["partial"][:, k], ref["partial_A"][:, k], ref["partial_K"][k])
            assert ok, (n, R.PARTIAL_KEYS[k], ratio)


def test_criterion_on_other_shapes_against_the_restatement(measured):
    """Q past a wavefront and past two, another class count, W = 14, frames beyond the device solver (33 targets: scipy from the
    device's cost block), num_boxes given by the caller"""
    from scipy.optimize import linear_sum_assignment
    rs = np.random.RandomState(31)
    for Q, sizes, n_logit, W, num_boxes in ((65, (3, 0, 32), 7, 14, None), (130, (31, 2), 19, 12, 7.5), (100, (33, 4), 19, 12, None),
                                            (63, (0, 0), 7, 12, None), (1, (2,), 19, 14, None)):
        out, targets = make_inputs(rs, len(sizes), Q, sizes, n_logit, W)
        crit = _criterion(n_logit - 1, 0.25, COSTS, WEIGHTS)
        blocks, status = _device_cost(out, targets, COSTS)
        assert not status.any()
        want = [linear_sum_assignment(c) for c in blocks]
        idx = crit.matcher(out, targets)      # host arrays are accepted
        for (gi, gj), (si, sj) in zip(idx, want):
            assert np.array_equal(gi.numpy(), si) and np.array_equal(gj.numpy(), sj), (Q, sizes)
        got = crit(out, targets) if num_boxes is None else crit(out, targets, num_boxes=num_boxes)
        ref = R.criterion(out, targets, want, n_logit - 1, 0.25, WEIGHTS, num_boxes=num_boxes)
        assert ref["card_margin"] > 0
        print("Q %d, targets %s" % (Q, sizes))
        _check_table(got, ref, measured, (Q, sizes))


def test_losses_subsets_and_a_callers_matcher():
    (num_classes, eos, costs, weights), cases = _fixture()
    out, targets, idx, _, _ = cases[0]
    full_crit = _criterion(num_classes, eos, costs, weights)
    full = full_crit(out, targets)
    for subset in (["labels"], ["boxes", "cardinality"], ["depth", "angle", "offset", "size"], ["cardinality"]):
        crit = _criterion(num_classes, eos, costs, weights, subset)
        got = crit(out, targets)
        assert sorted(got) == sorted(k for name in subset for k in R.KEYS_OF_LOSS[name])
        for k, v in got.items():
            assert float(v) == float(full[k]), (subset, k)
        assert float(crit.last_table[9]) == float(crit.total(got))
    # any callable that returns the reference's list of (index_i, index_j) serves as the matcher
    from odam_amd import criterion
    given = criterion.SetCriterion(num_classes, lambda o, t: [(torch.from_numpy(i), torch.from_numpy(j)) for i, j in idx], weights, eos,
                                   list(R.LOSS_NAMES))
    got = given(out, targets)
    for k, v in full.items():
        assert float(got[k]) == float(v), k


def test_same_bits_on_every_call_and_in_every_batch():
    """two calls return the same bits; a frame passed alone gives the partial sums it gives inside a batch"""
    (num_classes, eos, costs, weights), cases = _fixture()
    crit = _criterion(num_classes, eos, costs, weights)
    for n in (0, 2):
        out, targets, _, _, _ = cases[n]
        d_out = {k: torch.from_numpy(v).to(DEV) for k, v in out.items()}
        a = crit(d_out, targets); ta, pa = crit.last_table.cpu().numpy(), crit.last_partial.cpu().numpy()
        for _ in range(3):
            b = crit(d_out, targets); tb, pb = crit.last_table.cpu().numpy(), crit.last_partial.cpu().numpy()
            assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64)) and np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
            assert all(float(a[k]) == float(b[k]) for k in a)
        assert np.isfinite(pa).all() and pa.shape == (len(targets), len(R.PARTIAL_KEYS))
        for f in range(len(targets)):
            crit({k: v[f:f + 1] for k, v in d_out.items()}, targets[f:f + 1])
            alone = crit.last_partial.cpu().numpy()
            assert np.array_equal(alone[0].view(np.uint64), pa[f].view(np.uint64)), (n, f)


def test_refusals_on_the_device():
    (num_classes, eos, costs, weights), cases = _fixture()
    out, targets, idx, _, _ = cases[0]
    crit = _criterion(num_classes, eos, costs, weights)
    neg = {k: v.copy() for k, v in out.items()}
    neg["pred_boxes"][1, 7, 2] = -0.01      # frame 1 has no target: the matcher tests every query all the same
    with pytest.raises(AssertionError, match="degenerate"):
        crit.matcher(neg, targets)
    with pytest.raises(AssertionError, match="degenerate"):
        crit(neg, targets)
    bad_t = [{"objects": t["objects"].copy()} for t in targets]
    bad_t[2]["objects"][5, 3] = -0.3
    with pytest.raises(AssertionError, match="degenerate"):
        crit(out, bad_t)
    # the criterion's own test of the matched pairs, under a caller's assignment
    from odam_amd import criterion
    given = criterion.SetCriterion(num_classes, lambda o, t: idx, weights, eos, list(R.LOSS_NAMES))
    bad_t = [{"objects": t["objects"].copy()} for t in targets]
    bad_t[0]["objects"][idx[0][1][0], 4] = -0.2
    with pytest.raises(AssertionError, match="degenerate"):
        given(out, bad_t)
    lab = [{"objects": t["objects"].copy()} for t in targets]
    lab[0]["objects"][1, 0] = num_classes + 1
    with pytest.raises(IndexError):
        crit(out, lab)
    ang = [{"objects": t["objects"].copy()} for t in targets]
    ang[2]["objects"][0, -1] = 30
    with pytest.raises(IndexError):
        crit(out, ang)
    nan = {k: v.copy() for k, v in out.items()}
    nan["pred_logits"][0, 3, :] = np.nan      # a NaN cost row: where scipy raises ValueError
    with pytest.raises(ValueError, match="invalid numeric"):
        crit.matcher(nan, targets)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detector_outputs_through_the_criterion(dtype):
    """a small detector (ResNet-18, 192 x 256, synthetic weights): its outputs go to the criterion as they lie on the device"""
    from odam_amd import criterion, detector, weights
    det = detector.Detector(backbone="resnet18", max_batch=2, device=DEV, n_streams=1, dtype=dtype)
    try:
        det.load_state_dict(weights.make_state_dict(backbone="resnet18", seed=0))
        torch.manual_seed(4)
        out = det(torch.randn(2, 3, 192, 256).to(DEV))
        rs = np.random.RandomState(12)
        _, targets = make_inputs(rs, 2, 1, (6, 0), 19, 12)
        crit = criterion.build(dict(set_cost_class=1, set_cost_bbox=5, set_cost_giou=2, bbox_loss_coef=5, giou_loss_coef=2, eos_coef=0.1,
                                    dataset_file="scan_net"))
        got = crit(out, targets)
        assert sorted(got) == sorted(R.TABLE_KEYS[:9])
        assert all(np.isfinite(float(v)) for v in got.values()), got
        assert np.isfinite(float(crit.total(got)))
        if dtype == "fp32":
            back = {k: out[k].cpu().numpy() for k in OUT_KEYS}
            idx = [(i.numpy(), j.numpy()) for i, j in crit.matcher(out, targets)]
            ref = R.criterion(back, targets, idx, 18, 0.1, crit.weight_dict)
            for k, v in got.items():
                ok, ratio = R.within(float(v), *ref["table"][k])
                assert ok, (k, float(v), ref["table"][k], ratio)
    finally:
        det.close()
