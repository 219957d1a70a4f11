"""Golden for the validation loss: the reference's own HungarianMatcher (src/models/matcher.py) and SetCriterion
(src/models/detr.py), imported as they lie and run on the CPU in float32, on synthetic outputs and targets.  Stores the inputs
and, observed on the reference's run: the float32 cost block scipy was handed per frame, the indices it returned and every loss.

Cases: Q = 100 and Q = 2 (fewer queries than targets) against target counts (5, 0, 17), (0, 0), (32, 31, 1) and (3,): frames
without targets, a batch without any target, a frame at the solver's 32 rows; W = 12 and W = 14 (depth and angle bin are read
from the END of a target row).  18 classes + no-object, 30 angle bins.

Checked here before anything is written:
  - every assignment is unchanged under 50 random perturbations of +-1e-5 on every predicted value (a frame that fails would
    have to be left out: the cap on such frames is 0, asserted);
  - the reference's float32 cost entries and losses satisfy |x - x64| <= K 2^-24 A against tests/criterion_ref.py, the bound the
    device is held to, with the float32 sums of the reference counted (f32_sums=True);
  - the restated solver returns the reference's indices on the reference's cost block;
  - no query's largest object probability is within its error bound of the 0.7 threshold of cardinality_error.
Arrays only.  Run: python tests/golden/make_golden_criterion.py [--check]   (--check: regenerate and compare with the stored file,
array by array, bit for bit; nothing is written)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

SEED = 29
NUM_CLASSES, N_ANGLE = 18, 30
COSTS = dict(cost_class=1.0, cost_bbox=5.0, cost_giou=2.0)
EOS_COEF = 0.1
WEIGHTS = {"loss_ce": 1, "loss_bbox": 5, "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1, "loss_giou": 2}
LOSSES = ["labels", "boxes", "cardinality", "size", "angle", "offset", "depth"]
# (Q, target counts, W)
CASES = [(100, (5, 0, 17), 12), (100, (0, 0), 12), (100, (32, 31, 1), 14), (100, (3,), 12),
         (2, (5, 0, 17), 14), (2, (0, 0), 12), (2, (32, 31, 1), 12), (2, (3,), 12)]
N_PERTURB, PERTURB = 50, 1e-5
MAX_EXCLUDED = 0
OUT_KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
LOSS_KEYS = ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "loss_size", "loss_offset", "loss_depth", "loss_angle")


def make_case(rs, Q, sizes, W):
    B = len(sizes)
    f = lambda x: np.ascontiguousarray(x, np.float32)

    def boxes(n):
        return np.concatenate([rs.uniform(0.15, 0.85, (n, 2)), rs.uniform(0.04, 0.45, (n, 2))], 1)
    out = {"pred_logits": f(rs.normal(0, 2.5, (B, Q, NUM_CLASSES + 1))), "pred_boxes": f(boxes(B * Q).reshape(B, Q, 4)),
           "pred_angle": f(rs.normal(0, 2, (B, Q, N_ANGLE))), "pred_offset": f(rs.normal(0, 0.1, (B, Q, 2))),
           "pred_size": f(rs.uniform(0.2, 2.0, (B, Q, 3))), "pred_depth": f(rs.uniform(0.5, 5.0, (B, Q, 1)))}
    objects = []
    for n in sizes:
        o = rs.uniform(-1, 1, (n, W))      # the columns between 10 and W - 2 belong to nobody
        o[:, 0] = rs.randint(0, NUM_CLASSES, n); o[:, 1:5] = boxes(n); o[:, 5:8] = rs.uniform(0.2, 2.0, (n, 3))
        o[:, 8:10] = rs.normal(0, 0.1, (n, 2)); o[:, W - 2] = rs.uniform(0.5, 5.0, n); o[:, W - 1] = rs.randint(0, N_ANGLE, n)
        objects.append(f(o))
    return out, objects


def generate():
    import refenv
    refenv.setup()
    import torch
    import src.models.matcher as ref_matcher
    from src.models.detr import SetCriterion
    import criterion_ref as R

    seen = []
    real_lsa = ref_matcher.linear_sum_assignment
    ref_matcher.linear_sum_assignment = lambda c: (seen.append(c.numpy().copy()), real_lsa(c))[1]
    matcher = ref_matcher.HungarianMatcher(**COSTS)
    crit = SetCriterion(NUM_CLASSES, matcher=matcher, weight_dict=dict(WEIGHTS), eos_coef=EOS_COEF, losses=list(LOSSES))
    rs = np.random.RandomState(SEED)
    data = {"cases": np.asarray([(Q, len(s), W) for Q, s, W in CASES], np.int32), "num_classes": np.int32(NUM_CLASSES),
            "eos_coef": np.float64(EOS_COEF), "costs": np.asarray([COSTS["cost_class"], COSTS["cost_bbox"], COSTS["cost_giou"]]),
            "weight_keys": np.asarray(sorted(WEIGHTS)), "weight_values": np.asarray([float(WEIGHTS[k]) for k in sorted(WEIGHTS)]),
            "loss_keys": np.asarray(LOSS_KEYS)}
    excluded, worst = 0, {}

    def note(name, ratio, K):
        worst[name] = max(worst.get(name, (0.0, 0))[0], ratio), max(worst.get(name, (0.0, 0))[1], K)

    for n, (Q, sizes, W) in enumerate(CASES):
        out, objects = make_case(rs, Q, sizes, W)
        t_out = {k: torch.from_numpy(v) for k, v in out.items()}
        t_tgt = [{"objects": torch.from_numpy(o)} for o in objects]
        del seen[:]
        idx = matcher(t_out, t_tgt)
        blocks = [np.asarray(c, np.float32) for c in seen]
        assert len(blocks) == len(sizes) and all(c.shape == (Q, g) for c, g in zip(blocks, sizes)) and all(c.dtype == np.float32 for c in seen)
        idx = [(i.numpy(), j.numpy()) for i, j in idx]
        for (i, j), g in zip(idx, sizes):
            assert len(i) == len(j) == min(Q, g) and (np.diff(i) > 0).all()
        # the assignment is stable under perturbations of every predicted value
        prs = np.random.RandomState(1000 + n)
        changed = np.zeros(len(sizes), bool)
        for _ in range(N_PERTURB):
            p_out = {k: torch.from_numpy(v + prs.uniform(-PERTURB, PERTURB, v.shape).astype(np.float32)) for k, v in out.items()}
            for b, ((i, j), (pi, pj)) in enumerate(zip(idx, matcher(p_out, t_tgt))):
                changed[b] |= not (np.array_equal(i, pi.numpy()) and np.array_equal(j, pj.numpy()))
        excluded += int(changed.sum())
        # the restatement on the reference's numbers
        ref_cost = R.match_cost(out["pred_logits"], out["pred_boxes"], objects, **COSTS)
        for b, ((c64, A, K), c32) in enumerate(zip(ref_cost, blocks)):
            ok, ratio = R.within(c32, c64, A, K)
            assert ok, ("cost", n, b, ratio, K)
            note("cost", ratio, K)
            ri, rj = R.lsap(c32)
            assert np.array_equal(ri, idx[b][0]) and np.array_equal(rj, idx[b][1]), ("solver", n, b)
        del seen[:]
        losses = crit(t_out, t_tgt)
        assert sorted(losses) == sorted(LOSS_KEYS)
        ref = R.criterion(out, [{"objects": o} for o in objects], idx, NUM_CLASSES, EOS_COEF, WEIGHTS, f32_sums=True)
        assert ref["card_margin"] > 0, ("a probability at the cardinality threshold", n, ref["card_margin"])
        vals = np.asarray([float(losses[k]) for k in LOSS_KEYS], np.float64)
        assert np.isfinite(vals).all(), (n, vals)
        for k, v in zip(LOSS_KEYS, vals):
            x64, A, K = ref["table"][k]
            ok, ratio = R.within(v, x64, A, K)
            assert ok, (k, n, v, x64, ratio, K)
            note(k, ratio, K)
        if sum(sizes) == 0:
            assert vals[LOSS_KEYS.index("class_error")] == 100.0
        for k in OUT_KEYS:
            data[f"c{n}_{k}"] = out[k]
        data[f"c{n}_objects"] = np.concatenate(objects).astype(np.float32).reshape(-1, W)
        data[f"c{n}_sizes"] = np.asarray(sizes, np.int32)
        data[f"c{n}_index_i"] = np.concatenate([i for i, _ in idx]).astype(np.int64)
        data[f"c{n}_index_j"] = np.concatenate([j for _, j in idx]).astype(np.int64)
        data[f"c{n}_cost"] = np.concatenate([c.reshape(-1) for c in blocks]).astype(np.float32)
        data[f"c{n}_losses"] = vals
    ref_matcher.linear_sum_assignment = real_lsa
    assert excluded <= MAX_EXCLUDED, f"{excluded} frames change their assignment under +-{PERTURB}"
    for name, (ratio, K) in sorted(worst.items()):
        print("  reference float32 vs restatement  %-18s largest |x - x64| / (2^-24 A) = %8.3f   largest K = %d" % (name, ratio, K))
    return data


def main():
    data = generate()
    path = os.path.join(HERE, "criterion.npz")
    if "--check" in sys.argv[1:]:
        have = np.load(path, allow_pickle=False)
        assert sorted(have.files) == sorted(data), "the stored fixture has other arrays"
        for k, v in data.items():
            v = np.asarray(v)
            assert have[k].dtype == v.dtype and have[k].shape == v.shape and have[k].tobytes() == v.tobytes(), k
        print("criterion golden: %d arrays regenerate bit for bit" % len(data))
        return
    np.savez_compressed(path, **data)
    print("criterion golden: %d cases, %d bytes" % (len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
