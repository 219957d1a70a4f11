"""Golden for the outputs of every decoder layer and their losses (`aux_loss: True`, the shipped configs/detr_scan_net.yaml): the
reference's own DETR and SetCriterion (src/models/detr.py:70-93, 238-253, 441-481, 556-560), imported as they lie and run on the CPU
in float32 (ResNet body: the stand-in of make_golden_detr.py).

Forward: the model of make_golden_detr.py (weights seed 0) on the 2 x 3 x 256 x 320 image of detr_small.npz -> its five aux_outputs
dicts ("main_aux{l}_{key}"); the `pre` variant of make_golden_detr_variants.py on that generator's image -> frame 0 of its five
aux_outputs ("pre_aux{l}_{key}").  Both runs' last-layer tensors are asserted equal, bit for bit, to what detr_small.npz and
detr_variants.npz already hold.
Criterion: the criterion `build(cfg)` returns for the shipped yaml (aux weights included) on the main run's outputs and synthetic
targets drawn as make_golden_criterion.py draws them: frames with (3, 5) objects, W = 12, and (3, 0) objects, W = 14, from the first
seed whose assignments (every case, layer and frame) are unchanged under 50 perturbations of every cost entry by 8 x 2^-24 times its
magnitude sum -- more than four times the error of the reference's own float32 entries, asserted -- in the manner
make_golden_criterion.py demands stability of its own cases.  Stored per case:
the targets, every returned loss with its key in the order returned, the matcher's indices of every layer (decoder order: aux 0 .. 4,
then the last layer); once: weight_dict, the matcher's costs, eos_coef.
Label mask: "{run}_margin_ok" [5, B, Q] marks the queries of every aux layer whose two largest logits lie more than MARGIN = 1e-3
apart (10 x the 1e-4 the device's outputs are held to): arg-max labels are compared only there.  Nothing is written if more than 1 %
of the queries of any layer fall under the margin.
Checked here as well: tests/criterion_ref.py, layer by layer, returns the reference's indices and bounds its losses.
Arrays only.  Run: python tests/golden/make_golden_detr_aux.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
MARGIN, MAX_UNDER = 1e-3, 0.01
TARGET_SEED, MAX_SEEDS, N_PERTURB, PERTURB_K = 41, 64, 50, 8
CASES = [((3, 5), 12), ((3, 0), 14)]      # target counts per frame, W


def margin_ok(aux, name):
    """[L-1, B, Q] bool: the top-two logit margin of every query of every aux layer exceeds MARGIN"""
    ok = []
    for l, d in enumerate(aux):
        top = np.sort(d["pred_logits"].numpy().astype(np.float64), -1)
        ok.append(top[..., -1] - top[..., -2] > MARGIN)
        under = 1.0 - ok[-1].mean()
        assert under <= MAX_UNDER, f"{name}: {100 * under:.2f} % of layer {l}'s queries have a top-two margin below {MARGIN}"
    return np.stack(ok)


def main():
    import refenv
    refenv.setup()
    import torchvision
    from make_golden_detr import _ResNet
    from make_golden_detr_variants import VARIANTS, image
    from make_golden_criterion import make_case
    torchvision.models.resnet50 = lambda replace_stride_with_dilation=None, pretrained=False, norm_layer=None: _ResNet((3, 4, 6, 3), norm_layer, replace_stride_with_dilation)
    from src.config.configs import ConfigLoader
    from src.models.detr import build as build_detector
    from odam_amd import weights
    import criterion_ref as R

    def built(**kv):
        cfg = ConfigLoader().merge_cfg(["/root/reference/configs/detr_scan_net.yaml"])
        cfg.device = "cpu"
        for k, v in kv.items():
            setattr(cfg, k, v)
        assert cfg.aux_loss, "the shipped configuration sets aux_loss"
        model, criterion, _ = build_detector(cfg)
        return cfg, model.eval(), criterion

    data = {}
    # ---- forward: the shipped configuration on the image of detr_small.npz ----
    cfg, model, crit = built()
    res = model.load_state_dict(weights.make_state_dict(seed=0), strict=False)
    assert not res.unexpected_keys and all(k.startswith("backbone.0.body.fc") for k in res.missing_keys), res
    small = np.load(os.path.join(HERE, "detr_small.npz"))
    torch.manual_seed(int(small["img_seed"]))
    with torch.no_grad():
        out = model(torch.randn(2, 3, 256, 320))
    assert len(out["aux_outputs"]) == cfg.dec_layers - 1 == 5
    for k in KEYS:
        assert np.array_equal(out[k].numpy(), small[k]), ("the last layer differs from detr_small.npz", k)
        for l, d in enumerate(out["aux_outputs"]):
            assert sorted(d) == sorted(KEYS)
            data[f"main_aux{l}_{k}"] = np.ascontiguousarray(d[k].numpy(), np.float32)
    data["main_margin_ok"] = margin_ok(out["aux_outputs"], "main")

    # ---- forward: one frame of the pre_norm variant ----
    _, pre_model, _ = built(**VARIANTS["pre"])
    res = pre_model.load_state_dict(weights.add_variant_weights(weights.make_state_dict(seed=0)), strict=False)
    assert all(k.startswith("backbone.0.body.fc") for k in res.missing_keys), res.missing_keys
    variants = np.load(os.path.join(HERE, "detr_variants.npz"))
    with torch.no_grad():
        pre = model_out = pre_model(image())
    pre_aux = [{k: d[k][:1] for k in KEYS} for d in pre["aux_outputs"]]
    for k in KEYS:
        assert np.array_equal(model_out[k].numpy(), variants[f"pre_{k}"]), ("the last layer differs from detr_variants.npz", k)
        for l, d in enumerate(pre_aux):
            data[f"pre_aux{l}_{k}"] = np.ascontiguousarray(d[k].numpy(), np.float32)
    data["pre_margin_ok"] = margin_ok(pre_aux, "pre")

    # ---- criterion: the reference's SetCriterion with the aux weights on the main run's outputs ----
    costs = dict(cost_class=float(cfg.set_cost_class), cost_bbox=float(cfg.set_cost_bbox), cost_giou=float(cfg.set_cost_giou))
    wd = {k: float(v) for k, v in crit.weight_dict.items()}
    assert len(wd) == 7 * cfg.dec_layers
    data.update({"num_classes": np.int32(crit.num_classes), "eos_coef": np.float64(crit.eos_coef), "dec_layers": np.int32(cfg.dec_layers),
                 "costs": np.asarray([costs["cost_class"], costs["cost_bbox"], costs["cost_giou"]], np.float64),
                 "weight_keys": np.asarray(list(wd)), "weight_values": np.asarray(list(wd.values()), np.float64),
                 "cases": np.asarray([(len(s), W) for s, W in CASES], np.int32)})
    calls = []
    real_forward = crit.matcher.forward

    def recorded(o, t):
        idx = real_forward(o, t)
        calls.append([(i.numpy().copy(), j.numpy().copy()) for i, j in idx])
        return idx
    crit.matcher.forward = recorded
    layers_np = [{k: d[k].numpy() for k in KEYS} for d in out["aux_outputs"]] + [{k: out[k].numpy() for k in KEYS}]
    Q = out["pred_logits"].shape[1]

    def draw(seed):
        rs = np.random.RandomState(seed)
        return [make_case(rs, Q, sizes, W)[1] for sizes, W in CASES]

    def stable(drawn, seed):
        """every assignment of every layer survives N_PERTURB perturbations of its cost block by PERTURB_K 2^-24 A per entry (A: the
        entry's magnitude sum of tests/criterion_ref.py)"""
        prs = np.random.RandomState(1000 + seed)
        for objects in drawn:
            for d in layers_np:
                for c64, A, K in R.match_cost(d["pred_logits"], d["pred_boxes"], objects, **costs):
                    c32 = c64.astype(np.float32)
                    want = R.lsap(c32)
                    for _ in range(N_PERTURB):
                        got = R.lsap((c32 + prs.uniform(-1, 1, c32.shape) * PERTURB_K * R.U * A).astype(np.float32))
                        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                            return False
        return True

    # the synthetic weights leave the queries of a frame close to one another (their boxes differ by about 1e-4), so a draw of
    # targets can put two assignments within rounding of each other: the first seed from TARGET_SEED on whose draws are stable.
    # PERTURB_K is at least four times the error of the reference's own float32 cost entries, measured below on what scipy was handed
    seed = next(s for s in range(TARGET_SEED, TARGET_SEED + MAX_SEEDS) if stable(draw(s), s))
    data["target_seed"] = np.int32(seed)
    import src.models.matcher as ref_matcher
    seen, real_lsa, ref_ratio = [], ref_matcher.linear_sum_assignment, 0.0
    ref_matcher.linear_sum_assignment = lambda c: (seen.append(c.numpy().copy()), real_lsa(c))[1]
    for n, ((sizes, W), objects) in enumerate(zip(CASES, draw(seed))):
        t_tgt = [{"objects": torch.from_numpy(o)} for o in objects]
        del calls[:], seen[:]
        with torch.no_grad():
            losses = crit(out, t_tgt)
        assert len(calls) == cfg.dec_layers
        idx_layers = calls[1:] + calls[:1]      # the reference matches the last layer first: stored in decoder order
        keys = list(losses)
        assert not any(k.startswith("class_error_") for k in keys) and len(keys) == 9 + 8 * (cfg.dec_layers - 1), keys
        vals = np.asarray([float(losses[k]) for k in keys], np.float64)
        assert np.isfinite(vals).all(), (n, dict(zip(keys, vals)))
        # the restatement, layer by layer, on the reference's numbers
        targets = [{"objects": o} for o in objects]
        blocks = seen[len(sizes):] + seen[:len(sizes)]      # float32, as scipy was handed them; decoder order
        for l, (d, idx) in enumerate(zip(layers_np, idx_layers)):
            for c32, (c64, A, K) in zip(blocks[l * len(sizes):(l + 1) * len(sizes)], R.match_cost(d["pred_logits"], d["pred_boxes"], objects, **costs)):
                assert c32.dtype == np.float32 and c32.shape == c64.shape
                if c32.size:
                    ref_ratio = max(ref_ratio, float((np.abs(c32 - c64) / (R.U * A)).max()))
            got = R.matcher(d, targets, **costs)
            for (gi, gj), (ri, rj) in zip(got, idx):
                assert np.array_equal(gi, ri) and np.array_equal(gj, rj), ("solver", n, l)
            ref = R.criterion(d, targets, idx, int(crit.num_classes), float(crit.eos_coef), {k: wd[k] for k in R.WEIGHT_KEYS}, f32_sums=True)
            assert ref["card_margin"] > 0, ("a probability at the cardinality threshold", n, l)
            sfx = "" if l == cfg.dec_layers - 1 else f"_{l}"
            for k in R.TABLE_KEYS[:9]:
                if k + sfx not in losses:
                    assert k == "class_error" and sfx
                    continue
                ok, ratio = R.within(float(losses[k + sfx]), *ref["table"][k])
                assert ok, (n, l, k, float(losses[k + sfx]), ref["table"][k], ratio)
        data[f"c{n}_objects"] = np.concatenate(objects).astype(np.float32).reshape(-1, W)
        data[f"c{n}_sizes"] = np.asarray(sizes, np.int32)
        data[f"c{n}_index_i"] = np.concatenate([i for idx in idx_layers for i, _ in idx]).astype(np.int64)
        data[f"c{n}_index_j"] = np.concatenate([j for idx in idx_layers for _, j in idx]).astype(np.int64)
        data[f"c{n}_loss_keys"] = np.asarray(keys)
        data[f"c{n}_losses"] = vals
    ref_matcher.linear_sum_assignment = real_lsa
    assert 4 * ref_ratio <= PERTURB_K, ref_ratio
    print("targets from seed %d; the reference's float32 cost entries lie within %.3f x 2^-24 A of float64, perturbed by %d x" % (seed, ref_ratio, PERTURB_K))
    path = os.path.join(HERE, "detr_aux.npz")
    np.savez_compressed(path, **data)
    print("detr_aux.npz: %d arrays, %d bytes; queries under the margin: main %s, pre %s" % (
        len(data), os.path.getsize(path), (~data["main_margin_ok"]).sum((1, 2)).tolist(), (~data["pre_margin_ok"]).sum((1, 2)).tolist()))


if __name__ == "__main__":
    main()
