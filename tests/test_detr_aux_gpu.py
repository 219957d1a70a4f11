"""Every decoder layer's outputs and their losses on the device: odam_detr_forward_aux against the reference's own aux_outputs
(tests/golden/detr_aux.npz) and, in its last slot, bit for bit against the plain forward; the layered cost / criterion entries bit for
bit against the single-layer ones; SetCriterion over "aux_outputs" against the reference's run and against itself without them."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import criterion_ref as R
from test_criterion_gpu import COSTS, WEIGHTS, make_inputs
from test_criterion_host import OUT_KEYS
from test_detr_aux_host import CFG, aux_fixture, expected_keys

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_KEYS = OUT_KEYS + ("pred_obj_features",)
# the bound tests/test_detr_gpu.py::test_forward_vs_reference_golden holds the last layer to at this size, for every layer
LAYER_BOUND = 1e-4


@functools.lru_cache(maxsize=None)
def _z():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "detr_aux.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def model():
    from odam_amd import detector, weights
    det = detector.Detector(max_batch=4, device=DEV)
    det.load_state_dict(weights.make_state_dict(seed=0))
    yield det
    det.close()


def _main_image():
    from conftest import GOLDEN
    torch.manual_seed(int(np.load(os.path.join(GOLDEN, "detr_small.npz"))["img_seed"]))
    return torch.randn(2, 3, 256, 320)


def _check_layers(out, z, run, frames, measured):
    L = len(out["aux_outputs"]) + 1
    assert L == 6
    for l, d in enumerate(out["aux_outputs"]):
        assert sorted(d) == sorted(OUT_KEYS)
        for k in OUT_KEYS:
            want = z[f"{run}_aux{l}_{k}"]
            got = d[k][:frames].cpu().numpy()
            assert got.shape == want.shape, (l, k)
            err = float(np.abs(got - want).max())
            print("  %s layer %d %-12s max |device - reference| = %.3e" % (run, l, k, err))
            measured(f"aux_{run}_layer{l}_abs_err", err)
            assert err <= LAYER_BOUND, (run, l, k, err)
        ok = z[f"{run}_margin_ok"][l]
        labels = d["pred_logits"][:frames].argmax(-1).cpu().numpy()
        assert np.array_equal(labels[ok], z[f"{run}_aux{l}_pred_logits"].argmax(-1)[ok]), (run, l)


def test_every_layer_against_the_reference(model, measured):
    """R50, fp32, 2 x 3 x 256 x 320: each of the five aux layers' six tensors within 1e-4 of the reference's, labels exact where
    the fixture's top-two margin holds; the last slot within the same bound of detr_small.npz"""
    from conftest import GOLDEN
    z = _z()
    out = model(_main_image().to(DEV), aux=True)
    _check_layers(out, z, "main", 2, measured)
    small = np.load(os.path.join(GOLDEN, "detr_small.npz"))
    for k in OUT_KEYS:
        assert np.abs(out[k].cpu().numpy() - small[k]).max() <= LAYER_BOUND, k


def test_every_layer_of_the_pre_norm_variant_against_the_reference(measured):
    from odam_amd import detector, weights
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_detr_variants import image
    det, _, _ = detector.build({"pre_norm": True})
    try:
        det.load_state_dict(weights.add_variant_weights(weights.make_state_dict(seed=0)))
        out = det(image().to(DEV), aux=True)      # both frames, as the reference ran them; the fixture holds frame 0
        _check_layers(out, _z(), "pre", 1, measured)
    finally:
        det.close()


def _same(a, b):
    for k in ALL_KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_last_slot_is_the_plain_forward_bit_for_bit(dtype):
    """a same-size batch of 2, a mixed-size pair (forward_nested) and a batch of 3 on max_batch = 2 (two native calls into one
    block, frames_per_layer = 3 > B)"""
    from odam_amd import detector, weights
    det = detector.Detector(backbone="resnet18", max_batch=2, device=DEV, n_streams=1, dtype=dtype)
    try:
        det.load_state_dict(weights.make_state_dict(backbone="resnet18", seed=0))
        torch.manual_seed(11)
        x = torch.randn(3, 3, 192, 256).to(DEV)
        for xb in (x[:2], x):
            plain, aux = det(xb), det(xb, aux=True)
            assert sorted(aux) == sorted(list(plain) + ["aux_outputs"]) and aux["_hw"] == plain["_hw"]
            _same(aux, plain)
            assert len(aux["aux_outputs"]) == 5
            for d in aux["aux_outputs"]:
                assert sorted(d) == sorted(OUT_KEYS)
                for k in OUT_KEYS:
                    assert d[k].shape == plain[k].shape and torch.isfinite(d[k]).all()
            # views into one block per key: nothing was copied
            for k in OUT_KEYS:
                n = aux[k].numel() * 4
                for l, d in enumerate(aux["aux_outputs"]):
                    assert d[k].data_ptr() == aux["aux_outputs"][0][k].data_ptr() + l * n
                assert aux[k].data_ptr() == aux["aux_outputs"][0][k].data_ptr() + 5 * n
            assert not torch.equal(aux["aux_outputs"][0]["pred_logits"], aux["pred_logits"])
        # the chunked call: every frame's layers are those of the frame run in a batch of its own chunk
        first = det(x[:2], aux=True)
        for l in range(5):
            assert torch.equal(aux["aux_outputs"][l]["pred_boxes"][:2], first["aux_outputs"][l]["pred_boxes"])
        pair = [torch.randn(3, 192, 256), torch.randn(3, 160, 224)]
        plain, aux = det.forward_nested(pair), det.forward_nested(pair, aux=True)
        _same(aux, plain)
        assert len(aux["aux_outputs"]) == 5 and all(torch.isfinite(d[k]).all() for d in aux["aux_outputs"] for k in OUT_KEYS)
        _same(det(pair, aux=True), plain)      # __call__ hands a mixed-size list on, aux included
    finally:
        det.close()


@pytest.mark.parametrize("dec_layers", [1, 2])
def test_small_transformers(dec_layers):
    from odam_amd import detector, weights
    arch = dict(backbone="resnet18", hidden_dim=128, nheads=4, enc_layers=1, dec_layers=dec_layers, dim_feedforward=256)
    det = detector.Detector(max_batch=2, device=DEV, n_streams=1, **arch)
    try:
        det.load_state_dict(weights.make_state_dict(backbone="resnet18", hidden=128, ffn=256, enc_layers=1, dec_layers=dec_layers, seed=0))
        torch.manual_seed(5)
        x = torch.randn(2, 3, 128, 160).to(DEV)
        plain, aux = det(x), det(x, aux=True)
        _same(aux, plain)
        if dec_layers == 1:
            assert aux["aux_outputs"] == []
            return
        (d,) = aux["aux_outputs"]
        assert sorted(d) == sorted(OUT_KEYS)
        for k in OUT_KEYS:
            assert d[k].shape == plain[k].shape and d[k].dtype == torch.float32 and torch.isfinite(d[k]).all(), k
        assert d["pred_logits"].shape == (2, 100, 19) and d["pred_angle"].shape == (2, 100, 30)
        assert (d["pred_boxes"] > 0).all() and (d["pred_boxes"] < 1).all()
    finally:
        det.close()


# ---- the layered entries against the single-layer ones ---------------------------------------------------------------------

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _run(entry_cost, entry_crit, lead, t, objects, d_off, n_obj, W, B, Q, sizes, L):
    """cost -> solver -> criterion through the raw entries on tensors with (lead = (L,)) or without (lead = ()) a layer dimension;
    returns host copies (cost, cost status, col_of_row, partial, table, status)"""
    from odam_amd import _lib, criterion
    n_logit, n_angle = t["pred_logits"].shape[-1], t["pred_angle"].shape[-1]
    nl = max(L, 1)
    cost = torch.full((nl, max(Q * n_obj, 1)), -7.0, device=DEV)
    st_cost = torch.full((nl, B), -1, device=DEV, dtype=torch.int32)
    _lib.check(criterion._entry(entry_cost)(_ptr(t["pred_logits"]), _ptr(t["pred_boxes"]), *lead, B, Q, n_logit, _ptr(objects), _ptr(d_off), n_obj,
                                            W, COSTS["cost_class"], COSTS["cost_bbox"], COSTS["cost_giou"], _ptr(cost), _ptr(st_cost), _stream()),
               entry_cost)
    off = np.concatenate([[0], np.cumsum(sizes)])
    c_off = np.concatenate([l * Q * n_obj + Q * off[:-1] for l in range(nl)])
    col, _, _ = criterion.solve(cost, [(Q, g) for g in sizes] * nl, c_off, torch.device(DEV))
    match = col.view(nl, B, Q).contiguous()
    partial = torch.full((nl, B, 11), -3.0, device=DEV, dtype=torch.float64)
    table = torch.full((nl, 10), -3.0, device=DEV, dtype=torch.float64)
    status = torch.full((nl, B), -1, device=DEV, dtype=torch.int32)
    w = (ctypes.c_double * 7)(*[float(WEIGHTS[k]) for k in R.WEIGHT_KEYS])
    _lib.check(criterion._entry(entry_crit)(*[_ptr(t[k]) for k in OUT_KEYS], *lead, B, Q, n_logit, n_angle, _ptr(objects), _ptr(d_off), n_obj, W,
                                            _ptr(match), float(max(n_obj, 1)), 0.1, ctypes.cast(w, ctypes.c_void_p), _ptr(partial), _ptr(table),
                                            _ptr(status), _stream()), entry_crit)
    return [x.cpu().numpy() for x in (cost, st_cost, match, partial, table, status)]


def _layered_vs_single(rs, B, Q, sizes, W, L, n_logit=19, n_angle=30):
    layers, targets = [], None
    for l in range(L):
        out, tg = make_inputs(rs, B, Q, sizes, n_logit, W, n_angle)
        layers.append(out)
        targets = targets or tg      # the targets of frame b serve every layer
    objects = torch.from_numpy(np.concatenate([t["objects"] for t in targets] + [np.zeros((1, W), np.float32)])).to(DEV)
    n_obj = int(sum(sizes))
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(DEV)
    single = []
    for out in layers:
        t = {k: torch.from_numpy(out[k]).to(DEV) for k in OUT_KEYS}
        single.append(_run("odam_detr_match_cost", "odam_detr_criterion", (), t, objects, d_off, n_obj, W, B, Q, sizes, 0))

    def layered(order):
        t = {k: torch.from_numpy(np.stack([layers[l][k] for l in order])).to(DEV) for k in OUT_KEYS}
        return _run("odam_detr_match_cost_layers", "odam_detr_criterion_layers", (L,), t, objects, d_off, n_obj, W, B, Q, sizes, L)
    orders = [list(range(L))] + ([list(range(L))[::-1], [(l + 1) % L for l in range(L)]] if L > 1 else [])
    for order in orders:
        got = layered(order)
        for slot, l in enumerate(order):
            for name, g, s in zip(("cost", "cost status", "col_of_row", "partial", "table", "status"), got, single[l]):
                assert g[slot].tobytes() == s[0].tobytes(), (name, B, Q, sizes, W, L, order, slot)
        assert not got[1].any() and not got[5].any()
        assert np.isfinite(got[4]).all()


@pytest.mark.parametrize("L", [1, 3, 6])
def test_layered_entries_are_the_single_layer_entries_bit_for_bit(L):
    """Q = 20, 19 logits, 30 angle bins, W 12 and 14, B 1 and 3 with 0, 3 and 5 targets; layer l of a layered call holds the bits of
    the single-layer call on layer l's tensors -- cost block, status, assignment, partial sums, table -- in every position (the
    layers reversed and rotated), and L = 1 is the existing entries"""
    rs = np.random.RandomState(50 + L)
    for B, sizes, W in ((1, (3,), 12), (1, (0,), 14), (3, (0, 3, 5), 12), (3, (5, 0, 3), 14), (3, (0, 0, 0), 12)):
        _layered_vs_single(rs, B, 20, sizes, W, L)


def test_layered_entries_with_a_frame_beyond_the_device_solver():
    """33 targets at Q = 100: that problem of every layer goes to scipy from the device's cost block, the others stay on the device"""
    _layered_vs_single(np.random.RandomState(60), 2, 100, (33, 4), 12, 3)


# ---- SetCriterion over aux_outputs ------------------------------------------------------------------------------------------

def _criterion_of(weights, costs, num_classes, eos):
    from odam_amd import criterion
    return criterion.SetCriterion(num_classes, criterion.HungarianMatcher(**costs), weights, eos, list(R.LOSS_NAMES))


def _launches(monkeypatch):
    """counts the calls of the loss entries"""
    from odam_amd import criterion
    counts = {}
    real = criterion._entry

    def counting(name):
        f = real(name)

        def call(*a):
            counts[name] = counts.get(name, 0) + 1
            return f(*a)
        return call
    monkeypatch.setattr(criterion, "_entry", counting)
    return counts


def test_set_criterion_on_the_reference_aux_outputs(measured, monkeypatch):
    """the fixture's reference outputs, uploaded: every returned key within the sum of both bounds of the reference's float32 value
    (as test_criterion_against_the_reference_run, per layer), the indices the reference's; one layered cost call, one solver call,
    one layered criterion call for all six layers"""
    layers, (num_classes, eos, costs, weights), cases = aux_fixture(_z())
    L = len(layers)
    crit = _criterion_of(weights, costs, num_classes, eos)
    up = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    outputs = up(layers[-1])
    outputs["aux_outputs"] = [up(d) for d in layers[:-1]]
    base = {k: weights[k] for k in R.WEIGHT_KEYS}
    for n, (targets, idx, keys, losses) in enumerate(cases):
        counts = _launches(monkeypatch)
        got = crit(outputs, targets)
        monkeypatch.undo()
        assert counts == {"odam_detr_match_cost_layers": 1, "odam_lsap_batch": 1, "odam_detr_criterion_layers": 1}, counts
        assert list(got) == keys and sorted(got) == sorted(expected_keys(L))      # the reference's keys, in the reference's order
        assert all(v.dim() == 0 and v.dtype == torch.float64 for v in got.values())
        for l in range(L):
            sfx = "" if l == L - 1 else f"_{l}"
            ref = R.criterion(layers[l], targets, idx[l], num_classes, eos, base)
            ref32 = R.criterion(layers[l], targets, idx[l], num_classes, eos, base, f32_sums=True)
            for k in R.TABLE_KEYS[:9]:
                if k + sfx not in got:
                    continue
                x64, A, K = ref["table"][k]
                v, want = float(got[k + sfx]), losses[k + sfx]
                ok, ratio = R.within(v, x64, A, K)
                measured(f"aux_criterion_{k}_ratio", ratio)
                assert ok, (n, l, k, v, x64, ratio, K)
                assert abs(v - want) <= (K + ref32["table"][k][2]) * R.U * A or v == want, (n, l, k, v, want)
        assert crit.last_table_layers.shape == (L, 10) and crit.last_partial_layers.shape == (L, 2, 11)
        assert torch.equal(crit.last_table, crit.last_table_layers[L - 1]) and torch.equal(crit.last_partial, crit.last_partial_layers[L - 1])
        # the last layer's entries are those of the call without aux_outputs, bit for bit
        alone = crit({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets)
        assert all(float(alone[k]) == float(got[k]) for k in alone) and sorted(alone) == sorted(R.TABLE_KEYS[:9])
        assert crit.last_table_layers.shape == (1, 10)


def test_a_callers_matcher_is_called_once_per_layer():
    from odam_amd import criterion
    layers, (num_classes, eos, costs, weights), cases = aux_fixture(_z())
    targets, idx, keys, losses = cases[0]
    outputs = dict(layers[-1], aux_outputs=layers[:-1])      # host arrays are accepted
    full = _criterion_of(weights, costs, num_classes, eos)(outputs, targets)
    calls = []

    def given(o, t):
        l = next(l for l, d in enumerate(layers) if o["pred_logits"] is d["pred_logits"])
        calls.append(l)
        assert "aux_outputs" not in o
        return [(torch.from_numpy(i), torch.from_numpy(j)) for i, j in idx[l]]
    got = criterion.SetCriterion(num_classes, given, weights, eos, list(R.LOSS_NAMES))(outputs, targets, num_boxes=None)
    assert sorted(calls) == list(range(len(layers)))
    assert list(got) == list(full) and all(float(got[k]) == float(full[k]) for k in full)
    # num_boxes of the call serves every layer
    half = _criterion_of(weights, costs, num_classes, eos)(outputs, targets, num_boxes=4.0)
    for k in ("loss_bbox", "loss_bbox_0", "loss_angle_4"):
        assert float(half[k]) == pytest.approx(float(full[k]) * 8.0 / 4.0, rel=1e-12)
    assert float(half["loss_ce_2"]) == float(full["loss_ce_2"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detector_aux_outputs_through_the_criterion(dtype):
    from odam_amd import criterion, detector, weights
    det = detector.Detector(backbone="resnet18", max_batch=2, device=DEV, n_streams=1, dtype=dtype)
    try:
        det.load_state_dict(weights.make_state_dict(backbone="resnet18", seed=0))
        torch.manual_seed(4)
        out = det(torch.randn(2, 3, 192, 256).to(DEV), aux=True)
        _, targets = make_inputs(np.random.RandomState(12), 2, 1, (6, 0), 19, 12)
        crit = criterion.build(dict(CFG, aux_loss=True, dec_layers=6))
        # the blocks of the detector go to the kernels as they lie: a view, not a copy
        blk = criterion._layer_block([d["pred_logits"] for d in out["aux_outputs"]] + [out["pred_logits"]])
        assert blk.data_ptr() == out["aux_outputs"][0]["pred_logits"].data_ptr() and blk.shape == (6, 2, 100, 19)
        got = crit(out, targets)
        assert sorted(got) == sorted(expected_keys(6))
        assert all(np.isfinite(float(v)) for v in got.values()), got
        assert np.isfinite(float(crit.total(got)))
        alone = crit({k: v for k, v in out.items() if k != "aux_outputs"}, targets)
        assert all(float(alone[k]) == float(got[k]) for k in alone)
        # every layer alone, through the single-layer path, gives that layer's entries
        for i, d in enumerate(out["aux_outputs"]):
            one = crit(d, targets)
            for k in one:
                if k != "class_error":
                    assert float(one[k]) == float(got[f"{k}_{i}"]), (i, k)
    finally:
        det.close()


def test_a_degenerate_target_names_every_layer():
    """a target box with a negative width: a status word per (layer, frame), no device assert; the exception is the reference's
    AssertionError and a ValueError that names frame 1 for each of the six layers"""
    layers, (num_classes, eos, costs, weights), cases = aux_fixture(_z())
    targets, idx, _, _ = cases[0]
    outputs = dict(layers[-1], aux_outputs=layers[:-1])
    crit = _criterion_of(weights, costs, num_classes, eos)
    bad = [{"objects": t["objects"].copy()} for t in targets]
    bad[1]["objects"][2, 3] = -0.3
    with pytest.raises(ValueError, match="degenerate") as e:
        crit(outputs, bad)
    assert isinstance(e.value, AssertionError)
    msg = str(e.value)
    for l in range(6):
        assert ("layer %d%s: frame 1" % (l, " (last)" if l == 5 else "")) in msg, msg
    assert "frame 0" not in msg and "frames" not in msg
    lab = [{"objects": t["objects"].copy()} for t in targets]
    lab[0]["objects"][1, 0] = num_classes + 1
    with pytest.raises(IndexError, match="layer 0: frame 0"):
        crit(outputs, lab)
    crit(outputs, targets)      # and the criterion goes on working
