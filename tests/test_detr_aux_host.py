"""Every decoder layer's outputs and their losses, without a device: the new entry points are exported, declared as the Python layer
declares them and refuse bad arguments before any device call; tests/criterion_ref.py, applied layer by layer to the reference's
own aux outputs (tests/golden/detr_aux.npz, written by make_golden_detr_aux.py), reproduces the reference's aux losses, indices
and key set; criterion.build and SetCriterion.total with the aux weights."""
import ctypes
import os
import re

import numpy as np
import pytest

import criterion_ref as R
from conftest import REPO
from test_criterion_host import OUT_KEYS

P = ctypes.c_void_p(16)      # a pointer that only has to be non-null: every call below returns before it is followed
N = None
NEW_LOSS_ENTRIES = ("odam_detr_match_cost_layers", "odam_detr_criterion_layers")
CFG = dict(set_cost_class=1, set_cost_bbox=5, set_cost_giou=2, bbox_loss_coef=5, giou_loss_coef=2, eos_coef=0.1, dataset_file="scan_net")


def aux_fixture(z):
    """(layers: [L] dicts of the reference's outputs in decoder order, the last layer from detr_small.npz; setup; cases)"""
    small = np.load(os.path.join(REPO, "tests", "golden", "detr_small.npz"), allow_pickle=False)
    L = int(z["dec_layers"])
    layers = [{k: z[f"main_aux{l}_{k}"] for k in OUT_KEYS} for l in range(L - 1)] + [{k: small[k] for k in OUT_KEYS}]
    costs = dict(zip(("cost_class", "cost_bbox", "cost_giou"), z["costs"].tolist()))
    weights = dict(zip([str(k) for k in z["weight_keys"]], z["weight_values"].tolist()))
    B, Q = layers[0]["pred_logits"].shape[:2]
    cases = []
    for n, (nb, W) in enumerate(z["cases"].tolist()):
        sizes = z[f"c{n}_sizes"].tolist()
        assert len(sizes) == nb == B and z[f"c{n}_objects"].shape[1] == W
        o_off = np.concatenate([[0], np.cumsum(sizes)])
        targets = [{"objects": z[f"c{n}_objects"][o_off[b]:o_off[b + 1]]} for b in range(B)]
        lens = [min(Q, g) for g in sizes] * L
        i_off = np.concatenate([[0], np.cumsum(lens)])
        flat = [(z[f"c{n}_index_i"][i_off[k]:i_off[k + 1]], z[f"c{n}_index_j"][i_off[k]:i_off[k + 1]]) for k in range(L * B)]
        idx = [flat[l * B:(l + 1) * B] for l in range(L)]
        keys = [str(k) for k in z[f"c{n}_loss_keys"]]
        cases.append((targets, idx, keys, dict(zip(keys, z[f"c{n}_losses"].tolist()))))
    return layers, (int(z["num_classes"]), float(z["eos_coef"]), costs, weights), cases


def expected_keys(L):
    keys = list(R.TABLE_KEYS[:9])
    for i in range(L - 1):
        keys += [f"{k}_{i}" for k in R.TABLE_KEYS[:9] if k != "class_error"]
    return keys


def _declared(header, name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/{header}"
    c_types = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "float": ctypes.c_float}
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else c_types[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return want


def test_new_entries_are_exported_and_declared_as_python_declares_them():
    from odam_amd import _lib, criterion, detector
    L = _lib.lib()
    for name in NEW_LOSS_ENTRIES:
        assert hasattr(L, name), f"the built library has no {name}"
        assert criterion.LOSS_ARGTYPES[name] == _declared("odam_loss.h", name), name
        assert criterion._entry(name).restype is ctypes.c_int
    assert hasattr(L, "odam_detr_forward_aux")
    assert detector.FORWARD_AUX_ARGTYPES == _declared("odam_detr.h", "odam_detr_forward_aux")
    # the layered entries are the single-layer ones with L in front of B
    for old, new in (("odam_detr_match_cost", NEW_LOSS_ENTRIES[0]), ("odam_detr_criterion", NEW_LOSS_ENTRIES[1])):
        a, b = criterion.LOSS_ARGTYPES[old], criterion.LOSS_ARGTYPES[new]
        at = a.index(ctypes.c_int)
        assert b == a[:at] + [ctypes.c_int] + a[at:]


def test_forward_aux_refuses_before_the_device():
    """a handle that was never finalised owns no device memory: every refusal below comes back with code 1"""
    from odam_amd import _lib, detector
    from test_detr_ops_args_host import make_cfg
    L = _lib.lib()
    f = detector._forward_aux_entry()
    m = ctypes.c_void_p(0)
    cfg = make_cfg()
    assert L.odam_detr_create(ctypes.byref(cfg), ctypes.byref(m)) == 0 and m.value

    def call(handle=m, img=P, B=2, mask=N, pos=N, outs=(P,) * 6, feat=N, fpl=2):
        return f(handle, img, B, mask, pos, *outs, feat, fpl, N)
    try:
        def err():
            return L.odam_last_error().decode()
        assert call(handle=N) == 1 and err().startswith("odam_detr_forward_aux:") and "null pointer" in err()
        assert call(img=N) == 1 and "null pointer" in err()
        for k in range(6):
            assert call(outs=tuple(N if i == k else P for i in range(6))) == 1 and "null pointer" in err(), k
        assert call(mask=P) == 1 and "go together" in err()
        assert call(pos=P) == 1 and "go together" in err()
        assert call(B=2, fpl=1) == 1 and "frames_per_layer" in err()
        assert call(B=1, fpl=0) == 1 and "frames_per_layer" in err()
        assert call(B=2, fpl=2) == 1 and "call odam_detr_finalize first" in err()
        assert call(B=2, fpl=5, mask=P, pos=P, feat=P) == 1 and "call odam_detr_finalize first" in err()
        assert err().startswith("odam_detr_forward_aux:")
    finally:
        assert L.odam_detr_destroy(m) == 0


def test_layered_criterion_entries_refuse_before_the_device():
    from odam_amd import _lib, criterion
    L = _lib.lib()

    def cost(**kw):
        a = dict(logits=P, boxes=P, L=3, B=0, Q=100, n_logit=19, objects=P, obj_off=P, n_obj=5, W=12, out=P, status=P)
        a.update(kw)
        return criterion._entry("odam_detr_match_cost_layers")(a["logits"], a["boxes"], a["L"], a["B"], a["Q"], a["n_logit"], a["objects"],
                                                               a["obj_off"], a["n_obj"], a["W"], 1.0, 5.0, 2.0, a["out"], a["status"], None)
    for kw in [dict(L=0), dict(L=-1), dict(B=-1), dict(Q=-1), dict(n_obj=-1), dict(n_logit=1), dict(W=11), dict(logits=None), dict(boxes=None),
               dict(objects=None), dict(obj_off=None), dict(out=None), dict(status=None)]:
        assert cost(**kw) == 1 and b"odam_detr_match_cost_layers" in L.odam_last_error(), kw
    assert cost(L=0, B=2) == 1 and b"at least one layer" in L.odam_last_error()
    assert cost(B=0) == 0      # no frame: nothing to do, nothing launched

    w = (ctypes.c_double * 7)(1, 5, 2, 1, 3, 1, 1)

    def crit(**kw):
        a = dict(outs=[P] * 6, L=3, B=2, Q=100, n_logit=19, n_angle=30, objects=P, obj_off=P, n_obj=5, W=12, match=P, num_boxes=5.0,
                 weights=ctypes.cast(w, ctypes.c_void_p), partial=P, table=P, status=P)
        a.update(kw)
        return criterion._entry("odam_detr_criterion_layers")(*a["outs"], a["L"], a["B"], a["Q"], a["n_logit"], a["n_angle"], a["objects"],
                                                              a["obj_off"], a["n_obj"], a["W"], a["match"], a["num_boxes"], 0.1,
                                                              a["weights"], a["partial"], a["table"], a["status"], None)
    for kw in [dict(L=0), dict(L=-2), dict(B=0), dict(B=-1), dict(Q=-1), dict(n_obj=-1), dict(n_logit=1), dict(n_angle=0), dict(W=11),
               dict(num_boxes=0.0), dict(num_boxes=float("nan")), dict(objects=None), dict(obj_off=None), dict(match=None), dict(weights=None),
               dict(partial=None), dict(table=None), dict(status=None)]:
        assert crit(**kw) == 1 and b"odam_detr_criterion_layers" in L.odam_last_error(), kw
    assert crit(L=0) == 1 and b"at least one layer" in L.odam_last_error()
    for k in range(6):
        assert crit(outs=[None if i == k else P for i in range(6)]) == 1


def test_fixture_holds_what_the_issue_names(golden):
    z = golden("detr_aux.npz")
    layers, (num_classes, eos, costs, weights), cases = aux_fixture(z)
    L = len(layers)
    assert L == 6 and num_classes == 18
    for d in layers:
        assert d["pred_logits"].shape == (2, 100, 19) and all(v.dtype == np.float32 for v in d.values())
    for l in range(L - 1):
        assert z[f"pre_aux{l}_pred_logits"].shape == (1, 100, 19)
    sizes = [tuple(z[f"c{n}_sizes"].tolist()) for n in range(len(cases))]
    assert (3, 5) in sizes and any(0 in s for s in sizes)
    for run, B in (("main", 2), ("pre", 1)):
        ok = z[f"{run}_margin_ok"]
        assert ok.shape == (L - 1, B, 100) and ok.dtype == np.bool_
        assert ((~ok).reshape(L - 1, -1).mean(1) <= 0.01).all()
        for l in range(L - 1):      # the mask is the margin it says it is
            top = np.sort(z[f"{run}_aux{l}_pred_logits"].astype(np.float64), -1)
            assert np.array_equal(ok[l], top[..., -1] - top[..., -2] > 1e-3)
    for targets, idx, keys, losses in cases:
        assert sorted(keys) == sorted(expected_keys(L)) and not any(k.startswith("class_error_") for k in keys)
        assert np.isfinite(list(losses.values())).all()
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "detr_aux.npz")) < 1 << 20


def test_restatement_layer_by_layer_against_the_reference(golden):
    """tests/criterion_ref.py on every layer of the reference's outputs: the matcher's indices exactly, every aux loss of the
    reference (float32, sums included) within K 2^-24 A of the float64 restatement -- the bound
    test_criterion_gpu.py::test_criterion_against_the_reference_run holds that pair to"""
    layers, (num_classes, eos, costs, weights), cases = aux_fixture(golden("detr_aux.npz"))
    L = len(layers)
    base = {k: weights[k] for k in R.WEIGHT_KEYS}
    for n, (targets, idx, keys, losses) in enumerate(cases):
        seen = set()
        for l, d in enumerate(layers):
            got = R.matcher(d, targets, **costs)
            for b, ((gi, gj), (ri, rj)) in enumerate(zip(got, idx[l])):
                assert np.array_equal(gi, ri) and np.array_equal(gj, rj), (n, l, b)
            ref = R.criterion(d, targets, idx[l], num_classes, eos, base, f32_sums=True)
            assert ref["card_margin"] > 0
            sfx = "" if l == L - 1 else f"_{l}"
            for k in R.TABLE_KEYS[:9]:
                if k == "class_error" and sfx:
                    assert k + sfx not in losses
                    continue
                x64, A, K = ref["table"][k]
                ok, ratio = R.within(losses[k + sfx], x64, A, K)
                assert ok, (n, l, k, losses[k + sfx], x64, ratio, K)
                seen.add(k + sfx)
        assert seen == set(keys)


def test_build_adds_the_aux_weights_only_when_asked(golden):
    from odam_amd import criterion
    z = golden("detr_aux.npz")
    _, (num_classes, eos, costs, weights), _ = aux_fixture(z)
    cfg = dict(CFG, set_cost_class=costs["cost_class"], set_cost_bbox=costs["cost_bbox"], set_cost_giou=costs["cost_giou"], eos_coef=eos)
    today = {"loss_ce": 1, "loss_bbox": 5, "loss_angle": 1, "loss_offset": 3, "loss_size": 1, "loss_depth": 1, "loss_giou": 2}
    c = criterion.build(dict(cfg, aux_loss=True, dec_layers=6))
    assert c.weight_dict == weights and list(c.weight_dict) == list(weights)      # the reference's dict, key order included
    assert len(c.weight_dict) == 7 * 6 and c.num_classes == num_classes
    for args in (cfg, dict(cfg, aux_loss=False), dict(cfg, aux_loss=False, dec_layers=6), dict(cfg, dec_layers=6)):
        w = criterion.build(args).weight_dict
        assert w == today and list(w) == list(today)
    assert criterion.build(dict(cfg, aux_loss=True, dec_layers=1)).weight_dict == today
    with pytest.raises(KeyError):
        criterion.build(dict(cfg, aux_loss=True))


def test_total_over_the_layers(golden):
    from odam_amd import criterion
    _, (num_classes, eos, costs, weights), cases = aux_fixture(golden("detr_aux.npz"))
    c = criterion.SetCriterion(num_classes, criterion.HungarianMatcher(**costs), weights, eos, list(R.LOSS_NAMES))
    for targets, idx, keys, losses in cases:
        # the reference's engine: sum(loss_dict[k] * weight_dict[k] for k in loss_dict.keys() if k in weight_dict)
        want = sum(losses[k] * weights[k] for k in losses if k in weights)
        got = float(c.total(losses))
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
        # the order: today's keys first, then layer 0, 1, ... each in WEIGHT_KEYS order
        tot = 0.0
        for k in R.WEIGHT_KEYS:
            tot = tot + float(weights[k]) * losses[k]
        for i in range(5):
            for k in R.WEIGHT_KEYS:
                tot = tot + float(weights[f"{k}_{i}"]) * losses[f"{k}_{i}"]
        assert got == tot
        # a dict without aux keys: bitwise what it is today (the old formula)
        plain = {k: v for k, v in losses.items() if k in R.TABLE_KEYS}
        old = 0.0
        for k in criterion.WEIGHT_KEYS:
            if k in plain and k in c.weight_dict and float(c.weight_dict[k]) != 0.0:
                old = old + float(c.weight_dict[k]) * plain[k]
        assert float(c.total(plain)) == old and c.total(plain).dtype.is_floating_point
        assert np.float64(float(c.total(plain))).tobytes() == np.float64(old).tobytes()


def test_status_words_of_a_layered_call_name_their_layers():
    from odam_amd import _lib, criterion
    words = np.zeros((3, 2), np.int64)
    criterion._raise_for_status_layers(words, "criterion")
    words[0, 1] = words[2, 1] = criterion.ST_DEGENERATE
    with pytest.raises(ValueError, match=r"degenerate.*layer 0: frame 1; layer 2 \(last\): frame 1") as e:
        criterion._raise_for_status_layers(words, "criterion")
    assert isinstance(e.value, AssertionError)      # the reference's own refusal, as for a single layer
    words[1, 0] = criterion.ST_CLASS
    with pytest.raises(IndexError, match="layer 1: frame 0"):
        criterion._raise_for_status_layers(words, "criterion")
    words[1, :] = criterion.ST_OFFSETS
    with pytest.raises(_lib.OdamError, match="layer 1: frames 0, 1"):
        criterion._raise_for_status_layers(words, "criterion")
