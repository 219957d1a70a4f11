"""Detector oracle (oracle/detr_oracle.py) and the product's host-side detector code against vectors produced
by the reference's own DETR / postprocess / run_detector (tests/golden/make_golden_detr.py).  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import detr_oracle as O  # noqa: E402

K = np.array([[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]])
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
POST = ("bboxes", "dimensions", "angles", "translates", "classes", "scores")


@pytest.fixture(scope="module")
def sd():
    from odam_amd import weights
    return weights.make_state_dict(seed=0)


def test_bf16_attention_key_mask():
    """_attention_b with a key-padding mask: masked keys have no influence on the output bits, and the result is the float64
    masked softmax up to the bf16 roundings the oracle models (P and O, 2^-8 each); the fma form of the exponent agrees too"""
    g = torch.Generator().manual_seed(0)
    q = O._rb(torch.randn(2, 70, 256, generator=g))
    k, v = O._rb(torch.randn(2, 150, 256, generator=g)), O._rb(torch.randn(2, 150, 256, generator=g))
    mask = torch.zeros(2, 150, dtype=torch.bool)
    mask[0, :64] = True               # the whole first tile
    mask[1, 100:] = True              # the tail tile and part of the second
    s = (q.double().reshape(2, 70, 8, 32).transpose(1, 2) @ k.double().reshape(2, 150, 8, 32).permute(0, 2, 3, 1)) * (1 / 32) ** 0.5
    p = torch.softmax(s.masked_fill(mask[:, None, None, :], -float("inf")), -1)
    ref = (p @ v.double().reshape(2, 150, 8, 32).transpose(1, 2)).transpose(1, 2).reshape(2, 70, 256)
    k2, v2 = k.clone(), v.clone()
    k2[mask], v2[mask] = 64.0, -1000.0
    for fma in (False, True):
        got = O._attention_b(q, k, v, 8, key_mask=mask, fma=fma)
        assert torch.equal(got, O._attention_b(q, k2, v2, 8, key_mask=mask, fma=fma))
        assert ((got.double() - ref).abs() <= 2.0 ** -8 * (v.abs().max() + ref.abs()) + 1e-6).all()


def test_full_size_forward_matches_reference_detr(sd, golden):
    """oracle vs the reference's DETR on one 3x800x1066 frame"""
    z = golden("detr_full.npz")
    torch.manual_seed(int(z["img_seed"]))
    img = torch.randn(1, 3, 800, 1066)
    out = O.detr_forward(sd, img)
    for k in KEYS:
        assert np.abs(out[k].numpy() - z[k]).max() <= 2e-5 * max(1.0, float(np.abs(z[k]).max())), k
    assert np.array_equal(out["pred_logits"].argmax(-1).numpy(), z["pred_logits"].argmax(-1))


def test_forward_matches_reference_detr(sd, golden):
    z = golden("detr_small.npz")
    torch.manual_seed(int(z["img_seed"]))
    img = torch.randn(2, 3, 256, 320)
    out = O.detr_forward(sd, img)
    for k in KEYS:
        assert np.abs(out[k].numpy() - z[k]).max() <= 2e-5, k
    assert np.array_equal(out["pred_logits"].argmax(-1).numpy(), z["pred_logits"].argmax(-1))
    post = O.postprocess(out, (640, 480), 0.6, K)
    for b in range(2):
        assert np.array_equal(post["classes"][b], z[f"post{b}_classes"])
        for k in POST:
            assert np.allclose(post[k][b], z[f"post{b}_{k}"], rtol=1e-5, atol=1e-4), (b, k)


@pytest.mark.parametrize("variant", ["pre", "learned", "pre_learned", "dc5"])
def test_config_variants_match_reference_detr(sd, golden, variant):
    """`pre_norm: True` (transformer.py:169-188, 240-262, 26-28), `position_embedding: 'learned'` (position_encoding.py:49-74) and
    `dilation: True` (backbone.py:89-91; 16 x 20 tokens instead of 8 x 10):
    the oracle against the reference's DETR built with those config keys (tests/golden/make_golden_detr_variants.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_detr_variants import image
    from odam_amd import weights
    z = golden("detr_variants.npz")
    sdv = weights.add_variant_weights(dict(sd))
    out = O.detr_forward(sdv, image(), pre_norm=variant.startswith("pre"), learned_pos=variant.endswith("learned"), dilation=variant == "dc5")
    for k in KEYS:
        assert np.abs(out[k].numpy() - z[f"{variant}_{k}"]).max() <= 2e-5 * max(1.0, float(np.abs(z[f"{variant}_{k}"]).max())), k
    assert np.array_equal(out["pred_logits"].argmax(-1).numpy(), z[f"{variant}_pred_logits"].argmax(-1))


def test_learned_position_table_matches_oracle():
    from odam_amd import weights
    from odam_amd.detector import learned_position_embedding
    sdv = weights.add_variant_weights({})
    ref = O.position_embedding_learned(sdv, 25, 34)[0].permute(1, 2, 0).reshape(25 * 34, 256)
    mine = learned_position_embedding(sdv["backbone.1.row_embed.weight"], sdv["backbone.1.col_embed.weight"], 25, 34)
    assert torch.equal(mine, ref)


def test_position_embedding_bit_exact(golden):
    from odam_amd.detector import sine_position_embedding
    ref = golden("detr_small.npz")["pos_25x34"]                      # [1,256,25,34]
    assert np.array_equal(O.position_embedding(25, 34).numpy(), ref)
    mine = sine_position_embedding(25, 34).numpy().reshape(25, 34, 256).transpose(2, 0, 1)[None]
    assert np.array_equal(mine, ref)


def _rows16(pred, img_w, img_h):
    """numpy float32 restatement of the per-query arithmetic (what odam_detr_postprocess computes on device)"""
    f32 = np.float32
    lg = torch.from_numpy(pred["pred_logits"]).softmax(-1)[..., :-1]
    score, cls = lg.max(-1)
    bx = pred["pred_boxes"]
    x0 = (bx[..., 0] - f32(0.5) * bx[..., 2]) * f32(img_w); y0 = (bx[..., 1] - f32(0.5) * bx[..., 3]) * f32(img_h)
    x1 = (bx[..., 0] + f32(0.5) * bx[..., 2]) * f32(img_w); y1 = (bx[..., 1] + f32(0.5) * bx[..., 3]) * f32(img_h)
    d = pred["pred_depth"][..., 0]
    scx = pred["pred_offset"][..., 0] * f32(img_w) + (x0 + x1) / f32(2); scy = pred["pred_offset"][..., 1] * f32(img_h) + (y0 + y1) / f32(2)
    c3x = (scx - f32(K[0, 2])) / f32(K[0, 0]) * d; c3y = (scy - f32(K[1, 2])) / f32(K[1, 1]) * d
    rows = np.zeros(bx.shape[:2] + (16,), np.float32)
    rows[..., 0] = score.numpy(); rows[..., 1] = cls.numpy()
    rows[..., 2], rows[..., 3], rows[..., 4], rows[..., 5] = x0, y0, x1, y1
    rows[..., 6], rows[..., 7], rows[..., 8] = c3x, c3y, d
    rows[..., 9] = pred["pred_angle"].argmax(-1)
    rows[..., 10:13] = pred["pred_size"]
    return rows


def test_select_nms_matches_reference_postprocess(golden):
    """odam_detr_select (C++ threshold + greedy 3D/2D NMS) against DETR.postprocess/nms_3d of the reference on
    hand-built predictions with near-threshold scores and heavy overlaps."""
    from odam_amd.detector import Detector
    z = golden("detr_post.npz")
    pred = {k: z[k] for k in KEYS}
    rows = _rows16(pred, 640, 480)
    for b in range(rows.shape[0]):
        s = Detector.select(rows[b], 0.6, True, 30)
        assert len(s["scores"]) == len(z[f"post{b}_scores"]) > 5
        assert np.array_equal(s["classes"], z[f"post{b}_classes"])
        for k in POST:
            assert np.allclose(s[k], z[f"post{b}_{k}"], rtol=1e-6, atol=1e-4), (b, k)
    # the oracle's python NMS agrees as well
    post = O.postprocess({k: torch.from_numpy(v) for k, v in pred.items()}, (640, 480), 0.6, K)
    for b in range(rows.shape[0]):
        assert np.array_equal(post["classes"][b], z[f"post{b}_classes"])
        assert np.allclose(post["scores"][b], z[f"post{b}_scores"], rtol=1e-6)


def test_run_detector_rows_match_reference(sd, golden):
    """processor.detection_rows packing (79 columns) on the oracle's predictions for the frame the reference's
    OdamProcess.run_detector saw (same transforms object)."""
    from odam_amd import synth, transforms
    from odam_amd.processor import detection_rows
    ref = golden("detr_small.npz")["run_detector_rows"]
    frame = next(synth.make_frames(1, seed=5))
    x, _ = transforms.get_transforms()(frame, None)
    out = O.detr_forward(sd, x[None])
    post = O.postprocess(out, (640, 480), 0.6, K)
    rows = np.asarray(detection_rows(post, 0, 7, 1296, 968), np.float64).reshape(-1, 79)
    assert rows.shape == ref.shape and rows.shape[0] >= 1
    assert np.array_equal(rows[:, :2], ref[:, :2])                       # frame id, class label: exact
    assert np.allclose(rows, ref, rtol=1e-4, atol=1e-5)
    assert np.all(rows[:, 15:] == -1)


def test_select_nms_random_clusters_vs_oracle():
    """C++ threshold + greedy NMS (odam_detr_select) against the oracle's python nms_3d on 300 random frames of
    clustered, heavily overlapping detections (near-threshold scores, identical boxes with different scores, same /
    different classes): identical keep lists in identical order.  Exactly tied scores are left out: the reference
    orders them by numpy's unstable argsort."""
    from odam_amd.detector import Detector
    rs = np.random.RandomState(7)
    n_kept = 0
    for trial in range(300):
        Q = int(rs.choice([1, 5, 30, 100]))
        n_clu = int(rs.randint(1, 6))
        centres = rs.uniform(-2, 2, (n_clu, 3)).astype(np.float32) + np.array([0, 0, 3], np.float32)
        rows = np.zeros((Q, 16), np.float32)
        which = rs.randint(0, n_clu, Q)
        rows[:, 0] = rs.uniform(0.3, 1.0, Q).astype(np.float32)
        rows[rs.rand(Q) < 0.2, 0] = np.float32(0.6) - np.float32(2e-5)                # straddles the threshold once the ramp is added
        rows[:, 0] += np.arange(Q, dtype=np.float32) * np.float32(1e-6)              # no exact ties
        rows[:, 1] = rs.randint(0, 3, Q)
        jit = rs.choice([0.0, 0.02, 0.3], Q)[:, None].astype(np.float32)
        t = centres[which] + rs.normal(0, 1, (Q, 3)).astype(np.float32) * jit
        dims = np.abs(rs.normal(0.8, 0.3, (Q, 3))).astype(np.float32) + np.float32(0.05)
        dims[rs.rand(Q) < 0.3] = np.float32(0.7)                                     # identical sizes
        cx, cy = 320 + 100 * t[:, 0], 240 + 100 * t[:, 1]
        hw = 40 + 30 * rs.rand(Q, 2)
        rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = cx - hw[:, 0], cy - hw[:, 1], cx + hw[:, 0], cy + hw[:, 1]
        rows[:, 6:9] = t
        rows[:, 9] = rs.randint(0, 30, Q)
        rows[:, 10:13] = dims
        for nms_2d in (True, False):
            got = Detector.select(rows, 0.6, nms_2d, 30)
            keep = rows[:, 0] > np.float32(0.6)
            idx = np.flatnonzero(keep)
            k = O.nms_3d(rows[idx, 1].astype(np.int64), rows[idx, 0], rows[idx, 6:9], rows[idx, 10:13],
                         rows[idx, 2:6].reshape(-1, 2, 2), nms_2d=nms_2d)
            want = idx[np.asarray(k, np.int64)] if len(k) else np.zeros(0, np.int64)
            assert np.array_equal(got["scores"], rows[want, 0]), (trial, nms_2d)
            assert np.array_equal(got["classes"], rows[want, 1].astype(np.int64)), (trial, nms_2d)
            assert np.array_equal(got["translates"], rows[want, 6:9]), (trial, nms_2d)
            n_kept += len(want)
    assert n_kept > 1000


def _replay_f32(rec):
    """a record of F32_TRACE recomputed with the forward's own operations"""
    import torch.nn.functional as F
    if rec["kind"] == "linear":
        y = F.linear(rec["x"], rec["w"], rec["bias"])
    elif rec["scale"] is None:
        y = F.conv2d(rec["x"], rec["w"], rec["bias"], stride=rec["stride"], padding=rec["padding"], dilation=rec["dilation"])
    else:
        y = F.conv2d(rec["x"], rec["w"], None, stride=rec["stride"], padding=rec["padding"], dilation=rec["dilation"])
        y = y * rec["scale"].reshape(1, -1, 1, 1) + rec["bias"].reshape(1, -1, 1, 1)
    if rec["res"] is not None:
        y = y + rec["res"]
    return F.relu(y) if rec["relu"] else y


@pytest.mark.parametrize("dilation", [False, True])
def test_f32_trace(sd, dilation):
    """oracle.F32_TRACE (the fp32 teacher-forcing records): tracing leaves every output bit-identical, every record reproduces its own
    output bit for bit, and the counts are R50's -- 53 backbone convolutions + input_proj, 6 x 6 encoder and 6 x 10 decoder linears
    (four attention projections each, two feed-forward) + 16 head linears -- with 16 block records that point at their layers"""
    torch.manual_seed(5)
    img = torch.randn(1, 3, 96, 128)
    plain = O.detr_forward(sd, img, dilation=dilation)
    O.F32_TRACE = []
    try:
        traced = O.detr_forward(sd, img, dilation=dilation)
        trace = O.F32_TRACE
    finally:
        O.F32_TRACE = None
    for k in KEYS:
        assert torch.equal(plain[k], traced[k]), k
    convs = [r for r in trace if r["kind"] == "conv"]
    lins = [r for r in trace if r["kind"] == "linear"]
    blocks = [r for r in trace if r["kind"] == "block"]
    assert sum(r["name"].startswith("backbone.") for r in convs) == 53 and len(convs) == 54
    assert len(lins) == 6 * 6 + 6 * 10 + 16
    assert len(blocks) == 16 and sum(b["next_c1"] is None for b in blocks) == 1
    assert sum(r["dilation"] == 2 for r in convs) == (2 if dilation else 0)
    for r in convs + lins:
        assert torch.equal(_replay_f32(r), r["y"]), r["name"]
    for b in blocks:
        c2, c3 = trace[b["c2"]], trace[b["c3"]]
        assert c2["name"] == b["name"] + "conv2.weight" and c3["name"] == b["name"] + "conv3.weight"
        assert c3["x"] is c2["y"] and c3["res"] is not None
        if b["next_c1"] is not None:
            assert trace[b["next_c1"]]["x"] is c3["y"] and trace[b["next_c1"]]["name"].endswith("conv1.weight")
