"""ResNet-18/34 (torchvision BasicBlock) and ResNet-152 detector backbones on the device, through the C ABI, against the CPU
oracle: tests/basic_body.py (BasicBlock body, pinned against transformers.ResNetModel in tests/test_backbones_host.py) ->
oracle/detr_oracle.py transformer -> heads, fp32; the bf16 mode against the bf16-faithful restatement of the same network."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import basic_body as BB  # noqa: E402

pytestmark = pytest.mark.gpu
K = np.array([[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]])
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
DEV = "cuda:0"


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _detector(backbone, B, **kw):
    from odam_amd import detector, weights
    sd = weights.make_state_dict(backbone=backbone, seed=0)
    det = detector.Detector(backbone=backbone, max_batch=B, device=DEV, n_streams=1, **kw)
    det.load_state_dict(sd)
    return det, sd


def _check_fp32(det, sd, img, blocks, tap_tol=2e-5):
    """layer4 / memory taps, every output, labels and post-processed detections against the fp32 oracle (the bounds of
    tests/test_detr_gpu.py::test_full_size_forward_vs_oracle)"""
    import detr_oracle as O
    torch.set_num_threads(16)
    B, _, H, W = img.shape
    ref = BB.detr_forward_basic(sd, img, blocks, return_taps=True)
    out = det(img.to(DEV))
    l4, mem = det.debug_taps(B, H, W)
    assert l4.shape[1] == 512
    assert _rel(l4.cpu(), ref["_layer4"]) <= tap_tol
    assert _rel(mem.cpu(), ref["_memory"]) <= tap_tol
    for k in KEYS + ("pred_obj_features",):
        assert (out[k].cpu() - ref[k]).abs().max().item() <= 2e-4 * max(1.0, ref[k].abs().max().item()), k
    assert torch.equal(out["pred_logits"].cpu().argmax(-1), ref["pred_logits"].argmax(-1))
    pp = det.postprocess(out, (640, 480), 0.6, K)
    pref = O.postprocess(ref, (640, 480), 0.6, K)
    for b in range(B):
        assert np.array_equal(pp["classes"][b], pref["classes"][b])
        assert np.allclose(pp["translates"][b], pref["translates"][b], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("backbone,B,H,W,ring", [("resnet18", 2, 256, 320, 1), ("resnet34", 2, 256, 320, 1),
                                                 ("resnet18", 3, 487, 601, 1), ("resnet34", 3, 487, 601, 2)])
def test_basic_backbone_forward_vs_oracle(backbone, B, H, W, ring):
    """ring 2: every eligible layer on the 256-row ring kernel (ragged last tiles of the BasicBlock shapes there)"""
    from odam_amd import _lib
    old = _lib.config()["cg.ring"]
    _lib.set_config("cg.ring", ring)
    try:
        det, sd = _detector(backbone, B)
        torch.manual_seed(H + W + B)
        _check_fp32(det, sd, torch.randn(B, 3, H, W), BB.BASIC_BLOCKS[backbone])
        det.close()
    finally:
        _lib.set_config("cg.ring", old)


def test_resnet34_bench_size_vs_oracle():
    """3 x 800 x 1066 (the bench frame): the large-M paths of every BasicBlock shape (3x3 / 2 with Cin = Cout / 2, 3x3 + residual
    at 64 ... 512 channels, the 1x1 / 2 downsamples, input_proj with K = 512); then the same forward with fp32 layers on the
    fp32 matrix instruction (cg.f32 = 0)"""
    from odam_amd import _lib
    det, sd = _detector("resnet34", 2)
    torch.manual_seed(34)
    img = torch.randn(2, 3, 800, 1066)
    _check_fp32(det, sd, img, BB.BASIC_BLOCKS["resnet34"])
    old = _lib.config()["cg.f32"]
    _lib.set_config("cg.f32", 0)
    try:
        out = det(img.to(DEV))
    finally:
        _lib.set_config("cg.f32", old)
    ref = BB.detr_forward_basic(sd, img, BB.BASIC_BLOCKS["resnet34"])
    for k in KEYS:
        assert (out[k].cpu() - ref[k]).abs().max().item() <= 2e-4 * max(1.0, ref[k].abs().max().item()), k
    assert torch.equal(out["pred_logits"].cpu().argmax(-1), ref["pred_logits"].argmax(-1))
    det.close()


def test_resnet34_bf16_vs_bf16_faithful_oracle(measured):
    """bf16 mode end to end, held to the noise band of the bf16-faithful restatement itself (tests/test_detr_gpu.py::_bf16_check's
    criteria): that restatement evaluated four times -- as is and on inputs nudged by one bf16 ulp in 1 % of the pixels, each
    rounding independently from there on -- gives the spread two faithful bf16 evaluations show; the kernel must lie inside it.
    (These weights make every query of a frame decode alike, so each output has few independent values and ONE evaluation is a
    noisy yardstick: measured, the kernel's box rms against fp32 was 1.48x the unnudged restatement's.)"""
    det, sd = _detector("resnet34", 2, dtype="bf16")
    torch.manual_seed(3)
    torch.set_num_threads(16)
    img = torch.randn(2, 3, 192, 256)
    blocks = BB.BASIC_BLOCKS["resnet34"]
    ref_f = BB.detr_forward_basic(sd, img, blocks)
    refs = [BB.detr_forward_bf16_basic(sd, img, blocks)]
    for seed in (1, 2, 3):
        nudge = torch.rand(img.shape, generator=torch.Generator().manual_seed(seed)) < 1e-2
        refs.append(BB.detr_forward_bf16_basic(sd, torch.where(nudge, img * (1 + 2.0 ** -7), img), blocks))
    out = det(img.to(DEV))
    l4, _ = det.debug_taps(2, 192, 256)
    assert l4.shape[1] == 512

    def rms(a, b):
        return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-12)).item()

    def mx(a, b):
        return ((a - b).abs().max() / b.abs().max().clamp_min(1.0)).item()
    for k in KEYS:
        g = out[k].cpu()
        band_rms = max(rms(r[k], ref_f[k]) for r in refs)          # faithful bf16 vs fp32, the widest of the four
        band_mx = max(mx(r[k], ref_f[k]) for r in refs)
        self_rms = max(rms(r[k], refs[0][k]) for r in refs[1:])     # faithful bf16 vs itself
        for nm, v in (("gpu_vs_fp32_rms", rms(g, ref_f[k])), ("band_vs_fp32_rms", band_rms), ("gpu_vs_fp32_max", mx(g, ref_f[k])),
                      ("band_vs_fp32_max", band_mx), ("gpu_vs_bf16oracle_rms", rms(g, refs[0][k])), ("oracle_vs_nudged_self_rms", self_rms)):
            measured(f"detr_bf16.resnet34.{k}.{nm}", v)
        assert rms(g, ref_f[k]) <= 1.3 * band_rms + 1e-4, (k, rms(g, ref_f[k]), band_rms)
        assert mx(g, ref_f[k]) <= 2.0 * band_mx + 1e-4, (k, mx(g, ref_f[k]), band_mx)
        assert mx(g, refs[0][k]) <= 2.0 * band_mx + 1e-4, (k, mx(g, refs[0][k]), band_mx)
        assert rms(g, refs[0][k]) <= 1.5 * self_rms + 1e-4, (k, rms(g, refs[0][k]), self_rms)
        assert mx(g, ref_f[k]) <= 0.1, k
    lab = out["pred_logits"].cpu().argmax(-1)
    agree = [(r["pred_logits"].argmax(-1) == refs[0]["pred_logits"].argmax(-1)).float().mean().item() for r in refs[1:]]
    measured("detr_bf16.resnet34.label_agreement_gpu_vs_oracle", (lab == refs[0]["pred_logits"].argmax(-1)).float().mean().item())
    measured("detr_bf16.resnet34.label_agreement_oracle_vs_nudged_self_min", min(agree))
    assert (lab == refs[0]["pred_logits"].argmax(-1)).float().mean().item() >= min(agree) - 0.03
    det.close()


@pytest.mark.parametrize("ring", [1, 2])
def test_basic_block_bf16_layers_teacher_forced(measured, ring):
    """every contraction of the bf16 BasicBlock body (stem, 3x3 / stride with Cin = Cout / 2, 3x3 + residual, 1x1 / 2 downsample) on
    the restatement's own inputs returns the restatement's bf16 bits up to one-ulp ties of the fp32 summation order (the check of
    tests/test_detr_gpu.py::test_bf16_layers_teacher_forced): the rounding points of the bf16 plan are where tests/basic_body.py puts them"""
    import detr_oracle as O
    from odam_amd import _lib, weights
    from test_detr_gpu import _pack, _st, _to_bf16_bits
    L = _lib.lib()
    sd = weights.make_state_dict(backbone="resnet34", seed=0)
    torch.manual_seed(4)
    O.TRACE = []
    try:
        BB.basic_body_bf16(torch.randn(1, 3, 192, 256), sd, BB.BASIC_BLOCKS["resnet34"])
        trace = O.TRACE
    finally:
        O.TRACE = None
    assert len(trace) == 1 + 16 * 2 + 3
    worst_frac = 0.0
    _lib.check(L.odam_op_conv_bf16_mode(ring), "mode")
    try:
        for rec in trace:
            x, w, y, res = rec["x"], rec["w"], rec["y"], rec["res"]
            B, Cin, H, W = x.shape
            Cout, k = w.shape[0], w.shape[2]
            k_order = 1 if Cin % 64 == 0 and k > 1 else 0
            wpk, CinP, Kpad = _pack(w, 8, k_order)
            xh = torch.zeros(B, H, W, CinP); xh[..., :Cin] = x.permute(0, 2, 3, 1)
            dx, dw = _to_bf16_bits(xh).to(DEV), _to_bf16_bits(wpk).to(DEV)
            dsc, dbi = rec["scale"].contiguous().to(DEV), rec["bias"].contiguous().to(DEV)
            dr = _to_bf16_bits(res.permute(0, 2, 3, 1).contiguous()).to(DEV) if res is not None else None
            dy = torch.empty(B, y.shape[2], y.shape[3], Cout, device=DEV, dtype=torch.bfloat16)
            _lib.check(L.odam_op_conv2d_nhwc_bf16(_lib.ptr(dx), _lib.ptr(dw), _lib.ptr(dsc), _lib.ptr(dbi), _lib.ptr(dr), _lib.ptr(dy),
                                                  B, H, W, CinP, Cout, k, k, rec["stride"], rec["padding"], Kpad, int(rec["relu"]), 0,
                                                  k_order, _st()), "conv bf16")
            want = y.permute(0, 2, 3, 1).contiguous()
            gb, wb = dy.cpu().view(torch.int16).to(torch.int32), _to_bf16_bits(want).to(torch.int32)
            diff = (gb - wb).abs()
            diff = torch.where(((gb & 0x7fff) == 0) & ((wb & 0x7fff) == 0), torch.zeros_like(diff), diff)
            small = (dy.cpu().float() - want).abs() <= 1e-5 * want.abs().max().item()
            frac = (diff != 0).float().mean().item()
            worst_frac = max(worst_frac, frac)
            assert not ((diff > 1) & ~small).any() and frac <= 5e-3, (rec["name"], tuple(x.shape), frac, int(diff.max().item()))
    finally:
        _lib.check(L.odam_op_conv_bf16_mode(1), "mode")
    measured(f"detr_bf16.resnet34.teacher_forced_ring{ring}.worst_mismatch_share", worst_frac)


def test_resnet34_forward_nested():
    """images of two sizes in one call: the one that fills the batch maximum equals its own forward, and the other one does not
    depend on its batch companion (only on its own padding)"""
    det, _ = _detector("resnet34", 2)
    g = torch.Generator().manual_seed(5)
    a, b, c = torch.randn(3, 200, 280, generator=g), torch.randn(3, 256, 320, generator=g), torch.randn(3, 256, 320, generator=g)
    ab = det.forward_nested([a, b])
    ac = det.forward_nested([a, c])
    alone = det(b[None])
    for k in KEYS:
        ref = alone[k][0].cpu()
        assert (ab[k][1].cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item()), k
        assert (ab[k][0].cpu() - ac[k][0].cpu()).abs().max().item() <= 2e-5 * max(1.0, ab[k][0].abs().max().item()), k
    assert torch.equal(ab["pred_logits"][1].argmax(-1), alone["pred_logits"][0].argmax(-1))
    assert torch.equal(ab["pred_logits"][0].argmax(-1), ac["pred_logits"][0].argmax(-1))
    det.close()


def test_resnet152_forward_vs_oracle():
    import detr_oracle as O
    det, sd = _detector("resnet152", 2)
    torch.manual_seed(152)
    torch.set_num_threads(16)
    img = torch.randn(2, 3, 192, 256)
    ref = O.detr_forward(sd, img, blocks=(3, 8, 36, 3), return_taps=True)
    out = det(img.to(DEV))
    l4, mem = det.debug_taps(2, 192, 256)
    assert l4.shape[1] == 2048
    assert _rel(l4.cpu(), ref["_layer4"]) <= 2e-5
    assert _rel(mem.cpu(), ref["_memory"]) <= 2e-5
    for k in KEYS + ("pred_obj_features",):
        assert (out[k].cpu() - ref[k]).abs().max().item() <= 2e-4 * max(1.0, ref[k].abs().max().item()), k
    assert torch.equal(out["pred_logits"].cpu().argmax(-1), ref["pred_logits"].argmax(-1))
    det.close()


def test_resnet18_detect_resident_u8():
    """uint8 frames through the device transform, two streams: the rows of __call__ + postprocess_rows on the same frames"""
    from odam_amd import detector, weights
    det = detector.Detector(backbone="resnet18", max_batch=2, device=DEV, n_streams=2)
    det.load_state_dict(weights.make_state_dict(backbone="resnet18", seed=0))
    det.resize = (240, 400)
    raw = torch.from_numpy(np.random.default_rng(18).integers(0, 256, (5, 72, 96, 3), dtype=np.uint8)).to(DEV)
    got = det.detect_resident(raw, (96, 72), K)
    frames = torch.cat([det.preprocess_u8(raw[i:i + 2]) for i in range(0, 5, 2)])
    want = np.concatenate([det.postprocess_rows(det(frames[i:i + 2]), (96, 72), K) for i in range(0, 5, 2)])
    assert np.array_equal(got, want)
    det.close()
