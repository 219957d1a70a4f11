"""The detector's mxfp8 mode on the device (include/odam_detr.h "MXFP8", odam_amd/csrc/cg_mx8.hip) against the CPU restatement
tests/mxfp8_ref.py: the quantize / dequantize ops bit for bit; the MXFP8 convolution over a shape grid (fp32 values before the
output rounding against float64 of the same operands, the MXFP8 output bits against quantizing that float64 result, the bf16
copy); every body layer of R50 and R34 teacher-forced; whole forwards inside the spread of the MX-faithful restatement."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import basic_body as BB  # noqa: E402
import detr_oracle as O  # noqa: E402
import mxfp8_ref as MX  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
K = np.array([[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]])
# accumulation bound of the fp32 values before the output rounding: |gpu - float64| <= C_ACC 2^-24 |scale| sum |x w| (+ the
# epilogue's own roundings).  The block-scaled instruction does not sum its 64 products exactly in fp32: on the first run the
# 64-channel 1x1 case measured 551 x 2^-24 sum |x w| (about 2^-15 of it), so C_ACC = 2048 is that figure with a 3.7x margin
C_ACC = 2048
# share of MXFP8 output elements that may differ from quantizing the float64 result (a value within the summation error of a
# rounding boundary of its block, or of its block's scale boundary)
FLIP_SHARE = 1e-2


def _L():
    from odam_amd import _lib
    L = _lib.lib()
    L.odam_op_conv_paths.restype = ctypes.c_longlong
    return L


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _paths(reset=True):
    buf = ctypes.create_string_buffer(1 << 16)
    _L().odam_op_conv_paths(buf, len(buf), int(reset))
    return [t for t in buf.value.decode().split("\n") if t]


def _quantize_gpu(x, src_dtype=0):
    from odam_amd import _lib
    n = x.numel()
    q = torch.empty(n, dtype=torch.uint8, device=DEV)
    s = torch.empty(n // 32, dtype=torch.uint8, device=DEV)
    _lib.check(_L().odam_op_quantize_mxfp8(_lib.ptr(x), src_dtype, ctypes.c_longlong(n), _lib.ptr(q), _lib.ptr(s), _st()), "quantize")
    return q, s


def test_quantize_op_bit_identical():
    from odam_amd import _lib
    rng = np.random.default_rng(0)
    rnd = (rng.standard_normal((512, 256)) * np.exp2(rng.integers(-40, 40, (512, 1)))).astype(np.float32)
    # adversarial blocks: e4m3 rounding ties at many scales, amax at 448 * 2^e and one ulp either side, zero blocks, subnormal input
    grid = MX.e4m3_value(np.arange(1, 0x7E)).astype(np.float64)
    mids = ((grid[1:] + grid[:-1]) / 2)
    adv = []
    for e in (-126, -40, -3, 0, 5, 60, 118):
        blk = np.resize(mids, (8, 32)) * 2.0 ** e
        blk[:, 0] = 448 * 2.0 ** e
        blk[1, 0] = np.nextafter(np.float32(448 * 2.0 ** e), np.float32(np.inf))
        blk[2, 0] = np.nextafter(np.float32(448 * 2.0 ** e), np.float32(0))
        adv.append(blk)
    adv.append(np.zeros((4, 32)))
    adv.append(np.ldexp(rng.random((4, 32)), -140))
    x = np.concatenate([rnd.reshape(-1, 32), np.concatenate(adv).astype(np.float32)]).astype(np.float32)
    x[::3] *= -1
    xt = torch.from_numpy(x).to(DEV)
    q, s = _quantize_gpu(xt)
    wq, ws = MX.quantize(x)
    assert np.array_equal(q.cpu().numpy(), wq.reshape(-1)) and np.array_equal(s.cpu().numpy(), ws)
    # bf16 input
    xb = xt.to(torch.bfloat16)
    q2, s2 = _quantize_gpu(xb, 1)
    wq2, ws2 = MX.quantize(xb.float().cpu().numpy())
    assert np.array_equal(q2.cpu().numpy(), wq2.reshape(-1)) and np.array_equal(s2.cpu().numpy(), ws2)
    # dequantize round trip
    y = torch.empty(x.size, dtype=torch.float32, device=DEV)
    _lib.check(_L().odam_op_dequantize_mxfp8(_lib.ptr(q), _lib.ptr(s), ctypes.c_longlong(x.size), _lib.ptr(y), _st()), "dequantize")
    assert np.array_equal(y.cpu().numpy(), MX.dequantize(wq, ws).reshape(-1))


def _conv_gpu(xq_nchw, w, sc, bi, stride, pad, res=None, relu=False, want_mx=True):
    """xq: NCHW MXFP8 values; w: OIHW fp32 (quantized here); res: NCHW bf16 values.  -> (yf, yq, ys, yb) NHWC on the host"""
    from odam_amd import _lib
    B, Ci, H, W = xq_nchw.shape
    Co, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    M = B * Ho * Wo
    xn = xq_nchw.permute(0, 2, 3, 1).contiguous().to(DEV)
    xq, xs = _quantize_gpu(xn)
    wq, ws, _ = MX.pack_filter(w)
    dwq, dws = torch.from_numpy(wq).to(DEV), torch.from_numpy(ws).to(DEV)
    dsc, dbi = sc.float().contiguous().to(DEV), bi.float().contiguous().to(DEV)
    dres = res.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV) if res is not None else None
    yq = torch.empty(M * Co, dtype=torch.uint8, device=DEV) if want_mx else None
    ys = torch.empty(M * Co // 32, dtype=torch.uint8, device=DEV) if want_mx else None
    yb = torch.empty(M, Co, dtype=torch.bfloat16, device=DEV)
    yf = torch.empty(M, Co, dtype=torch.float32, device=DEV)
    _paths()
    _lib.check(_L().odam_op_conv2d_nhwc_mxfp8(_lib.ptr(xq), _lib.ptr(xs), _lib.ptr(dwq), _lib.ptr(dws), _lib.ptr(dsc), _lib.ptr(dbi),
                                              _lib.ptr(dres), _lib.ptr(yq), _lib.ptr(ys), _lib.ptr(yb), _lib.ptr(yf), B, H, W, Ci, Co,
                                              KH, KW, stride, pad, 1, KH * KW * Ci, int(relu), 0, _st()), "conv mxfp8")
    torch.cuda.synchronize()
    toks = _paths()
    assert toks == ["mx8.128x128.w4"], toks
    yf = yf.cpu().reshape(B, Ho, Wo, Co)
    return yf, (yq.cpu().numpy() if want_mx else None), (ys.cpu().numpy() if want_mx else None), yb.cpu().reshape(B, Ho, Wo, Co)


def _check_conv(tag, xq, w, sc, bi, stride, pad, res, relu, measured):
    """the three checks of one convolution; returns the flip share"""
    _, _, wd = MX.pack_filter(w)
    yf, yq, ys, yb = _conv_gpu(xq, w, sc, bi, stride, pad, res, relu)
    ref = MX.mx_conv(xq, wd, sc, bi, stride, pad, res, relu).permute(0, 2, 3, 1)
    sabs = torch.nn.functional.conv2d(xq.double().abs(), wd.double().abs(), stride=stride, padding=pad).float().permute(0, 2, 3, 1)
    extra = ref.abs() + bi.abs().reshape(1, 1, 1, -1) + (res.abs().permute(0, 2, 3, 1) if res is not None else 0)
    tol = C_ACC * 2.0 ** -24 * sabs * sc.abs().reshape(1, 1, 1, -1) + 4 * 2.0 ** -24 * extra + 1e-30
    err = (yf - ref).abs()
    ratio = (err / tol).max().item()
    measured(f"mxfp8.conv.{tag}.err_over_bound", ratio)
    assert ratio <= 1.0, (tag, ratio)
    # the kernel's own rounding of its fp32 values: bit for bit the format's quantizer; the bf16 copy: RNE of the same values
    mq, ms = MX.quantize(yf.numpy())
    assert np.array_equal(yq, mq.reshape(-1)) and np.array_equal(ys, ms), tag
    assert torch.equal(yb, yf.to(torch.bfloat16)), tag
    # against quantizing the float64 result: rounding-boundary flips only
    rq, rs = MX.quantize(ref.contiguous().numpy())
    flips = float((yq != rq.reshape(-1)).mean())
    measured(f"mxfp8.conv.{tag}.flip_share", flips)
    assert flips <= FLIP_SHARE, (tag, flips)
    assert float((ys != rs).mean()) <= FLIP_SHARE, tag
    return flips


# B, H, W, Cin, Cout, k, stride, residual, relu: 1x1 / 3x3, strides 1 / 2, the downsample (1x1 / 2, no ReLU), ragged M and N
# (Cout 96 / 160 are not multiples of the 128-channel tile; M is not a multiple of 128 anywhere), Cin 64 .. 2048
GRID = [
    (2, 9, 11, 64, 96, 1, 1, False, True),
    (1, 13, 10, 64, 64, 3, 1, True, True),
    (2, 12, 9, 128, 160, 3, 2, False, True),
    (1, 15, 14, 256, 512, 1, 2, False, False),
    (1, 5, 6, 2048, 512, 1, 1, True, True),
    (1, 6, 5, 512, 2048, 1, 1, True, True),
    (1, 8, 7, 512, 512, 3, 1, False, True),
]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "b%d_%dx%d_c%d_o%d_k%d_s%d%s%s" % (c[:7] + ("_res" if c[7] else "", "_relu" if c[8] else "")))
def test_conv_op_grid(case, measured):
    B, H, W, Ci, Co, k, stride, has_res, relu = case
    g = torch.Generator().manual_seed(Ci * 7 + Co + k)
    x = torch.randn(B, Ci, H, W, generator=g)
    if relu:
        x = x.clamp_min(0)             # body inputs are post-ReLU except the stem's
    xq = MX.qdq(x)
    w = torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (Ci * k * k)) ** 0.5
    sc, bi = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = O._rb(torch.randn(B, Co, Ho, Wo, generator=g)) if has_res else None
    _check_conv("b%d_%dx%d_c%d_o%d_k%d_s%d" % case[:7], xq, w, sc, bi, stride, pad, res, relu, measured)


@pytest.mark.parametrize("backbone", ["resnet50", "resnet34"])
def test_body_layers_teacher_forced(backbone, measured):
    """every body convolution of the MX-faithful restatement, run on the restatement's own input, matches its own output"""
    from odam_amd import weights
    sd = weights.make_state_dict(backbone=backbone, seed=0)
    torch.manual_seed(4)
    img = torch.randn(1, 3, 96, 128)
    trace = []
    basic = backbone == "resnet34"
    blocks = BB.BASIC_BLOCKS["resnet34"] if basic else (3, 4, 6, 3)
    (MX.basic_body if basic else MX.bottleneck_body)(img, sd, blocks, trace=trace)
    worst = 0.0
    for r in trace:
        sc, bi = O._bn_fold(sd, r["bn"])
        w = sd[r["key"]]
        worst = max(worst, _check_conv(f"{backbone}.tf", r["x"], w, sc, bi, r["stride"], r["padding"], r["res"], r["relu"], measured))
    measured(f"mxfp8.{backbone}.teacher_forced.worst_flip_share", worst)
    assert len(trace) == (52 if not basic else 35)


def _detector(backbone, B, **kw):
    from odam_amd import detector, weights
    sd = weights.make_state_dict(backbone=backbone, seed=0)
    det = detector.Detector(backbone=backbone, max_batch=B, device=DEV, n_streams=1, **kw)
    det.load_state_dict(sd)
    return det, sd


def _rms(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-12)).item()


def _mx(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1.0)).item()


@pytest.mark.parametrize("backbone,H,W", [("resnet50", 256, 320), ("resnet34", 192, 256)])
def test_forward_vs_mx_faithful_restatement(backbone, H, W, measured):
    """mxfp8 end to end inside the spread of the MX-faithful restatement evaluated four times (as is, and on inputs nudged by one
    bf16 ulp in 1 % of the pixels), with the criteria of tests/test_backbones_gpu.py::test_resnet34_bf16_vs_bf16_faithful_oracle"""
    basic = backbone == "resnet34"
    blocks = BB.BASIC_BLOCKS["resnet34"] if basic else (3, 4, 6, 3)
    det, sd = _detector(backbone, 1, dtype="mxfp8")
    torch.manual_seed(3)
    torch.set_num_threads(16)
    img = torch.randn(1, 3, H, W)
    ref_f = (BB.detr_forward_basic if basic else O.detr_forward)(sd, img, blocks)
    refs = [MX.detr_forward_mxfp8(sd, img, blocks, basic)]
    for seed in (1, 2, 3):
        nudge = torch.rand(img.shape, generator=torch.Generator().manual_seed(seed)) < 1e-2
        refs.append(MX.detr_forward_mxfp8(sd, torch.where(nudge, img * (1 + 2.0 ** -7), img), blocks, basic))
    _paths()
    out = det(img.to(DEV))
    toks = _paths()
    assert sum(t.startswith("mx8.") for t in toks) == (35 if basic else 52) and not any(".fused." in t for t in toks)
    l4, _ = det.debug_taps(1, H, W)
    assert torch.isfinite(l4).all()
    bdet, _ = _detector(backbone, 1, dtype="bf16")
    bout = bdet(img.to(DEV))
    for k in KEYS:
        g = out[k].cpu()
        assert torch.isfinite(g).all(), k
        band_rms = max(_rms(r[k], ref_f[k]) for r in refs)
        band_mx = max(_mx(r[k], ref_f[k]) for r in refs)
        self_rms = max(_rms(r[k], refs[0][k]) for r in refs[1:])
        for nm, v in (("gpu_vs_fp32_rms", _rms(g, ref_f[k])), ("band_vs_fp32_rms", band_rms), ("gpu_vs_fp32_max", _mx(g, ref_f[k])),
                      ("band_vs_fp32_max", band_mx), ("gpu_vs_mxoracle_rms", _rms(g, refs[0][k])), ("oracle_vs_nudged_self_rms", self_rms)):
            measured(f"mxfp8.{backbone}.{k}.{nm}", v)
        assert _rms(g, ref_f[k]) <= 1.3 * band_rms + 1e-4, (k, _rms(g, ref_f[k]), band_rms)
        assert _mx(g, ref_f[k]) <= 2.0 * band_mx + 1e-4, (k, _mx(g, ref_f[k]), band_mx)
        assert _mx(g, refs[0][k]) <= 2.0 * band_mx + 1e-4, (k, _mx(g, refs[0][k]), band_mx)
        assert _rms(g, refs[0][k]) <= 1.5 * self_rms + 1e-4, (k, _rms(g, refs[0][k]), self_rms)
    lab = out["pred_logits"].cpu().argmax(-1)
    agree = [(r["pred_logits"].argmax(-1) == refs[0]["pred_logits"].argmax(-1)).float().mean().item() for r in refs[1:]]
    measured(f"mxfp8.{backbone}.label_agreement_vs_fp32", (lab == ref_f["pred_logits"].argmax(-1)).float().mean().item())
    measured(f"mxfp8.{backbone}.label_agreement_vs_bf16_mode", (lab == bout["pred_logits"].cpu().argmax(-1)).float().mean().item())
    measured(f"mxfp8.{backbone}.label_agreement_vs_mxoracle", (lab == refs[0]["pred_logits"].argmax(-1)).float().mean().item())
    assert (lab == refs[0]["pred_logits"].argmax(-1)).float().mean().item() >= min(agree) - 0.03
    det.close()
    bdet.close()


# loose sanity bound of the mxfp8 forward against the fp32 mode at the bench's R101 size (relative rms of each output): the first
# run measured 0.163 at worst (pred_offset; bf16 mode 0.036), so 0.5 is about 3x that
R101_RMS_BOUND = 0.5


def test_resnet101_full_size_vs_fp32_and_bf16(measured):
    """R101 at 800 x 1066, one frame: finite, within a loose bound of fp32; rms / max / label agreement recorded against fp32 and
    against the bf16 mode"""
    from odam_amd import detector, weights
    sd = weights.make_state_dict(backbone="resnet101", seed=0)
    torch.manual_seed(7)
    img = torch.randn(1, 3, 800, 1066).to(DEV)
    outs = {}
    for dt in ("fp32", "bf16", "mxfp8"):
        det = detector.Detector(backbone="resnet101", max_batch=1, device=DEV, n_streams=1, dtype=dt)
        det.load_state_dict(sd)
        outs[dt] = {k: v.cpu() for k, v in det(img).items() if k in KEYS}
        det.close()
    for k in KEYS:
        g = outs["mxfp8"][k]
        assert torch.isfinite(g).all(), k
        for ref in ("fp32", "bf16"):
            measured(f"mxfp8.resnet101_800x1066.{k}.rms_vs_{ref}", _rms(g, outs[ref][k]))
            measured(f"mxfp8.resnet101_800x1066.{k}.max_vs_{ref}", _mx(g, outs[ref][k]))
        measured(f"bf16.resnet101_800x1066.{k}.rms_vs_fp32", _rms(outs["bf16"][k], outs["fp32"][k]))
        assert _rms(g, outs["fp32"][k]) <= R101_RMS_BOUND, (k, _rms(g, outs["fp32"][k]))
    lab = outs["mxfp8"]["pred_logits"].argmax(-1)
    for ref in ("fp32", "bf16"):
        measured(f"mxfp8.resnet101_800x1066.label_agreement_vs_{ref}", (lab == outs[ref]["pred_logits"].argmax(-1)).float().mean().item())


def test_forward_nested_mxfp8():
    """images of two sizes in one call, mxfp8: the one that fills the batch maximum equals its own forward, the other does not
    depend on its batch companion"""
    det, _ = _detector("resnet34", 2, dtype="mxfp8")
    g = torch.Generator().manual_seed(5)
    a, b, c = torch.randn(3, 200, 280, generator=g), torch.randn(3, 256, 320, generator=g), torch.randn(3, 256, 320, generator=g)
    ab = det.forward_nested([a, b])
    ac = det.forward_nested([a, c])
    alone = det(b[None])
    for k in KEYS:
        ref = alone[k][0].cpu()
        assert torch.isfinite(ab[k]).all(), k
        assert (ab[k][1].cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item()), k
        assert (ab[k][0].cpu() - ac[k][0].cpu()).abs().max().item() <= 2e-5 * max(1.0, ab[k][0].abs().max().item()), k
    assert torch.equal(ab["pred_logits"][1].argmax(-1), alone["pred_logits"][0].argmax(-1))
    det.close()


def test_detect_resident_u8_mxfp8():
    """uint8 frames through the device transform in mxfp8 mode: the rows of __call__ + postprocess_rows on the same frames"""
    from odam_amd import detector, weights
    det = detector.Detector(backbone="resnet50", max_batch=2, device=DEV, n_streams=2, dtype="mxfp8")
    det.load_state_dict(weights.make_state_dict(backbone="resnet50", seed=0))
    det.resize = (240, 400)
    raw = torch.from_numpy(np.random.default_rng(18).integers(0, 256, (5, 72, 96, 3), dtype=np.uint8)).to(DEV)
    got = det.detect_resident(raw, (96, 72), K)
    frames = torch.cat([det.preprocess_u8(raw[i:i + 2]) for i in range(0, 5, 2)])
    want = np.concatenate([det.postprocess_rows(det(frames[i:i + 2]), (96, 72), K) for i in range(0, 5, 2)])
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)
    det.close()
