"""The MXFP8 format of the detector's mxfp8 mode (include/odam_detr.h "MXFP8") pinned on the CPU: the restatement in
tests/mxfp8_ref.py against torch.float8_e4m3fn (encoding and rounding), the scale rule at its boundaries, zero blocks, the
MX-faithful convolution against float64 F.conv2d, and the Detector's validation of dtype="mxfp8"."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_ref as MX  # noqa: E402


def _torch_e4m3(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_elements_match_torch_float8_e4m3fn_all_exponents():
    """every finite fp32 binade that can reach an element (|v| <= 448, down past the subnormals), with ties, both signs"""
    rng = np.random.default_rng(0)
    vals = []
    for ex in range(-140, 9):
        m = rng.integers(0, 1 << 23, 64).astype(np.uint32)
        vals.append(((np.uint32(ex + 127) << 23) | m).view(np.float32) if ex >= -126 else
                    np.ldexp(rng.random(64).astype(np.float32), ex).astype(np.float32))
    # ties: midpoints between neighbouring e4m3 values (normal and subnormal), and the exact values
    grid = MX.e4m3_value(np.arange(0, 0x7F)).astype(np.float64)
    mids = ((grid[1:] + grid[:-1]) / 2).astype(np.float32)
    vals += [mids, grid.astype(np.float32), np.array([448.0, 447.9999, 2.0 ** -6, 2.0 ** -9, 2.0 ** -10, 0.0], np.float32)]
    v = np.concatenate(vals).astype(np.float32)
    v = v[np.abs(v) <= 448]
    v = np.concatenate([v, -v])
    assert np.array_equal(MX.e4m3_bits(v), _torch_e4m3(v))
    # every byte decodes to what torch decodes
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).float().numpy()
    got = MX.e4m3_value(b).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_quantizer_elements_equal_torch_after_scaling():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((64, 256)) * np.exp2(rng.integers(-30, 30, (64, 1)))).astype(np.float32)
    q, s = MX.quantize(x)
    e = s.astype(np.int64) - 127
    scaled = np.ldexp(x.reshape(-1, 32), -e[:, None]).astype(np.float32)
    assert np.abs(scaled).max() <= 448
    assert np.array_equal(q.reshape(-1, 32), _torch_e4m3(scaled))


@pytest.mark.parametrize("e", [-120, -3, 0, 1, 17, 110])
def test_scale_rule_at_the_boundary(e):
    """amax = 448 * 2^e exactly -> e; one ulp above -> e + 1; one ulp below -> e"""
    a = np.float32(np.ldexp(448.0, e))
    up, dn = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(0))
    for amax, want in ((a, e), (up, e + 1), (dn, e)):
        blk = np.zeros(32, np.float32)
        blk[7] = -amax
        q, s = MX.quantize(blk)
        assert int(s[0]) - 127 == want, (amax, s[0])
        assert q[7] in (0xFE, 0xFF) or want != e or amax != a   # the maximum maps to -448 exactly at the boundary
    blk = np.zeros(32, np.float32)
    blk[0] = a
    q, _ = MX.quantize(blk)
    assert q[0] == 0x7E                                            # 448, no saturation


def test_scale_clamps_and_zero_blocks():
    z = np.zeros(64, np.float32)
    q, s = MX.quantize(z)
    assert (s == 0).all() and (q == 0).all()                       # e = -127
    tiny = np.zeros(32, np.float32)
    tiny[3] = np.float32(1e-45)                                    # subnormal amax: clamped to -127
    q, s = MX.quantize(tiny)
    assert s[0] == 0
    big = np.full(32, np.finfo(np.float32).max, np.float32)
    q, s = MX.quantize(big)
    assert s[0] == 120 + 127                                       # the largest finite fp32 needs e = 120
    bad = np.ones(32, np.float32)
    bad[5] = np.inf
    _, s = MX.quantize(bad)
    assert s[0] == 255 and np.isnan(MX.dequantize(*MX.quantize(bad))).all()


def test_round_trip_error_bound():
    """x -> MXFP8 -> x: each element within half an e4m3 ulp of its block scale (relative 2^-4 of a normal element)"""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((128, 64)).astype(np.float32)
    q, s = MX.quantize(x)
    d = MX.dequantize(q, s)
    e = np.repeat(s.astype(np.int64) - 127, 32).reshape(x.shape)
    assert (np.abs(d - x) <= np.ldexp(2.0 ** -10, e) + np.abs(x) * 2.0 ** -4).all()
    assert np.array_equal(MX.dequantize(*MX.quantize(d)), d)        # MXFP8 values are fixed points of the quantizer


def test_mx_conv_equals_float64_conv_of_dequantized_operands():
    torch.manual_seed(0)
    x = torch.randn(2, 64, 9, 11)
    w = torch.randn(96, 64, 3, 3) * 0.05
    xq = MX.qdq(x)
    _, _, wq = MX.pack_filter(w)
    sc, bi = torch.rand(96) + 0.5, torch.randn(96)
    y = MX.mx_conv(xq, wq, sc, bi, stride=2, padding=1, relu=True)
    ref = F.relu((F.conv2d(xq.double(), wq.double(), stride=2, padding=1).float() * sc.reshape(1, -1, 1, 1)) + bi.reshape(1, -1, 1, 1))
    assert torch.equal(y, ref)
    # the filter blocks are 32 consecutive input channels of one tap of one output channel
    q, s, _ = MX.pack_filter(w)
    assert q.shape == (96, 9 * 64) and s.shape == (96 * 9 * 64 // 32,)
    blk = w[5, 32:64, 1, 2].numpy()
    qb, sb = MX.quantize(blk)
    assert np.array_equal(q[5, (1 * 3 + 2) * 64 + 32:(1 * 3 + 2) * 64 + 64], qb) and s[5 * 18 + 11] == sb[0]
    # the operands really are MXFP8 values: quantizing them again changes nothing
    assert torch.equal(MX.qdq(xq), xq)


def test_detector_accepts_mxfp8_and_refuses_dc5():
    from odam_amd import detector
    det = detector.Detector(backbone="resnet50", dtype="mxfp8", device="cpu")
    assert det.dtype == "mxfp8"
    det = detector.Detector(backbone="resnet34", dtype="mxfp8", device="cpu")
    assert det.dtype == "mxfp8"
    with pytest.raises(ValueError, match="mxfp8"):
        detector.Detector(backbone="resnet50", dtype="mxfp8", dilation=True, device="cpu")
    with pytest.raises(ValueError):
        detector.Detector(dtype="fp8")
