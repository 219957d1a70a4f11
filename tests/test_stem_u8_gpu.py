"""conv1 on the centred uint8 frame (odam_config stem.u8, include/odam_detr.h odam_detr_forward_u8 / odam_op_stem_u8): the resize writes
(u - c, 1) as ONE bf16 plane, framed, and conv1 reads it with the normalisation folded into its pre-split filters -- three products per
block on conv_gemm_big_kernel MODE 5 -- against float64 of the real chain (tests/stem_u8_ref.py), and the forward against the CPU oracle.

Error model, in the form of tests/test_conv_f32_gpu.py.  u = 2^-24; an output is y = relu(s * sum_k a_k w'_k + b) over the folded operands
a = (u8 - c, indicator), w' = fl32(fold(w)); A' = |s| sum_k |a_k w'_k| + |b|.
  * the fold: every w' is rounded ONCE to fp32 (computed in double): at most 1 u A';
  * the contraction: a is exact in bf16 and w' = hi + mid + lo exactly, so NO product term is dropped; the fp32 accumulation along
    3 x 7 matrix instructions of 32 k rounds as the split mode's does (tests/test_conv_f32_gpu.py: up to 3.2 u of sum |a w'| for six
    products, of which three remain here);
  * the epilogue rounds twice (s * acc, + b): 2 u A'.
The cap is that file's C_MODEL = 12; the measured factor per case goes to the `measured` fixture under stem_u8.<case>.  The maximum of the
pooling window and the ReLU are 1-Lipschitz: the pooled output is held to the window's largest A'."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import stem_u8_ref as R
from conftest import REPO
from test_conv_f32_gpu import C_MODEL, U, _guarded, _guards_intact, clear_paths, config, paths

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")


def _mean_std():
    from odam_amd.transforms import MEAN, STD
    return np.asarray(MEAN, np.float32), np.asarray(STD, np.float32)


@pytest.fixture(scope="module")
def conv1():
    """conv1 [64, 3, 7, 7], the folded FrozenBN scale (both signs) and bias: one set for the module"""
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.05).numpy()
    s = (torch.rand(64, generator=g) + 0.5).numpy() * np.where(np.arange(64) % 5 == 0, -1.0, 1.0).astype(np.float32)
    b = (torch.randn(64, generator=g) * 0.2).numpy()
    return w.astype(np.float32), s.astype(np.float32), b.astype(np.float32)


def _L():
    from odam_amd import _lib
    L = _lib.lib()
    L.odam_op_conv_paths.restype = ctypes.c_longlong
    L.odam_op_pooled_stem_launches.restype = ctypes.c_longlong
    return L


def stem_op(raw, H, W, conv1):
    """uint8 [B, h, w, 3] (numpy) -> (pooled [B, H2, W2, 64] on the CPU, path, tokens, pooled launches, guards intact)"""
    w, s, b = conv1
    mean, std = _mean_std()
    L = _L()
    B, h, w_in, _ = raw.shape
    H2, W2 = R.conv_out(R.conv_out(H, 7, 2, 3), 3, 2, 1), R.conv_out(R.conv_out(W, 7, 2, 3), 3, 2, 1)
    d_raw = torch.from_numpy(raw).to(DEV)
    d_s, d_b = torch.from_numpy(s).to(DEV), torch.from_numpy(b).to(DEV)
    buf, y = _guarded(B * H2 * W2, 64)
    path = ctypes.c_int(-1)
    wc = np.ascontiguousarray(w)
    clear_paths()
    n0 = L.odam_op_pooled_stem_launches()
    with torch.cuda.device(DEV):
        rc = L.odam_op_stem_u8(d_raw.data_ptr(), B, h, w_in, H, W, wc.ctypes.data, d_s.data_ptr(), d_b.data_ptr(), mean.ctypes.data,
                               std.ctypes.data, y.data_ptr(), ctypes.addressof(path), torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    assert rc == 0, L.odam_last_error()
    torch.cuda.synchronize()
    return y.view(B, H2, W2, 64).cpu(), path.value, paths(), L.odam_op_pooled_stem_launches() - n0, _guards_intact(buf, B * H2 * W2)


def check(tag, got, raw, H, W, conv1, measured):
    w, s, b = conv1
    mean, std = _mean_std()
    y64, A = R.stem64(R.resize_u8(raw, H, W), w, s, b, mean, std)
    assert torch.isfinite(got).all(), tag
    ratio = ((got.double() - y64).abs() / (U * A.clamp_min(1e-300))).max().item()
    print(f"stem_u8.{tag}: {ratio:.3f} u A'")
    measured(f"stem_u8.{tag}", ratio)
    assert ratio <= C_MODEL, (tag, ratio)


def _impulses(H, W, c):
    """every pixel at the centres (A is zero but for the indicator), one pixel at 255 in one channel: the four corners, the four mid-edges and
    the centre, each channel in turn = 27 frames"""
    pos = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]
    out = np.empty((len(pos) * 3, H, W, 3), np.uint8)
    out[:] = np.asarray(c, np.uint8)[None, None, None, :]
    for i, (y, x) in enumerate(pos):
        for k in range(3):
            out[i * 3 + k, y, x, k] = 255
    return out


def _data(kind, B, h, w):
    mean, _ = _mean_std()
    c = R.centres(mean)
    if kind == "random":
        return np.random.default_rng(3).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((B, h, w, 3), np.uint8)
    if kind == "all255":
        return np.full((B, h, w, 3), 255, np.uint8)
    if kind == "centres":
        return np.broadcast_to(np.asarray(c, np.uint8), (B, h, w, 3)).copy()
    assert kind == "impulses"
    return _impulses(h, w, c)


# (frames, raw size, model size): the small odd shape the pooled stem is tested at (ragged last patch column, patches on all four
# borders), one frame smaller than a patch row, and both resample branches (a raw frame smaller in both axes)
@pytest.mark.parametrize("kind,B,hw,HW", [
    ("random", 2, (230, 310), (230, 310)),
    ("zeros", 2, (230, 310), (230, 310)),
    ("all255", 2, (230, 310), (230, 310)),
    ("centres", 2, (230, 310), (230, 310)),
    ("impulses", 27, (40, 72), (40, 72)),
    ("random", 1, (40, 72), (40, 72)),
    ("random", 2, (150, 205), (230, 310)),
])
def test_stem_vs_float64(kind, B, hw, HW, conv1, measured):
    raw = _data(kind, B, *hw)
    with config(cg_pin=1):
        got, path, toks, pooled, guards = stem_op(raw, *HW, conv1)
    assert guards
    assert path == 1 and toks == ["f32.ring.m5.512x64.pool"] and pooled == 1, (path, toks, pooled)
    check(f"{kind}.{B}x{hw[0]}x{hw[1]}.to.{HW[0]}x{HW[1]}", got, raw, *HW, conv1, measured)


def test_unpooled_and_fallback_paths(conv1, measured):
    """stem.pool = 0: the same kernel without the pool on its tile, then the max-pool kernel; stem.u8 = 0: the normalised fp32 image and the
    six-product stem -- both held to the same float64 truth"""
    raw = _data("random", 2, 230, 310)
    with config(cg_pin=1, stem_pool=0):
        got, path, toks, pooled, guards = stem_op(raw, 230, 310, conv1)
    assert guards and path == 1 and toks == ["f32.ring.m5.512x64"] and pooled == 0, (path, toks, pooled)
    check("unpooled.2x230x310", got, raw, 230, 310, conv1, measured)
    with config(cg_pin=1, stem_u8=0):
        got0, path, toks, pooled, guards = stem_op(raw, 230, 310, conv1)
    assert guards and path == 0 and toks == ["f32.ring.m4.512x64.pool"] and pooled == 1, (path, toks, pooled)
    w, s, b = conv1
    mean, std = _mean_std()
    y64, _ = R.stem64(R.resize_u8(raw, 230, 310), w, s, b, mean, std)
    assert (got0.double() - y64).abs().max().item() <= 1e-5 * max(1.0, y64.abs().max().item())


def test_batch_independence(conv1):
    """a frame alone and the same frame as the 2nd of 3 give equal bits (one patch never spans two images)"""
    raw = _data("random", 3, 230, 310)
    with config(cg_pin=1):
        three = stem_op(raw, 230, 310, conv1)[0]
        one = stem_op(raw[1:2], 230, 310, conv1)[0]
    assert torch.equal(three[1], one[0])


def _forward_u8(det, raw):
    out = det.forward_u8(torch.from_numpy(raw).to(DEV))
    return {k: out[k].cpu() for k in KEYS + ("pred_obj_features",)}


def _two_call(det, raw):
    out = det(det.preprocess_u8(torch.from_numpy(raw).to(DEV)))
    return {k: out[k].cpu() for k in KEYS + ("pred_obj_features",)}


@pytest.fixture(scope="module")
def scene_sd():
    from odam_amd import weights
    return weights.make_state_dict(seed=0, scene=True)


@pytest.mark.parametrize("hw,resize,pin", [((230, 310), (230, 1333), 1), ((600, 800), (800, 1333), 0)])
def test_forward_vs_oracle(hw, resize, pin, scene_sd, measured):
    """stem.u8 = 1 and 0 on the same raw frames, both against the CPU oracle with the criterion tests/test_detr_gpu.py holds alternative
    paths to: |d| <= 2e-4 max(1, |ref|max) per output, class arg-max equal.  stem.u8 = 0 equals the two-call path bit for bit."""
    import detr_oracle as O
    from odam_amd import detector, synth
    raw = np.stack(list(synth.make_frames(2, h=hw[0], w=hw[1], seed=4)))
    det = detector.Detector(max_batch=2, device=DEV, n_streams=1)
    det.load_state_dict(scene_sd)
    det.resize = resize
    L = _L()
    try:
        with config(cg_pin=pin):
            img = det.preprocess_u8(torch.from_numpy(raw).to(DEV))
            torch.set_num_threads(8)
            ref = O.detr_forward(scene_sd, img.cpu())
            two = _two_call(det, raw)
            outs = {}
            for v in (1, 0):
                with config(stem_u8=v):
                    clear_paths()
                    outs[v] = _forward_u8(det, raw)
                    toks = paths()
                    assert ("f32.ring.m5.512x64.pool" in toks) == (v == 1), toks[:3]
    finally:
        det.close()
    for k in KEYS + ("pred_obj_features",):
        assert torch.equal(outs[0][k], two[k]), k
    for v in (1, 0):
        for k in KEYS:
            err = (outs[v][k] - ref[k]).abs().max().item()
            measured(f"stem_u8.forward.{hw[0]}x{hw[1]}.u8_{v}.{k}", err / max(1.0, ref[k].abs().max().item()))
            assert err <= 2e-4 * max(1.0, ref[k].abs().max().item()), (v, k, err)
        assert torch.equal(outs[v]["pred_logits"].argmax(-1), ref["pred_logits"].argmax(-1)), v


@pytest.mark.parametrize("what", ["bf16", "cg.f32=0", "stem.rows=0"])
def test_fallbacks_equal_the_two_call_path(what, scene_sd):
    """a bf16 model, the fp32 matrix instruction, conv1 off the row convolution: the new entry is preprocess_u8 + forward, bit for bit"""
    from odam_amd import detector, synth
    raw = np.stack(list(synth.make_frames(2, h=230, w=310, seed=5)))
    kv = {"cg_pin": 1}
    if what != "bf16":
        k, v = what.split("=")
        kv[k.replace(".", "_")] = int(v)
    with config(**kv):
        det = detector.Detector(max_batch=2, device=DEV, n_streams=1, dtype="bf16" if what == "bf16" else "fp32")
        det.load_state_dict(scene_sd)
        det.resize = (230, 1333)
        try:
            clear_paths()
            one = _forward_u8(det, raw)
            assert not [t for t in paths() if ".m5." in t]
            two = _two_call(det, raw)
        finally:
            det.close()
    for k in one:
        assert torch.equal(one[k], two[k]), (what, k)
