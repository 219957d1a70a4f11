"""The fp32 contraction kernels (odam_amd/csrc/conv_gemm.hip launch_conv_gemm and what it dispatches to) against float64 computed
from the same fp32 operands, element by element, on every fp32 branch of the dispatch, the fused bottleneck launches, every
contraction of R50 on the fp32 oracle's own inputs, and the row-count independence of the kernel choice under cg.pin.

Error model.  An output element is y = act(s * sum_k x_k w_k + b + r).  Let A = |s| sum_k |x_k w_k| + |b| + |r| and u = 2^-24.
  * The contraction: the split mode takes every product as six exact bf16 x bf16 products of the three-way split (hi + mid + lo of
    each operand) and drops mid*lo, lo*mid and lo*lo, each at most 2^-22 |x w| and signed like an independent
    rounding; the fp32 instruction has no dropped terms.  Both accumulate in fp32 along chains of matrix instructions, each step
    rounding by at most u of a partial sum.  DESIGN.md 4.1's probe (tests/native/x3_probe.hip, K = 64 ... 4608) puts the whole
    contraction at 0.8-1.4e-7 of sum |x w| for the split and 1.1-1.9e-7 for the fp32 instruction, i.e. up to 3.2 u.  Budget: 5 u A.
  * The epilogue rounds three times, each by at most u of a value not larger than A in magnitude: s * acc, + b, + r.  Budget: 3 u A
    (the tails of the fused launches round the same three times).
So |y - y64| <= C u A with C = 8 by this budget; ReLU is 1-Lipschitz and is applied to both sides.  (A first budget of 1 u for the
contraction, C = 4, ignored the probe's figures and was exceeded.)  Measured on an MI355X (`measured`, conftest.py, under
conv_f32.<case>): single layers up to 7.0 (an R50 layer on f32.small.64x64.w4.ut.x3.s4), the fused expand up to 3.8, the chained reduce of
f32.fused.m4.chain128 (K = 256 over the block's non-negative output) up to 8.4 -- above the probe's contraction figure, not
explained by this model.  C_MODEL = 12 covers it with the same margin as the rest (1.4x the worst measured).

Each case also names the kernel that ran by its token (include/odam_detr.h odam_op_conv_paths), and output rows just before and
after the tensor are NaN-filled guards that must come back untouched."""
import contextlib
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
C_MODEL = 12.0      # see above: budget 8, worst measured 8.4 (the chained 128-channel reduce)
GUARD = 300         # NaN rows on either side of every output tensor
COVERED = set()     # tokens the cases of this module asserted


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _L():
    from odam_amd import _lib
    L = _lib.lib()
    L.odam_op_conv_paths.restype = ctypes.c_longlong
    return L


def paths(reset=True):
    """tokens of the contraction launches since the last reset"""
    buf = ctypes.create_string_buffer(1 << 17)
    n = _L().odam_op_conv_paths(buf, len(buf), int(reset))
    toks = [t for t in buf.value.decode().split("\n") if t]
    assert n == len(toks), (n, len(toks))
    return toks


def clear_paths():
    _L().odam_op_conv_paths(None, 0, 1)


def documented_f32_tokens():
    txt = open(f"{REPO}/include/odam_detr.h").read()
    block = txt[txt.index("FP32-TOKENS-BEGIN"):txt.index("FP32-TOKENS-END")]
    return set(re.findall(r"\bf32\.[a-z0-9.]+[a-z0-9]", block))


@contextlib.contextmanager
def config(**kv):
    from odam_amd import _lib
    keys = {k.replace("_", ".", 1): v for k, v in kv.items()}
    old = {k: _lib.get_config(k) for k in keys}
    try:
        for k, v in keys.items():
            _lib.set_config(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_config(k, v)


def _pack(w, k_order=0):
    """[Cout,Cin,KH,KW] -> [Cout][Kpad] fp32, K order 0 = (tap, ci), 1 = (ci // 32, tap, ci % 32) (include/odam_detr.h)"""
    Cout, Cin, KH, KW = w.shape
    CinP = (Cin + 3) // 4 * 4
    wp = torch.zeros(Cout, KH, KW, CinP); wp[..., :Cin] = w.permute(0, 2, 3, 1)
    Kk = KH * KW * CinP; Kpad = (Kk + 31) // 32 * 32
    if k_order:
        wp = wp.reshape(Cout, KH * KW, CinP // 32, 32).permute(0, 2, 1, 3)
    out = torch.zeros(Cout, Kpad); out[:, :Kk] = wp.reshape(Cout, Kk)
    return out, CinP, Kpad


def _guarded(rows, cols):
    """[GUARD + rows + GUARD, cols] NaN on the device; returns (whole, the middle view)"""
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    return bool(torch.isnan(buf[:GUARD]).all().item() and torch.isnan(buf[GUARD + rows:]).all().item())


def ref64(x, w, s, b, r, stride, pad, dil, relu):
    """float64 of act(s conv(x, w) + b + r) and A = |s| conv(|x|, |w|) + |b| + |r|, NCHW on the CPU"""
    xd, wd = x.double(), w.double()
    acc = F.conv2d(xd, wd, None, stride, pad, dil)
    mag = F.conv2d(xd.abs(), wd.abs(), None, stride, pad, dil)
    sv = (s.double() if s is not None else torch.ones(w.shape[0], dtype=torch.float64)).view(1, -1, 1, 1)
    bv = (b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)).view(1, -1, 1, 1)
    y = acc * sv + bv
    A = mag * sv.abs() + bv.abs()
    if r is not None:
        y = y + r.double(); A = A + r.double().abs()
    return (F.relu(y) if relu else y), A


def check(tag, got, y64, A, measured, C=C_MODEL):
    """|got - y64| <= C u A element by element (NCHW float32 vs float64); records the worst ratio"""
    assert torch.isfinite(got).all(), tag
    err = (got.double() - y64).abs()
    ratio = (err / (U * A.clamp_min(1e-300))).max().item()
    measured(f"conv_f32.{tag}", ratio)
    assert ratio <= C, (tag, ratio)
    return ratio


def conv_op(x, w, s, b, r, stride, pad, dil, relu, k_order=0):
    """x NCHW fp32 CPU -> the kernel's output NCHW on the CPU and the token of the launch"""
    from odam_amd import _lib
    L = _L()
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    wp, CinP, Kpad = _pack(w, k_order)
    xh = torch.zeros(B, H, W, CinP); xh[..., :Cin] = x.permute(0, 2, 3, 1)
    Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    M = B * Ho * Wo
    buf, dy = _guarded(M, Cout)
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    dx, dw, ds, db = d(xh), d(wp), d(s), d(b)
    dr = d(r.permute(0, 2, 3, 1)) if r is not None else None
    clear_paths()
    _lib.check(L.odam_op_conv2d_nhwc_ex(_lib.ptr(dx), _lib.ptr(dw), _lib.ptr(ds), _lib.ptr(db), _lib.ptr(dr), _lib.ptr(dy), B, H, W, CinP,
                                        Cout, KH, KW, stride, pad, dil, Kpad, int(relu), k_order, 0, 0, _st()), "conv")
    torch.cuda.synchronize()
    toks = paths()
    assert len(toks) == 1, toks
    assert _guards_intact(buf, M), "write outside the output rows"
    return dy.cpu().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2), toks[0]


def _operands(seed, B, H, W, Cin, Cout, k, stride, pad, dil, res, scale=True, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    s = torch.rand(Cout, generator=g) + 0.5 if scale else None
    b = torch.randn(Cout, generator=g) * 0.5 if bias else None
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = torch.randn(B, Cout, Ho, Wo, generator=g) if res else None
    return x, w, s, b, r


# (token, config, B, H, W, Cin, Cout, k, stride, pad, dil, relu, res, what)
SMALL = "f32.small."
CASES = [
    # small tiles, default switches: 128 x 64 (8 waves), 64 x 64 four-stage, 128 x 128 (8 waves); split in registers
    (SMALL + "128x64.w8.ut.x3", {}, 2, 37, 45, 64, 64, 1, 1, 0, 1, True, True, "1x1, ragged rows"),
    (SMALL + "128x64.w8.ut", {"cg_small_x3": 0}, 2, 37, 45, 64, 64, 3, 1, 1, 1, True, False, "3x3, fp32 instruction"),
    (SMALL + "128x64.w8", {}, 2, 19, 23, 16, 48, 3, 2, 1, 1, True, True, "Cin 16: register-staged gather, ragged columns"),
    (SMALL + "128x64.w4.ut.x3", {"cg_tiles": 29}, 3, 21, 17, 32, 40, 3, 1, 1, 1, False, True, "4-wave, ragged columns"),
    (SMALL + "128x64.w4.ut", {"cg_tiles": 29, "cg_small_x3": 0}, 3, 21, 17, 32, 40, 1, 1, 0, 1, True, False, ""),
    (SMALL + "128x64.w4", {"cg_tiles": 29, "cg_ut": 0}, 1, 33, 31, 64, 64, 3, 2, 1, 1, True, True, ""),
    (SMALL + "64x64.w4.ut.x3.s4", {}, 2, 37, 45, 64, 96, 3, 1, 1, 1, True, True, "tiles128 < 128"),
    (SMALL + "64x64.w4.ut.s4", {"cg_small_x3": 0}, 2, 37, 45, 64, 96, 1, 1, 0, 1, False, False, ""),
    (SMALL + "64x64.w4.ut.x3", {"cg_tiles": 27}, 5, 5, 5, 32, 72, 3, 1, 1, 1, False, False, "a 64-row tile spans three images"),
    (SMALL + "64x64.w4.ut", {"cg_tiles": 27, "cg_small_x3": 0}, 1, 1, 300, 256, 100, 1, 1, 0, 1, False, False, "linear rows"),
    (SMALL + "64x64.w4", {"cg_ut": 0}, 2, 25, 34, 128, 100, 1, 1, 0, 1, True, True, ""),
    (SMALL + "128x128.w8.ut.x3", {}, 1, 128, 129, 64, 256, 1, 1, 0, 1, True, True, "M = 16512"),
    (SMALL + "128x128.w8.ut", {"cg_small_x3": 0}, 1, 128, 129, 64, 256, 1, 1, 0, 1, False, False, ""),
    (SMALL + "128x128.w8", {"cg_ut": 0}, 1, 130, 129, 32, 200, 3, 1, 1, 1, True, False, "ragged columns"),
    (SMALL + "128x128.w4.ut.x3", {"cg_tiles": 30}, 1, 128, 129, 64, 256, 1, 1, 0, 1, True, True, ""),
    (SMALL + "128x128.w4.ut", {"cg_tiles": 30, "cg_small_x3": 0}, 1, 128, 129, 64, 256, 1, 1, 0, 1, True, False, ""),
    (SMALL + "128x128.w4", {"cg_tiles": 30, "cg_ut": 0}, 1, 128, 129, 64, 256, 1, 1, 0, 1, False, True, ""),
    (SMALL + "128x64.w8.ut.x3", {}, 2, 23, 29, 64, 64, 3, 1, 2, 2, True, False, "dilation 2 on the small tiles"),
    # ring kernel, 256 / 128 / 64 columns x MODE 4 / 3 / 2 (cg.pin = 1: the choice a full device gets)
    ("f32.ring.m4.256x256", {"cg_pin": 1}, 2, 37, 45, 64, 256, 1, 1, 0, 1, True, True, "expand shape"),
    ("f32.ring.m3.256x256", {"cg_pin": 1, "cg_mfma16": 0}, 2, 37, 45, 64, 256, 1, 1, 0, 1, True, True, ""),
    ("f32.ring.m2.256x256", {"cg_pin": 1, "cg_presplit": 0}, 2, 37, 45, 64, 256, 1, 1, 0, 1, True, True, ""),
    ("f32.ring.m4.256x128", {"cg_pin": 1}, 2, 33, 41, 128, 200, 3, 2, 1, 1, True, True, "stride 2, ragged columns"),
    ("f32.ring.m3.256x128", {"cg_pin": 1, "cg_mfma16": 0}, 2, 33, 41, 128, 200, 3, 2, 1, 1, True, True, ""),
    ("f32.ring.m2.256x128", {"cg_pin": 1, "cg_presplit": 0}, 2, 33, 41, 128, 200, 3, 2, 1, 1, True, True, ""),
    ("f32.ring.m4.512x64", {"cg_pin": 1}, 2, 37, 45, 64, 64, 3, 1, 1, 1, True, False, "sixteen waves"),
    ("f32.ring.m4.256x64", {"cg_ring": 2}, 2, 37, 45, 64, 64, 3, 1, 1, 1, True, False, ""),
    ("f32.ring.m3.256x64", {"cg_ring": 2, "cg_mfma16": 0}, 2, 37, 45, 64, 48, 3, 1, 1, 1, True, True, "ragged columns"),
    ("f32.ring.m2.256x64", {"cg_ring": 2, "cg_presplit": 0}, 2, 37, 45, 64, 48, 3, 1, 1, 1, True, True, ""),
    ("f32.ring.m4.256x128", {}, 1, 160, 160, 64, 256, 1, 1, 0, 1, True, True, "BN128 fallback: 100 256-wide tiles, 200 128-wide"),
    ("f32.ring.m4.256x128", {"cg_pin": 1}, 2, 23, 29, 64, 128, 3, 1, 2, 2, True, True, "dilation 2 on the ring"),
    ("f32.ring.m4.512x64", {"cg_pin": 1}, 1, 27, 33, 64, 64, 3, 1, 2, 2, True, False, "dilation 2, sixteen waves"),
    # ragged rows and short K on the ring
    ("f32.ring.m4.256x128", {"cg_pin": 1}, 1, 27, 19, 64, 128, 3, 1, 1, 1, True, True, "M % 256 == 1"),
    ("f32.ring.m4.512x64", {"cg_pin": 1}, 1, 7, 73, 64, 64, 3, 1, 1, 1, True, True, "M % 256 == 255, M < 512"),
    ("f32.ring.m4.256x256", {"cg_pin": 1}, 1, 15, 17, 256, 256, 1, 1, 0, 1, True, True, "M % 256 == 255"),
    ("f32.ring.m4.256x256", {"cg_pin": 1}, 3, 9, 13, 64, 256, 3, 2, 1, 1, True, True, "M = 105 < 256: one tile, three images"),
    ("f32.ring.m3.256x256", {"cg_pin": 1, "cg_mfma16": 0}, 3, 9, 13, 64, 256, 3, 2, 1, 1, True, True, ""),
    ("f32.ring.m4.256x128", {"cg_pin": 1}, 2, 16, 16, 16, 128, 1, 1, 0, 1, False, False, "K = 32: fewer k-tiles than stages"),
    ("f32.ring.m3.256x128", {"cg_pin": 1, "cg_mfma16": 0}, 2, 16, 16, 16, 128, 1, 1, 0, 1, False, False, ""),
    ("f32.ring.m2.256x128", {"cg_pin": 1, "cg_presplit": 0}, 2, 16, 16, 16, 128, 1, 1, 0, 1, False, False, ""),
    ("f32.ring.m4.512x64", {"cg_pin": 1}, 2, 23, 29, 32, 64, 3, 1, 1, 1, True, True, "K = 288: an odd number of 32-wide k-tiles"),
    ("f32.ring.m4.256x256", {"cg_pin": 1}, 2, 23, 29, 32, 256, 3, 1, 1, 1, True, True, ""),
    ("f32.ring.m3.256x64", {"cg_ring": 2, "cg_mfma16": 0}, 2, 23, 29, 32, 64, 3, 1, 1, 1, True, True, ""),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[-1] or 'plain'}".replace(" ", "_"))
def test_dispatch_vs_float64(case, measured):
    tok, cfg, B, H, W, Cin, Cout, k, s, p, dil, relu, res, what = case
    x, w, sc, bi, r = _operands(B * 7919 + H * 31 + W + Cin + Cout + k + dil, B, H, W, Cin, Cout, k, s, p, dil, res)
    y64, A = ref64(x, w, sc, bi, r, s, p, dil, relu)
    orders = (0, 1) if Cin % 32 == 0 and k > 1 else (0,)
    with config(**cfg):
        for k_order in orders:
            got, ran = conv_op(x, w, sc, bi, r, s, p, dil, relu, k_order)
            assert ran == tok, (what, ran)
            check(tok, got, y64, A, measured)
    COVERED.add(tok)


@pytest.mark.parametrize("drop", ["scale", "bias", "both"])
def test_ring_without_scale_or_bias(drop, measured):
    """a null scale acts as 1, a null bias as 0 on the ring kernel and the small tiles"""
    for tok, cfg, Cout in (("f32.ring.m4.256x128", {"cg_pin": 1}, 128), ("f32.ring.m4.512x64", {"cg_pin": 1}, 64),
                           ("f32.small.128x64.w8.ut.x3", {}, 64)):
        x, w, sc, bi, r = _operands(len(drop) + Cout, 2, 21, 27, 64, Cout, 3, 1, 1, 1, True, scale=drop == "bias", bias=drop == "scale")
        y64, A = ref64(x, w, sc, bi, r, 1, 1, 1, True)
        with config(**cfg):
            got, ran = conv_op(x, w, sc, bi, r, 1, 1, 1, True, 1)
        assert ran == tok
        check(tok + ".null", got, y64, A, measured)


# ---- the bottleneck on the tile (conv_gemm.hip fused_second_ok / launch_big_fused) -------------------------------------------
def bottleneck_op(x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride):
    """x NHWC fp32 CPU; returns (y, y_next or None) NHWC on the CPU and the token, or None where the entry refuses (code 4)"""
    from odam_amd import _lib
    L = _L()
    B, H, W, P = x.shape
    PN = w1.shape[0] if w1 is not None else 0
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    w2p, _, K2 = _pack(w2, 1); w3p, _, K3 = _pack(w3); assert K2 == 9 * P and K3 == P
    w1p = _pack(w1)[0] if PN else None
    ybuf, dy = _guarded(M, 4 * P)
    nbuf, dn = _guarded(M, max(PN, 1))
    args = [d(x), d(w2p), d(s2), d(b2), d(w3p), d(s3), d(b3), d(r), dy, d(w1p), d(s1), d(b1), dn if PN else None]
    clear_paths()
    rc = L.odam_op_bottleneck_f32(*[_lib.ptr(a) for a in args], B, H, W, P, stride, PN, _st())
    torch.cuda.synchronize()
    if rc == 4:
        return None
    _lib.check(rc, "bottleneck f32")
    toks = paths()
    assert len(toks) == 1, toks
    assert _guards_intact(ybuf, M) and _guards_intact(nbuf, M), "write outside the output rows"
    return dy.cpu().reshape(B, Ho, Wo, 4 * P), (dn.cpu().reshape(B, Ho, Wo, PN) if PN else None), toks[0]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def check_bottleneck(tag, x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride, measured):
    """fused launch: y against float64 of the expand applied to the SEPARATE launch's 3x3 output (the design says the fused launch
    computes that output bit for bit), y_next against float64 of the reduce applied to the kernel's own y; returns the token"""
    got = bottleneck_op(x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride)
    assert got is not None, f"{tag}: odam_op_bottleneck_f32 refused the shape"
    y, yn, tok = got
    t, tok2 = conv_op(_nchw(x), w2, s2, b2, None, stride, 1, 1, True, 1)
    t64, tA = ref64(_nchw(x), w2, s2, b2, None, stride, 1, 1, True)
    check(tok2, t, t64, tA, measured)
    y64, A = ref64(t, w3, s3, b3, _nchw(r) if r is not None else None, 1, 0, 1, True)
    check(tok + ".y", _nchw(y), y64, A, measured)
    if w1 is not None:
        n64, nA = ref64(_nchw(y), w1, s1, b1, None, 1, 0, 1, True)
        check(tok + ".y_next", _nchw(yn), n64, nA, measured)
    COVERED.add(tok)
    return tok


def _block_operands(seed, B, H, W, P, PN, stride, res=True, drop=""):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = F.relu(torch.randn(B, H, W, P, generator=g))
    w2 = torch.randn(P, P, 3, 3, generator=g) / (9 * P) ** 0.5
    w3 = torch.randn(4 * P, P, 1, 1, generator=g) / P ** 0.5
    w1 = torch.randn(PN, 4 * P, 1, 1, generator=g) / (4 * P) ** 0.5 if PN else None
    sc = lambda n: None if drop in ("scale", "both") else torch.rand(n, generator=g) + 0.5
    bi = lambda n: None if drop in ("bias", "both") else torch.randn(n, generator=g) * 0.3
    s2, b2, s3, b3 = sc(P), bi(P), sc(4 * P), bi(4 * P)
    s1, b1 = (sc(PN), bi(PN)) if PN else (None, None)
    r = torch.randn(B, Ho, Wo, 4 * P, generator=g) if res else None
    return x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1


FUSED = {(64, 0): "l1", (64, 64): "chain64", (64, 128): "chain128", (128, 0): "l2"}


@pytest.mark.parametrize("mode", [4, 3])
@pytest.mark.parametrize("P,PN", list(FUSED))
@pytest.mark.parametrize("stride", [1, 2])
def test_fused_bottleneck_vs_float64(P, PN, stride, mode, measured):
    """all eight fused launches (FUSE 1-4 x 16x16x32 / 32x32x16 products), stride 1 and 2, ragged last row tile"""
    B, H, W = 2, 37, 45
    ops = _block_operands(P * 10 + PN + stride, B, H, W, P, PN, stride)
    with config(cg_pin=1, cg_mfma16=3 if mode == 4 else 0):
        tok = check_bottleneck(f"fused.{P}.{PN}.s{stride}", *ops, stride, measured)
    assert tok == f"f32.fused.m{mode}.{FUSED[(P, PN)]}"


@pytest.mark.parametrize("B,H,W,what", [(1, 27, 19, "M % 256 == 1"), (1, 15, 17, "M % 256 == 255"), (3, 5, 7, "M = 105: one tile, three images")])
@pytest.mark.parametrize("P,PN", [(64, 128), (64, 64), (128, 0)])
def test_fused_bottleneck_ragged_rows(B, H, W, what, P, PN, measured):
    ops = _block_operands(B + H + W + P + PN, B, H, W, P, PN, 1)
    with config(cg_pin=1):
        check_bottleneck(f"fused.ragged.{P}.{PN}", *ops, 1, measured)


@pytest.mark.parametrize("P,PN,res,drop", [(64, 0, False, ""), (64, 128, False, ""), (128, 0, False, ""), (64, 64, True, "scale"),
                                           (64, 128, True, "bias"), (128, 0, True, "both"), (64, 0, True, "both")])
def test_fused_bottleneck_null_operands(P, PN, res, drop, measured):
    """no residual; no scale (acts as 1) / no bias (0) on every layer of the launch (TailAffine's record-less descriptors,
    fused_chain's G_scale ? ... : 1)"""
    ops = _block_operands(P + PN + len(drop), 2, 21, 27, P, PN, 1, res=res, drop=drop)
    with config(cg_pin=1):
        check_bottleneck(f"fused.null.{P}.{PN}", *ops, 1, measured)


def test_fused_bottleneck_refusals():
    """the entry says 4 where the fused kernel does not apply: too few rows without cg.pin, the fusion switched off, a P not built"""
    ops = _block_operands(1, 1, 20, 20, 64, 64, 1)
    with config(cg_pin=0, cg_ring=1):
        assert bottleneck_op(*ops, 1) is None
    with config(cg_pin=1, cg_fuse=0):
        assert bottleneck_op(*ops, 1) is None
    with config(cg_pin=1, cg_fuse=1):          # expand only: the chained reduce is refused, the plain launch is not
        assert bottleneck_op(*ops, 1) is None
        assert bottleneck_op(*ops[:8], None, None, None, 1) is not None
    ops = _block_operands(2, 1, 12, 12, 256, 0, 1)
    with config(cg_pin=1):
        assert bottleneck_op(*ops, 1) is None


# ---- every contraction of R50 on the oracle's own inputs ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def r50_trace():
    import os
    import sys
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import detr_oracle as O
    from odam_amd import weights
    sd = weights.make_state_dict(seed=0, scene=True)
    torch.manual_seed(3)
    img = torch.randn(2, 3, 192, 256)
    O.F32_TRACE = []
    try:
        O.detr_forward(sd, img)
        return O.F32_TRACE
    finally:
        O.F32_TRACE = None


def _rec_as_conv(rec):
    """a trace record as (x, w, s, b, r, stride, pad, dil, relu) in NCHW; linear rows [.., K] -> a 1 x 1 x rows image"""
    if rec["kind"] == "linear":
        K_ = rec["x"].shape[-1]
        x = rec["x"].reshape(1, -1, K_).permute(0, 2, 1).unsqueeze(2)
        w = rec["w"].reshape(rec["w"].shape[0], K_, 1, 1)
        return x, w, None, rec["bias"], None, 1, 0, 1, rec["relu"]
    return rec["x"], rec["w"], rec["scale"], rec["bias"], rec["res"], rec["stride"], rec["padding"], rec["dilation"], rec["relu"]


@pytest.mark.parametrize("pin", [0, 1])
def test_r50_layers_teacher_forced(r50_trace, pin, measured):
    """R50 + transformer + heads at 2 x 3 x 192 x 256: every convolution and linear layer on the fp32 oracle's own operands, and every
    bottleneck the fused launch takes (cg.pin = 1: layer1 and layer2) through odam_op_bottleneck_f32, each against float64"""
    trace = r50_trace
    n_checked, n_fused, outs = 0, 0, {}
    with config(cg_pin=pin):
        for i, rec in enumerate(trace):
            if rec["kind"] == "block":
                continue
            x, w, s, b, r, stride, pad, dil, relu = _rec_as_conv(rec)
            k_order = 1 if x.shape[1] % 32 == 0 and w.shape[2] > 1 else 0
            y64, A = ref64(x, w, s, b, r, stride, pad, dil, relu)
            got, tok = conv_op(x, w, s, b, r, stride, pad, dil, relu, k_order)
            check(f"teacher_forced.pin{pin}.{tok}", got, y64, A, measured)
            outs[i] = got
            n_checked += 1
        for rec in trace:
            if rec["kind"] != "block":
                continue
            c2, c3 = trace[rec["c2"]], trace[rec["c3"]]
            P = c2["w"].shape[0]
            if P not in (64, 128) or c2["dilation"] != 1:
                continue
            nx = trace[rec["next_c1"]] if rec["next_c1"] is not None else None
            PN = nx["w"].shape[0] if (nx is not None and P == 64 and nx["w"].shape[0] in (64, 128)) else 0
            nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous() if t is not None else None
            args = [nhwc(c2["x"]), c2["w"], c2["scale"], c2["bias"], c3["w"], c3["scale"], c3["bias"], nhwc(c3["res"]),
                    nx["w"] if PN else None, nx["scale"] if PN else None, nx["bias"] if PN else None]
            got = bottleneck_op(*args, c2["stride"])
            if got is None:
                assert not pin, rec["name"]         # pinned: layer1 and layer2 always fuse
                continue
            y, yn, tok = got
            t = outs[rec["c2"]]                     # the separate launch's 3x3 output
            y64, A = ref64(t, c3["w"], c3["scale"], c3["bias"], c3["res"], 1, 0, 1, True)
            check(f"teacher_forced.pin{pin}.{tok}.y", _nchw(y), y64, A, measured)
            if PN:
                n64, nA = ref64(_nchw(y), nx["w"], nx["scale"], nx["bias"], None, 1, 0, 1, True)
                check(f"teacher_forced.pin{pin}.{tok}.y_next", _nchw(yn), n64, nA, measured)
            n_fused += 1
    assert n_checked >= 53 + 1 + 112
    if pin:
        assert n_fused == 3 + 4


# ---- cg.pin: the kernel choice and the bits of a frame do not depend on the batch --------------------------------------------
def test_pin_choice_and_bits_do_not_depend_on_batch():
    """Under cg.pin = 1 the token sequence of a 2-frame 192 x 256 forward equals a 42-frame 800 x 1066 one (what Detector.batch_for
    gives a shard of <= 300 frames; layer1's output is 2.3 GB there, past the fused launch's 31-bit offsets), and frames 0 and 41
    of the 42-frame forward equal, bit for bit, the same frames forwarded as a pair"""
    from odam_amd import detector, weights
    sd = weights.make_state_dict(seed=0, scene=True)
    keys = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")
    with config(cg_pin=1):
        small = detector.Detector(max_batch=2, device=DEV, n_streams=1)
        small.load_state_dict(sd)
        torch.manual_seed(3)
        clear_paths()
        small(torch.randn(2, 3, 192, 256, device=DEV))
        torch.cuda.synchronize()
        seq_small = paths()
        small.close()
        det = detector.Detector(max_batch=42, device=DEV, n_streams=1)
        det.load_state_dict(sd)
        g = torch.Generator(device=DEV).manual_seed(5)
        img = torch.randn(42, 3, 800, 1066, device=DEV, generator=g)
        clear_paths()
        big = {k: v.clone() for k, v in det(img).items() if torch.is_tensor(v)}
        torch.cuda.synchronize()
        seq_big = paths()
        pair = det(img[[0, 41]].contiguous())
        torch.cuda.synchronize()
        det.close()
    assert "f32.ring.m4.512x64.pool" in seq_small and "f32.fused.m4.chain128" in seq_small
    COVERED.update(t for t in seq_small if t.startswith("f32."))
    diff = [(i, a, b) for i, (a, b) in enumerate(zip(seq_small, seq_big)) if a != b]
    assert seq_small == seq_big, (len(seq_small), len(seq_big), diff[:8])
    for k in keys:
        assert torch.equal(big[k][[0, 41]], pair[k]), k


def test_every_documented_f32_path_is_covered():
    """the union of the tokens the cases above name is the documented fp32 list (include/odam_detr.h): a branch of the dispatch
    cannot drop out of this file's coverage unnoticed"""
    named = {c[0] for c in CASES} | {f"f32.fused.m{m}.{v}" for m in (3, 4) for v in FUSED.values()} | {"f32.ring.m4.512x64.pool"}
    assert named == documented_f32_tokens(), sorted(named ^ documented_f32_tokens())
    assert COVERED <= named, sorted(COVERED - named)        # every token a case observed is documented
