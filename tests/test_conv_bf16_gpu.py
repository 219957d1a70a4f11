"""The bf16 contraction kernels (odam_amd/csrc/conv_gemm.hip launch_conv_gemm with dtype 1 and what it dispatches to) against
float64 computed from the same bf16 operands, element by element, on every bf16 branch of the dispatch: the small tiles, the ring
kernel's five tile shapes, the 3x3 stride-1 window loop at image borders, the fused bottleneck launches, the pooled stem.

Error model, reference and check: tests/conv_bf16_ref.py (its CPU-only tests: tests/test_conv_bf16_ref_host.py).  In short, the
kernel's fp32 value v of an element obeys |v - y64| <= C u A (A the magnitude sum, u = 2^-24); an fp32 output is held to that, a bf16
output to the interval [rne_bf16(y64 - C u A), rne_bf16(y64 + C u A)], which is one or two bf16 values wide and so rejects
truncation, a second rounding point and a missing tap.  Budget C = 8; asserted C_BF16 = 1.4 x the worst ratio measured = 2.97.
Measured on an MI355X (`measured`, conftest.py, under conv_bf16.<tag>; profiles/conv_bf16_test_measured.json), worst
|v - y64| / (u A) of the fp32-output launches per token:
  bf16.small.128x64.w8.ut 1.74   .w8 1.46   .w4.ut 1.46   .w4 1.10      bf16.small.64x64.w4.ut.s4 1.77   .w4.ut 1.38   .w4 2.12
  bf16.small.128x128.w8.ut 1.90  .w8 1.79   .w4.ut 1.97   .w4 2.06
  bf16.ring.256x64 1.40   256x128 1.88   256x256 1.93   512x64 1.74      null scale / bias 1.21 - 1.66
  3x3 stride 1 at image borders: window loop 1.34 / 1.37 / 2.09 (256 x 64 / 128 / 256), generic gather 1.60 / 1.22 / 2.09
The fused launches have bf16 outputs only; in the measuring run theirs and every other bf16 output lay inside the interval
already at C = 1 (the intervals nest, so they hold at every larger C).
profiles/conv_bf16_planted_mistake.txt: which of these tests fail on a library with truncation, a border mask one pixel off, or the
residual added after the rounding planted in it.

Every case names the kernel that ran by its token (include/odam_detr.h odam_op_conv_paths) and runs with out_f32 1 and 0 and, where
Cin % 64 == 0 and the filter has more than one tap, in both k orders.  bf16 outputs are prefilled with the NaN bits 0x7FC0 and
fp32 outputs with NaN, 300 guard rows on either side: an element the kernel never wrote is not finite, a write outside the tensor
changes a guard.  Every first tile starts at pixel 0 of image 0, where the window loop's rebased descriptor (one row and one pixel
before the tensor) begins before the tensor.

bf16.ring.512x64.pool (conv1 with the max-pool on its tile) has no operator entry: test_pooled_stem_token_in_a_forward asserts
that a pinned bf16 forward takes it; its arithmetic is pinned by tests/test_detr_gpu.py::test_pooled_stem_is_bit_identical."""
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from conv_bf16_ref import C_BF16, interval_violations, ratio_f32, ref64, to_bf16
from test_conv_f32_gpu import DEV, GUARD, _L, _st, clear_paths, config, paths

pytestmark = pytest.mark.gpu
NAN_BF16 = 0x7FC0
COVERED = set()     # tokens the cases of this module asserted


def documented_bf16_tokens():
    txt = open(f"{REPO}/include/odam_detr.h").read()
    block = txt[txt.index("BF16-TOKENS-BEGIN"):txt.index("BF16-TOKENS-END")]
    return set(re.findall(r"\bbf16\.[a-z0-9.]+[a-z0-9]", block))


def _bits(t):
    """float32 holding bf16 values -> the raw bf16 words on the device"""
    return t.contiguous().to(torch.bfloat16).view(torch.int16).to(DEV)


def _pack(w, k_order=0):
    """[Cout,Cin,KH,KW] -> [Cout][Kpad], Cin padded to a power of two >= 8, K to a multiple of 64; K order 0 = (tap, ci),
    1 = (ci // 64, tap, ci % 64) (include/odam_detr.h)"""
    Cout, Cin, KH, KW = w.shape
    CinP = max(8, 1 << (Cin - 1).bit_length())
    wp = torch.zeros(Cout, KH, KW, CinP); wp[..., :Cin] = w.permute(0, 2, 3, 1)
    Kk = KH * KW * CinP; Kpad = (Kk + 63) // 64 * 64
    if k_order:
        wp = wp.reshape(Cout, KH * KW, CinP // 64, 64).permute(0, 2, 1, 3)
    out = torch.zeros(Cout, Kpad); out[:, :Kk] = wp.reshape(Cout, Kk)
    return out, CinP, Kpad


def _guarded(rows, cols, f32=False):
    """[GUARD + rows + GUARD, cols] of NaN (fp32) or of the bf16 NaN bits 0x7FC0 on the device; (whole, the middle view)"""
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device=DEV) if f32 else \
        torch.full((rows + 2 * GUARD, cols), NAN_BF16, device=DEV, dtype=torch.int16)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    g = torch.cat([buf[:GUARD], buf[GUARD + rows:]])
    return bool((torch.isnan(g) if buf.dtype == torch.float32 else g == NAN_BF16).all().item())


def _values(dy):
    """the middle view of a guarded output -> float32 on the CPU"""
    return (dy if dy.dtype == torch.float32 else dy.contiguous().view(torch.bfloat16).float()).cpu()


def check(tag, got, y64, A, out_f32, measured, C=C_BF16):
    """fp32 output: |got - y64| <= C u A, the worst ratio recorded; bf16 output: the interval test"""
    if out_f32:
        ratio = ratio_f32(got, y64, A)
        measured(f"conv_bf16.{tag}", ratio)
        print(f"conv_bf16.{tag} fp32 output: ratio {ratio:.3f}")
        assert ratio <= C, (tag, ratio)
        return
    bad = interval_violations(got, y64, A, C)
    print(f"conv_bf16.{tag} bf16 output: {bad} of {got.numel()} outside the interval")
    assert bad == 0, (tag, bad, got.numel())


def conv_op(x, w, s, b, r, stride, pad, dil, relu, k_order=0, out_f32=0):
    """x NCHW (bf16 values) on the CPU -> the kernel's output NCHW float32 on the CPU and the token of the launch"""
    from odam_amd import _lib
    L = _L()
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    wp, CinP, Kpad = _pack(w, k_order)
    xh = torch.zeros(B, H, W, CinP); xh[..., :Cin] = x.permute(0, 2, 3, 1)
    Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    M = B * Ho * Wo
    buf, dy = _guarded(M, Cout, out_f32)
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    dx, dw, ds, db = _bits(xh), _bits(wp), d(s), d(b)
    dr = _bits(r.permute(0, 2, 3, 1)) if r is not None else None
    clear_paths()
    _lib.check(L.odam_op_conv2d_nhwc_ex(_lib.ptr(dx), _lib.ptr(dw), _lib.ptr(ds), _lib.ptr(db), _lib.ptr(dr), _lib.ptr(dy), B, H, W, CinP,
                                        Cout, KH, KW, stride, pad, dil, Kpad, int(relu), k_order, 1, int(out_f32), _st()), "conv bf16")
    torch.cuda.synchronize()
    toks = paths()
    assert len(toks) == 1, toks
    assert _guards_intact(buf, M), "write outside the output rows"
    return _values(dy).reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2), toks[0]


def _operands(seed, B, H, W, Cin, Cout, k, stride, pad, dil, res, scale=True, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = to_bf16(torch.randn(B, Cin, H, W, generator=g))
    w = to_bf16(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    s = torch.rand(Cout, generator=g) + 0.5 if scale else None
    b = torch.randn(Cout, generator=g) * 0.5 if bias else None
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = to_bf16(torch.randn(B, Cout, Ho, Wo, generator=g)) if res else None
    return x, w, s, b, r


def run_case(tok, cfg, x, w, s, b, r, stride, pad, dil, relu, measured, tag=None):
    """one layer under `cfg`: out_f32 1 and 0, both k orders where legal; every launch must note `tok`"""
    y64, A = ref64(x, w, s, b, r, stride, pad, dil, relu)
    orders = (0, 1) if x.shape[1] % 64 == 0 and w.shape[2] > 1 else (0,)
    with config(**cfg):
        for k_order in orders:
            for out_f32 in (1, 0):
                got, ran = conv_op(x, w, s, b, r, stride, pad, dil, relu, k_order, out_f32)
                assert ran == tok, (ran, k_order, out_f32)
                check(tag or tok, got, y64, A, out_f32, measured)
    COVERED.add(tok)


# (token, config, B, H, W, Cin, Cout, k, stride, pad, dil, relu, res, what)
SMALL = "bf16.small."
RING = {"cg_pin": 1, "cg_ring": 2}      # what the ring branches of launch_conv_gemm need on a problem this small
CASES = [
    # small tiles, default switches: 128 x 64 (8 waves), 64 x 64 four-stage, 128 x 128 (8 waves); cg.tiles takes a bit away
    (SMALL + "128x64.w8.ut", {}, 2, 37, 45, 64, 64, 1, 1, 0, 1, True, True, "1x1, ragged rows"),
    (SMALL + "128x64.w8.ut", {}, 2, 23, 29, 64, 64, 3, 1, 2, 2, True, False, "dilation 2"),
    (SMALL + "128x64.w8", {}, 1, 31, 29, 3, 64, 7, 2, 3, 1, True, False, "stem: Cin 3 -> 8, K 392 -> 448, 7x7 stride 2"),
    (SMALL + "128x64.w8", {}, 2, 19, 23, 16, 40, 3, 2, 1, 1, True, True, "Cin 16: register-staged gather, ragged columns"),
    (SMALL + "128x64.w4.ut", {"cg_tiles": 29}, 3, 21, 17, 64, 40, 3, 1, 1, 1, False, True, "ragged columns"),
    (SMALL + "128x64.w4", {"cg_tiles": 29}, 1, 33, 31, 32, 64, 3, 2, 1, 1, True, True, "Cin 32"),
    (SMALL + "64x64.w4.ut.s4", {}, 2, 37, 45, 64, 96, 3, 1, 1, 1, True, True, "tiles128 < 128"),
    (SMALL + "64x64.w4.ut", {"cg_tiles": 27}, 1, 1, 300, 256, 100, 1, 1, 0, 1, False, False, "linear rows, ragged columns"),
    (SMALL + "64x64.w4", {}, 5, 5, 5, 32, 72, 3, 1, 1, 1, False, False, "Cin 32: a 64-row tile spans three images"),
    (SMALL + "64x64.w4", {"cg_ut": 0}, 2, 25, 34, 128, 100, 1, 1, 0, 1, True, True, "cg.ut 0"),
    (SMALL + "128x128.w8.ut", {}, 1, 128, 129, 64, 256, 1, 1, 0, 1, True, True, "M = 16512"),
    (SMALL + "128x128.w8", {}, 1, 130, 129, 32, 200, 3, 1, 1, 1, True, False, "Cin 32, ragged columns"),
    (SMALL + "128x128.w4.ut", {"cg_tiles": 30}, 1, 128, 129, 64, 256, 1, 1, 0, 1, False, True, "M = 16512"),
    (SMALL + "128x128.w4", {"cg_tiles": 30, "cg_ut": 0}, 1, 128, 129, 64, 256, 1, 1, 0, 1, True, False, "M = 16512"),
    # ring kernel.  256 x 256: sixteen waves (1024 threads: plain layers under cg.tiles bit 4) and eight waves (512 threads)
    ("bf16.ring.256x256", RING, 2, 37, 45, 64, 256, 1, 1, 0, 1, True, True, "1024 threads, K = 64: fewer k-tiles than stages"),
    ("bf16.ring.256x256", RING, 1, 15, 17, 256, 256, 1, 1, 0, 1, True, True, "1024 threads, M % 256 == 255"),
    ("bf16.ring.256x256", RING, 3, 9, 13, 64, 256, 3, 2, 1, 1, True, True, "1024 threads, stride 2, M = 105: one tile, three images"),
    ("bf16.ring.256x256", {**RING, "cg_tiles": 15}, 1, 27, 19, 128, 256, 1, 1, 0, 1, True, True, "512 threads, M % 256 == 1"),
    ("bf16.ring.256x256", {**RING, "cg_tiles": 15}, 2, 23, 29, 32, 512, 3, 1, 1, 1, False, False, "512 threads, five 64-wide k-tiles"),
    ("bf16.ring.256x128", RING, 2, 33, 41, 128, 200, 3, 2, 1, 1, True, True, "stride 2, ragged columns"),
    ("bf16.ring.256x128", RING, 2, 23, 29, 64, 128, 3, 1, 2, 2, True, True, "dilation 2"),
    ("bf16.ring.256x128", RING, 2, 23, 29, 32, 128, 3, 1, 1, 1, True, True, "five 64-wide k-tiles (odd)"),
    ("bf16.ring.256x128", RING, 1, 27, 19, 64, 128, 1, 1, 0, 1, False, False, "K = 64, M % 256 == 1"),
    ("bf16.ring.256x64", {**RING, "cg_tiles": 23}, 1, 27, 19, 64, 48, 1, 1, 0, 1, True, True, "K = 64, M % 256 == 1, ragged columns"),
    ("bf16.ring.256x64", RING, 1, 27, 33, 64, 64, 3, 1, 2, 2, True, False, "dilation 2"),
    ("bf16.ring.256x64", {**RING, "cg_tiles": 23}, 3, 9, 13, 64, 64, 3, 2, 1, 1, True, True, "stride 2, M = 105: one tile, three images"),
    ("bf16.ring.512x64", RING, 2, 37, 45, 64, 64, 1, 1, 0, 1, True, True, "K = 64"),
    ("bf16.ring.512x64", RING, 1, 15, 17, 128, 64, 1, 1, 0, 1, True, True, "M = 255 < 512"),
    ("bf16.ring.512x64", RING, 2, 33, 41, 64, 64, 3, 2, 1, 1, True, False, "stride 2"),
    ("bf16.ring.512x64", RING, 1, 23, 29, 32, 64, 3, 2, 1, 1, True, True, "five 64-wide k-tiles (odd), M < 512"),
    ("bf16.ring.512x64", RING, 3, 9, 13, 64, 64, 3, 2, 1, 1, False, True, "M = 105: one tile, three images"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[-1]}".replace(" ", "_"))
def test_dispatch_vs_float64(case, measured):
    tok, cfg, B, H, W, Cin, Cout, k, s, p, dil, relu, res, what = case
    ops = _operands(B * 7919 + H * 31 + W + Cin + Cout + k + dil, B, H, W, Cin, Cout, k, s, p, dil, res)
    run_case(tok, cfg, *ops, s, p, dil, relu, measured)


@pytest.mark.parametrize("drop", ["scale", "bias", "both"])
def test_without_scale_or_bias(drop, measured):
    """a null scale acts as 1, a null bias as 0 on the ring kernel's tiles and the small tiles"""
    for tok, cfg, Cout, stride in (("bf16.ring.256x128", RING, 128, 1), ("bf16.ring.512x64", RING, 64, 2), ("bf16.ring.256x256", RING, 256, 2),
                                   ("bf16.small.128x64.w8.ut", {}, 64, 1)):
        ops = _operands(len(drop) + Cout, 2, 21, 27, 64, Cout, 3, stride, 1, 1, True, scale=drop == "bias", bias=drop == "scale")
        run_case(tok, cfg, *ops, stride, 1, 1, True, measured, tag=tok + ".null")


# ---- the 3x3 stride-1 window loop (cg_big.hpp, cg.s1) where its shifted window leaves the image --------------------------------
WINDOW_SHAPES = [(2, 9, 1, "W = 1: kx 0 and 2 never valid"), (2, 1, 11, "H = 1"), (3, 7, 2, "W = 2"),
                 (3, 5, 7, "three images in one tile"), (1, 27, 19, "M % 256 == 1")]


@pytest.mark.parametrize("s1", [1, 0])
@pytest.mark.parametrize("Cout", [64, 128, 256])
@pytest.mark.parametrize("B,H,W,what", WINDOW_SHAPES, ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else str(v))
def test_window_loop_at_image_borders(B, H, W, what, Cout, s1, measured):
    """3x3, stride 1, pad 1 on the 512-thread ring tiles: the window loop (cg.s1 = 1; taken in k order 1) and the generic tap gather
    (cg.s1 = 0) against float64, Cin 64 and 128"""
    Cin = 128 if (H + W + Cout // 64) % 2 else 64
    ops = _operands(B + H * 31 + W + Cout + 5, B, H, W, Cin, Cout, 3, 1, 1, 1, True)
    run_case(f"bf16.ring.256x{Cout}", {**RING, "cg_s1": s1}, *ops, 1, 1, 1, True, measured, tag=f"window.s1_{s1}.256x{Cout}")


# ---- the bottleneck on the tile (conv_gemm.hip fused_bf16_ok / launch_fused_bf16, cg_tail_bf16.hpp) ----------------------------
def bottleneck_op(x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride):
    """x NHWC (bf16 values) on the CPU; returns (y, y_next or None) NHWC float32 on the CPU and the token, or None where the entry
    refuses (code 4)"""
    from odam_amd import _lib
    L = _L()
    B, H, W, P = x.shape
    PN = w1.shape[0] if w1 is not None else 0
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    bt = lambda t: _bits(t) if t is not None else None
    w2p, _, K2 = _pack(w2, 1); w3p, _, K3 = _pack(w3); assert K2 == 9 * P and K3 == P
    w1p = _pack(w1)[0] if PN else None
    ybuf, dy = _guarded(M, 4 * P)
    nbuf, dn = _guarded(M, max(PN, 1))
    args = [bt(x), bt(w2p), d(s2), d(b2), bt(w3p), d(s3), d(b3), bt(r), dy, bt(w1p), d(s1), d(b1), dn if PN else None]
    clear_paths()
    rc = L.odam_op_bottleneck_bf16(*[_lib.ptr(a) for a in args], B, H, W, P, stride, PN, _st())
    torch.cuda.synchronize()
    if rc == 4:
        assert paths() == []
        return None
    _lib.check(rc, "bottleneck bf16")
    toks = paths()
    assert len(toks) == 1, toks
    assert _guards_intact(ybuf, M) and _guards_intact(nbuf, M), "write outside the output rows"
    return _values(dy).reshape(B, Ho, Wo, 4 * P), (_values(dn).reshape(B, Ho, Wo, PN) if PN else None), toks[0]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def check_bottleneck(tag, x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride, measured):
    """fused launch: the SEPARATE launch's 3x3 output against float64; y against float64 of the expand applied to that output (the
    fused launch computes it bit for bit: same kernel, same k order); y_next against float64 of the reduce applied to the kernel's
    own y; returns the token"""
    got = bottleneck_op(x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1, stride)
    assert got is not None, f"{tag}: odam_op_bottleneck_bf16 refused the shape"
    y, yn, tok = got
    t, tok2 = conv_op(_nchw(x), w2, s2, b2, None, stride, 1, 1, True, 1)
    assert tok2.startswith("bf16.ring."), tok2
    t64, tA = ref64(_nchw(x), w2, s2, b2, None, stride, 1, 1, True)
    check(f"{tag}.t", t, t64, tA, 0, measured)
    y64, A = ref64(t, w3, s3, b3, _nchw(r) if r is not None else None, 1, 0, 1, True)
    check(f"{tag}.y", _nchw(y), y64, A, 0, measured)
    if w1 is not None:
        n64, nA = ref64(_nchw(y), w1, s1, b1, None, 1, 0, 1, True)
        check(f"{tag}.y_next", _nchw(yn), n64, nA, 0, measured)
    COVERED.add(tok)
    return tok


def _block_operands(seed, B, H, W, P, PN, stride, res=True, drop=""):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = to_bf16(F.relu(torch.randn(B, H, W, P, generator=g)))
    w2 = to_bf16(torch.randn(P, P, 3, 3, generator=g) / (9 * P) ** 0.5)
    w3 = to_bf16(torch.randn(4 * P, P, 1, 1, generator=g) / P ** 0.5)
    w1 = to_bf16(torch.randn(PN, 4 * P, 1, 1, generator=g) / (4 * P) ** 0.5) if PN else None
    sc = lambda n: None if drop in ("scale", "both") else torch.rand(n, generator=g) + 0.5
    bi = lambda n: None if drop in ("bias", "both") else torch.randn(n, generator=g) * 0.3
    s2, b2, s3, b3 = sc(P), bi(P), sc(4 * P), bi(4 * P)
    s1, b1 = (sc(PN), bi(PN)) if PN else (None, None)
    r = to_bf16(torch.randn(B, Ho, Wo, 4 * P, generator=g)) if res else None
    return x, w2, s2, b2, w3, s3, b3, r, w1, s1, b1


FUSED = {(64, 0): "p64", (64, 64): "p64.chain64", (64, 128): "p64.chain128", (128, 0): "p128", (128, 128): "p128.chain128", (256, 0): "p256"}


@pytest.mark.parametrize("stride,s1", [(1, 1), (1, 0), (2, 1)])
@pytest.mark.parametrize("P,PN", list(FUSED))
def test_fused_bottleneck_vs_float64(P, PN, stride, s1, measured):
    """all six fused launches, stride 1 (window loop and generic gather) and 2, ragged last row tile (3330 / 874 rows)"""
    B, H, W = 2, 37, 45
    ops = _block_operands(P * 10 + PN + stride, B, H, W, P, PN, stride)
    with config(**RING, cg_s1=s1):
        tok = check_bottleneck(f"fused.{FUSED[(P, PN)]}.stride{stride}.s1_{s1}", *ops, stride, measured)
    assert tok == "bf16.fused." + FUSED[(P, PN)]


@pytest.mark.parametrize("B,H,W,what", [(1, 27, 19, "M % 256 == 1"), (3, 5, 7, "M = 105: one tile, three images")])
@pytest.mark.parametrize("P,PN", list(FUSED))
def test_fused_bottleneck_ragged_rows(B, H, W, what, P, PN, measured):
    ops = _block_operands(B + H + W + P + PN, B, H, W, P, PN, 1)
    with config(**RING):
        check_bottleneck(f"fused.ragged.{FUSED[(P, PN)]}", *ops, 1, measured)


@pytest.mark.parametrize("P,PN,res,drop", [(64, 0, False, ""), (64, 128, False, ""), (128, 128, False, ""), (256, 0, False, ""),
                                           (64, 64, True, "scale"), (64, 128, True, "bias"), (128, 128, True, "both"),
                                           (256, 0, True, "both"), (128, 0, True, "scale")])
def test_fused_bottleneck_null_operands(P, PN, res, drop, measured):
    """no residual; no scale (acts as 1) / no bias (0) on every layer of the launch (descriptors that hold no records)"""
    ops = _block_operands(P + PN + len(drop), 2, 21, 27, P, PN, 1, res=res, drop=drop)
    with config(**RING):
        check_bottleneck(f"fused.null.{FUSED[(P, PN)]}", *ops, 1, measured)


def test_fused_bottleneck_refusals():
    """the entry says 4 where the fused kernel does not apply: too few rows without cg.pin, the fusion switched off, a chain with
    cg.fuse_bf16 = 1, a (P, PN) that is not built"""
    ops = _block_operands(1, 1, 20, 20, 64, 64, 1)
    with config(cg_pin=0, cg_ring=1):
        assert bottleneck_op(*ops, 1) is None
    with config(**RING, cg_fuse_bf16=0):
        assert bottleneck_op(*ops, 1) is None
        assert bottleneck_op(*ops[:8], None, None, None, 1) is None
    with config(**RING, cg_fuse_bf16=1):        # expand only: the chained reduce is refused, the plain launch is not
        assert bottleneck_op(*ops, 1) is None
        assert bottleneck_op(*ops[:8], None, None, None, 1) is not None
    with config(**RING):
        for P, PN in ((128, 64), (256, 128), (256, 256), (512, 0), (64, 256)):
            assert bottleneck_op(*_block_operands(2, 1, 12, 12, P, PN, 1), 1) is None, (P, PN)


# ---- the pooled stem -------------------------------------------------------------------------------------------------------
def test_pooled_stem_token_in_a_forward():
    """one 2-frame 192 x 256 bf16 forward under cg.pin = 1 runs conv1 with the max-pool on its tile, and every bf16 token it notes
    is a documented one"""
    from odam_amd import detector, weights
    sd = weights.make_state_dict(seed=0, scene=True)
    with config(cg_pin=1):
        det = detector.Detector(max_batch=2, device=DEV, n_streams=1, dtype="bf16")
        det.load_state_dict(sd)
        torch.manual_seed(3)
        img = torch.randn(2, 3, 192, 256, device=DEV)
        clear_paths()
        out = det(img)
        torch.cuda.synchronize()
        seq = paths()
        det.close()
    assert all(torch.isfinite(v).all() for v in out.values() if torch.is_tensor(v))
    assert "bf16.ring.512x64.pool" in seq, sorted(set(seq))
    assert {t for t in seq if t.startswith("bf16.")} <= documented_bf16_tokens()
    COVERED.add("bf16.ring.512x64.pool")


def test_every_documented_bf16_path_is_covered():
    """the union of the tokens the cases above name is the documented bf16 list (include/odam_detr.h): a branch of the dispatch
    cannot drop out of this file's coverage unnoticed"""
    named = {c[0] for c in CASES} | {"bf16.fused." + v for v in FUSED.values()} | {"bf16.ring.512x64.pool"}
    assert named == documented_bf16_tokens(), sorted(named ^ documented_bf16_tokens())
    assert COVERED <= named, sorted(COVERED - named)        # every token a case observed is documented
