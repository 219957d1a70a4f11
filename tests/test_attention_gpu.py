"""The transformer's attention and LayerNorm kernels (odam_amd/csrc/detr_kernels.hip) one launch at a time, through
odam_op_attention_ex / odam_op_add_layernorm_ex, at the detector's and the associator's layouts:

  * against float64 on the exact input values (bf16: the bf16-rounded values), with bounds derived from the arithmetic;
  * in bf16, against the rounding points of the bf16-faithful oracle (oracle/detr_oracle.py), on random tensors and on
    every attention / LayerNorm call of a traced config-4 forward (teacher forcing);
  * at forward level: the masked path with an all-false mask equals the unmasked one bit for bit, and a frame's outputs do
    not depend on the other frames of a mixed-size batch.

Every head-dim-32 kernel is selected in-process with the att.x3 / att.bf16_mfma switches (odam_config.h).  Bounds:
U = 2^-24 (fp32 unit roundoff); A = scale * max over the row's keys of sum_d |q_d k_d| (a logit's rounding scale); bf16 unit
roundoff is 2^-8 (8 significant bits)."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
UB = 2.0 ** -8                                       # bf16 unit roundoff: RN(x) - x <= 2^-8 |x|
SCALE = float(np.float32(0.1767766952966369))        # the kernels' q scale, sqrt(1/32) in float32
SENTINEL = -448.0                                    # exact in fp32 and bf16, far outside any output here

# |O - O64| <= C U (1 + A) max|V| per row and head (fp32 arithmetic).  C from an MI355X run (test_measured.json, keys
# attention.<kernel>.c), about 2x the largest value measured: x3 0.61 unmasked / 1.27 masked, fp32 instruction 0.92 / 2.23, head dim
# 64 2.04.  Dropping one of x3's six split products (kl qh) gives 32.8.
C_X3 = 2.5
C_F32 = 4.5
C_D64 = 4.0
# attention_bf16_kernel<32> vs the bf16-faithful oracle: share of the outputs that differ (one-ulp ties), per logit regime, about 2x
# the measured share (attention.bf16.oracle_tie_share.*): randn 6.0e-4, near one-hot 1.2e-4, duplicated keys 6.4e-5, +60 offset
# 0.059 (logits of ~340 / sqrt(32): their fp32 summation noise moves P across bf16 rounding boundaries).  A kernel whose P is not
# rounded to bf16 (the fp32-instruction kernel on bf16 storage) differs in 0.27-0.40 of the outputs, 0.061 near one-hot.
TIE_SHARE_ATT = {"randn": 1.2e-3, "sharp": 2.5e-4, "dup": 1.5e-4, "offset": 0.12}
TIE_SHARE_TF = 1e-3          # the 18 traced attention calls: measured 4.7e-4 (6.6e-4 against the oracle without the fma exponent)
# LayerNorm fp32: |y - y64| <= C_LN U ((1 + |mean| / std) |gamma| + |beta|); measured 9.15 (randn rows), 2.02 (mean 30, std 0.5).
# bf16 vs the oracle: share of one-ulp ties measured 7.8e-4 (random rows), 1.2e-4 (traced).
C_LN = 18.0
TIE_SHARE_LN = 2e-3


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t, off=0):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


@contextlib.contextmanager
def _cfg(key, value):
    from odam_amd import _lib
    old = _lib.get_config(key)
    _lib.set_config(key, value)
    try:
        yield
    finally:
        _lib.set_config(key, old)


def _rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _ulps(a, b):
    """bf16 tensors -> |distance in ulps| (+0 and -0 equal)"""
    def o(t):
        t = t.view(torch.int16).to(torch.int32)
        mag = t & 0x7fff
        return torch.where(t < 0, -mag, mag)
    return (o(a) - o(b)).abs()


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _qkv(B, Lq, Lk, regime, seed, E=256, hd=32, scale=SCALE):
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(B, Lq, E, generator=g), torch.randn(B, Lk, E, generator=g), torch.randn(B, Lk, E, generator=g)
    if regime == "sharp":          # logit std ~ 16: near one-hot rows
        q, k = q * 4, k * 4
    elif regime == "offset":       # a shared channel per head adds ~ +60 to every logit of every row (running-max rescale)
        a = (60.0 / scale) ** 0.5
        q[..., ::hd] = a
        k[..., ::hd] = a
    elif regime == "dup":          # duplicated keys: exact ties in the logits
        k = k[:, torch.arange(Lk) % 5]
    return q, k, v


def _ref64(q, k, v, H, scale, mask=None):
    """float64 attention on the given values -> O64 [B, Lq, E], A [B, Lq, H], max|V| [B, H] over the unmasked keys"""
    B, Lq, E = q.shape
    Lk, D = k.shape[1], E // H
    qh = q.double().reshape(B, Lq, H, D).transpose(1, 2)
    kh = k.double().reshape(B, Lk, H, D).transpose(1, 2)
    vh = v.double().reshape(B, Lk, H, D).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale
    a = (qh.abs() @ kh.abs().transpose(-1, -2)) * scale
    if mask is not None:
        mk = mask.bool()[:, None, None, :]
        s = s.masked_fill(mk, -float("inf"))
        a = a.masked_fill(mk, 0.0)
        vh = vh.masked_fill(mask.bool()[:, None, :, None], 0.0)
    o = torch.softmax(s, -1) @ vh
    return o.transpose(1, 2).reshape(B, Lq, E), a.amax(-1).transpose(1, 2), vh.abs().amax((-1, -2))


# ---- launches at the detector's layouts -------------------------------------------------------------------------------
def _attention(q, k, v, layout, dtype, mask=None, ldo=256):
    """q [B, Lq, 256], k / v [B, Lk, 256] placed as the detector places them, H = 8, head dim 32.
    self:  Q at column 0 and K at column 256 of [rows, 512] (one buffer when Lq == Lk, as the forward has it), V [rows, 256];
    cross: Q [rows, 256], K and V at column 1280 of [rows, 1536] (the last decoder layer's slice of the cross K / V).
    Columns the kernel must not read hold NaN.  O: [B Lq + 5, ldo] filled with SENTINEL; returns O[:B Lq, :256] as float32
    [B, Lq, 256] after checking that nothing else was written."""
    from odam_amd import _lib
    B, Lq, E = q.shape
    Lk = k.shape[1]
    tdt = torch.bfloat16 if dtype else torch.float32

    def buf(rows, width, parts):
        t = torch.full((rows, width), float("nan"))
        for col, x in parts:
            t[:, col:col + E] = x.reshape(rows, E)
        return t.to(tdt).to(DEV)
    if layout == "self":
        if Lq == Lk:
            dq = dk = buf(B * Lq, 512, [(0, q), (256, k)])
        else:
            dq, dk = buf(B * Lq, 512, [(0, q)]), buf(B * Lk, 512, [(256, k)])
        dv = buf(B * Lk, 256, [(0, v)])
        args = (_p(dq), 512, _p(dk, 256), 512, _p(dv), 256)
    else:
        dq, dk, dv = buf(B * Lq, 256, [(0, q)]), buf(B * Lk, 1536, [(1280, k)]), buf(B * Lk, 1536, [(1280, v)])
        args = (_p(dq), 256, _p(dk, 1280), 1536, _p(dv, 1280), 1536)
    do = torch.full((B * Lq + 5, ldo), SENTINEL, dtype=tdt, device=DEV)
    dm = mask.to(torch.uint8).contiguous().to(DEV) if mask is not None else None
    _lib.check(_lib.lib().odam_op_attention_ex(*args, _p(do), ldo, B, 8, Lq, Lk, 32, dtype, _p(dm), _st()), "attention_ex")
    torch.cuda.synchronize()
    o = do.cpu().float()
    rest = o.clone()
    rest[:B * Lq, :E] = SENTINEL
    assert torch.all(rest == SENTINEL), "attention wrote outside rows < B Lq x the head columns"
    return o[:B * Lq, :E].reshape(B, Lq, E), do[:B * Lq, :E].cpu().reshape(B, Lq, E)


FP32_KERNELS = (("x3", ("att.x3", 1)), ("f32", ("att.x3", 0)))
BF16_KERNELS = (("bf16", ("att.bf16_mfma", 1)), ("bf16_f32", ("att.bf16_mfma", 0)))

#         B   Lq   Lk  layout   regime    ldo
CASES = [(1, 1, 1, "self", "randn", 256),
         (3, 100, 31, "cross", "randn", 256),
         (1, 127, 32, "self", "sharp", 256),
         (3, 128, 33, "cross", "offset", 256),
         (1, 129, 63, "self", "dup", 256),
         (3, 850, 64, "cross", "randn", 256),
         (1, 100, 65, "cross", "sharp", 384),
         (3, 1, 127, "self", "offset", 256),
         (1, 850, 129, "cross", "dup", 256),
         (3, 129, 850, "cross", "sharp", 256),
         (1, 850, 850, "self", "offset", 256),
         (3, 100, 850, "cross", "randn", 384),
         (3, 850, 850, "self", "randn", 256),
         (1, 100, 100, "self", "sharp", 256)]


def _ids(c):
    return "B%d-Lq%d-Lk%d-%s-%s-ldo%d" % c


def _f32_ratio(got, o64, A, vmax, H=8):
    B, Lq, E = got.shape
    err = (got.double() - o64).abs().reshape(B, Lq, H, E // H).amax(-1)          # [B, Lq, H]
    return (err / (U * (1.0 + A) * vmax[:, None, :])).max().item()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_fp32_vs_float64(case, measured):
    """x3 (three-way bf16 split, the default) and the fp32-instruction kernel: |O - O64| <= C U (1 + A) max|V|.  For x3 the
    bound is tight enough to see one dropped split product (an error of ~2^-16 of the logit scale)."""
    B, Lq, Lk, layout, regime, ldo = case
    q, k, v = _qkv(B, Lq, Lk, regime, seed=Lq * 1000 + Lk)
    o64, A, vmax = _ref64(q, k, v, 8, SCALE)
    ratios = {}
    for name, (key, val) in FP32_KERNELS:
        with _cfg(key, val):
            got, _ = _attention(q, k, v, layout, 0, ldo=ldo)
        ratios[name] = _f32_ratio(got, o64, A, vmax)
        measured(f"attention.{name}.c", ratios[name])
        measured(f"attention.{name}.{regime}.c", ratios[name])
    assert ratios["x3"] <= C_X3, ratios
    assert ratios["f32"] <= C_F32, ratios


def _oracle_diff(got_b, want, v, H=8):
    """bf16 outputs against the oracle's -> (share of elements that differ, max ulps, worst |d| / (2^-7 max|V| of the head) over
    the elements off by more than one ulp).  The oracle's fp32 logits differ from the kernel's in summation order, so now and then
    a probability rounds to the neighbouring bf16 value (one ulp <= 2^-7 of p): O then moves by <= 2^-7 (p / l) max|V|."""
    d = _ulps(got_b, want.to(torch.bfloat16))
    B, Lk, E = v.shape
    vmax = v.abs().amax(1).reshape(B, H, E // H).amax(-1).repeat_interleave(E // H, -1)[:, None, :]
    over = d > 1
    excess = ((got_b.float() - want.float()).abs() / (2.0 ** -7 * vmax))[over].max().item() if over.any() else 0.0
    return (d != 0).float().mean().item(), int(d.max().item()), excess


def _bf16_vs_oracle(got, q, k, v, mask, tag, regime, measured):
    """attention_bf16_kernel<32>'s bits against oracle _attention_b on the same (bf16) inputs: elements off by one ulp no more than
    the measured share of the regime, larger differences no more than one probability rounding flip explains.  Recorded beside
    it: the same comparison for the oracle without the fma exponent, and for the fp32-instruction kernel on bf16 storage, whose P
    is not rounded (what the share cap tells apart)."""
    import detr_oracle as O
    want = O._attention_b(q, k, v, 8, key_mask=mask)
    share, ulp, excess = _oracle_diff(got["bf16"], want, v)
    measured(f"attention.bf16.oracle_tie_share.{regime}", share)
    measured("attention.bf16.oracle_max_ulp", ulp)
    measured("attention.bf16.oracle_excess_over_p_flip", excess)
    measured(f"attention.bf16.oracle_tie_share_nofma.{regime}",
             _oracle_diff(got["bf16"], O._attention_b(q, k, v, 8, key_mask=mask, fma=False), v)[0])
    if "bf16_f32" in got:
        measured(f"attention.bf16_f32.oracle_tie_share.{regime}", _oracle_diff(got["bf16_f32"], want, v)[0])
    assert share <= TIE_SHARE_ATT[regime] and excess <= 1.0, (tag, share, ulp, excess)


def _bf16_checks(q, k, v, layout, mask, ldo, tag, regime, measured, kernels=BF16_KERNELS):
    """both bf16 kernels on bf16-rounded inputs against float64; the bf16 matrix-instruction kernel also against the oracle.
    The bounds are derived, not fitted: measured err / bound 0.46 (bf16 instruction) and 0.99 (fp32 instruction on bf16 storage,
    where the output rounding alone reaches its worst case, half an ulp at the bottom of a binade)."""
    q, k, v = _rb(q), _rb(k), _rb(v)
    o64, A, vmax = _ref64(q, k, v, 8, SCALE, mask)
    B, Lq, E = q.shape
    fp = (U * (1.0 + A) * vmax[:, None, :]).repeat_interleave(32, -1)             # [B, Lq, E]
    out = {}
    for name, (key, val) in kernels:
        with _cfg(key, val):
            got, got_b = _attention(q, k, v, layout, 1, mask=mask, ldo=ldo)
        err = (got.double() - o64).abs()
        if name == "bf16":      # P rounded to bf16 (<= 2^-8 of each p: <= 2^-8 max|V| in O), O rounded (<= 2^-8 |O|), fp32 logits
            bound = UB * vmax[:, None, :].repeat_interleave(32, -1) + UB * o64.abs() + C_F32 * fp
        else:                   # P in fp32: the fp32 kernel's error, then O rounded
            bound = UB * o64.abs() + (1 + UB) * C_F32 * fp
        r = (err / bound).max().item()
        measured(f"attention.{name}.bound_ratio", r)
        out[name] = (r, got_b)
    for name, (r, _) in out.items():
        assert r <= 1.0, (tag, name, r)
    if "bf16" in out:
        _bf16_vs_oracle({n: o[1] for n, o in out.items()}, q, k, v, mask, tag, regime, measured)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_bf16_vs_float64_and_oracle(case, measured):
    B, Lq, Lk, layout, regime, ldo = case
    q, k, v = _qkv(B, Lq, Lk, regime, seed=Lq * 1000 + Lk + 7)
    _bf16_checks(q, k, v, layout, None, ldo, _ids(case), regime, measured)


# ---- key-padding masks ------------------------------------------------------------------------------------------------
def _nested_masks():
    """forward_nested's token masks for images of 25x34, 19x34, 25x20 and 7x5 tokens padded to 800 x 1088 pixels (a 25 x 34
    grid): the pixel mask reduced to the grid by nearest interpolation (backbone.py:79), as odam_amd/detector.py builds it"""
    sizes = [(25, 34), (19, 34), (25, 20), (7, 5)]
    m = torch.ones(len(sizes), 800, 1088, dtype=torch.bool)
    for i, (th, tw) in enumerate(sizes):
        m[i, :th * 32, :tw * 32] = False
    return F.interpolate(m[None].float(), size=(25, 34)).to(torch.bool)[0].reshape(len(sizes), 850)


def _edge_masks(Lk=850, seed=5):
    """a different mask per batch element: the whole first 64-key tile, the first 32-key tile, all but the last key (in the
    tail tile), random 50 %"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(4, Lk, dtype=torch.bool)
    m[0, :64] = True
    m[1, :32] = True
    m[2, :Lk - 1] = True
    m[3] = torch.rand(Lk, generator=g) < 0.5
    return m


MASK_CASES = [("nested_self", "self", 850, "randn"), ("nested_cross", "cross", 100, "sharp"),
              ("edges_cross", "cross", 100, "randn"), ("edges_self", "self", 850, "offset")]


@pytest.mark.parametrize("name,layout,Lq,regime", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_attention_key_mask(name, layout, Lq, regime, measured):
    """every kernel that takes a mask (x3, fp32 instruction, bf16 instruction, fp32 instruction on bf16 storage) against float64
    softmax over the unmasked keys; per-batch masks so that indexing by batch is checked"""
    mask = _nested_masks() if name.startswith("nested") else _edge_masks()
    B, Lk = mask.shape
    assert not mask.all(-1).any()
    q, k, v = _qkv(B, Lq, Lk, regime, seed=len(name) * 31 + Lq)
    if layout == "self":
        k = q.clone() if Lq == Lk and regime == "randn" else k     # q = k as the encoder has it (x + pos for both)
    o64, A, vmax = _ref64(q, k, v, 8, SCALE, mask)
    for kname, (key, val) in FP32_KERNELS:
        with _cfg(key, val):
            got, _ = _attention(q, k, v, layout, 0, mask=mask)
        r = _f32_ratio(got, o64, A, vmax)
        measured(f"attention.{kname}.masked.c", r)
        assert r <= (C_X3 if kname == "x3" else C_F32), (name, kname, r)
    _bf16_checks(q, k, v, layout, mask, 256, name, regime, measured)


# ---- head dim 64 (the associator's GNN) ------------------------------------------------------------------------------
D64_CASES = [(1, 1, 1, 256), (5, 7, 7, 512), (1, 31, 33, 256), (5, 32, 32, 256), (1, 33, 64, 512), (5, 64, 100, 256),
             (1, 100, 7, 512), (5, 100, 100, 512), (1, 7, 31, 256)]


@pytest.mark.parametrize("B,Lq,Lk,ldo", D64_CASES)
def test_attention_d64_vs_float64(B, Lq, Lk, ldo, measured):
    """attention_kernel<float, 64>, H = 4, scale 1/8, as assoc.hip calls it: rows q | k | v of 768 floats (one buffer when the
    queries attend to their own rows), output at pitch 256 or into columns 256 .. 511 of 512-float rows (the merged form)"""
    from odam_amd import _lib
    E = 256
    regime = ("randn", "sharp", "offset")[(Lq + Lk) % 3]
    q, k, v = _qkv(B, Lq, Lk, regime, seed=B * 100 + Lq * 7 + Lk, hd=64, scale=0.125)
    o64, A, vmax = _ref64(q, k, v, 4, 0.125)
    if Lq == Lk:
        rows = torch.cat([q, k, v], -1).reshape(B * Lq, 768)
        dq = dkv = rows.to(DEV)
    else:
        dq = torch.cat([q, torch.full((B, Lq, 512), float("nan"))], -1).reshape(B * Lq, 768).to(DEV)
        dkv = torch.cat([torch.full((B, Lk, 256), float("nan")), k, v], -1).reshape(B * Lk, 768).to(DEV)
    off = 256 if ldo == 512 else 0
    do = torch.full((B * Lq + 3, ldo), SENTINEL, device=DEV)
    _lib.check(_lib.lib().odam_op_attention_ex(_p(dq), 768, _p(dkv, 256), 768, _p(dkv, 512), 768, _p(do, off), ldo,
                                               B, 4, Lq, Lk, 64, 0, None, _st()), "attention_ex d64")
    torch.cuda.synchronize()
    o = do.cpu()
    got = o[:B * Lq, off:off + E].clone().reshape(B, Lq, E)
    o[:B * Lq, off:off + E] = SENTINEL
    assert torch.all(o == SENTINEL)
    r = _f32_ratio(got, o64, A, vmax, H=4)
    measured("attention.d64.c", r)
    assert r <= C_D64, r


def test_attention_ex_argument_checks():
    from odam_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, 512, device=DEV)
    m = torch.zeros(1, 8, dtype=torch.uint8, device=DEV)
    call = lambda ld, hd, dt, mk=None, Q=t: L.odam_op_attention_ex(_p(Q), ld, _p(t), ld, _p(t), ld, _p(t), ld, 1, 4, 8, 8, hd,
                                                                   dt, _p(mk), _st())
    assert call(256, 32, 0) == 0 and call(256, 64, 0) == 0 and call(256, 32, 1, m) == 0
    assert call(256, 48, 0) == 1 and call(256, 64, 1) == 1 and call(256, 64, 0, m) == 1 and call(256, 32, 2) == 1
    assert call(260, 32, 1) == 1 and call(258, 32, 0) == 1 and call(256, 32, 0, Q=None) == 1
    assert L.odam_op_add_layernorm_ex(_p(t), None, _p(t), _p(t), _p(t), None, 1, _p(t), 4, 0, _st()) == 1    # y_pos without pos
    assert L.odam_op_add_layernorm_ex(_p(t), None, _p(t), _p(t), _p(t), None, 1, None, 4, 3, _st()) == 1
    torch.cuda.synchronize()


# ---- LayerNorm --------------------------------------------------------------------------------------------------------
def _ln_rows(M, seed):
    """rows cycling through randn, mean 30 / std 0.5, and constant (the output must be beta)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 256, generator=g)
    r = torch.randn(M, 256, generator=g)
    kind = torch.arange(M) % 3
    x[kind == 1] = 30.0 + 0.5 * x[kind == 1]
    r[kind == 1] = 0.5 * r[kind == 1]
    const = torch.randn(M, 1, generator=g) * 10
    x[kind == 2] = const[kind == 2].expand(-1, 256)
    r[kind == 2] = 0.25
    gamma, beta = torch.randn(256, generator=g), torch.randn(256, generator=g)
    pos = torch.randn(max(M, 850), 256, generator=g)
    return x, r, gamma, beta, pos, kind


def _layernorm(x, r, gamma, beta, pos, L, M, dtype):
    from odam_amd import _lib
    tdt = torch.bfloat16 if dtype else torch.float32
    dx = x.to(tdt).to(DEV)
    dr = r.to(tdt).to(DEV) if r is not None else None
    dy = torch.full((M + 5, 256), SENTINEL, dtype=tdt, device=DEV)
    dyp = torch.full((M + 5, 256), SENTINEL, dtype=tdt, device=DEV) if L else None
    dpos = pos[:L].contiguous().to(DEV) if L else None
    dg, db = gamma.to(DEV), beta.to(DEV)
    _lib.check(_lib.lib().odam_op_add_layernorm_ex(_p(dx), _p(dr), _p(dg), _p(db), _p(dy), _p(dpos),
                                                   L or 1, _p(dyp), M, dtype, _st()), "add_layernorm_ex")
    torch.cuda.synchronize()
    y, yp = dy.cpu(), (dyp.cpu() if L else None)
    assert torch.all(y[M:].float() == SENTINEL)
    if L:
        assert torch.all(yp[M:].float() == SENTINEL)
    return y[:M], (yp[:M] if L else None)


def _ln_ref64(v, gamma, beta):
    """float64 LayerNorm of the rows v [M, 256] (eps 1e-5, biased variance) -> y64 and the unit of the fp32 bound,
    U ((1 + |mean| / std) |gamma| + |beta|) per element: a value of size |mean| + |x - mean| rounded in fp32 moves x - mean by
    U (|mean| + |x - mean|), i.e. the normalised value by U (|mean| / std + |x_hat|)"""
    v = v.double()
    mean = v.mean(-1, keepdim=True)
    var = (v - mean).pow(2).mean(-1, keepdim=True)
    y64 = (v - mean) / (var + 1e-5).sqrt() * gamma.double() + beta.double()
    unit = U * ((1 + mean.abs() / var.sqrt().clamp_min(1e-30)) * gamma.double().abs() + beta.double().abs())
    return y64, unit


def _ln_bf16_diff(got, want, unit):
    """bf16 LayerNorm outputs against the oracle's -> (share that differs, max ulps, worst excess): two fp32 evaluations within
    C_LN unit of the exact value may round apart by more than one ulp only where they differ by <= 2 C_LN unit + one ulp"""
    d = _ulps(got, want)
    over = d > 1
    slack = 2 * C_LN * unit + 2.0 ** -7 * want.double().abs()
    excess = ((got.double() - want.double()).abs() / slack)[over].max().item() if over.any() else 0.0
    return (d != 0).float().mean().item(), int(d.max().item()), excess


#           M    residual  L (None: no y_pos)
LN_CASES = [(1, False, 1), (3, True, None), (4, False, None), (5, True, 5), (777, True, None), (1700, False, 850),
            (1700, True, 1700)]


@pytest.mark.parametrize("M,res,L", LN_CASES)
def test_layernorm_fp32_vs_float64(M, res, L, measured):
    x, r, gamma, beta, pos, kind = _ln_rows(M, seed=M + 3 * res)
    if not res:
        r = None
    y, yp = _layernorm(x, r, gamma, beta, pos, L, M, 0)
    y64, unit = _ln_ref64(x.double() + (r.double() if r is not None else 0), gamma, beta)      # the exact sum
    const = kind == 2
    assert torch.equal(y[const], beta.expand(int(const.sum()), 256)), "constant rows must give beta exactly"
    live = ~const
    ratio = ((y.double() - y64).abs()[live] / unit[live]).max().item() if live.any() else 0.0
    measured("layernorm.f32.c", ratio)
    for kk, nm in ((0, "randn"), (1, "mean30")):
        sel = kind == kk
        if sel.any():
            measured(f"layernorm.f32.{nm}.c", ((y.double() - y64).abs()[sel] / unit[sel]).max().item())
    assert ratio <= C_LN, ratio
    if L:      # y_pos = fp32(y + pos[row % L]) of the kernel's own y: exact
        want = y + pos[torch.arange(M) % L]
        assert torch.equal(yp, want)


@pytest.mark.parametrize("M,res,L", LN_CASES)
def test_layernorm_bf16_vs_oracle(M, res, L, measured):
    """bf16 storage: y and y + pos rounded from the fp32 values, as oracle _ln_b rounds them; one-ulp ties (share capped), more
    only near a cancellation (see _ln_bf16_diff)"""
    x, r, gamma, beta, pos, kind = _ln_rows(M, seed=M + 3 * res + 1)
    x = _rb(x)
    r = _rb(r) if res else None
    y, yp = _layernorm(x, r, gamma, beta, pos, L, M, 1)
    yf = F.layer_norm(x + r if r is not None else x, (256,), gamma, beta, 1e-5)
    const = kind == 2
    assert torch.equal(y[const].float(), _rb(beta).expand(int(const.sum()), 256))
    pairs = [("y", y, yf.to(torch.bfloat16))]
    if L:
        pairs.append(("y_pos", yp, (yf + pos[torch.arange(M) % L]).to(torch.bfloat16)))
    _, unit = _ln_ref64(x.double() + (r.double() if r is not None else 0), gamma, beta)
    for nm, got, want in pairs:
        share, ulp, excess = _ln_bf16_diff(got, want, unit)
        measured(f"layernorm.bf16.{nm}.tie_share", share)
        measured(f"layernorm.bf16.{nm}.max_ulp", ulp)
        measured("layernorm.bf16.excess", excess)
        assert share <= TIE_SHARE_LN and excess <= 1.0, (nm, share, ulp, excess)


# ---- teacher forcing on a traced config-4 forward ---------------------------------------------------------------------
def test_bf16_attention_and_layernorm_teacher_forced(measured):
    """R50 scene weights at 1 x 3 x 640 x 800 (20 x 25 = 500 tokens: eight key tiles, the last one ragged; 100 x 500
    cross-attention): every attention call (18) and every LayerNorm (31) of detr_forward_bf16, each on its own traced inputs at
    the detector's pitches, must return the oracle's bf16 bits up to one-ulp ties (attention: beyond one ulp only what a
    probability rounding flip explains, see _oracle_diff)"""
    import detr_oracle as O
    from odam_amd import _lib, weights
    sd = weights.make_state_dict(seed=0, scene=True)
    torch.manual_seed(11)
    img = torch.randn(1, 3, 640, 800)
    O.OPS_TRACE = []
    try:
        O.detr_forward_bf16(sd, img)
        trace = O.OPS_TRACE
    finally:
        O.OPS_TRACE = None
    att = [t for t in trace if t["kind"] == "attention"]
    lns = [t for t in trace if t["kind"] == "layernorm"]
    assert len(att) == 18 and len(lns) == 31
    worst = {"att": 0.0, "att_nofma": 0.0, "ln": 0.0}
    bad = []
    n_cross = 0
    with _cfg("att.bf16_mfma", 1):
        for t in att:
            q, k, v = t["q"], t["k"], t["v"]
            cross = q.shape[1] != k.shape[1]
            if cross:      # decoder layer i reads columns 256 i of the [L, 1536] cross K / V
                layout_off, n_cross = 256 * n_cross, n_cross + 1
                B, Lq, E = q.shape
                Lk = k.shape[1]
                dq = q.reshape(B * Lq, E).to(torch.bfloat16).to(DEV)
                dk = torch.full((B * Lk, 1536), float("nan")); dk[:, layout_off:layout_off + E] = k.reshape(-1, E)
                dv = torch.full((B * Lk, 1536), float("nan")); dv[:, layout_off:layout_off + E] = v.reshape(-1, E)
                dk, dv = dk.to(torch.bfloat16).to(DEV), dv.to(torch.bfloat16).to(DEV)
                do = torch.empty(B * Lq, E, dtype=torch.bfloat16, device=DEV)
                _lib.check(_lib.lib().odam_op_attention_ex(_p(dq), 256, _p(dk, layout_off), 1536, _p(dv, layout_off), 1536,
                                                           _p(do), 256, B, 8, Lq, Lk, 32, 1, None, _st()), "attention_ex")
                torch.cuda.synchronize()
                got = do.cpu().reshape(B, Lq, E)
            else:
                _, got = _attention(q, k, v, "self", 1)
            share, ulp, excess = _oracle_diff(got, t["y"], v)
            worst["att"] = max(worst["att"], share)
            worst["att_nofma"] = max(worst["att_nofma"], _oracle_diff(got, O._attention_b(q, k, v, 8, fma=False), v)[0])
            measured("attention.bf16.teacher_forced.max_ulp", ulp)
            measured("attention.bf16.teacher_forced.excess_over_p_flip", excess)
            if share > TIE_SHARE_TF or excess > 1.0:
                bad.append(("attention", tuple(q.shape), tuple(k.shape), share, ulp, excess))
    assert n_cross == 6
    for t in lns:
        x, pos = t["x"], t["pos"]
        B, Lr, E = x.shape
        L = pos.shape[1] if pos is not None else None
        y, yp = _layernorm(x.reshape(B * Lr, E), None, t["gamma"], t["beta"], pos[0] if pos is not None else None, L, B * Lr, 1)
        pairs = [(y, t["y"])] + ([(yp, t["y_pos"])] if pos is not None else [])
        _, unit = _ln_ref64(x.reshape(B * Lr, E), t["gamma"], t["beta"])
        for got, want in pairs:
            share, ulp, excess = _ln_bf16_diff(got, want.reshape(B * Lr, E).to(torch.bfloat16), unit)
            worst["ln"] = max(worst["ln"], share)
            measured("layernorm.bf16.teacher_forced.max_ulp", ulp)
            measured("layernorm.bf16.teacher_forced.excess", excess)
            if share > TIE_SHARE_LN or excess > 1.0:
                bad.append(("layernorm", tuple(x.shape), share, ulp, excess))
    measured("attention.bf16.teacher_forced.tie_share", worst["att"])
    measured("attention.bf16.teacher_forced.tie_share_nofma", worst["att_nofma"])
    measured("layernorm.bf16.teacher_forced.tie_share", worst["ln"])
    assert not bad, bad


# ---- forward-level identities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_nested_identities(dtype):
    """(1) forward_nested on equal-size images (an all-false mask, per-image position tables) equals the plain batched forward
    bit for bit; (2) in [A, X] and [A, Y] -- A the largest image, X and Y of other sizes and content -- A's outputs are
    bit-identical: the mask and the per-image tables of one frame do not reach the other (for bf16 the first mixed-size run)."""
    from odam_amd import detector, weights
    det = detector.Detector(max_batch=2, device=DEV, dtype=dtype, n_streams=1)
    det.load_state_dict(weights.make_state_dict(seed=0, scene=True))
    try:
        torch.manual_seed(21)
        imgs = torch.randn(2, 3, 160, 224)
        keys = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth", "pred_obj_features")
        plain = det(imgs.to(DEV))
        nested = det.forward_nested([imgs[0], imgs[1]])
        for k in keys:
            assert torch.equal(plain[k], nested[k]), k
        A, X, Y = imgs[0], torch.randn(3, 96, 224), torch.randn(3, 160, 128)
        ax, ay = det.forward_nested([A, X]), det.forward_nested([A, Y])
        for k in keys:
            assert torch.equal(ax[k][0], ay[k][0]), k
        assert not torch.equal(ax["pred_logits"][1], ay["pred_logits"][1])
        assert torch.isfinite(ax["pred_logits"]).all() and torch.isfinite(ay["pred_logits"]).all()
    finally:
        det.close()
