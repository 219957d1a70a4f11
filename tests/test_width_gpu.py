"""Transformer widths beyond 256 / 8 heads on the device: the head-dim-64 attention kernels and the any-C LayerNorm one launch at
a time (odam_op_attention_hd / odam_op_add_layernorm_c) against float64 and the bf16-faithful restatement, and whole forwards at
other (hidden_dim, nheads) pairs against tests/width_ref.py.  Error models and bounds are those of tests/test_attention_gpu.py
and tests/test_backbones_gpu.py; every ratio is recorded with `measured`."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import width_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
UB = 2.0 ** -8
SENTINEL = -448.0
K = np.array([[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]])
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")

# |O - O64| <= C U (1 + A) max|V| per row and head (tests/test_attention_gpu.py's model), head dim 64.  C about 2x the largest
# value an MI355X run measured (attention_d64.<kernel>.c): x3 0.75 (0.48 masked), fp32 instruction 0.90 (0.80 masked)
C_X3_64 = 1.5
C_F32_64 = 2.0
# the fp32-logit term of the bf16 bounds (tests/test_attention_gpu.py::_bf16_checks, there C_F32 = 4.5): measured bound ratios 0.42
# (bf16 instruction) and 0.99 (fp32 instruction on bf16 storage, where the output rounding reaches its worst case)
C_BF16_LOGIT = 6.0
# attention_bf16_kernel<64> against width_ref.attention_b: share of one-ulp ties per logit regime, about 2x the measured share
# (randn 8.7e-4, sharp 2.0e-5, dup 5.9e-5, offset 0.058)
TIE_SHARE_64 = {"randn": 2e-3, "sharp": 2.5e-4, "dup": 1.5e-4, "offset": 0.12}
C_LN = 18.0                  # as tests/test_attention_gpu.py; measured 3.4 (C = 128) .. 11.5 (C = 384)
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
    def o(t):
        t = t.view(torch.int16).to(torch.int32)
        mag = t & 0x7fff
        return torch.where(t < 0, -mag, mag)
    return (o(a) - o(b)).abs()


# ---- attention at head dim 64 ----------------------------------------------------------------------------------------
def _qkv(B, Lq, Lk, E, regime, seed, hd=64):
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(B, Lq, E, generator=g), torch.randn(B, Lk, E, generator=g), torch.randn(B, Lk, E, generator=g)
    if regime == "sharp":
        q, k = q * 4, k * 4
    elif regime == "offset":       # ~ +60 on every logit (running-max rescale)
        a = (60.0 / float(WR.head_scale(hd))) ** 0.5
        q[..., ::hd] = a
        k[..., ::hd] = a
    elif regime == "dup":
        k = k[:, torch.arange(Lk) % 5]
    return q, k, v


def _mask(B, Lk, seed):
    """per batch element: the first 64-key tile (when there is a second), the first 32 keys, all but the last key, random 50 %"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, Lk, dtype=torch.bool)
    for b in range(B):
        kind = b % 4
        if kind == 0 and Lk > 64:
            m[b, :64] = True
        elif kind == 1 and Lk > 32:
            m[b, :32] = True
        elif kind == 2:
            m[b, :Lk - 1] = True
        else:
            m[b] = torch.rand(Lk, generator=g) < 0.5
            m[b, Lk - 1] = False
    return m


def _ref64(q, k, v, H, scale, mask=None):
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


def _attention(q, k, v, layout, dtype, H, hd, mask=None, ldo=None, entry="hd"):
    """q [B, Lq, E], k / v [B, Lk, E] placed as the detector places them at width E:
    self:  Q at column 0 and K at column E of [rows, 2E] (one buffer when Lq == Lk), V [rows, E];
    cross: Q [rows, E], K and V at column 5E of [rows, 6E] (the last decoder layer's slice of the stacked cross K / V).
    Columns the kernel must not read hold NaN; O [B Lq + 5, ldo] holds SENTINEL outside the result."""
    from odam_amd import _lib
    B, Lq, E = q.shape
    Lk = k.shape[1]
    ldo = ldo or E
    tdt = torch.bfloat16 if dtype else torch.float32

    def buf(rows, width, parts):
        t = torch.full((rows, width), float("nan"))
        for col, x in parts:
            t[:, col:col + E] = x.reshape(rows, E)
        return t.to(tdt).to(DEV)
    if layout == "self":
        if Lq == Lk:
            dq = dk = buf(B * Lq, 2 * E, [(0, q), (E, k)])
        else:
            dq, dk = buf(B * Lq, 2 * E, [(0, q)]), buf(B * Lk, 2 * E, [(E, k)])
        dv = buf(B * Lk, E, [(0, v)])
        args = (_p(dq), 2 * E, _p(dk, E), 2 * E, _p(dv), E)
    else:
        dq, dk, dv = buf(B * Lq, E, [(0, q)]), buf(B * Lk, 6 * E, [(5 * E, k)]), buf(B * Lk, 6 * E, [(5 * E, v)])
        args = (_p(dq), E, _p(dk, 5 * E), 6 * E, _p(dv, 5 * E), 6 * E)
    do = torch.full((B * Lq + 5, ldo), SENTINEL, dtype=tdt, device=DEV)
    dm = mask.to(torch.uint8).contiguous().to(DEV) if mask is not None else None
    fn = _lib.lib().odam_op_attention_hd if entry == "hd" else _lib.lib().odam_op_attention_ex
    _lib.check(fn(*args, _p(do), ldo, B, H, Lq, Lk, hd, dtype, _p(dm), _st()), "attention_" + entry)
    torch.cuda.synchronize()
    o = do.cpu().float()
    rest = o.clone()
    rest[:B * Lq, :E] = SENTINEL
    assert torch.all(rest == SENTINEL), "attention wrote outside rows < B Lq x the head columns"
    return o[:B * Lq, :E].reshape(B, Lq, E), do[:B * Lq, :E].cpu().reshape(B, Lq, E)


#          B   Lq   Lk  layout   regime    E    masked
CASES = [(1, 1, 1, "self", "randn", 256, False),
         (3, 7, 7, "self", "sharp", 512, True),
         (2, 31, 33, "cross", "offset", 256, False),
         (1, 33, 64, "cross", "dup", 512, False),
         (4, 64, 100, "cross", "randn", 256, True),
         (1, 100, 31, "cross", "sharp", 512, True),
         (2, 100, 850, "cross", "randn", 512, True),
         (1, 850, 850, "self", "offset", 256, False),
         (2, 850, 7, "cross", "randn", 256, False),
         (4, 850, 850, "self", "randn", 512, True)]


def _ids(c):
    return "B%d-Lq%d-Lk%d-%s-%s-E%d%s" % (c[:6] + ("-masked" if c[6] else "",))


def _f32_ratio(got, o64, A, vmax, H):
    B, Lq, E = got.shape
    err = (got.double() - o64).abs().reshape(B, Lq, H, E // H).amax(-1)
    return (err / (U * (1.0 + A) * vmax[:, None, :])).max().item()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_d64_fp32_vs_float64(case, measured):
    """attention_x3_kernel<64> (att.x3 = 1, the default) and attention_kernel<float, 64> with the mask (att.x3 = 0)"""
    B, Lq, Lk, layout, regime, E, masked = case
    H = E // 64
    q, k, v = _qkv(B, Lq, Lk, E, regime, seed=Lq * 1000 + Lk + E)
    mask = _mask(B, Lk, seed=Lq + Lk) if masked else None
    o64, A, vmax = _ref64(q, k, v, H, 0.125, mask)
    ratios = {}
    for name, val in (("x3", 1), ("f32", 0)):
        with _cfg("att.x3", val):
            got, _ = _attention(q, k, v, layout, 0, H, 64, mask=mask)
        ratios[name] = _f32_ratio(got, o64, A, vmax, H)
        measured(f"attention_d64.{name}.c", ratios[name])
        measured(f"attention_d64.{name}.{regime}{'.masked' if masked else ''}.c", ratios[name])
    assert ratios["x3"] <= C_X3_64 and ratios["f32"] <= C_F32_64, ratios


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_d64_bf16_vs_float64_and_restatement(case, measured):
    """attention_bf16_kernel<64> (att.bf16_mfma = 1) and attention_kernel<bf16, 64> (= 0) on bf16 inputs against float64 with the
    bounds of tests/test_attention_gpu.py::_bf16_checks; the first also against width_ref.attention_b, one-ulp ties only"""
    B, Lq, Lk, layout, regime, E, masked = case
    H = E // 64
    q, k, v = (_rb(t) for t in _qkv(B, Lq, Lk, E, regime, seed=Lq * 1000 + Lk + E + 7))
    mask = _mask(B, Lk, seed=Lq + Lk + 1) if masked else None
    o64, A, vmax = _ref64(q, k, v, H, 0.125, mask)
    fp = (U * (1.0 + A) * vmax[:, None, :]).repeat_interleave(64, -1)
    vm = vmax[:, None, :].repeat_interleave(64, -1)
    got = {}
    for name, val in (("bf16", 1), ("bf16_f32", 0)):
        with _cfg("att.bf16_mfma", val):
            g, gb = _attention(q, k, v, layout, 1, H, 64, mask=mask)
        err = (g.double() - o64).abs()
        if name == "bf16":
            bound = UB * vm + UB * o64.abs() + C_BF16_LOGIT * fp
        else:
            bound = UB * o64.abs() + (1 + UB) * C_BF16_LOGIT * fp
        r = (err / bound).max().item()
        measured(f"attention_d64.{name}.bound_ratio", r)
        assert r <= 1.0, (name, r)
        got[name] = gb
    want = WR.attention_b(q, k, v, H, key_mask=mask)
    d = _ulps(got["bf16"], want.to(torch.bfloat16))
    share = (d != 0).float().mean().item()
    vmx = v.abs().amax(1).reshape(B, H, 64).amax(-1).repeat_interleave(64, -1)[:, None, :]
    over = d > 1
    excess = ((got["bf16"].float() - want).abs() / (2.0 ** -7 * vmx))[over].max().item() if over.any() else 0.0
    measured(f"attention_d64.bf16.restatement_tie_share.{regime}", share)
    measured("attention_d64.bf16.restatement_excess_over_p_flip", excess)
    assert share <= TIE_SHARE_64[regime] and excess <= 1.0, (share, int(d.max().item()), excess)


@pytest.mark.parametrize("dtype", [0, 1])
def test_attention_hd_at_d32_is_attention_ex(dtype):
    """the new entry at head dim 32 returns exactly the bits of odam_op_attention_ex (same launcher, same kernels)"""
    q, k, v = _qkv(2, 100, 850, 256, "randn", seed=9, hd=32)
    mask = _mask(2, 850, seed=3)
    for layout in ("self", "cross"):
        a = _attention(q, k, v, layout, dtype, 8, 32, mask=mask, entry="hd")[1]
        b = _attention(q, k, v, layout, dtype, 8, 32, mask=mask, entry="ex")[1]
        assert torch.equal(a.view(torch.int16) if dtype else a, b.view(torch.int16) if dtype else b)


def test_attention_hd_argument_checks():
    from odam_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, 1024, device=DEV)
    m = torch.zeros(1, 8, dtype=torch.uint8, device=DEV)
    call = lambda ld, hd, dt, mk=None, Q=t: L.odam_op_attention_hd(_p(Q), ld, _p(t), ld, _p(t), ld, _p(t), ld, 1, 4, 8, 8, hd,
                                                                   dt, _p(mk), _st())
    assert call(256, 32, 0) == 0 and call(256, 64, 0) == 0 and call(256, 64, 1, m) == 0 and call(256, 64, 0, m) == 0
    assert call(256, 48, 0) == 1 and call(256, 128, 0) == 1 and call(256, 16, 1) == 1 and call(256, 64, 2) == 1
    assert call(260, 64, 1) == 1 and call(258, 64, 0) == 1 and call(256, 64, 0, Q=None) == 1
    for C in (64, 96, 1088, 200):
        assert L.odam_op_add_layernorm_c(_p(t), None, _p(t), _p(t), _p(t), None, 1, None, 4, C, 0, _st()) == 1
    assert L.odam_op_add_layernorm_c(_p(t), None, _p(t), _p(t), _p(t), None, 1, _p(t), 4, 512, 0, _st()) == 1
    assert L.odam_op_add_layernorm_c(_p(t), None, _p(t), _p(t), _p(t), None, 1, None, 4, 512, 2, _st()) == 1
    torch.cuda.synchronize()


# ---- LayerNorm over C channels ---------------------------------------------------------------------------------------
def _ln_rows(M, C, seed):
    """rows cycling through randn, mean 30 / std 0.5, and constant (the output must be beta)"""
    g = torch.Generator().manual_seed(seed)
    x, r = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    kind = torch.arange(M) % 3
    x[kind == 1] = 30.0 + 0.5 * x[kind == 1]
    r[kind == 1] = 0.5 * r[kind == 1]
    const = torch.randn(M, 1, generator=g) * 10
    x[kind == 2] = const[kind == 2].expand(-1, C)
    r[kind == 2] = 0.25
    return x, r, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g), kind


def _layernorm(x, r, gamma, beta, pos, L, M, C, dtype, entry="c"):
    from odam_amd import _lib
    tdt = torch.bfloat16 if dtype else torch.float32
    dx = x.to(tdt).to(DEV)
    dr = r.to(tdt).to(DEV) if r is not None else None
    dy = torch.full((M + 5, C), SENTINEL, dtype=tdt, device=DEV)
    dyp = torch.full((M + 5, C), SENTINEL, dtype=tdt, device=DEV) if L else None
    dpos = pos[:L].contiguous().to(DEV) if L else None
    dg, db = gamma.to(DEV), beta.to(DEV)
    if entry == "c":
        rc = _lib.lib().odam_op_add_layernorm_c(_p(dx), _p(dr), _p(dg), _p(db), _p(dy), _p(dpos), L or 1, _p(dyp), M, C, dtype, _st())
    else:
        rc = _lib.lib().odam_op_add_layernorm_ex(_p(dx), _p(dr), _p(dg), _p(db), _p(dy), _p(dpos), L or 1, _p(dyp), M, dtype, _st())
    _lib.check(rc, "add_layernorm_" + entry)
    torch.cuda.synchronize()
    y, yp = dy.cpu(), (dyp.cpu() if L else None)
    assert torch.all(y[M:].float() == SENTINEL)
    if L:
        assert torch.all(yp[M:].float() == SENTINEL)
    return y[:M], (yp[:M] if L else None)


def _ln_ref64(v, gamma, beta):
    v = v.double()
    mean = v.mean(-1, keepdim=True)
    var = (v - mean).pow(2).mean(-1, keepdim=True)
    y64 = (v - mean) / (var + 1e-5).sqrt() * gamma.double() + beta.double()
    unit = U * ((1 + mean.abs() / var.sqrt().clamp_min(1e-30)) * gamma.double().abs() + beta.double().abs())
    return y64, unit


#            C    M    residual  L (None: no y_pos)
LN_CASES = [(128, 5, True, 5), (192, 777, False, None), (384, 1700, True, 850), (512, 3, False, 3), (1024, 700, True, 100),
            (512, 1700, True, None), (1024, 4, False, None)]


@pytest.mark.parametrize("C,M,res,L", LN_CASES)
def test_layernorm_c(C, M, res, L, measured):
    """fp32 against float64 (|y - y64| <= C_LN U ((1 + |mean| / std) |gamma| + |beta|), y_pos = fp32(y + pos) exactly); bf16 against
    F.layer_norm's fp32 value rounded (one-ulp ties, share capped, more only near a cancellation)"""
    x, r, gamma, beta, pos, kind = _ln_rows(M, C, seed=C + M)
    r = r if res else None
    y, yp = _layernorm(x, r, gamma, beta, pos, L, M, C, 0)
    y64, unit = _ln_ref64(x.double() + (r.double() if r is not None else 0), gamma, beta)
    const = kind == 2
    assert torch.equal(y[const], beta.expand(int(const.sum()), C)), "constant rows must give beta exactly"
    live = ~const
    ratio = ((y.double() - y64).abs()[live] / unit[live]).max().item()
    measured(f"layernorm_c.f32.C{C}.c", ratio)
    assert ratio <= C_LN, ratio
    if L:
        assert torch.equal(yp, y + pos[torch.arange(M) % L])
    xb, rb = _rb(x), (_rb(r) if r is not None else None)
    y, yp = _layernorm(xb, rb, gamma, beta, pos, L, M, C, 1)
    yf = F.layer_norm(xb + rb if rb is not None else xb, (C,), gamma, beta, 1e-5)
    _, unit = _ln_ref64(xb.double() + (rb.double() if rb is not None else 0), gamma, beta)
    pairs = [("y", y, yf.to(torch.bfloat16))] + ([("y_pos", yp, (yf + pos[torch.arange(M) % L]).to(torch.bfloat16))] if L else [])
    for nm, got, want in pairs:
        d = _ulps(got, want)
        over = d > 1
        slack = 2 * C_LN * unit + 2.0 ** -7 * want.double().abs()
        excess = ((got.double() - want.double()).abs() / slack)[over].max().item() if over.any() else 0.0
        share = (d != 0).float().mean().item()
        measured(f"layernorm_c.bf16.{nm}.tie_share", share)
        # the share cap, or two ties where the rows are too few for a share to mean anything
        assert int((d != 0).sum()) <= max(2, TIE_SHARE_LN * d.numel()) and excess <= 1.0, (nm, share, int(d.max().item()), excess)


def test_layernorm_c_at_256_is_the_default_kernel():
    x, r, gamma, beta, pos, _ = _ln_rows(300, 256, seed=1)
    for dt in (0, 1):
        a = _layernorm(x, r, gamma, beta, pos, 100, 300, 256, dt, entry="c")
        b = _layernorm(x, r, gamma, beta, pos, 100, 300, 256, dt, entry="ex")
        for u, w in zip(a, b):
            assert torch.equal(u.view(torch.int16) if dt else u, w.view(torch.int16) if dt else w)


# ---- whole forward -----------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _detector(E, H, B, backbone="resnet50", variant=False, **kw):
    from odam_amd import detector, weights
    sd = weights.make_state_dict(backbone=backbone, hidden=E, seed=0)
    if variant:
        weights.add_variant_weights(sd, hidden=E)
    det = detector.Detector(backbone=backbone, hidden_dim=E, nheads=H, max_batch=B, device=DEV, n_streams=1, **kw)
    det.load_state_dict(sd)
    return det, sd


def _check_fp32(det, sd, img, H, tag, measured, blocks=(3, 4, 6, 3), basic=False, run=True, **ref_kw):
    """tests/test_backbones_gpu.py::_check_fp32's bounds: memory tap 2e-5, outputs 2e-4, labels and post-processed classes exact"""
    import detr_oracle as O
    torch.set_num_threads(16)
    B, _, Hh, Ww = img.shape
    ref = WR.detr_forward(sd, img, blocks, nheads=H, return_taps=True, basic=basic, **ref_kw)
    out = det(img.to(DEV))
    _, mem = det.debug_taps(B, Hh, Ww)
    assert mem.shape[-1] == sd["input_proj.weight"].shape[0]
    measured(f"width.{tag}.memory_rel", _rel(mem.cpu(), ref["_memory"]))
    assert _rel(mem.cpu(), ref["_memory"]) <= 2e-5
    for k in KEYS + ("pred_obj_features",):
        d = (out[k].cpu() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item())
        measured(f"width.{tag}.{k}", d)
        assert d <= 2e-4, k
    assert torch.equal(out["pred_logits"].cpu().argmax(-1), ref["pred_logits"].argmax(-1))
    pp = det.postprocess(out, (640, 480), 0.6, K)
    pref = O.postprocess(ref, (640, 480), 0.6, K)
    for b in range(B):
        assert np.array_equal(pp["classes"][b], pref["classes"][b])
    return ref


@pytest.mark.parametrize("E,H", [(512, 8), (384, 12), (256, 4), (128, 4)])
def test_forward_fp32_vs_width_ref(E, H, measured):
    det, sd = _detector(E, H, 2)
    try:
        torch.manual_seed(E + H)
        _check_fp32(det, sd, torch.randn(2, 3, 256, 320), H, f"E{E}_H{H}", measured)
    finally:
        det.close()


def test_forward_512_bench_frame_both_x3_settings(measured):
    """(512, 8) at 800 x 1066 (850 tokens: 14 key tiles of 64 / 27 of 32, a ragged last one), with the split attention kernel
    (att.x3 = 1) and with the fp32 instruction (att.x3 = 0)"""
    det, sd = _detector(512, 8, 1)
    try:
        torch.manual_seed(8)
        img = torch.randn(1, 3, 800, 1066)
        ref = _check_fp32(det, sd, img, 8, "E512_H8_800x1066", measured)
        with _cfg("att.x3", 0):
            out = det(img.to(DEV))
        for k in KEYS:
            d = (out[k].cpu() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item())
            measured(f"width.E512_H8_800x1066_x3off.{k}", d)
            assert d <= 2e-4, k
        assert torch.equal(out["pred_logits"].cpu().argmax(-1), ref["pred_logits"].argmax(-1))
    finally:
        det.close()


def test_forward_512_pre_norm_learned_pos(measured):
    det, sd = _detector(512, 8, 2, variant=True, pre_norm=True, position_embedding="learned")
    try:
        torch.manual_seed(9)
        _check_fp32(det, sd, torch.randn(2, 3, 256, 320), 8, "E512_H8_prenorm_learned", measured, pre_norm=True, learned_pos=True)
    finally:
        det.close()


def test_forward_512_nested_masks():
    """(512, 8) through forward_nested with two image sizes: the key masks reach the head-dim-64 kernels.  The image that fills the
    batch maximum equals its own forward; the other one does not depend on its batch companion"""
    det, _ = _detector(512, 8, 2)
    try:
        g = torch.Generator().manual_seed(5)
        a, b, c = torch.randn(3, 200, 280, generator=g), torch.randn(3, 256, 320, generator=g), torch.randn(3, 256, 320, generator=g)
        ab, ac, alone = det.forward_nested([a, b]), det.forward_nested([a, c]), det(b[None].to(DEV))
        for k in KEYS:
            ref = alone[k][0].cpu()
            assert (ab[k][1].cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item()), k
            assert (ab[k][0].cpu() - ac[k][0].cpu()).abs().max().item() <= 2e-5 * max(1.0, ab[k][0].abs().max().item()), k
        assert torch.equal(ab["pred_logits"][1].argmax(-1), alone["pred_logits"][0].argmax(-1))
        assert torch.isfinite(ab["pred_logits"]).all()
    finally:
        det.close()


def test_forward_resnet18_384_6(measured):
    import basic_body as BB
    det, sd = _detector(384, 6, 2, backbone="resnet18")
    try:
        torch.manual_seed(18)
        _check_fp32(det, sd, torch.randn(2, 3, 256, 320), 6, "resnet18_E384_H6", measured, blocks=BB.BASIC_BLOCKS["resnet18"],
                    basic=True)
    finally:
        det.close()


def _rms(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-12)).item()


def _mx(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1.0)).item()


@pytest.mark.parametrize("E,H", [(512, 8), (384, 12)])
def test_forward_bf16_in_faithful_band(E, H, measured):
    """bf16 mode against width_ref.detr_forward_bf16 evaluated four times (as is and on inputs nudged by one bf16 ulp in 1 % of
    the pixels), the criteria of tests/test_backbones_gpu.py::test_resnet34_bf16_vs_bf16_faithful_oracle"""
    det, sd = _detector(E, H, 2, dtype="bf16")
    try:
        torch.manual_seed(3)
        torch.set_num_threads(16)
        img = torch.randn(2, 3, 192, 256)
        ref_f = WR.detr_forward(sd, img, nheads=H)
        refs = [WR.detr_forward_bf16(sd, img, nheads=H)]
        for seed in (1, 2, 3):
            nudge = torch.rand(img.shape, generator=torch.Generator().manual_seed(seed)) < 1e-2
            refs.append(WR.detr_forward_bf16(sd, torch.where(nudge, img * (1 + 2.0 ** -7), img), nheads=H))
        out = det(img.to(DEV))
        for k in KEYS:
            g = out[k].cpu()
            band_rms = max(_rms(r[k], ref_f[k]) for r in refs)
            band_mx = max(_mx(r[k], ref_f[k]) for r in refs)
            self_rms = max(_rms(r[k], refs[0][k]) for r in refs[1:])
            measured(f"width_bf16.E{E}_H{H}.{k}.gpu_vs_fp32_rms", _rms(g, ref_f[k]))
            measured(f"width_bf16.E{E}_H{H}.{k}.band_vs_fp32_rms", band_rms)
            measured(f"width_bf16.E{E}_H{H}.{k}.gpu_vs_bf16ref_rms", _rms(g, refs[0][k]))
            assert _rms(g, ref_f[k]) <= 1.3 * band_rms + 1e-4, (k, _rms(g, ref_f[k]), band_rms)
            assert _mx(g, ref_f[k]) <= 2.0 * band_mx + 1e-4, (k, _mx(g, ref_f[k]), band_mx)
            assert _mx(g, refs[0][k]) <= 2.0 * band_mx + 1e-4, (k, _mx(g, refs[0][k]), band_mx)
            assert _rms(g, refs[0][k]) <= 1.5 * self_rms + 1e-4, (k, _rms(g, refs[0][k]), self_rms)
            assert _mx(g, ref_f[k]) <= 0.1, k
        lab = out["pred_logits"].cpu().argmax(-1)
        agree = [(r["pred_logits"].argmax(-1) == refs[0]["pred_logits"].argmax(-1)).float().mean().item() for r in refs[1:]]
        assert (lab == refs[0]["pred_logits"].argmax(-1)).float().mean().item() >= min(agree) - 0.03
    finally:
        det.close()


def test_forward_mxfp8_512(measured):
    """mxfp8 at (512, 8) end to end: finite, logits within the sanity bound of tests/test_mxfp8_gpu.py against the fp32 mode"""
    torch.manual_seed(12)
    img = torch.randn(2, 3, 256, 320)
    outs = {}
    for dt in ("fp32", "mxfp8"):
        det, _ = _detector(512, 8, 2, dtype=dt)
        try:
            out = det(img.to(DEV))
            outs[dt] = {k: out[k].cpu() for k in KEYS}
        finally:
            det.close()
    for k in KEYS:
        assert torch.isfinite(outs["mxfp8"][k]).all(), k
        measured(f"width_mxfp8.E512_H8.{k}.rms_vs_fp32", _rms(outs["mxfp8"][k], outs["fp32"][k]))
    assert _rms(outs["mxfp8"]["pred_logits"], outs["fp32"]["pred_logits"]) <= 0.5
