"""CPU restatement of the detector's mxfp8 mode (include/odam_detr.h "MXFP8", odam_amd/csrc/cg_mx8.h) -- test infrastructure
for tests/test_mxfp8_host.py and tests/test_mxfp8_gpu.py.

quantize / dequantize restate the format bit for bit (elements e4m3fn, round to nearest even, subnormals kept; one E8M0 scale per
32 values with e = the smallest integer such that amax <= 448 * 2^e, clamped to [-127, 127]).  mx_conv is the MX-faithful
convolution: dequantized operands contracted in float64, epilogue in fp32.  The bodies store what the library stores: MXFP8
where a convolution reads, bf16 for the residual stream; everything after the body is oracle/detr_oracle.py's bf16 mode, statement
for statement as tests/basic_body.py::detr_forward_bf16_basic restates it."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import detr_oracle as O  # noqa: E402


def scale_exp(ab):
    """block exponent from the bits of |amax| (uint32 array); 128 marks a non-finite block"""
    ab = ab.astype(np.int64)
    E = (ab >> 23) - 127
    e = E - 8 + ((ab & 0x7FFFFF) > 0x600000)
    e = np.clip(e, -127, 127)
    e = np.where(ab < 0x00800000, -127, e)
    return np.where(ab >= 0x7F800000, 128, e)


def e4m3_bits(v):
    """float32 array (|v| <= 448) -> e4m3fn bytes, round to nearest even, subnormals kept (cg_mx8.h e4m3)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    s = (u >> 24) & 0x80
    a = u & 0x7FFFFFFF
    sub = np.rint(np.abs(v.astype(np.float32)) * np.float32(512.0)).astype(np.int64)
    r = ((a + 0x7FFFF + ((a >> 20) & 1)) >> 20) - (120 << 3)
    out = np.where(a < 0x3C800000, sub, np.minimum(r, 0x7E))
    out = np.where(a >= 0x7F800000, 0x7F, out)
    return (s | out).astype(np.uint8)


def e4m3_value(b):
    b = b.astype(np.int64)
    ex, mn = (b >> 3) & 15, b & 7
    v = np.where(ex == 0, mn / 512.0, (8 + mn) * np.exp2(ex - 10.0))
    v = np.where((ex == 15) & (mn == 7), np.nan, v)
    return np.where(b & 0x80, -v, v)


def quantize(x):
    """x: float32 array or tensor whose element count is a multiple of 32, blocks = consecutive 32 of the flattened order ->
    (elements uint8, same shape; scales uint8, [n / 32])"""
    x = np.ascontiguousarray(x.numpy() if torch.is_tensor(x) else x, dtype=np.float32)
    blk = x.reshape(-1, 32)
    ab = (blk.view(np.uint32) & 0x7FFFFFFF).max(axis=1)
    e = scale_exp(ab)
    fin = e != 128
    scaled = np.where(fin[:, None], np.ldexp(blk, -np.where(fin, e, 0)[:, None]).astype(np.float32), blk)
    q = e4m3_bits(scaled).reshape(x.shape)
    s = np.where(fin, e + 127, 255).astype(np.uint8)
    return q, s


def dequantize(q, s):
    v = e4m3_value(q.reshape(-1, 32))
    sc = np.where(s == 255, np.nan, np.exp2(s.astype(np.float64) - 127.0))
    return (v * sc[:, None]).astype(np.float32).reshape(q.shape)


def qdq_nhwc(x):
    """NHWC float32 tensor -> its MXFP8 values (blocks of 32 channels of a pixel)"""
    q, s = quantize(x.contiguous())
    return torch.from_numpy(dequantize(q, s))


def qdq(x):
    """NCHW tensor -> its MXFP8 values, blocks along the channels of a pixel"""
    return qdq_nhwc(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).contiguous()


def pack_filter(w):
    """[Cout, Cin, KH, KW] -> MXFP8 of the packed [Cout][KH KW Cin] (k = (ky KW + kx) Cin + ci): (elements, scales, the
    dequantized filter back in [Cout, Cin, KH, KW])"""
    Co, Ci, KH, KW = w.shape
    p = w.permute(0, 2, 3, 1).reshape(Co, KH * KW * Ci).contiguous()
    q, s = quantize(p)
    d = torch.from_numpy(dequantize(q, s)).reshape(Co, KH, KW, Ci).permute(0, 3, 1, 2).contiguous()
    return q, s, d


def mx_conv(xq, wq, scale=None, bias=None, stride=1, padding=0, res=None, relu=False):
    """the MX-faithful convolution before its output rounding: operands are already MXFP8 values (NCHW / OIHW float32), the
    contraction in float64 rounded once to fp32, then the epilogue in fp32 as the kernel runs it:
    ((acc * scale) + bias) + residual, ReLU"""
    y = F.conv2d(xq.double(), wq.double(), None, stride=stride, padding=padding).float()
    if scale is not None:
        y = y * scale.reshape(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.reshape(1, -1, 1, 1)
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return y


_WCACHE = {}


def _wq(sd, key):
    k = (id(sd), key)
    if k not in _WCACHE:
        _WCACHE[k] = pack_filter(sd[key])[2]
    return _WCACHE[k]


def _c(x, sd, key, bn, stride=1, padding=0, res=None, relu=False):
    sc, bi = O._bn_fold(sd, bn)
    return mx_conv(x, _wq(sd, key), sc, bi, stride, padding, res, relu)


@torch.no_grad()
def stem(img, sd, prefix="backbone.0.body."):
    """the bf16 stem and max-pool (the library's bf16 mode), then the pooled map in both forms: (MXFP8 values, bf16 values)"""
    x = O._conv_b(O._rb(img), sd, prefix + "conv1.weight", bn=prefix + "bn1", stride=2, padding=3, relu=True)
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    return qdq(x), x


@torch.no_grad()
def bottleneck_body(img, sd, blocks=(3, 4, 6, 3), prefix="backbone.0.body.", trace=None):
    """MX-faithful Bottleneck body; returns layer4 (bf16 values, what input_proj reads).  trace (a list): one record per
    convolution -- x (MXFP8 values), key, bn, stride, padding, res, relu, y (fp32 before rounding)"""
    xq, xb = stem(img, sd, prefix)

    def conv(x, key, bn, stride=1, padding=0, res=None, relu=False):
        y = _c(x, sd, key, bn, stride, padding, res, relu)
        if trace is not None:
            trace.append(dict(x=x, key=key, bn=bn, stride=stride, padding=padding, res=res, relu=relu, y=y))
        return y
    nb = sum(blocks)
    n = 0
    for l in range(4):
        for i in range(blocks[l]):
            p = f"{prefix}layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            t = qdq(conv(xq, p + "conv1.weight", p + "bn1", relu=True))
            t = qdq(conv(t, p + "conv2.weight", p + "bn2", stride, 1, relu=True))
            idt = O._rb(conv(xq, p + "downsample.0.weight", p + "downsample.1", stride)) if i == 0 else xb
            v = conv(t, p + "conv3.weight", p + "bn3", res=idt, relu=True)
            n += 1
            xb = O._rb(v)
            xq = qdq(v) if n < nb else None
    return xb


@torch.no_grad()
def basic_body(img, sd, blocks=(3, 4, 6, 3), prefix="backbone.0.body.", trace=None):
    """MX-faithful BasicBlock body (resnet18 / resnet34); returns layer4 (bf16 values)"""
    xq, xb = stem(img, sd, prefix)

    def conv(x, key, bn, stride=1, padding=0, res=None, relu=False):
        y = _c(x, sd, key, bn, stride, padding, res, relu)
        if trace is not None:
            trace.append(dict(x=x, key=key, bn=bn, stride=stride, padding=padding, res=res, relu=relu, y=y))
        return y
    nb = sum(blocks)
    n = 0
    for l in range(4):
        for i in range(blocks[l]):
            p = f"{prefix}layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            t = qdq(conv(xq, p + "conv1.weight", p + "bn1", stride, 1, relu=True))
            idt = xb
            if p + "downsample.0.weight" in sd:
                idt = O._rb(conv(xq, p + "downsample.0.weight", p + "downsample.1", stride))
            v = conv(t, p + "conv2.weight", p + "bn2", 1, 1, res=idt, relu=True)
            n += 1
            xb = O._rb(v)
            xq = qdq(v) if n < nb else None
    return xb


@torch.no_grad()
def after_body(sd, feat, nheads=8, enc_layers=6, dec_layers=6):
    """input_proj, the transformer and the heads of the bf16 mode on the layer4 map feat [B, C4, h, w] -- O.detr_forward_bf16's
    statements, as tests/basic_body.py::detr_forward_bf16_basic has them"""
    B, _, h, w = feat.shape
    E = sd["input_proj.weight"].shape[0]
    pos = O.position_embedding(h, w, batch=1).flatten(2).permute(0, 2, 1)
    src = O._conv_b(feat, sd, "input_proj.weight", bias=sd["input_proj.bias"]).flatten(2).permute(0, 2, 1)
    srcpos = O._rb(src + pos)
    tp = "transformer."
    for i in range(enc_layers):
        p = f"{tp}encoder.layers.{i}."
        W, b = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        qk = O._lin_b(srcpos, W[:2 * E], b[:2 * E])
        v = O._lin_b(src, W[2 * E:], b[2 * E:])
        att = O._attention_b(qk[..., :E], qk[..., E:], v, nheads)
        tmp = O._lin_b(att, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], res=src)
        src, _ = O._ln_b(tmp, sd, p + "norm1")
        ffn = O._lin_b(src, sd[p + "linear1.weight"], sd[p + "linear1.bias"], relu=True)
        tmp = O._lin_b(ffn, sd[p + "linear2.weight"], sd[p + "linear2.bias"], res=src)
        src, srcpos = O._ln_b(tmp, sd, p + "norm2", pos)
    memory = src
    qpos = sd["query_embed.weight"].unsqueeze(0)
    Q = qpos.shape[1]
    tgt = torch.zeros(B, Q, E)
    tgtpos = O._rb(qpos).expand(B, Q, E)
    for i in range(dec_layers):
        p = f"{tp}decoder.layers.{i}."
        W, b = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        qk = O._lin_b(tgtpos, W[:2 * E], b[:2 * E])
        v = O._lin_b(tgt, W[2 * E:], b[2 * E:])
        att = O._attention_b(qk[..., :E], qk[..., E:], v, nheads)
        tmp = O._lin_b(att, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], res=tgt)
        tgt, tgtpos = O._ln_b(tmp, sd, p + "norm1", qpos)
        W, b = sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"]
        cq = O._lin_b(tgtpos, W[:E], b[:E])
        kc = O._lin_b(srcpos, W[E:2 * E], b[E:2 * E])
        vc = O._lin_b(memory, W[2 * E:], b[2 * E:])
        att = O._attention_b(cq, kc, vc, nheads)
        tmp = O._lin_b(att, sd[p + "multihead_attn.out_proj.weight"], sd[p + "multihead_attn.out_proj.bias"], res=tgt)
        tgt, _ = O._ln_b(tmp, sd, p + "norm2")
        ffn = O._lin_b(tgt, sd[p + "linear1.weight"], sd[p + "linear1.bias"], relu=True)
        tmp = O._lin_b(ffn, sd[p + "linear2.weight"], sd[p + "linear2.bias"], res=tgt)
        tgt, tgtpos = O._ln_b(tmp, sd, p + "norm3", qpos)
    hs, _ = O._ln_b(tgt, sd, tp + "decoder.norm")

    def mlp(p):
        h1 = O._lin_b(hs, sd[p + ".layers.0.weight"], sd[p + ".layers.0.bias"], relu=True)
        h2 = O._lin_b(h1, sd[p + ".layers.1.weight"], sd[p + ".layers.1.bias"], relu=True)
        return O._lin_b(h2, sd[p + ".layers.2.weight"], sd[p + ".layers.2.bias"], out_f32=True)
    return {
        "pred_logits": O._lin_b(hs, sd["class_embed.weight"], sd["class_embed.bias"], out_f32=True),
        "pred_boxes": mlp("bbox_embed").sigmoid(),
        "pred_angle": mlp("angle_embed"),
        "pred_offset": mlp("offset_embed"),
        "pred_size": mlp("size_embed"),
        "pred_depth": mlp("depth_embed"),
        "pred_obj_features": hs,
    }


@torch.no_grad()
def detr_forward_mxfp8(sd, img, blocks=(3, 4, 6, 3), basic=False, nheads=8, enc_layers=6, dec_layers=6):
    """the whole mxfp8-mode forward: MX-faithful body, then the bf16 mode after it"""
    feat = (basic_body if basic else bottleneck_body)(img, sd, blocks)
    return after_body(sd, feat, nheads, enc_layers, dec_layers)
