"""CPU restatement of the torchvision BasicBlock ResNet body (resnet18 / resnet34, as src/models/backbone.py:90 builds it from
torchvision) and of the whole detector forward on top of it, in fp32 and in the bf16-faithful form -- test infrastructure for
tests/test_backbones_host.py and tests/test_backbones_gpu.py.

The Bottleneck restatement lives in oracle/detr_oracle.py (resnet_body, detr_forward, detr_forward_bf16); everything after the
body -- input_proj, the transformer, the heads, the rounding points of the bf16 mode -- is that file's, reused or restated here
unchanged."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import detr_oracle as O  # noqa: E402

BASIC_BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def basic_body(x, sd, blocks=(3, 4, 6, 3), prefix="backbone.0.body."):
    """torchvision ResNet-18/34 body: stem (7x7/2, FrozenBN, ReLU, 3x3/2 max-pool), then per block
    relu(bn2(conv2(relu(bn1(conv1(x))))) + identity), conv1 3x3 with the stage's stride, identity = bn(1x1/stride conv) where the
    stride or the width changes (torchvision BasicBlock, expansion 1)."""
    x = F.conv2d(x, sd[prefix + "conv1.weight"], None, stride=2, padding=3)
    x = F.relu(O.frozen_bn(x, sd, prefix + "bn1"))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for i in range(blocks[l]):
            p = f"{prefix}layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            out = F.relu(O.frozen_bn(F.conv2d(x, sd[p + "conv1.weight"], None, stride=stride, padding=1), sd, p + "bn1"))
            out = O.frozen_bn(F.conv2d(out, sd[p + "conv2.weight"], None, padding=1), sd, p + "bn2")
            idt = x
            if p + "downsample.0.weight" in sd:
                idt = O.frozen_bn(F.conv2d(x, sd[p + "downsample.0.weight"], None, stride=stride), sd, p + "downsample.1")
            x = F.relu(out + idt)
    return x


@torch.no_grad()
def detr_forward_basic(sd, img, blocks=(3, 4, 6, 3), nheads=8, enc_layers=6, dec_layers=6, return_taps=False):
    """O.detr_forward with the BasicBlock body: basic_body -> input_proj -> O.transformer -> O.heads, fp32."""
    feat = basic_body(img, sd, blocks)
    B, _, h, w = feat.shape
    pos = O.position_embedding(h, w, batch=B)
    src = F.conv2d(feat, sd["input_proj.weight"], sd["input_proj.bias"])
    hs, memory = O.transformer(src, pos, sd["query_embed.weight"], sd, nheads, enc_layers, dec_layers)
    out = O.heads(hs[-1], sd)
    if return_taps:
        out["_layer4"] = feat
        out["_memory"] = memory.permute(1, 0, 2)
    return out


@torch.no_grad()
def basic_body_bf16(img, sd, blocks=(3, 4, 6, 3), prefix="backbone.0.body."):
    """basic_body with bf16 storage where the library's bf16 mode stores (O._conv_b: operands and outputs rounded, fp32
    epilogue): conv1's output, the downsample's output, and conv2's output after bn2 + identity + ReLU."""
    x = O._conv_b(O._rb(img), sd, prefix + "conv1.weight", bn=prefix + "bn1", stride=2, padding=3, relu=True)
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for i in range(blocks[l]):
            p = f"{prefix}layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            t = O._conv_b(x, sd, p + "conv1.weight", bn=p + "bn1", stride=stride, padding=1, relu=True)
            idt = x
            if p + "downsample.0.weight" in sd:
                idt = O._conv_b(x, sd, p + "downsample.0.weight", bn=p + "downsample.1", stride=stride)
            x = O._conv_b(t, sd, p + "conv2.weight", bn=p + "bn2", padding=1, res=idt, relu=True)
    return x


@torch.no_grad()
def detr_forward_bf16_basic(sd, img, blocks=(3, 4, 6, 3), nheads=8, enc_layers=6, dec_layers=6):
    """O.detr_forward_bf16 with the BasicBlock body; the part after the body is O.detr_forward_bf16's, statement for statement."""
    feat = basic_body_bf16(img, sd, blocks)
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
