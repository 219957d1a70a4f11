"""CPU restatement of the detector forward at any transformer width (hidden_dim E, nheads, head dim E / nheads = 32 or 64), fp32
and bf16-faithful -- test infrastructure for tests/test_width_host.py and tests/test_width_gpu.py.

oracle/detr_oracle.py states the reference at E = 256 / 8 heads: its detr_forward builds the sine table with 128 features per
axis, and its bf16-faithful attention (_attention_b) folds the head-dim-32 scale into the exponent.  Those are the only width
assumptions; everything else -- the bodies, input_proj, O.transformer (nn.MultiheadAttention's functional form at any width),
the heads and the rounding points of the bf16 mode -- is that file's, reused or restated here statement for statement."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basic_body as BB  # noqa: E402
import detr_oracle as O  # noqa: E402


def head_scale(head_dim):
    """the q scale F.multi_head_attention_forward applies: float(head_dim) ** -0.5 in float64, used as float32"""
    return torch.tensor(float(head_dim) ** -0.5, dtype=torch.float32)


def position_embedding(h, w, E, batch=1):
    """PositionEmbeddingSine with num_pos_feats = E // 2 (detr.py build: N_steps = hidden_dim // 2) -> [B, E, h, w]"""
    return O.position_embedding(h, w, num_pos_feats=E // 2, batch=batch)


@torch.no_grad()
def detr_forward(sd, img, blocks=(3, 4, 6, 3), nheads=8, enc_layers=6, dec_layers=6, return_taps=False, pre_norm=False,
                 learned_pos=False, basic=False):
    """O.detr_forward at the width of `sd` (E = input_proj's output channels); basic: the BasicBlock body of tests/basic_body.py"""
    feat = BB.basic_body(img, sd, blocks) if basic else O.resnet_body(img, sd, blocks)
    B, _, h, w = feat.shape
    E = sd["input_proj.weight"].shape[0]
    pos = O.position_embedding_learned(sd, h, w, batch=B) if learned_pos else position_embedding(h, w, E, batch=B)
    src = F.conv2d(feat, sd["input_proj.weight"], sd["input_proj.bias"])
    hs, memory = O.transformer(src, pos, sd["query_embed.weight"], sd, nheads, enc_layers, dec_layers, pre_norm=pre_norm)
    out = O.heads(hs[-1], sd)
    if return_taps:
        out["_layer4"] = feat
        out["_memory"] = memory.permute(1, 0, 2)
    return out


def attention_b(q, k, v, nheads, tile=64, key_mask=None, fma=True):
    """O._attention_b with the scale of the head dim E / nheads folded into the exponent (attention_bf16_kernel<D>,
    D = 32 or 64): 64-key tiles, running max, P rounded to bf16 as the PV operand, O rounded."""
    B, Lq, E = q.shape
    Lk, D = k.shape[1], E // nheads
    qh = q.reshape(B, Lq, nheads, D).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, nheads, D).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, nheads, D).permute(0, 2, 1, 3)
    c = head_scale(D) * torch.tensor(1.44269504088896341, dtype=torch.float32)
    dead = -1e30 if D == 32 else -2.0 ** 100      # a padded key's score (attention_bf16_kernel<D>: ATT_DEAD_BF16<D>)
    m = torch.full((B, nheads, Lq, 1), -1e30)
    l = torch.zeros(B, nheads, Lq, 1)
    o = torch.zeros(B, nheads, Lq, D)
    for t in range(0, Lk, tile):
        s = qh @ kh[:, :, t:t + tile].transpose(-1, -2)
        if key_mask is not None:
            s = s.masked_fill(key_mask[:, None, None, t:t + tile].bool(), dead)
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2((m - m_new) * c)
        if fma:
            p = torch.exp2((s.double() * c.double() - (m_new * c).double()).float())
        else:
            p = torch.exp2(s * c - m_new * c)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + O._rb(p) @ vh[:, :, t:t + tile]
        m = m_new
    return O._rb(o * (1.0 / l)).permute(0, 2, 1, 3).reshape(B, Lq, E)


@torch.no_grad()
def detr_forward_bf16(sd, img, blocks=(3, 4, 6, 3), nheads=8, enc_layers=6, dec_layers=6):
    """O.detr_forward_bf16 (Bottleneck body) at the width of `sd`: the sine table of E // 2 features, attention_b"""
    _rb, _conv_b, _lin_b, _ln_b = O._rb, O._conv_b, O._lin_b, O._ln_b
    pre = "backbone.0.body."
    x = _conv_b(_rb(img), sd, pre + "conv1.weight", bn=pre + "bn1", stride=2, padding=3, relu=True)
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for i in range(blocks[l]):
            p = f"{pre}layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            t = _conv_b(x, sd, p + "conv1.weight", bn=p + "bn1", relu=True)
            t = _conv_b(t, sd, p + "conv2.weight", bn=p + "bn2", stride=stride, padding=1, relu=True)
            idt = _conv_b(x, sd, p + "downsample.0.weight", bn=p + "downsample.1", stride=stride) if i == 0 else x
            x = _conv_b(t, sd, p + "conv3.weight", bn=p + "bn3", res=idt, relu=True)
    feat = x
    B, _, h, w = feat.shape
    E = sd["input_proj.weight"].shape[0]
    pos = position_embedding(h, w, E, batch=1).flatten(2).permute(0, 2, 1)
    src = _conv_b(feat, sd, "input_proj.weight", bias=sd["input_proj.bias"]).flatten(2).permute(0, 2, 1)
    srcpos = _rb(src + pos)
    tp = "transformer."
    for i in range(enc_layers):
        p = f"{tp}encoder.layers.{i}."
        W, b = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        qk = _lin_b(srcpos, W[:2 * E], b[:2 * E])
        v = _lin_b(src, W[2 * E:], b[2 * E:])
        att = attention_b(qk[..., :E], qk[..., E:], v, nheads)
        tmp = _lin_b(att, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], res=src)
        src, _ = _ln_b(tmp, sd, p + "norm1")
        ffn = _lin_b(src, sd[p + "linear1.weight"], sd[p + "linear1.bias"], relu=True)
        tmp = _lin_b(ffn, sd[p + "linear2.weight"], sd[p + "linear2.bias"], res=src)
        src, srcpos = _ln_b(tmp, sd, p + "norm2", pos)
    memory = src
    qpos = sd["query_embed.weight"].unsqueeze(0)
    Q = qpos.shape[1]
    tgt = torch.zeros(B, Q, E)
    tgtpos = _rb(qpos).expand(B, Q, E)
    for i in range(dec_layers):
        p = f"{tp}decoder.layers.{i}."
        W, b = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        qk = _lin_b(tgtpos, W[:2 * E], b[:2 * E])
        v = _lin_b(tgt, W[2 * E:], b[2 * E:])
        att = attention_b(qk[..., :E], qk[..., E:], v, nheads)
        tmp = _lin_b(att, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], res=tgt)
        tgt, tgtpos = _ln_b(tmp, sd, p + "norm1", qpos)
        W, b = sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"]
        cq = _lin_b(tgtpos, W[:E], b[:E])
        kc = _lin_b(srcpos, W[E:2 * E], b[E:2 * E])
        vc = _lin_b(memory, W[2 * E:], b[2 * E:])
        att = attention_b(cq, kc, vc, nheads)
        tmp = _lin_b(att, sd[p + "multihead_attn.out_proj.weight"], sd[p + "multihead_attn.out_proj.bias"], res=tgt)
        tgt, _ = _ln_b(tmp, sd, p + "norm2")
        ffn = _lin_b(tgt, sd[p + "linear1.weight"], sd[p + "linear1.bias"], relu=True)
        tmp = _lin_b(ffn, sd[p + "linear2.weight"], sd[p + "linear2.bias"], res=tgt)
        tgt, tgtpos = _ln_b(tmp, sd, p + "norm3", qpos)
    hs, _ = _ln_b(tgt, sd, tp + "decoder.norm")

    def mlp(p):
        h1 = _lin_b(hs, sd[p + ".layers.0.weight"], sd[p + ".layers.0.bias"], relu=True)
        h2 = _lin_b(h1, sd[p + ".layers.1.weight"], sd[p + ".layers.1.bias"], relu=True)
        return _lin_b(h2, sd[p + ".layers.2.weight"], sd[p + ".layers.2.bias"], out_f32=True)
    return {
        "pred_logits": _lin_b(hs, sd["class_embed.weight"], sd["class_embed.bias"], out_f32=True),
        "pred_boxes": mlp("bbox_embed").sigmoid(),
        "pred_angle": mlp("angle_embed"),
        "pred_offset": mlp("offset_embed"),
        "pred_size": mlp("size_embed"),
        "pred_depth": mlp("depth_embed"),
        "pred_obj_features": hs,
    }


def module_transformer(src, pos, query_embed, sd, nheads, enc_layers=6, dec_layers=6, prefix="transformer."):
    """the post-norm transformer built from torch.nn modules (nn.MultiheadAttention, nn.LayerNorm, nn.Linear) loaded from `sd`,
    as src/models/transformer.py composes them: an independent statement of O.transformer for the width checks"""
    E = src.shape[1]
    nn = torch.nn

    def mha(p):
        m = nn.MultiheadAttention(E, nheads, dropout=0.0)
        m.load_state_dict({"in_proj_weight": sd[p + "in_proj_weight"], "in_proj_bias": sd[p + "in_proj_bias"],
                           "out_proj.weight": sd[p + "out_proj.weight"], "out_proj.bias": sd[p + "out_proj.bias"]})
        return m.eval()

    def ln(p):
        m = nn.LayerNorm(E)
        m.load_state_dict({"weight": sd[p + ".weight"], "bias": sd[p + ".bias"]})
        return m

    def ffn(p, x):
        l1 = nn.Linear(E, sd[p + "linear1.weight"].shape[0])
        l1.load_state_dict({"weight": sd[p + "linear1.weight"], "bias": sd[p + "linear1.bias"]})
        l2 = nn.Linear(sd[p + "linear2.weight"].shape[1], E)
        l2.load_state_dict({"weight": sd[p + "linear2.weight"], "bias": sd[p + "linear2.bias"]})
        return l2(torch.relu(l1(x)))

    bs = src.shape[0]
    x = src.flatten(2).permute(2, 0, 1)
    pe = pos.flatten(2).permute(2, 0, 1)
    qe = query_embed.unsqueeze(1).repeat(1, bs, 1)
    with torch.no_grad():
        for i in range(enc_layers):
            p = f"{prefix}encoder.layers.{i}."
            q = k = x + pe
            x = ln(p + "norm1")(x + mha(p + "self_attn.")(q, k, x)[0])
            x = ln(p + "norm2")(x + ffn(p, x))
        memory = x
        tgt = torch.zeros_like(qe)
        for i in range(dec_layers):
            p = f"{prefix}decoder.layers.{i}."
            q = k = tgt + qe
            tgt = ln(p + "norm1")(tgt + mha(p + "self_attn.")(q, k, tgt)[0])
            tgt = ln(p + "norm2")(tgt + mha(p + "multihead_attn.")(tgt + qe, memory + pe, memory)[0])
            tgt = ln(p + "norm3")(tgt + ffn(p, tgt))
        hs = ln(prefix + "decoder.norm")(tgt)
    return hs.transpose(0, 1), memory

