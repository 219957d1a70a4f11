"""Deterministic synthetic detector weights under the reference's state_dict key names
(the trained checkpoints of the reference are a Google-Drive download, README.md:13 -- not available
offline).  Same generator on every box: torch's CPU Philox/MT streams are version-stable.

Scaling keeps activations O(1) through the 8-50 residual blocks (He-uniform filters, residual branch
damped through its last batch norm: bn3.weight of a bottleneck, bn2.weight of a basic block) and spreads the class logits so that some queries clear the 0.6 detection
threshold, which exercises post-processing, NMS and everything downstream."""
import math

import torch

RESNET_BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3), "resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3),
                 "resnet152": (3, 8, 36, 3)}
# torchvision's block type per model (src/models/backbone.py:90 builds whichever ResNet the config names): BasicBlock = two 3x3
# convolutions, expansion 1 (layer4 has 512 channels); Bottleneck = 1x1 reduce, 3x3, 1x1 expand, expansion 4 (2048)
RESNET_BLOCK_TYPE = {"resnet18": "basic", "resnet34": "basic", "resnet50": "bottleneck", "resnet101": "bottleneck",
                     "resnet152": "bottleneck"}


def layer4_channels(backbone):
    return 512 if RESNET_BLOCK_TYPE[backbone] == "basic" else 2048


def _u(gen, shape, bound):
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1) * bound


def _conv(gen, cout, cin, k):
    return _u(gen, (cout, cin, k, k), math.sqrt(6.0 / (cin * k * k)))


def _bn(sd, p, gen, n, gain=1.0):
    sd[p + ".weight"] = gain * (1.0 + 0.1 * _u(gen, (n,), 1.0))
    sd[p + ".bias"] = 0.05 * _u(gen, (n,), 1.0)
    sd[p + ".running_mean"] = 0.05 * _u(gen, (n,), 1.0)
    sd[p + ".running_var"] = 1.0 + 0.2 * _u(gen, (n,), 1.0)


def _linear(sd, p, gen, nout, nin, wscale=1.0, bias=0.0):
    sd[p + ".weight"] = _u(gen, (nout, nin), wscale * math.sqrt(3.0 / nin))
    sd[p + ".bias"] = bias + 0.02 * _u(gen, (nout,), 1.0)


def make_state_dict(backbone="resnet50", hidden=256, ffn=2048, enc_layers=6, dec_layers=6, num_queries=100,
                    num_classes=18, angle_bins=30, seed=0, scene=False):
    """`scene=False`: the round-1 generator (identity-like batch-norm statistics; every query collapses onto one
    detection per frame -- kept because the committed detector goldens were generated with it).
    `scene=True`: the same random tensors with (a) FrozenBN running statistics calibrated on synthetic frames
    (tools/make_synth_calib.py, stored under odam_amd/data/) so that features keep their spatial variation and the
    100 queries decode to different objects, and (b) head biases that keep labels inside CLASS_MAPPER's 0..7
    (sq_libs.py:13-22), boxes small and spread, depths 1.5-4.5 m: 5-30 detections per frame after NMS."""
    sd = _make_state_dict(backbone, hidden, ffn, enc_layers, dec_layers, num_queries, num_classes, angle_bins, seed)
    if scene:
        _scene_heads(sd, backbone, seed, num_classes, enc_layers, dec_layers)
    return sd


def add_variant_weights(sd, hidden=256, seed=0):
    """The tensors only the configuration VARIANTS read, under the reference's key names, drawn from their own generator so that
    the entries of `sd` stay what they are: the encoder's final LayerNorm of `pre_norm` models (transformer.py:26-28) and the
    two 50-row tables of the learned position embedding (position_encoding.py:53-60, uniform in [0, 1) as reset_parameters)."""
    g = torch.Generator().manual_seed(7000 + seed)
    sd["transformer.encoder.norm.weight"] = 1.0 + 0.1 * _u(g, (hidden,), 1.0)
    sd["transformer.encoder.norm.bias"] = 0.05 * _u(g, (hidden,), 1.0)
    sd["backbone.1.row_embed.weight"] = torch.rand((50, hidden // 2), generator=g, dtype=torch.float32)
    sd["backbone.1.col_embed.weight"] = torch.rand((50, hidden // 2), generator=g, dtype=torch.float32)
    return sd


def scene_backbone_gains(sd):
    """residual branches of the backbone damped further (bn3 gain 0.4 -> 0.1): with calibrated (centring) batch-norm
    statistics a random 50-layer network amplifies a last-bit perturbation of its input about 30x by layer4; damped it
    is about 4x, so fp32 summation-order differences stay far from the detection thresholds.  Applied before the
    statistics are calibrated (tools/make_synth_calib.py) and before they are loaded."""
    for k in sd:
        if k.endswith("bn3.weight"):
            sd[k] = sd[k] * 0.25


def scene_transformer(sd, enc_layers=6, dec_layers=6):
    """transformer of the scene weights: residual branches damped, so that tokens / queries keep their identity through
    6 + 6 post-norm layers of random weights (undamped, every token converges to the sequence mean).  Attention is left
    as soft as the generator makes it: sharper cross-attention gives more distinct queries but makes the decoder
    amplify perturbations of its input 3x; as it is the transformer is contractive."""
    for i in range(enc_layers):
        p = f"transformer.encoder.layers.{i}."
        sd[p + "self_attn.out_proj.weight"] = sd[p + "self_attn.out_proj.weight"] * 0.2
        sd[p + "linear2.weight"] = sd[p + "linear2.weight"] * 0.2
    for i in range(dec_layers):
        p = f"transformer.decoder.layers.{i}."
        sd[p + "self_attn.out_proj.weight"] = sd[p + "self_attn.out_proj.weight"] * 0.3
        sd[p + "linear2.weight"] = sd[p + "linear2.weight"] * 0.3


def _scene_heads(sd, backbone, seed, num_classes, enc_layers=6, dec_layers=6):
    import os
    import numpy as np
    if RESNET_BLOCK_TYPE[backbone] != "bottleneck":
        raise ValueError(f"scene weights: no batch-norm calibration for the {backbone} body (bottleneck backbones only)")
    scene_backbone_gains(sd)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", f"synth_calib_{backbone}_s{seed}.npz")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: run tests/golden/make_synth_calib.py {backbone} {seed}")
    z = np.load(path)
    for k in z.files:
        if k.startswith("hs_"):
            continue
        assert k in sd and tuple(sd[k].shape) == z[k].shape, k
        sd[k] = torch.from_numpy(z[k].astype(np.float32))
    scene_transformer(sd, enc_layers, dec_layers)
    # heads: centred on the mean decoder output and rescaled by the spread between queries, so that every output
    # follows what distinguishes one query from another
    hbar = torch.from_numpy(z["hs_mean"].astype(np.float32))
    gain = 1.0 / float(z["hs_std"])
    for key in ["class_embed"] + [n + ".layers.0" for n in ("bbox_embed", "offset_embed", "angle_embed", "size_embed", "depth_embed")]:
        w = sd[key + ".weight"] * gain
        sd[key + ".bias"] = sd[key + ".bias"] - w @ hbar
        sd[key + ".weight"] = w
    # labels inside CLASS_MAPPER's 0..7, box centres spread over the image, boxes small, sizes positive, depths 1.5-5 m
    b = sd["class_embed.bias"].clone()
    b[8:num_classes] -= 40.0
    sd["class_embed.bias"] = b
    w = sd["bbox_embed.layers.2.weight"].clone(); w[:2] *= 3.0
    bb = sd["bbox_embed.layers.2.bias"].clone(); bb[2:] -= 1.5
    sd["bbox_embed.layers.2.weight"] = w; sd["bbox_embed.layers.2.bias"] = bb
    sd["size_embed.layers.2.bias"] = sd["size_embed.layers.2.bias"] + 0.4
    sd["offset_embed.layers.2.weight"] = sd["offset_embed.layers.2.weight"] * 0.3
    sd["depth_embed.layers.2.weight"] = sd["depth_embed.layers.2.weight"] * 2.0


def _make_state_dict(backbone, hidden, ffn, enc_layers, dec_layers, num_queries, num_classes, angle_bins, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    bb = "backbone.0.body."
    sd[bb + "conv1.weight"] = _conv(g, 64, 3, 7)
    _bn(sd, bb + "bn1", g, 64)
    inplanes = 64
    basic = RESNET_BLOCK_TYPE[backbone] == "basic"
    for l, nb in enumerate(RESNET_BLOCKS[backbone]):
        planes = 64 * 2 ** l
        for i in range(nb):
            p = f"{bb}layer{l + 1}.{i}."
            if basic:
                # torchvision BasicBlock: conv1 3x3 (stride on the first block of layers 2-4), conv2 3x3; a downsample only where
                # the stride or the width changes (expansion 1: layer1.0 has none)
                stride = 2 if (i == 0 and l > 0) else 1
                sd[p + "conv1.weight"] = _conv(g, planes, inplanes, 3); _bn(sd, p + "bn1", g, planes)
                sd[p + "conv2.weight"] = _conv(g, planes, planes, 3); _bn(sd, p + "bn2", g, planes, gain=0.4)
                if stride != 1 or inplanes != planes:
                    sd[p + "downsample.0.weight"] = _conv(g, planes, inplanes, 1)
                    _bn(sd, p + "downsample.1", g, planes, gain=0.7)
                inplanes = planes
                continue
            sd[p + "conv1.weight"] = _conv(g, planes, inplanes, 1); _bn(sd, p + "bn1", g, planes)
            sd[p + "conv2.weight"] = _conv(g, planes, planes, 3); _bn(sd, p + "bn2", g, planes)
            sd[p + "conv3.weight"] = _conv(g, planes * 4, planes, 1); _bn(sd, p + "bn3", g, planes * 4, gain=0.4)
            if i == 0:
                sd[p + "downsample.0.weight"] = _conv(g, planes * 4, inplanes, 1)
                _bn(sd, p + "downsample.1", g, planes * 4, gain=0.7)
            inplanes = planes * 4
    sd["input_proj.weight"] = _u(g, (hidden, inplanes, 1, 1), math.sqrt(3.0 / inplanes))
    sd["input_proj.bias"] = 0.02 * _u(g, (hidden,), 1.0)

    def attn(p):
        sd[p + "in_proj_weight"] = _u(g, (3 * hidden, hidden), 1.5 * math.sqrt(3.0 / hidden))
        sd[p + "in_proj_bias"] = 0.02 * _u(g, (3 * hidden,), 1.0)
        _linear(sd, p + "out_proj", g, hidden, hidden)

    def ln(p):
        sd[p + ".weight"] = 1.0 + 0.1 * _u(g, (hidden,), 1.0)
        sd[p + ".bias"] = 0.05 * _u(g, (hidden,), 1.0)

    for i in range(enc_layers):
        p = f"transformer.encoder.layers.{i}."
        attn(p + "self_attn.")
        _linear(sd, p + "linear1", g, ffn, hidden); _linear(sd, p + "linear2", g, hidden, ffn)
        ln(p + "norm1"); ln(p + "norm2")
    for i in range(dec_layers):
        p = f"transformer.decoder.layers.{i}."
        attn(p + "self_attn."); attn(p + "multihead_attn.")
        _linear(sd, p + "linear1", g, ffn, hidden); _linear(sd, p + "linear2", g, hidden, ffn)
        ln(p + "norm1"); ln(p + "norm2"); ln(p + "norm3")
    ln("transformer.decoder.norm")
    sd["query_embed.weight"] = torch.randn((num_queries, hidden), generator=g, dtype=torch.float32)
    _linear(sd, "class_embed", g, num_classes + 1, hidden, wscale=4.0)
    for name, nout, bias in (("bbox_embed", 4, 0.0), ("offset_embed", 2, 0.0), ("angle_embed", angle_bins, 0.0),
                             ("size_embed", 3, 0.8), ("depth_embed", 1, 2.5)):
        _linear(sd, name + ".layers.0", g, hidden, hidden)
        _linear(sd, name + ".layers.1", g, hidden, hidden)
        _linear(sd, name + ".layers.2", g, nout, hidden, wscale=0.5, bias=bias)
    return sd


def make_associator_state_dict(n_self=2, n_gnn=8, seed=0):
    """Deterministic synthetic weights under the reference Associator's key names (src/models/associator.py:163-200;
    configs/detr_scan_net.yaml: keypoint_encoder [78,256,256], 8 GNN layers, 2 self layers): random tensors.  They exercise
    the arithmetic, but every descriptor comes out nearly equal and the assignment is uniform.  The hand-written weights
    that make the same architecture associate by position and class (whole-chain fixture) are test scaffolding and live
    in tools/scene_weights.py."""
    return _make_associator_state_dict(n_self, n_gnn, seed)


def _make_associator_state_dict(n_self, n_gnn, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}

    def conv1d(p, nout, nin, wscale=1.0):
        sd[p + ".weight"] = _u(g, (nout, nin, 1), wscale * math.sqrt(3.0 / nin))
        sd[p + ".bias"] = 0.02 * _u(g, (nout,), 1.0)

    conv1d("encoder.0", 256, 78, 0.3)
    conv1d("encoder.2", 256, 256)
    for grp, n in (("fuser", n_self), ("gnn", n_gnn)):
        for i in range(n):
            p = f"{grp}.layers.{i}."
            conv1d(p + "attn.merge", 256, 256)
            for k in range(3):
                conv1d(p + f"attn.proj.{k}", 256, 256, 1.5)
            conv1d(p + "mlp.0", 512, 512)
            conv1d(p + "mlp.2", 256, 512, 0.5)
            sd[p + "mlp.2.bias"] = torch.zeros(256)
    conv1d("final_proj", 256, 256, 2.0)
    sd["bin_score"] = torch.tensor(1.0)
    return sd
