"""ResNet-18/34 (torchvision BasicBlock) and ResNet-152 backbones, host side: the BasicBlock restatement the GPU tests use as
their oracle (tests/basic_body.py) pinned against an independent implementation of the same architecture, the weight
generator's key set, and the configurations build(cfg) refuses before any device work."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from basic_body import BASIC_BLOCKS, basic_body  # noqa: E402


def hf_basic_resnet(sd, depths, prefix="backbone.0.body."):
    """transformers.ResNetModel (layer_type "basic") carrying the torchvision-named weights of `sd`; BatchNorm in eval mode is
    FrozenBatchNorm2d (eps 1e-5 on both sides)"""
    from transformers import ResNetConfig, ResNetModel
    cfg = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[64, 128, 256, 512], depths=list(depths),
                       layer_type="basic", hidden_act="relu", downsample_in_first_stage=False)
    m = ResNetModel(cfg).eval()
    new = {}

    def bn(dst, src):
        for k in ("weight", "bias", "running_mean", "running_var"):
            new[dst + "normalization." + k] = sd[prefix + src + "." + k]

    new["embedder.embedder.convolution.weight"] = sd[prefix + "conv1.weight"]
    bn("embedder.embedder.", "bn1")
    for s, n in enumerate(depths):
        for i in range(n):
            src, dst = f"layer{s + 1}.{i}.", f"encoder.stages.{s}.layers.{i}."
            for j in range(2):
                new[dst + f"layer.{j}.convolution.weight"] = sd[prefix + src + f"conv{j + 1}.weight"]
                bn(dst + f"layer.{j}.", src + f"bn{j + 1}")
            if prefix + src + "downsample.0.weight" in sd:
                new[dst + "shortcut.convolution.weight"] = sd[prefix + src + "downsample.0.weight"]
                bn(dst + "shortcut.", src + "downsample.1")
    missing, unexpected = m.load_state_dict(new, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing), missing
    return m


@pytest.mark.parametrize("backbone", ["resnet18", "resnet34"])
def test_basic_body_matches_transformers_resnet(backbone):
    pytest.importorskip("transformers")
    from odam_amd import weights
    depths = BASIC_BLOCKS[backbone]
    sd = weights.make_state_dict(backbone=backbone, seed=0)
    torch.manual_seed(0)
    x = torch.randn(2, 3, 160, 224)
    hf = hf_basic_resnet(sd, depths)
    # the independent model's own structure: no shortcut in the first stage, one on the first block of every later stage
    assert not hasattr(hf.encoder.stages[0].layers[0].shortcut, "convolution")
    assert hasattr(hf.encoder.stages[1].layers[0].shortcut, "convolution")
    with torch.no_grad():
        ours = basic_body(x, sd, depths)
        theirs = hf(x).last_hidden_state
    assert ours.shape == theirs.shape == (2, 512, 5, 7)
    scale = theirs.abs().max().item()
    assert scale > 0.1      # the damped residual branches keep layer4 O(1) over the 8 / 16 blocks
    assert (ours - theirs).abs().max().item() <= 1e-5 * scale


def test_resnet34_state_dict_keys():
    from odam_amd import weights
    sd = weights.make_state_dict(backbone="resnet34", seed=0)
    body = "backbone.0.body."
    blocks = [k[len(body):].rsplit(".", 2)[0] for k in sd if k.startswith(body + "layer")]
    names = sorted({b.split(".")[0] + "." + b.split(".")[1] for b in blocks})
    assert len(names) == 16
    for n in names:
        for part in ("conv1", "bn1", "conv2", "bn2"):
            assert any(k.startswith(f"{body}{n}.{part}.") for k in sd), (n, part)
        assert not any(k.startswith(f"{body}{n}.conv3") or k.startswith(f"{body}{n}.bn3") for k in sd), n
    ds = sorted({k.split(".downsample")[0][len(body):] for k in sd if ".downsample." in k})
    assert ds == ["layer2.0", "layer3.0", "layer4.0"]
    assert sd[body + "layer1.0.conv1.weight"].shape == (64, 64, 3, 3)
    assert sd[body + "layer2.0.conv1.weight"].shape == (128, 64, 3, 3)
    assert sd[body + "layer2.0.downsample.0.weight"].shape == (128, 64, 1, 1)
    assert sd[body + "layer4.2.conv2.weight"].shape == (512, 512, 3, 3)
    assert tuple(sd["input_proj.weight"].shape) == (256, 512, 1, 1)


def test_resnet152_state_dict_keys():
    from odam_amd import weights
    sd = weights.make_state_dict(backbone="resnet152", seed=0)
    body = "backbone.0.body."
    per_stage = [len({k.split(".")[4] for k in sd if k.startswith(f"{body}layer{l}.")}) for l in range(1, 5)]
    assert per_stage == [3, 8, 36, 3]
    assert sd[body + "layer3.35.conv3.weight"].shape == (1024, 256, 1, 1)
    assert tuple(sd["input_proj.weight"].shape) == (256, 2048, 1, 1)


def test_bottleneck_draws_unchanged():
    """the Bottleneck generator is one code path for every depth: a ResNet-152 state dict repeats R101's draws for as long as
    the two bodies agree (through layer2.3; the committed goldens pin resnet50 / resnet101 themselves)"""
    from odam_amd import weights
    a = weights.make_state_dict(backbone="resnet101", seed=0)
    b = weights.make_state_dict(backbone="resnet152", seed=0)
    for k in ("backbone.0.body.conv1.weight", "backbone.0.body.layer1.2.conv3.weight", "backbone.0.body.layer2.3.bn3.bias"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cfg,match", [
    (dict(backbone="resnext50_32x4d"), "resnext50_32x4d"),
    (dict(backbone="wide_resnet50_2"), "wide_resnet50_2"),
    (dict(backbone="resnet34", dilation=True), "dilation"),
    (dict(backbone="resnet18", dilation=True), "dilation"),
])
def test_build_refuses(cfg, match):
    from odam_amd import _lib, detector
    with pytest.raises(_lib.OdamError, match=match):
        detector.build(cfg)


def test_detector_validates_backbone_at_construction():
    from odam_amd import detector
    with pytest.raises(ValueError, match="resnet200"):
        detector.Detector(backbone="resnet200")
    with pytest.raises(ValueError, match="dilation"):
        detector.Detector(backbone="resnet34", dilation=True)
    for bb in ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152"):
        det, _, _ = detector.build(dict(backbone=bb))
        assert det.arch["backbone"] == bb and det.basic_block == (bb in ("resnet18", "resnet34"))


def test_cfg_struct_matches_header():
    """the ctypes mirror of odam_detr_cfg ends in the appended basic_block field, as the header does"""
    import ctypes
    from odam_amd import detector
    src = open(os.path.join(ROOT, "include", "odam_detr.h")).read()
    body = src[src.index("typedef struct {"):src.index("} odam_detr_cfg;")]
    assert body.rstrip().rsplit("int ", 1)[1].startswith("basic_block;")
    fields = [f[0] for f in detector._Cfg._fields_]
    assert fields[-1] == "basic_block"
    assert ctypes.sizeof(detector._Cfg) == 4 * (4 + len(fields) - 1)      # resnet_blocks[4] + one int per other field
