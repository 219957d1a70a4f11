"""Transformer widths other than 256 / 8 heads on the CPU: tests/width_ref.py pinned bit for bit against oracle/detr_oracle.py at
the default width and against a torch.nn-module transformer at E = 512, and the width rule that Detector / build() enforce."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import width_ref as WR  # noqa: E402
from width_ref import O  # noqa: E402

KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth", "pred_obj_features")


def _small_sd(hidden, nheads, seed=0):
    from odam_amd import weights
    return weights.make_state_dict(hidden=hidden, seed=seed, enc_layers=2, dec_layers=2, num_queries=20)


def test_head_scale_is_the_kernels():
    assert WR.head_scale(32).item() == float(torch.tensor(0.1767766952966369, dtype=torch.float32))
    assert WR.head_scale(64).item() == 0.125


def test_width_ref_equals_oracle_at_256():
    """at E = 256 / 8 heads the restatement IS the oracle: fp32 and bf16-faithful outputs equal bit for bit"""
    torch.set_num_threads(16)
    sd = _small_sd(256, 8)
    img = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(1))
    a = WR.detr_forward(sd, img, enc_layers=2, dec_layers=2, return_taps=True)
    b = O.detr_forward(sd, img, enc_layers=2, dec_layers=2, return_taps=True)
    for k in KEYS + ("_memory",):
        assert torch.equal(a[k], b[k]), k
    a = WR.detr_forward_bf16(sd, img, enc_layers=2, dec_layers=2)
    b = O.detr_forward_bf16(sd, img, enc_layers=2, dec_layers=2)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_attention_b_equals_oracle_at_d32():
    g = torch.Generator().manual_seed(2)
    q, k, v = (O._rb(torch.randn(2, n, 256, generator=g)) for n in (37, 150, 150))
    mask = torch.rand(2, 150, generator=g) < 0.3
    assert torch.equal(WR.attention_b(q, k, v, 8, key_mask=mask), O._attention_b(q, k, v, 8, key_mask=mask))


def test_attention_b_d64_matches_float64():
    """the D = 64 bf16-faithful attention stays within its bf16 rounding of float64 softmax attention at scale 1/8"""
    g = torch.Generator().manual_seed(3)
    q, k, v = (O._rb(torch.randn(1, n, 256, generator=g)) for n in (20, 130, 130))
    got = WR.attention_b(q, k, v, 4)
    qh, kh, vh = (t.double().reshape(1, -1, 4, 64).transpose(1, 2) for t in (q, k, v))
    want = (torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, -1) @ vh).transpose(1, 2).reshape(1, 20, 256)
    assert ((got.double() - want).abs() <= 2.0 ** -7 * vh.abs().max() + 2.0 ** -8 * want.abs()).all()


@pytest.mark.parametrize("E,H", [(512, 8), (384, 6)])
def test_width_ref_transformer_equals_nn_modules(E, H):
    """O.transformer at E / H against nn.MultiheadAttention / nn.LayerNorm / nn.Linear modules on the same tensors"""
    torch.set_num_threads(16)
    sd = _small_sd(E, H, seed=4)
    g = torch.Generator().manual_seed(5)
    src = torch.randn(2, E, 6, 7, generator=g)
    pos = WR.position_embedding(6, 7, E, batch=2)
    assert pos.shape == (2, E, 6, 7)
    hs, mem = O.transformer(src, pos, sd["query_embed.weight"], sd, H, 2, 2)
    hs_m, mem_m = WR.module_transformer(src, pos, sd["query_embed.weight"], sd, H, 2, 2)
    assert ((hs[-1] - hs_m).abs().max() / hs_m.abs().max()).item() <= 1e-5
    assert ((mem - mem_m).abs().max() / mem_m.abs().max()).item() <= 1e-5


ACCEPT = [(512, 8), (384, 12), (256, 4), (128, 4), (384, 6), (1024, 16), (128, 2), (256, 8)]
REFUSE = [(256, 16, "head dim"), (512, 4, "head dim"), (320, 7, "multiple of nheads"), (1088, 17, "multiple of 64 in 128 .. 1024"),
          (64, 2, "multiple of 64 in 128 .. 1024"), (200, 4, "multiple of 64"), (256, 0, "multiple of nheads"),
          (1024, 8, "16 and 128 are not built")]


@pytest.mark.parametrize("E,H", ACCEPT)
def test_widths_accepted(E, H):
    from odam_amd import detector
    det = detector.Detector(hidden_dim=E, nheads=H, device="cpu")
    assert det.arch["hidden_dim"] == E and det.arch["nheads"] == H
    det, _, _ = detector.build(dict(hidden_dim=E, nheads=H))
    assert det.arch["hidden_dim"] == E and det.arch["nheads"] == H


@pytest.mark.parametrize("E,H,match", REFUSE)
def test_widths_refused(E, H, match):
    from odam_amd import _lib, detector
    with pytest.raises(ValueError, match=match):
        detector.Detector(hidden_dim=E, nheads=H, device="cpu")
    with pytest.raises((ValueError, _lib.OdamError), match=match):
        detector.build(dict(hidden_dim=E, nheads=H))


def test_build_passes_width_to_every_table():
    """the learned position tables and the sine table follow hidden_dim"""
    from odam_amd import detector, weights
    sd = weights.add_variant_weights(_small_sd(384, 6), hidden=384)
    pos = detector.learned_position_embedding(sd["backbone.1.row_embed.weight"], sd["backbone.1.col_embed.weight"], 5, 7)
    assert pos.shape == (35, 384)
    want = O.position_embedding_learned(sd, 5, 7)[0].flatten(1).T
    assert torch.equal(pos, want)
    sine = detector.sine_position_embedding(5, 7, 384 // 2)
    assert torch.allclose(torch.as_tensor(sine).reshape(35, 384),
                          WR.position_embedding(5, 7, 384)[0].flatten(1).T, rtol=0, atol=1e-6)
