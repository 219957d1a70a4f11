"""The argument contract of the detector's C entry points: which checks each entry runs, its return code and its error
text.  Every call here returns before the library touches the device (dummy non-null pointers are never dereferenced), so
the file runs without a GPU.  It pins behaviour, not an implementation: it passes unchanged on the tree before and after
the split of the detector's host code."""
import ctypes

import pytest

P = ctypes.c_void_p(16)      # a pointer that only has to be non-null
N = None                     # a null pointer
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def L():
    from odam_amd import _lib
    return _lib.lib()


def att(q=P, ldq=32, ldk=32, ldv=32, ldo=32, B=1, H=1, Lq=4, Lk=4):
    return (q, ldq, P, ldk, P, ldv, P, ldo, B, H, Lq, Lk)


def conv_ex(dil=1, dtype=0, out_f32=0):
    # x, w, scale, bias, residual, y, B, H, W, Cin, Cout, KH, KW, stride, pad, dil, Kpad, relu, k_order, dtype, out_f32, stream
    return (P, P, N, N, N, P, 1, 8, 8, 32, 32, 1, 1, 1, 0, dil, 32, 0, 0, dtype, out_f32, N)


def conv_mx(dil=1, k_order=0):
    # x, xs, w, ws, scale, bias, residual, y, ys, y_bf16, y_f32, B, H, W, Cin, Cout, KH, KW, stride, pad, dil, Kpad, relu, k_order, stream
    return (P, P, P, P, N, N, N, P, P, N, N, 1, 8, 8, 64, 32, 1, 1, 1, 0, dil, 64, 0, k_order, N)


def bottleneck_f32(P_=64, PN=0, w1n=N, y_next=N):
    # x, w2, s2, b2, w3, s3, b3, residual, y, w1n, s1n, b1n, y_next, B, H, W, P, stride, PN, stream
    return (P, P, N, N, P, N, N, N, P, w1n, N, N, y_next, 1, 8, 8, P_, 1, PN, N)


# (entry, arguments, return code, fragment of odam_last_error() or None)
CASES = [
    ("odam_op_attention", att(q=N) + (N,), 1, "null pointer"),
    ("odam_op_attention_bf16", att(ldq=33) + (N,), 1, "row pitches must be multiples of 8 / 8 / 8 / 4 elements"),
    ("odam_op_attention_ex", att(H=1) + (48, 0, N, N), 1,
     "head_dim 32 (fp32 / bf16, optional key mask) or 64 (fp32, no mask) only"),
    ("odam_op_attention_ex", att(H=0) + (48, 0, N, N), 0, None),
    ("odam_op_attention_hd", att() + (48, 0, N, N), 1, "head_dim must be 32 or 64"),
    ("odam_op_attention_hd", att() + (32, 2, N, N), 1, "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_attention_hd", att(ldq=36) + (32, 1, N, N), 1, "row pitches"),
    ("odam_op_attention_hd", att(H=0, ldq=64, ldk=64, ldv=64, ldo=64) + (64, 1, N, N), 0, None),
    ("odam_op_add_layernorm", (N, N, P, P, P, 4, N), 1, "null pointer"),
    # x, r, gamma, beta, y, pos, L, y_pos, M, dtype, stream
    ("odam_op_add_layernorm_ex", (P, N, P, P, P, N, 4, P, 4, 0, N), 1, "y_pos needs pos and L > 0"),
    # x, r, gamma, beta, y, pos, L, y_pos, M, C, dtype, stream
    ("odam_op_add_layernorm_c", (P, N, P, P, P, N, 1, N, 4, 96, 0, N), 1, "C must be a multiple of 64 in 128 .. 1024"),
    ("odam_op_conv2d_nhwc_ex", conv_ex(dil=0), 1, "dilation must be >= 1"),
    ("odam_op_conv2d_nhwc_ex", conv_ex(dtype=0, out_f32=1), 1, "out_f32 is for bf16 operands"),
    ("odam_op_conv2d_nhwc_ex", conv_ex(dtype=2), 1, ""),
    ("odam_op_conv2d_nhwc_mxfp8", conv_mx(dil=2), 1, ""),
    ("odam_op_conv2d_nhwc_mxfp8", conv_mx(k_order=1), 1, ""),
    ("odam_op_bottleneck_f32", bottleneck_f32(P_=32), 4, "built for P = 64 and 128"),
    ("odam_op_bottleneck_f32", bottleneck_f32(PN=64, w1n=N, y_next=P), 1, ""),
    # the two mode setters are process-wide switches: only their rejected values are safe to pass here
    ("odam_op_conv_f32_mode", (1,), 1, "mode must be 0 or 2"),
    ("odam_op_conv_bf16_mode", (3,), 1, ""),
    ("odam_op_quantize_mxfp8", (P, 2, LL(32), P, P, N), 1, ""),
    ("odam_op_maxpool3x3s2_nhwc", (P, P, 1, 8, 8, 6, N), 1, ""),
]


@pytest.mark.parametrize("entry,args,code,fragment", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_op_entry_argument_contract(L, entry, args, code, fragment):
    assert getattr(L, entry)(*args) == code
    if code:      # a call that succeeds leaves the last error's old text in place
        err = L.odam_last_error().decode()
        assert err.startswith(entry + ":"), err
        assert fragment in err, err


def make_cfg(**kw):
    from odam_amd.detector import _Cfg
    cfg = _Cfg()
    for i, n in enumerate((3, 4, 6, 3)):
        cfg.resnet_blocks[i] = n
    cfg.hidden_dim, cfg.nheads, cfg.dim_feedforward, cfg.enc_layers, cfg.dec_layers = 256, 8, 2048, 6, 6
    cfg.num_queries, cfg.num_classes1, cfg.angle_bins = 100, 19, 30
    cfg.max_batch, cfg.img_h, cfg.img_w = 2, 256, 320
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("kw,code", [
    (dict(hidden_dim=200), 3),
    (dict(nheads=3), 3),
    (dict(nheads=16), 3),              # head dim 16
    (dict(dtype=2, dilation=1), 3),
    (dict(dtype=3), 1),
])
def test_create_refuses(L, kw, code):
    m = ctypes.c_void_p(0)
    cfg = make_cfg(**kw)
    assert L.odam_detr_create(ctypes.byref(cfg), ctypes.byref(m)) == code
    assert L.odam_last_error().decode().startswith("odam_detr_create:")
    assert not m.value


def test_model_without_weights(L):
    """a fresh valid model: finalize names the first missing weight, weights can still be set, the forward refuses to run"""
    m = ctypes.c_void_p(0)
    cfg = make_cfg()
    assert L.odam_detr_create(ctypes.byref(cfg), ctypes.byref(m)) == 0 and m.value
    try:
        assert L.odam_detr_finalize(m) == 1
        err = L.odam_last_error().decode()
        assert err.startswith("odam_detr_finalize:") and "missing weight backbone.0.body.conv1.weight" in err, err
        w = (ctypes.c_float * 4)(1, 2, 3, 4)
        shape = (ctypes.c_longlong * 1)(4)
        assert L.odam_detr_set_weight(m, b"backbone.0.body.bn1.weight", w, shape, 1) == 0
        assert L.odam_detr_forward(m, P, 1, P, P, P, P, P, P, N, N) == 1
        err = L.odam_last_error().decode()
        assert err.startswith("odam_detr_forward:") and "call odam_detr_finalize first" in err, err
    finally:
        assert L.odam_detr_destroy(m) == 0
