"""tests/detr_elementwise_ref.py against what it restates, and the argument contract of the op-level entries of the detector's
non-contraction kernels.  No device: the refusals return before any HIP call, and the restatements are numpy.

  * the postprocess restatement reproduces the reference's own DETR.postprocess outputs (tests/golden/detr_post.npz);
  * its bounds, and the sigmoid's, hold for the same operation sequences evaluated in numpy float32 (an independent float32 run);
  * the bfloat16 rounding and the pool restatement equal torch's on the CPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detr_elementwise_ref as ref

P = ctypes.c_void_p(16)      # a pointer that only has to be non-null
N = None
LL = ctypes.c_longlong
FL = ctypes.c_float
K = np.array([[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]])
KEYS = ("pred_logits", "pred_boxes", "pred_angle", "pred_offset", "pred_size", "pred_depth")


@pytest.fixture(scope="module")
def L():
    from odam_amd import _lib
    return _lib.lib()


def post_args(logits=P, K9=P, n=4, n_cls1=19, n_bins=30, rows=P):
    # logits, boxes, angle, offset, size, depth, n, n_cls1, n_bins, K9, img_w, img_h, rows, stream
    return (logits, P, P, P, P, P, n, n_cls1, n_bins, K9, FL(640), FL(480), rows, N)


# (entry, arguments, fragment of odam_last_error()): every call returns 1 (ODAM_E_INVALID)
REFUSALS = [
    # x, y, B, H, W, C, dtype, stream
    ("odam_op_maxpool3x3s2_nhwc_ex", (N, P, 1, 8, 8, 8, 0, N), "null pointer"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, N, 1, 8, 8, 8, 1, N), "null pointer"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 8, 8, 2, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 8, 8, -1, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, -1, 8, 8, 8, 0, N), "negative extent"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, -8, 8, 8, 0, N), "negative extent"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, -8, 8, 0, N), "negative extent"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 8, -8, 0, N), "negative extent"),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 8, 6, 1, N), "C must be a multiple of 4"),
    ("odam_op_maxpool3x3s2_nhwc", (N, P, 1, 8, 8, 8, N), "null pointer"),
    ("odam_op_maxpool3x3s2_nhwc", (P, P, 1, 8, 8, 6, N), "C must be a multiple of 4"),
    # in, out, B, H, W, dtype, framed, stream
    ("odam_op_nchw_to_nhwc4", (N, P, 1, 8, 8, 0, 0, N), "null pointer"),
    ("odam_op_nchw_to_nhwc4", (P, N, 1, 8, 8, 0, 1, N), "null pointer"),
    ("odam_op_nchw_to_nhwc4", (P, P, 1, 8, 8, 2, 0, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_nchw_to_nhwc4", (P, P, -1, 8, 8, 0, 0, N), "negative extent"),
    ("odam_op_nchw_to_nhwc4", (P, P, 1, -1, 8, 1, 1, N), "negative extent"),
    ("odam_op_nchw_to_nhwc4", (P, P, 1, 8, -1, 1, 1, N), "negative extent"),
    # in, out, B, H, W, C, dtype, stream
    ("odam_op_nhwc_to_nchw", (N, P, 1, 8, 8, 8, 0, N), "null pointer"),
    ("odam_op_nhwc_to_nchw", (P, N, 1, 8, 8, 8, 0, N), "null pointer"),
    ("odam_op_nhwc_to_nchw", (P, P, 1, 8, 8, 8, 3, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_nhwc_to_nchw", (P, P, 1, 8, 8, -5, 0, N), "negative extent"),
    ("odam_op_nhwc_to_nchw", (P, P, -2, 8, 8, 8, 1, N), "negative extent"),
    # x, pos, L, out, M, C, dtype, stream
    ("odam_op_add_pos", (P, N, 4, P, 4, 256, 0, N), "null pointer"),
    ("odam_op_add_pos", (P, P, 4, N, 4, 256, 0, N), "null pointer"),
    ("odam_op_add_pos", (N, P, 4, P, 4, 256, 2, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_add_pos", (P, P, 4, P, -4, 256, 0, N), "negative extent"),
    ("odam_op_add_pos", (P, P, 4, P, 4, -256, 0, N), "negative extent"),
    ("odam_op_add_pos", (P, P, 4, P, 4, 258, 0, N), "C must be a multiple of 4"),
    ("odam_op_add_pos", (P, P, 4, P, 4, 6, 1, N), "C must be a multiple of 4"),
    ("odam_op_add_pos", (P, P, 0, P, 4, 256, 0, N), "L must be positive"),
    ("odam_op_add_pos", (P, P, -3, P, 4, 128, 1, N), "L must be positive"),
    # in, out, n, dtype, stream
    ("odam_op_to_f32", (N, P, LL(8), 0, N), "null pointer"),
    ("odam_op_to_f32", (P, N, LL(8), 1, N), "null pointer"),
    ("odam_op_to_f32", (P, P, LL(8), 2, N), "dtype must be 0 (fp32) or 1 (bf16)"),
    ("odam_op_to_f32", (P, P, LL(-4), 0, N), "negative extent"),
    ("odam_op_to_f32", (P, P, LL(1023), 0, N), "n must be a multiple of 4"),
    ("odam_op_to_f32", (P, P, LL(2), 1, N), "n must be a multiple of 4"),
    # x, n, stream
    ("odam_op_sigmoid", (N, 4, N), "null pointer"),
    ("odam_op_sigmoid", (P, -1, N), "negative extent"),
    ("odam_op_postprocess", post_args(logits=N), "null pointer"),
    ("odam_op_postprocess", post_args(K9=N), "null pointer"),
    ("odam_op_postprocess", post_args(rows=N), "null pointer"),
    ("odam_op_postprocess", post_args(n=-1), "negative extent"),
    ("odam_op_postprocess", post_args(n_cls1=1), "n_cls1 must be at least 2"),
    ("odam_op_postprocess", post_args(n_cls1=0), "n_cls1 must be at least 2"),
    ("odam_op_postprocess", post_args(n_bins=0), "n_bins must be at least 1"),
]

# extents of 0: nothing to do, no launch, code 0 -- with pointers that could not be dereferenced
EMPTY = [
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 0, 8, 8, 8, 0, N)),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 0, 8, 8, 1, N)),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 0, 8, 0, N)),
    ("odam_op_maxpool3x3s2_nhwc_ex", (P, P, 1, 8, 8, 0, 0, N)),
    ("odam_op_nchw_to_nhwc4", (P, P, 0, 8, 8, 0, 0, N)),
    ("odam_op_nchw_to_nhwc4", (P, P, 0, 8, 8, 1, 1, N)),       # framed: no image, no frame
    ("odam_op_nchw_to_nhwc4", (P, P, 1, 0, 8, 0, 1, N)),
    ("odam_op_nhwc_to_nchw", (P, P, 1, 8, 8, 0, 0, N)),
    ("odam_op_add_pos", (N, P, 1, P, 0, 256, 0, N)),
    ("odam_op_add_pos", (N, P, 1, P, 4, 0, 1, N)),
    ("odam_op_to_f32", (P, P, LL(0), 1, N)),
    ("odam_op_sigmoid", (P, 0, N)),
    ("odam_op_postprocess", post_args(n=0)),
]


@pytest.mark.parametrize("entry,args,fragment", REFUSALS, ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_entry_refuses_before_any_device_call(L, entry, args, fragment):
    assert getattr(L, entry)(*args) == 1
    err = L.odam_last_error().decode()
    assert err.startswith(entry + ":"), err
    assert fragment in err, err


@pytest.mark.parametrize("entry,args", EMPTY, ids=["%s-%d" % (c[0], i) for i, c in enumerate(EMPTY)])
def test_entry_accepts_an_empty_extent(L, entry, args):
    assert getattr(L, entry)(*args) == 0


# ---- the restatements ---------------------------------------------------------------------------------------------------
def test_bf16_rounding_equals_torch():
    rng = np.random.default_rng(0)
    v = np.concatenate([ref.bf16_tie_values(rng, 4096), np.float32([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 3.3895314e38, 65280.0])])
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = ref.bf16_bits(v)
    assert np.array_equal(got, want)
    assert np.array_equal(ref.bf16_to_f32(got).view(np.uint32), torch.from_numpy(v).to(torch.bfloat16).float().numpy().view(np.uint32))
    ties = (v[:4096].view(np.uint32) & 0xffff) == 0x8000
    assert ties.sum() > 1000      # and both directions of a tie occur
    kept = v[:4096].view(np.uint32)[ties] >> 16
    assert np.array_equal(got[:4096][ties], ((kept + (kept & 1)) & 0xffff).astype(np.uint16)) and 0 < (kept & 1).mean() < 1


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 1, 8, 4), (1, 2, 2, 8), (3, 7, 4, 4), (1, 41, 8, 4)])
def test_pool_restatement_equals_torch(B, H, W, C):
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32) - np.float32(4.0)
    x[0, 0, 0, 0] = -np.inf
    want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ref.maxpool3x3s2(x).view(np.uint32), want.view(np.uint32))


def test_layout_restatements_place_every_element():
    img = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7) + 1
    a = ref.nchw_to_nhwc4(img, 0, False)
    assert a.shape == (2, 5, 7, 4) and a[1, 4, 6, 2] == img[1, 2, 4, 6] and not a[..., 3].any()
    b = ref.nchw_to_nhwc4(img, 1, False)
    assert b.shape == (2, 5, 7, 8) and b.dtype == np.uint16 and not b[..., 3:].any()
    assert np.array_equal(ref.bf16_to_f32(b[..., :3]), a[..., :3])      # small integers are exact in bf16
    for dt in (0, 1):
        c = ref.nchw_to_nhwc4(img, dt, True)
        assert c.shape == (2, 11, 15, 4)
        inner = c[:, 3:8, 3:10]
        assert np.array_equal(inner, a if dt == 0 else b[..., :4])
        frame = c.copy(); frame[:, 3:8, 3:10] = 0
        assert not frame.any() and c[1, 3, 3, 0] != 0 and c[1, 7, 9, 2] != 0
    assert np.array_equal(ref.nhwc_to_nchw(a, 0)[:, :3], img)


def _f32_sigmoid(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))


def test_sigmoid_bound_holds_for_a_float32_evaluation():
    x = np.concatenate([np.linspace(-104, 104, 200001).astype(np.float32), np.float32([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 88.72, -88.72])])
    v, b = ref.sigmoid(x)
    err = np.abs(_f32_sigmoid(x).astype(np.float64) - v)
    assert np.all(np.isfinite(b)) and np.all(err <= b + 2.0 ** -126)
    assert np.all(b <= 8 * ref.U * v + 2.0 ** -124)        # 2 (2 U e + U s + U s) / s^2 <= 8 U r: units in the last place, no blanket tolerance
    # a value-only mistake is outside it: exp(-x) taken as exp2(-x), and a one-sided rounding of the result by two ulps
    with np.errstate(over="ignore"):
        wrong = np.float32(1) / (np.float32(1) + np.exp2(-x[:200001], dtype=np.float32))
    mid = (np.abs(x[:200001]) < 16) & (np.abs(x[:200001]) > 1e-3)      # beyond 16 the result is 1 to the last bit either way
    assert np.mean((np.abs(wrong.astype(np.float64) - v[:200001]) > b[:200001] + 2.0 ** -126)[mid]) > 0.99
    got = _f32_sigmoid(x[:200001][mid])
    off = (got.view(np.uint32) + np.uint32(16)).view(np.float32)        # sixteen units in the last place up: outside 8 U r
    assert np.all(np.abs(off.astype(np.float64) - v[:200001][mid]) > b[:200001][mid] + 2.0 ** -126)


def _f32_postprocess(lg, bx, an, of, sz, dp, K9, img_w, img_h):
    """the kernel's operation sequence in numpy float32 (no contraction)"""
    f = np.float32
    n, n_cls1 = lg.shape
    mx = lg.max(1, keepdims=True)
    e = np.exp(lg - mx, dtype=f)
    den = np.zeros(n, f)
    for c in range(n_cls1):
        den = den + e[:, c]
    p = e[:, :-1] / den[:, None]
    rows = np.zeros((n, 16), f)
    rows[:, 0] = p.max(1); rows[:, 1] = p.argmax(1)
    w, h = f(img_w), f(img_h)
    x0 = (bx[:, 0] - f(0.5) * bx[:, 2]) * w; y0 = (bx[:, 1] - f(0.5) * bx[:, 3]) * h
    x1 = (bx[:, 0] + f(0.5) * bx[:, 2]) * w; y1 = (bx[:, 1] + f(0.5) * bx[:, 3]) * h
    scx = of[:, 0] * w + (x0 + x1) / f(2); scy = of[:, 1] * h + (y0 + y1) / f(2)
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = x0, y0, x1, y1
    rows[:, 6] = ((scx - K9[2]) / K9[0]) * dp; rows[:, 7] = ((scy - K9[5]) / K9[4]) * dp
    rows[:, 8] = dp; rows[:, 9] = an.argmax(1); rows[:, 10:13] = sz
    return rows


def _random_heads(rng, n, n_cls1, n_bins):
    f = np.float32
    return ((rng.standard_normal((n, n_cls1)) * 3).astype(f), rng.uniform(0.02, 0.98, (n, 4)).astype(f),
            (rng.standard_normal((n, n_bins)) * 3).astype(f), (rng.standard_normal((n, 2)) * 0.1).astype(f),
            rng.uniform(0.1, 3.0, (n, 3)).astype(f), rng.uniform(0.3, 8.0, n).astype(f))


@pytest.mark.parametrize("n_cls1,n_bins", [(2, 1), (10, 12), (19, 24)])
def test_postprocess_bound_holds_for_a_float32_evaluation(n_cls1, n_bins):
    rng = np.random.default_rng(n_cls1)
    heads = _random_heads(rng, 20000, n_cls1, n_bins)
    K9 = K.astype(np.float32).reshape(9)
    r = ref.postprocess(*heads, K9, 640, 480)
    got = _f32_postprocess(*heads, K9, 640, 480).astype(np.float64)
    assert np.all(np.abs(got - r["rows"]) <= r["bound"])
    exact = [1, 8, 9, 10, 11, 12, 13, 14, 15]
    assert not r["bound"][:, exact].any()
    # the bounds are a few units in the last place of the column's own scale
    assert np.all(r["bound"][:, 0] <= (8 + 4 * n_cls1) * ref.U)
    assert np.all(r["bound"][:, 2:6] <= 8 * ref.U * 640)
    # the skipped share of the class comparison (issue: none at 8 U, under 5e-5 at 1e-5)
    assert np.mean(r["gap"] <= r["bound"][:, 0]) <= 1e-3


def test_postprocess_restatement_reproduces_the_reference_golden(golden):
    """tests/golden/detr_post.npz: the reference's DETR.postprocess (threshold 0.6, its own nms_3d) on four frames of head outputs.
    Classes and angle bins equal; every other column within the restatement's bound (the reference runs the same float32 operations
    in torch) plus the rounding of the fixture's float32, U |value|."""
    from odam_amd import _lib
    z = golden("detr_post.npz")
    K9 = K.astype(np.float32).reshape(9)
    for b in range(4):
        lg, bx, an, of, sz, dp = [z[k][b].reshape(100, -1) for k in KEYS]
        r = ref.postprocess(lg, bx, an, of, sz, dp.reshape(100), K9, 640, 480)
        rows32 = np.ascontiguousarray(r["rows"], np.float32)      # threshold + greedy NMS as the library's host code does them
        keep = np.zeros(100, np.int32); nk = ctypes.c_int()
        _lib.check(_lib.lib().odam_detr_select(rows32.ctypes.data_as(_lib.c_float_p), 100, FL(0.6), 1,
                                               keep.ctypes.data_as(_lib.c_int_p), ctypes.byref(nk)), "odam_detr_select")
        keep = keep[:nk.value]
        assert len(keep) == len(z[f"post{b}_classes"]) > 0
        assert np.array_equal(r["cls"][keep], z[f"post{b}_classes"])
        assert np.array_equal((r["ab"][keep] * np.float32(180 / 30)).astype(np.float32), z[f"post{b}_angles"])
        want = {"scores": (slice(0, 1), (-1,)), "bboxes": (slice(2, 6), (-1, 2, 2)), "translates": (slice(6, 9), (-1, 3)),
                "dimensions": (slice(10, 13), (-1, 3))}
        for name, (cols, shape) in want.items():
            v = r["rows"][keep][:, cols].reshape(shape) if name != "scores" else r["rows"][keep, 0]
            bd = r["bound"][keep][:, cols].reshape(shape) if name != "scores" else r["bound"][keep, 0]
            fix = z[f"post{b}_{name}"].astype(np.float64)
            assert fix.shape == v.shape
            assert np.all(np.abs(fix - v) <= bd + ref.U * np.abs(v)), (b, name, np.abs(fix - v).max())
