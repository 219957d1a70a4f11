"""The detector's kernels that are not contractions (odam_amd/csrc/detr_kernels.hip: maxpool, nchw_to_nhwc4 plain and framed,
nhwc_to_nchw, add_pos / add_pos_c, to_f32, sigmoid, postprocess), one launch at a time through their odam_op_* entries
(include/odam_detr.h), against tests/detr_elementwise_ref.py:

  * pool, layouts, convert and the position add bit for bit (the pool against torch.nn.functional.max_pool2d on the same values);
  * sigmoid and postprocess against float64 within the restatement's running error bound, which is derived from the kernel's
    operation sequence alone (never from an output); class and angle bin as integers, ties by rule (the first maximum wins);
  * every output buffer is longer than the kernel owns and pre-filled with a NaN bit pattern no result can have: the tail must be
    untouched and every owned word written -- zero channels and frame pixels included.

NaN inputs of the pool are outside the contract (include/odam_detr.h).  max err / bound of the two bounded kernels is recorded under
detr.sigmoid.err_over_bound and detr.postprocess.<columns>.err_over_bound (profiles/detr_elementwise_test_measured.json)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detr_elementwise_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96                   # words behind what the kernel owns
S32 = 0x7fc5a5a5             # a quiet NaN: no kernel here produces one from these inputs
S16 = 0x7fa5                 # the same for bfloat16
FL = ctypes.c_float
LL = ctypes.c_longlong


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _lib():
    from odam_amd import _lib as m
    return m


def _call(entry, *args):
    m = _lib()
    m.check(getattr(m.lib(), entry)(*args), entry)


def _dev(a):
    """numpy float32 / uint16 (raw bfloat16) / uint8 -> device tensor of the same bits"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def _ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded(n, dtype):
    """n + GUARD words of the sentinel: int32 (fp32 outputs) or int16 (bf16 outputs)"""
    if dtype == 1:
        return torch.full((n + GUARD,), S16, dtype=torch.int16, device=DEV)
    return torch.full((n + GUARD,), S32, dtype=torch.int32, device=DEV)


def _bits(buf):
    a = buf.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32)


def _expect_bits(want):
    want = np.ascontiguousarray(want)
    return want.view(np.uint32) if want.dtype == np.float32 else want


def _assert_owned_and_tail(buf, want, what):
    """the first want.size words equal `want` bit for bit (so each was written: the sentinel is no expected value), the rest untouched"""
    got = _bits(buf)
    w = _expect_bits(want).reshape(-1)
    sent = S16 if got.dtype == np.uint16 else S32
    assert not (w == sent).any()
    n = w.size
    assert np.array_equal(got[n:], np.full(GUARD, sent, got.dtype)), f"{what}: wrote behind its output"
    bad = np.flatnonzero(got[:n] != w)
    assert bad.size == 0, f"{what}: {bad.size} of {n} words differ, first at {bad[0]}: got {got[bad[0]]:#x} want {w[bad[0]]:#x}" + \
        (" (never written)" if got[bad[0]] == sent else "")


def _values(rng, shape, dtype):
    """float32 with bf16 rounding ties and both signs; dtype 1: raw bfloat16 of them"""
    v = ref.bf16_tie_values(rng, shape)
    return ref.bf16_bits(v) if dtype == 1 else v


def _widen(a, dtype):
    return ref.bf16_to_f32(a) if dtype == 1 else a


# ---- max-pool ------------------------------------------------------------------------------------------------------------
# H, W from {1, 2, 3, 4, 7, 8, 41} in odd / even mixes, C from {4, 8, 64, 68}; the last three: B Ho Wo C / 4 = 255, 256, 257 float4 groups
POOL_CASES = [(1, 1, 1, 4), (1, 1, 8, 8), (3, 2, 2, 4), (1, 3, 4, 64), (3, 4, 7, 68), (1, 7, 8, 4), (1, 8, 3, 68), (3, 41, 2, 8),
              (1, 8, 41, 64), (3, 7, 41, 4), (1, 2, 1, 64), (3, 1, 9, 68), (1, 8, 8, 64), (1, 1, 513, 4)]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,H,W,C", POOL_CASES)
def test_maxpool_bit_for_bit(B, H, W, C, dtype):
    rng = np.random.default_rng(B * 1000 + H * 50 + W + C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if (B, H, W, C) in POOL_CASES[-3:]:
        assert B * Ho * Wo * C // 4 == {9: 255, 8: 256, 513: 257}[W]
    base = rng.standard_normal((B, H, W, C)).astype(np.float32) * np.float32(2.0)
    negative = -np.abs(base) - np.float32(0.125)             # every window maximum is negative: a zero pad would win
    holes = base.copy()
    holes[rng.random(base.shape) < 0.4] = -np.inf             # whole windows of -inf occur at the small sizes
    holes[0, 0, 0, :] = -np.inf
    for name, x in (("random", base), ("negative", negative), ("-inf", holes)):
        xin = ref.bf16_bits(x) if dtype == 1 else x
        xv = _widen(xin, dtype)
        want = F.max_pool2d(torch.from_numpy(xv).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().numpy()
        assert want.shape == (B, Ho, Wo, C)
        if name == "negative":
            assert (want < 0).all()
        want = ref.bf16_bits(want) if dtype == 1 else want      # exact: a maximum of bf16 values is one of them
        dx, dy = _dev(xin), _guarded(want.size, dtype)
        _call("odam_op_maxpool3x3s2_nhwc_ex", _ptr(dx), _ptr(dy), B, H, W, C, dtype, _st())
        _assert_owned_and_tail(dy, want, f"maxpool {name}")
    if dtype == 0:      # the fp32 entry is the same launch
        dy2 = _guarded(want.size, 0)
        _call("odam_op_maxpool3x3s2_nhwc", _ptr(dx), _ptr(dy2), B, H, W, C, _st())
        assert np.array_equal(_bits(dy2), _bits(dy))


# ---- layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framed", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7), (3, 16, 16), (1, 31, 33)])
def test_nchw_to_nhwc4_bit_for_bit(B, H, W, dtype, framed):
    rng = np.random.default_rng(B * 100 + H + 7 * framed)
    first, second = ref.bf16_tie_values(rng, (B, 3, H, W)), ref.bf16_tie_values(rng, (B, 3, H, W))
    assert (first < 0).any() or first.size < 8
    want1, want2 = ref.nchw_to_nhwc4(first, dtype, framed), ref.nchw_to_nhwc4(second, dtype, framed)
    assert want1.shape == ((B, H + 6, W + 8, 4) if framed else (B, H, W, 8 if dtype == 1 else 4))
    out = _guarded(want1.size, dtype)
    for img, want in ((first, want1), (second, want2)):      # the second call into the SAME buffer: nothing of the first remains
        d_in = _dev(img)
        _call("odam_op_nchw_to_nhwc4", _ptr(d_in), _ptr(out), B, H, W, dtype, framed, _st())
        _assert_owned_and_tail(out, want, f"nchw_to_nhwc4 framed={framed}")
        got = _bits(out)[:want.size].reshape(want.shape)
        assert not got[..., 3:].any()                          # +0.0, not -0.0, in every padding channel
        if framed:
            fr = got.copy(); fr[:, 3:H + 3, 3:W + 3] = 0
            assert not fr.any()                                # every frame pixel is +0.0
    assert not np.array_equal(want1, want2)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [4, 5, 64, 2048])
def test_nhwc_to_nchw_bit_for_bit(C, dtype):
    rng = np.random.default_rng(C + dtype)
    for B in (1, 2):
        for H, W in ((1, 1), (5, 7), (16, 16), (1, 257)):      # HW = 1, 35, 256, 257
            x = _values(rng, (B, H, W, C), dtype)
            want = ref.nhwc_to_nchw(x, dtype)
            out = _guarded(want.size, 0)
            dx = _dev(x)
            _call("odam_op_nhwc_to_nchw", _ptr(dx), _ptr(out), B, H, W, C, dtype, _st())
            _assert_owned_and_tail(out, want, f"nhwc_to_nchw B={B} HW={H * W}")


# ---- position add: C = 256 runs add_pos_kernel, every other C add_pos_c_kernel; each against the restatement on its own ---------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [256, 4, 128, 252, 260, 384, 512])
def test_add_pos_bit_for_bit(C, dtype):
    rng = np.random.default_rng(C * 2 + dtype)
    crossed, ties = set(), 0
    for L in (1, 7, 100):
        pos = ref.bf16_tie_values(rng, (L, C))
        d_pos = _dev(pos)
        for M in sorted({1, L, 3 * L, 3 * L + 1}):
            x = _values(rng, (M, C), dtype)
            if dtype == 1 and L == 7:
                # sums that land exactly between two bfloat16 in the first rows: pos = tie - x, wherever that difference is exact
                k = min(M, L)
                pos = pos.copy()
                pos[:k] = ref.bf16_tie_values(rng, (k, C)) - ref.bf16_to_f32(x[:k])
                d_pos = _dev(pos)
            for with_x in (True, False):
                want = ref.add_pos(x if with_x else None, pos, M, dtype)
                if dtype == 1 and with_x:
                    s = ref.bf16_to_f32(x) + pos[np.arange(M) % L]
                    ties += int(((s.view(np.uint32) & 0xffff) == 0x8000).sum())
                out = _guarded(want.size, dtype)
                dx = _dev(x) if with_x else None
                _call("odam_op_add_pos", _ptr(dx), _ptr(d_pos), L, _ptr(out), M, C, dtype, _st())
                _assert_owned_and_tail(out, want, f"add_pos C={C} L={L} M={M} x={'yes' if with_x else 'null'}")
            crossed.add(M * C // 4 > 256)
    assert crossed == {False, True}        # launches of one block and of several
    if dtype == 1:
        assert ties > 0                    # nearest-even was exercised on exact ties


# ---- convert ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_to_f32_bit_for_bit_and_refuses_a_tail(dtype):
    rng = np.random.default_rng(dtype)
    m = _lib()
    for n in (4, 1020, 1024, 1028):
        x = _values(rng, n, dtype)
        out = _guarded(n, 0)
        dx = _dev(x)
        _call("odam_op_to_f32", _ptr(dx), _ptr(out), LL(n), dtype, _st())
        _assert_owned_and_tail(out, ref.to_f32(x, dtype), f"to_f32 n={n}")
    x = _values(rng, 1024, dtype)
    out = _guarded(1024, 0)
    dx = _dev(x)
    assert m.lib().odam_op_to_f32(_ptr(dx), _ptr(out), LL(1023), dtype, _st()) == 1
    assert m.lib().odam_last_error().decode().startswith("odam_op_to_f32:")
    torch.cuda.synchronize()
    assert (_bits(out) == S32).all()       # refused whole: not 1020 elements converted and three dropped


# ---- sigmoid ---------------------------------------------------------------------------------------------------------------
def _sigmoid_inputs():
    f = np.float32
    grid = np.linspace(-104.0, 104.0, 1 << 17, dtype=np.float64).astype(f)
    near = []
    # where expf saturates (ln FLT_MAX = 88.7228), leaves the normal range (ln 2^126 = 87.3365) and the denormal range (ln 2^149 = 103.279)
    for c in (88.72, 88.72283905206835, 87.33654475055311, 103.27892990343185, 16.635532, 17.328680):
        for s in (-1.0, 1.0):
            v = f(s * c)
            lo = hi = v
            near.append(v)
            for _ in range(8):
                lo, hi = np.nextafter(lo, f(-np.inf)), np.nextafter(hi, f(np.inf))
                near += [lo, hi]
    special = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38]
    return np.concatenate([grid, np.asarray(near, f), np.asarray(special, f)])


def _run_sigmoid(x):
    buf = _guarded(x.size, 0)
    buf[:x.size] = _dev(x).view(torch.int32)
    _call("odam_op_sigmoid", _ptr(buf), int(x.size), _st())
    got = _bits(buf)
    assert (got[x.size:] == S32).all(), "sigmoid: wrote behind its output"
    return got[:x.size].view(np.float32)


def test_sigmoid_within_bound(measured):
    x = _sigmoid_inputs()
    v, b = ref.sigmoid(x)
    got = _run_sigmoid(x)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - v)
    ratio = err / (b + 2.0 ** -126)
    worst = int(ratio.argmax())
    print(f"sigmoid: max err / bound {ratio.max():.4f} at x = {x[worst]!r}: got {got[worst]!r}, float64 {v[worst]!r}")
    measured("detr.sigmoid.err_over_bound", ratio.max())
    assert ratio.max() <= 1.0, (x[worst], got[worst], v[worst], b[worst])
    assert got[np.isposinf(x)].tolist() == [1.0] and got[np.isneginf(x)].tolist() == [0.0]
    assert (got[x == 0] == 0.5).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sigmoid_block_boundaries(n, measured):
    x = np.random.default_rng(n).uniform(-20, 20, n).astype(np.float32)
    v, b = ref.sigmoid(x)
    got = _run_sigmoid(x)
    ratio = np.abs(got.astype(np.float64) - v) / (b + 2.0 ** -126)
    measured("detr.sigmoid.err_over_bound", ratio.max())
    assert ratio.max() <= 1.0


# ---- postprocess -----------------------------------------------------------------------------------------------------------
INTRINSICS = {"640x480": (640, 480, [[577.87, 0.0, 319.5], [0.0, 577.87, 239.5], [0.0, 0.0, 1.0]]),
              "1296x968": (1296, 968, [[1169.62, 0.0, 646.295], [0.0, 1167.11, 489.927], [0.0, 0.0, 1.0]])}
GROUPS = {"score": [0], "box": [2, 3, 4, 5], "centre": [6, 7]}
EXACT = [8, 10, 11, 12]


def _heads(rng, n, n_cls1, n_bins):
    f = np.float32
    return [(rng.standard_normal((n, n_cls1)) * 3).astype(f), rng.uniform(0.0, 1.0, (n, 4)).astype(f),
            (rng.standard_normal((n, n_bins)) * 3).astype(f), (rng.standard_normal((n, 2)) * 0.1).astype(f),
            rng.uniform(0.05, 4.0, (n, 3)).astype(f), rng.uniform(0.2, 10.0, n).astype(f)]


def _run_postprocess(heads, n_cls1, n_bins, size):
    img_w, img_h, Kmat = INTRINSICS[size]
    K9 = np.ascontiguousarray(np.asarray(Kmat, np.float64), np.float32).reshape(9)
    n = heads[0].shape[0]
    dev = [_dev(h) for h in heads]
    rows = _guarded(n * 16, 0)
    _call("odam_op_postprocess", *[_ptr(t) for t in dev], n, n_cls1, n_bins, K9.ctypes.data_as(ctypes.c_void_p), FL(img_w), FL(img_h),
          _ptr(rows), _st())
    bits = _bits(rows)
    assert (bits[n * 16:] == S32).all(), "postprocess: wrote behind its rows"
    assert not (bits[:n * 16] == S32).any(), "postprocess: a word of its rows was never written"
    r = ref.postprocess(*heads, K9, img_w, img_h)
    return bits[:n * 16].reshape(n, 16), r


def _check_rows(bits, r, heads, measured, by_rule=None):
    """bits [n,16] uint32 of the kernel's rows against the restatement r; returns the share of rows whose class was not compared"""
    got = bits.view(np.float32).astype(np.float64)
    rows, bound = r["rows"], r["bound"]
    assert not np.isnan(got).any()
    assert not bits[:, 13:16].any()                                             # +0.0
    assert np.array_equal(bits[:, EXACT], np.ascontiguousarray(rows[:, EXACT], np.float32).view(np.uint32))   # copies of the inputs
    gi = bits.view(np.float32)[:, [1, 9]].astype(np.int64)
    assert np.array_equal(gi.astype(np.float32), bits.view(np.float32)[:, [1, 9]])      # whole numbers
    assert np.array_equal(gi[:, 1], r["ab"]), "angle bin: the first largest angle logit"
    err = np.abs(got - rows)
    for name, cols in GROUPS.items():
        e, bd = err[:, cols], bound[:, cols]
        assert not e[bd == 0].any(), name
        ratio = np.where(bd > 0, e / np.where(bd > 0, bd, 1.0), 0.0)
        print(f"postprocess {name}: max err / bound {ratio.max():.4f}")
        measured(f"detr.postprocess.{name}.err_over_bound", ratio.max())
        assert ratio.max() <= 1.0, (name, np.unravel_index(ratio.argmax(), ratio.shape), e.max())
    # the class where float64 separates the two best foreground classes by more than the score's bound (each of the two
    # probabilities is off by at most half of it); exact ties of the logits by rule: the first one wins
    clear = (r["gap"] > bound[:, 0]) | r["tie"]
    if by_rule is not None:
        clear = clear | by_rule
    assert np.array_equal(gi[clear, 0], r["cls"][clear]), "class"
    assert ((gi[:, 0] >= 0) & (gi[:, 0] < heads[0].shape[1] - 1)).all()
    return 1.0 - clear.mean()


@pytest.mark.parametrize("size", list(INTRINSICS))
@pytest.mark.parametrize("n_cls1,n_bins", [(2, 1), (10, 12), (19, 24)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_postprocess_within_bound(n, n_cls1, n_bins, size, measured):
    rng = np.random.default_rng(n * 100 + n_cls1 + len(size))
    heads = _heads(rng, n, n_cls1, n_bins)
    bits, r = _run_postprocess(heads, n_cls1, n_bins, size)
    skipped = _check_rows(bits, r, heads, measured)
    measured("detr.postprocess.class_skipped_share", skipped)
    assert skipped <= 0.01


@pytest.mark.parametrize("size", list(INTRINSICS))
@pytest.mark.parametrize("n_cls1,n_bins", [(2, 1), (10, 12), (19, 24)])
def test_postprocess_hand_made_rows(n_cls1, n_bins, size, measured):
    rng = np.random.default_rng(n_cls1)
    n = 70                                           # two blocks of 64 threads; the hand-made rows straddle the boundary
    heads = _heads(rng, n, n_cls1, n_bins)
    lg, bx, an, of, sz, dp = heads
    fg = n_cls1 - 1
    a, b2 = (1 % fg, (fg - 1)), (2 % n_bins, n_bins - 1)
    # 60: equal top logits (class a[0] and the last foreground class; angle bins b2[0] and the last): the first wins
    lg[60] = -1.0; lg[60, a[0]] = 5.0; lg[60, a[1]] = 5.0
    an[60] = -2.0; an[60, b2[0]] = 4.0; an[60, b2[1]] = 4.0
    # 61: the same with the first and the last of each
    lg[61] = rng.standard_normal(n_cls1) - 3.0; lg[61, 0] = 2.5; lg[61, fg - 1] = 2.5
    an[61] = rng.standard_normal(n_bins) - 3.0; an[61, 0] = 1.25; an[61, n_bins - 1] = 1.25
    # 62: "no object" is the largest logit: the class is still the best FOREGROUND class
    lg[62, fg] = 10.0
    # 63: all logits equal, all angle logits equal: class 0, bin 0, score 1 / n_cls1
    lg[63] = 1.5; an[63] = -0.75
    # 64, 65: logits of +-80, alternating, and "no object" at +80 with every class at -80 (the score underflows float32)
    lg[64] = np.where(np.arange(n_cls1) % 2 == 0, 80.0, -80.0)
    lg[65] = -80.0; lg[65, fg] = 80.0
    # 66: a zero-size box; 67: depth 0; 68: both, at the image corner
    bx[66, 2:] = 0.0
    dp[67] = 0.0
    bx[68] = (1.0, 1.0, 0.0, 0.0); dp[68] = 0.0
    bits, r = _run_postprocess(heads, n_cls1, n_bins, size)
    by_rule = np.zeros(n, bool); by_rule[[60, 61, 63, 64, 65]] = True        # exact ties (or none at all): first maximum, asserted
    _check_rows(bits, r, heads, measured, by_rule)
    got = bits.view(np.float32)
    assert got[60, 1] == a[0] and got[60, 9] == b2[0]
    assert got[61, 1] == 0 and got[61, 9] == 0
    assert got[62, 1] < fg and got[62, 1] == int(lg[62, :fg].argmax())
    assert got[63, 1] == 0 and got[63, 9] == 0 and abs(float(got[63, 0]) - 1.0 / n_cls1) <= 4 * ref.U
    assert got[64, 1] == 0
    assert got[65, 1] == 0 and 0.0 <= got[65, 0] <= 2.0 ** -126
    assert got[66, 2] == got[66, 4] and got[66, 3] == got[66, 5]
    assert got[67, 6] == 0 and got[67, 7] == 0 and got[67, 8] == 0
    assert got[68, 6] == 0 and got[68, 7] == 0 and got[68, 2] == INTRINSICS[size][0] and got[68, 5] == INTRINSICS[size][1]
