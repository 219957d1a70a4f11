"""Plain numpy restatements of the detector's kernels that are not contractions (odam_amd/csrc/detr_kernels.hip: maxpool,
nchw_to_nhwc4 plain and framed, nhwc_to_nchw, add_pos, to_f32, sigmoid, postprocess), as include/odam_detr.h describes them.

Exact kernels (pool, layouts, convert, position add) return the expected BITS: float32 arrays, or uint16 arrays of raw bfloat16.
The position add in bf16 is one float32 addition followed by one rounding to nearest even.

sigmoid and postprocess return the float64 value and a BOUND on |fp32 kernel - float64|, by a running error analysis of the kernel's
own sequence of float32 operations.  With U = 2^-24 (the unit roundoff: a correctly rounded result z carries at most U |z|):

  * every float32 operation adds U |its float64 result| to the error its inputs bring along, and the inputs' errors go through the
    operation to first order (a + b: ea + eb;  a * b: ea |b| + eb |a|;  a / b: ea / |b| + eb |a / b| / |b|;  exp(a): ea exp(a));
  * expf counts as one ulp of its result, 2 U |result| (an ulp is at most 2^-23 of the value);
  * an expf or a quotient may underflow: below 2^-126 a float32 loses bits or is flushed to zero, so each carries 2^-126 absolute;
  * operations that are exact in float32 add nothing: negation, a product with 0.5, a quotient by 2, max, a copy;
  * the total is doubled: the first-order terms above use the float64 magnitudes where the kernel has its own rounded ones.

A multiply-add counts as a multiply and an add, two roundings: a compiler that contracts the pair into one fused operation rounds
once, which the same sum covers.  Nothing here is computed from a kernel's output."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


# ---- bfloat16 as raw uint16 --------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> raw bfloat16, round to nearest even (finite values and infinities)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_tie_values(rng, shape):
    """float32 values of both signs, a third of them exactly half way between two neighbouring bfloat16 (the low 16 bits are 0x8000:
    nearest-even decides, up where the kept mantissa is odd, down where it is even) and a third one float32 ulp off such a tie"""
    v = rng.standard_normal(shape).astype(np.float32) * np.float32(3.0)
    u = v.view(np.uint32).copy()
    kind = rng.integers(0, 3, shape)
    off = rng.integers(0, 2, shape).astype(np.uint32) * np.uint32(2) + np.uint32(0x7fff)      # 0x7fff or 0x8001
    u = np.where(kind == 1, (u & np.uint32(0xffff0000)) | np.uint32(0x8000), u)
    u = np.where(kind == 2, (u & np.uint32(0xffff0000)) | off, u)
    return u.astype(np.uint32).view(np.float32)


# ---- exact kernels -----------------------------------------------------------------------------------------------------
def maxpool3x3s2(x):
    """x [B,H,W,C] float -> [B,Ho,Wo,C]: window 3, stride 2, padding 1 with -inf; no NaNs"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = np.full((B, H + 2, W + 2, C), -np.inf, x.dtype)
    p[:, 1:H + 1, 1:W + 1] = x
    out = np.full((B, Ho, Wo, C), -np.inf, x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, p[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2][:, :Ho, :Wo])
    return out


def nchw_to_nhwc4(img, dtype, framed):
    """img [B,3,H,W] float32 -> the stem's input layout (include/odam_detr.h, odam_op_nchw_to_nhwc4): float32, or uint16 bfloat16"""
    B, _, H, W = img.shape
    px = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1)), np.float32)
    if framed:
        out = np.zeros((B, H + 6, W + 8, 4), np.float32)
        out[:, 3:H + 3, 3:W + 3, :3] = px
    else:
        out = np.zeros((B, H, W, 8 if dtype == 1 else 4), np.float32)
        out[..., :3] = px
    return bf16_bits(out) if dtype == 1 else out


def nhwc_to_nchw(x, dtype):
    """x [B,H,W,C] float32 or uint16 bfloat16 -> [B,C,H,W] float32"""
    v = bf16_to_f32(x) if dtype == 1 else np.asarray(x, np.float32)
    return np.ascontiguousarray(np.transpose(v, (0, 3, 1, 2)))


def add_pos(x, pos, M, dtype):
    """x [M,C] (float32, uint16 bfloat16, or None), pos [L,C] float32 -> out [M,C] float32 / uint16: one float32 add, then RNE"""
    p = np.asarray(pos, np.float32)[np.arange(M) % pos.shape[0]]
    if x is not None:
        p = (bf16_to_f32(x) if dtype == 1 else np.asarray(x, np.float32)) + p      # numpy float32 addition is the IEEE one
    return bf16_bits(p) if dtype == 1 else p.astype(np.float32)


def to_f32(x, dtype):
    return bf16_to_f32(x) if dtype == 1 else np.asarray(x, np.float32).copy()


# ---- float64 values with running error bounds --------------------------------------------------------------------------
def sigmoid(x):
    """x float32 -> (float64 1 / (1 + exp(-x)), bound).  Kernel: e = expf(-x); s = 1 + e; r = 1 / s."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-x)
        s = 1.0 + e
        r = 1.0 / s
        err_e = 2 * U * e + TINY
        err_s = err_e + U * s
        err_r = err_s / (s * s) + U * r + TINY
    # e = +inf (x = -inf): the kernel's 1 / (1 + inf) is exactly 0, as here
    return r, np.where(np.isfinite(e), 2.0 * err_r, 0.0)


def postprocess(logits, boxes, angle, offset, size, depth, K9, img_w, img_h):
    """float32 inputs -> dict(rows [n,16] float64, bound [n,16], cls [n], ab [n], gap [n], tie [n]).

    rows / bound: as postprocess_kernel writes them; bound 0 marks an exact column (class, angle bin, depth, size, padding).
    cls / ab: first index of the largest foreground probability / angle logit.  gap: the float64 distance between the two largest
    foreground probabilities (inf with one foreground class); tie: the two largest foreground LOGITS are equal, so that the
    probabilities are equal in any arithmetic and the first one must win."""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    n, n_cls1 = lg.shape
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    bx, an, of, sz, dp = f(boxes).reshape(n, 4), f(angle).reshape(n, -1), f(offset).reshape(n, 2), f(size).reshape(n, 3), f(depth).reshape(n)
    K9 = f(K9).reshape(9)
    fx, fy, cx, cy = K9[0], K9[4], K9[2], K9[5]
    img_w, img_h = float(np.float32(img_w)), float(np.float32(img_h))
    rows = np.zeros((n, 16)); bound = np.zeros((n, 16))

    # softmax: t = lg - mx; e = expf(t); den = sum in class order; p = e / den
    mx = lg.max(1, keepdims=True)
    t = lg - mx
    err_t = U * np.abs(t)
    e = np.exp(t)
    err_e = err_t * e + 2 * U * e + TINY
    den = np.zeros(n); err_den = np.zeros(n)
    for c in range(n_cls1):
        den = den + e[:, c]
        err_den = err_den + err_e[:, c] + U * den       # the first add, 0 + e, is exact: U den on it only widens
    p = e / den[:, None]
    err_p = err_e / den[:, None] + p * err_den[:, None] / den[:, None] + U * p + TINY
    fg, err_fg = p[:, :-1], err_p[:, :-1]
    cls = fg.argmax(1)
    rows[:, 0] = fg.max(1); bound[:, 0] = 2.0 * err_fg.max(1)
    rows[:, 1] = cls
    if n_cls1 > 2:
        top = np.sort(fg, 1)
        gap = top[:, -1] - top[:, -2]
        ltop = np.sort(lg[:, :-1], 1)
        tie = ltop[:, -1] == ltop[:, -2]
    else:
        gap = np.full(n, np.inf); tie = np.zeros(n, bool)

    # box corners: a = c -+ 0.5 w (the product is exact), corner = a * extent
    def corner(c, w, sign, ext):
        a = c + sign * 0.5 * w
        v = a * ext
        return v, (U * np.abs(a)) * abs(ext) + U * np.abs(v)
    x0, ex0 = corner(bx[:, 0], bx[:, 2], -1.0, img_w); y0, ey0 = corner(bx[:, 1], bx[:, 3], -1.0, img_h)
    x1, ex1 = corner(bx[:, 0], bx[:, 2], +1.0, img_w); y1, ey1 = corner(bx[:, 1], bx[:, 3], +1.0, img_h)
    for k, (v, ev) in enumerate(((x0, ex0), (y0, ey0), (x1, ex1), (y1, ey1))):
        rows[:, 2 + k] = v; bound[:, 2 + k] = 2.0 * ev

    # 3D centre: sc = off * extent + (lo + hi) / 2;  c3 = ((sc - c) / f) * d
    def centre(off, ext, lo, elo, hi, ehi, c0, f0):
        m = off * ext; em = U * np.abs(m)
        s = lo + hi; es = elo + ehi + U * np.abs(s)
        sc = m + s / 2.0; esc = em + es / 2.0 + U * np.abs(sc)
        u = sc - c0; eu = esc + U * np.abs(u)
        v = u / f0; ev = eu / abs(f0) + U * np.abs(v) + TINY
        c3 = v * dp
        return c3, ev * np.abs(dp) + U * np.abs(c3)
    c3x, ecx = centre(of[:, 0], img_w, x0, ex0, x1, ex1, cx, fx)
    c3y, ecy = centre(of[:, 1], img_h, y0, ey0, y1, ey1, cy, fy)
    rows[:, 6] = c3x; bound[:, 6] = 2.0 * ecx
    rows[:, 7] = c3y; bound[:, 7] = 2.0 * ecy
    rows[:, 8] = dp
    ab = an.argmax(1)
    rows[:, 9] = ab
    rows[:, 10:13] = sz
    return dict(rows=rows, bound=bound, cls=cls, ab=ab, gap=gap, tie=tie)
