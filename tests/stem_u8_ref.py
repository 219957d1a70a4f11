"""The uint8 stem in numpy float64 (odam_amd/csrc/stem_u8_fold.h, detr_kernels.hip preprocess_u8_bf16x4_framed_kernel, detr_forward.hip
stem_from_u8): Pillow's 8-bit bilinear resize, the integer centres, the folded filters, the framed bf16 image, and the truth the GPU
tests compare with -- the real chain s * sum w (u / 255 - mean) / std + b -> ReLU -> max-pool, every input taken as the exact value of
its fp32 / uint8 form."""
import numpy as np


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _coeffs(in_size, out_size):
    """Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc, bilinear: (xmin, cnt, K [out][ksize] int, 22 fractional bits)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    xmin, cnt, K = np.zeros(out_size, int), np.zeros(out_size, int), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = np.array([max(0.0, 1.0 - abs((x + lo - center + 0.5) * (1.0 / fs))) for x in range(hi - lo)])
        if w.sum() != 0.0:
            w = w / w.sum()
        K[xx, :hi - lo] = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
        xmin[xx], cnt[xx] = lo, hi - lo
    return xmin, cnt, K


def _pass(img, out_size, axis):
    """one integer pass along `axis` of a uint8 array: clip8((2^21 + sum px K) >> 22)"""
    if img.shape[axis] == out_size:
        return img
    xmin, cnt, K = _coeffs(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        k = K[xx, :cnt[xx]].reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = ((1 << 21) + (src[xmin[xx]:xmin[xx] + cnt[xx]] * k).sum(0)) >> 22
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_u8(frames, H, W):
    """uint8 [B, h, w, 3] -> [B, H, W, 3] as PIL's Image.resize(BILINEAR): the horizontal pass, then the vertical one; an axis that already
    has its size is not resampled"""
    return _pass(_pass(frames, W, 2), H, 1)


def centres(mean):
    """c_k = lrint(255 mean_k) in double (round half to even, as lrint in the default rounding mode)"""
    return np.rint(255.0 * np.asarray(mean, np.float32).astype(np.float64)).astype(np.int64)


def fold(w, mean, std):
    """conv1 [Cout, 3, 7, 7] fp32 -> the folded filters [Cout, 7, 8, 4] in float64 (before their one rounding to fp32): k = 0..2 the channels
    over 255 std, k = 3 what the indicator multiplies; the kx = 7 slot zero"""
    w = np.asarray(w, np.float32).astype(np.float64)
    mean, std = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    c = centres(mean).astype(np.float64)
    out = np.zeros((w.shape[0], 7, 8, 4))
    out[:, :, :7, :3] = (w / (255.0 * std)[None, :, None, None]).transpose(0, 2, 3, 1)
    ind = np.zeros(w.shape[:1] + (7, 7))
    for k in range(3):      # the order of stem_u8_fold.h (a double sum of three terms: its own rounding is far below the fp32 one)
        ind = ind + w[:, k] * (c[k] / 255.0 - mean[k]) / std[k]
    out[:, :, :7, 3] = ind
    return out


def bf16_bits(d):
    """an integer array of magnitude <= 256 as bf16 bit patterns (exact: the top half of the fp32 form)"""
    return (np.asarray(d, np.float32).view(np.uint32) >> 16).astype(np.uint32)


def frame(img, c):
    """uint8 [H, W, 3] -> the framed image [H + 6, W + 8, 2] of uint32 words: (u0 - c0 | u1 - c1 << 16, u2 - c2 | 1 << 16) at rows 3 .. H + 2,
    columns 3 .. W + 2, zeros in the frame"""
    H, W, _ = img.shape
    d = img.astype(np.int64) - np.asarray(c)[None, None, :]
    out = np.zeros((H + 6, W + 8, 2), np.uint32)
    out[3:H + 3, 3:W + 3, 0] = bf16_bits(d[..., 0]) | (bf16_bits(d[..., 1]) << 16)
    out[3:H + 3, 3:W + 3, 1] = bf16_bits(d[..., 2]) | (np.uint32(0x3f80) << 16)
    return out


def stem64(u8, w, s, b, mean, std):
    """The truth and the magnitude the error is measured in, both pooled: u8 [B, H, W, 3] resized frames ->
       y  [B, H2, W2, 64] float64 = maxpool3x3s2p1(relu(s * conv7x7s2p3(w, (u / 255 - mean) / std) + b))
       A' [B, H2, W2, 64]         = the window's maximum of |s| sum |a w'| + |b| over the folded operands a = (u - c, 1), w' = fl32(fold)
    (|max_i g_i - max_i y_i| <= max_i |g_i - y_i|, and ReLU is 1-Lipschitz: a bound C u A' on the conv outputs holds for the pooled ones
    with the window's largest A')"""
    import torch
    import torch.nn.functional as F
    f64 = lambda t: torch.from_numpy(np.asarray(t, np.float32).astype(np.float64))
    mean64, std64 = f64(mean), f64(std)
    x = (torch.from_numpy(u8.astype(np.float64)) / 255.0 - mean64) / std64
    y = F.conv2d(x.permute(0, 3, 1, 2), f64(w), None, 2, 3)
    sv, bv = f64(s).view(1, -1, 1, 1), f64(b).view(1, -1, 1, 1)
    y = F.relu(y * sv + bv)
    c = centres(mean)
    a = np.concatenate([np.abs(u8.astype(np.float64) - c[None, None, None, :]), np.ones(u8.shape[:3] + (1,))], -1)
    wf = np.abs(fold(w, mean, std).astype(np.float32).astype(np.float64))[:, :, :7, :]       # [Cout, ky, kx, 4], rounded once as the model's
    A = F.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), torch.from_numpy(wf).permute(0, 3, 1, 2).contiguous(), None, 2, 3)
    A = A * sv.abs() + bv.abs()
    pool = lambda t: F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    return pool(y), pool(A)
