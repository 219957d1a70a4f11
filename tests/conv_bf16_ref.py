"""Reference and check for the bf16 contraction kernels (tests/test_conv_bf16_gpu.py; no GPU needed here,
tests/test_conv_bf16_ref_host.py runs this module alone on the CPU).

Error model.  The operands x, w and the residual r are bf16, so every product x_k w_k is exact in fp32.  An output element is
y = act(s * sum_k x_k w_k + b + r); let A = |s| sum_k |x_k w_k| + |b| + |r| and u = 2^-24.
  * The contraction accumulates in fp32 along a chain of v_mfma_f32_32x32x16_bf16 (K / 16 steps, no dropped terms); the fp32 file's
    budget for such a chain is 5 u A (tests/test_conv_f32_gpu.py).
  * The epilogue rounds three times in fp32 (the library is built with -ffp-contract=off): s * acc, + b, + r.  Budget 3 u A.
So the kernel's fp32 value v obeys |v - y64| <= C u A with a budget of C = 8 (C_BUDGET); ReLU is 1-Lipschitz.
  * fp32 output (out_f32 = 1): that inequality itself, element by element.
  * bf16 output: v is rounded to nearest even ONCE.  Rounding is monotone, so the stored value lies in
    [rne_bf16(y64 - C u A), rne_bf16(y64 + C u A)] -- one or two points of the bf16 grid.  Truncation, a second rounding point (a
    residual added after the rounding) or a dropped tap leaves that interval; near a cancellation the interval stays absolute.
    -0 and +0 compare equal, any non-finite output fails.

Measured on an MI355X against float64 (profiles/conv_bf16_test_measured.json, the conv_bf16.* entries; worst |v - y64| / (u A) of
the fp32-output runs): small tiles 1.10 - 2.12, ring tiles 1.40 - 1.93, the 3x3 stride-1 shapes at image borders 1.22 - 2.09, null
scale / bias 1.21 - 1.66.  The worst is 2.12, well inside the budget of 8 as expected of a chain an eighth as long as the fp32
instruction's, and far below the fp32 file's 12; the asserted constant is C_BF16 = 1.4 x 2.1215 = 2.97.  Every bf16 output,
the fused launches' included, lies inside its interval already at C = 1."""
import torch
import torch.nn.functional as F

# ref64(x, w, s, b, r, stride, pad, dil, relu) -> (y64, A): the fp32 file's formula y64 = act(s conv(x, w) + b + r) in float64 and
# A = |s| conv(|x|, |w|) + |b| + |r|, one definition for both files (importing that module touches no GPU)
from test_conv_f32_gpu import ref64  # noqa: F401

U = 2.0 ** -24
C_BUDGET = 8.0      # 5 (fp32-accumulated matrix-instruction chain) + 3 (epilogue roundings): what the CPU emulation is held to
# The asserted constant of the GPU tests: 1.4 x the worst ratio measured on the MI355X (the fp32 file's margin; never below the
# worst measured).  The operands are seeded and the kernels deterministic, so a rerun reproduces the ratios.
WORST_MEASURED = 2.1215     # bf16.small.64x64.w4 (5 x 5 x 5 pixels, Cin 32, 3x3); every ring tile and the window loop stay below 2.09
C_BF16 = 1.4 * WORST_MEASURED


def rne_bf16(v64):
    """float64 -> the nearest bf16 value, ties to even, as float64.  Exact: one rounding, done on the float64's own exponent
    (frexp), never through a float32 cast.  bf16 subnormals (spacing 2^-133) and overflow to infinity as in IEEE arithmetic."""
    v = v64.double()
    _, e = torch.frexp(v)                                   # |v| = m 2^e, m in [0.5, 1): 8 significant bits -> quantum 2^(e - 8)
    qe = torch.clamp(e.to(torch.int64) - 8, min=-133)
    q = torch.ldexp(torch.ones_like(v), qe)
    out = torch.round(v / q) * q                            # torch.round: half to even; v / q and the product are exact
    out = torch.where(out.abs() >= 2.0 ** 128, torch.sign(out) * float("inf"), out)
    return torch.where(torch.isfinite(v), out, v)


def to_bf16(t):
    """float32 values rounded to bf16 (ties to even), kept as float32: what the tests feed every implementation"""
    return t.to(torch.bfloat16).float()


def ratio_f32(got, y64, A):
    """fp32 output: the worst |got - y64| / (u A) over the tensor (inf where an element is not finite)"""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return ((got.double() - y64).abs() / (U * A.clamp_min(1e-300))).max().item()


def interval_violations(got, y64, A, C):
    """bf16 output (any float dtype holding bf16 values): how many elements lie outside
    [rne_bf16(y64 - C u A), rne_bf16(y64 + C u A)] or are not finite"""
    g = got.double()
    lo, hi = rne_bf16(y64 - C * U * A), rne_bf16(y64 + C * U * A)
    ok = torch.isfinite(g) & (g >= lo) & (g <= hi)          # -0 == +0 in a float comparison
    return int((~ok).sum().item())


def emulate(x, w, s, b, r, stride, pad, dil, relu, out_f32=False, trunc=False, res_after=False, zero_tap=False):
    """The kernel restated on the CPU: float32 conv of the bf16 operands, the epilogue in fp32 (three roundings), one
    round-to-nearest-even to bf16.  The three switches are the mistakes the interval test has to notice:
    trunc = the low 16 bits are cut off instead; res_after = the residual joins after the rounding (and the sum is rounded
    again); zero_tap = the last output column misses the tap (ky, kx) = (0, 0), which lies inside the image there -- a border mask one pixel off."""
    acc = F.conv2d(x, w, None, stride, pad, dil)
    if zero_tap:
        wz = w.clone(); wz[:, :, 0, 0] = 0
        acc[..., -1] = F.conv2d(x, wz, None, stride, pad, dil)[..., -1]
    one = torch.ones(w.shape[0]); zero = torch.zeros(w.shape[0])
    v = acc * (s if s is not None else one).view(1, -1, 1, 1)
    v = v + (b if b is not None else zero).view(1, -1, 1, 1)
    cut = lambda t: (t.view(torch.int32) & -65536).view(torch.float32)
    rnd = cut if trunc else to_bf16
    if r is not None:
        v = rnd(v) + r if res_after else v + r
    if relu:
        v = F.relu(v)
    return v if out_f32 else rnd(v.contiguous())
