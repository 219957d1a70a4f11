"""The reference of the bf16 contraction tests (tests/conv_bf16_ref.py) on the CPU alone: rne_bf16 is the exact rounding, a
faithful restatement of the kernel stays inside the interval test at the budgeted constant, and the test has teeth -- the same
restatement with truncation, with the residual added after the rounding, or with one border tap missing is rejected."""
import pytest
import torch

from conv_bf16_ref import C_BUDGET, emulate, interval_violations, ratio_f32, ref64, rne_bf16, to_bf16

# (B, H, W, Cin, Cout, k, stride, pad, dil, relu): three of the small shapes of tests/test_conv_bf16_gpu.py
SHAPES = [
    (5, 5, 5, 32, 72, 3, 1, 1, 1, False),       # a 64-row tile spans three images
    (1, 1, 300, 256, 100, 1, 1, 0, 1, True),    # linear rows
    (2, 23, 29, 64, 40, 3, 1, 2, 2, True),      # dilation 2, ragged columns
]


def _operands(seed, B, H, W, Cin, Cout, k, stride, pad, dil):
    g = torch.Generator().manual_seed(seed)
    x = to_bf16(torch.randn(B, Cin, H, W, generator=g))
    w = to_bf16(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    s = torch.rand(Cout, generator=g) + 0.5
    b = torch.randn(Cout, generator=g) * 0.5
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1; Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = to_bf16(torch.randn(B, Cout, Ho, Wo, generator=g))
    return x, w, s, b, r


def test_rne_bf16_is_torchs_conversion():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(100000, generator=g) * torch.exp2(torch.randint(-140, 128, (100000,), generator=g).float())
    v = torch.cat([v, torch.tensor([0.0, -0.0, 1.0, -1.0, 3.3895314e38, 3.4028235e38, -3.4028235e38, 1e-45, 2.0 ** -133, 2.0 ** -134,
                                    3 * 2.0 ** -134, float("inf"), -float("inf")])])
    want = v.to(torch.bfloat16).double()
    got = rne_bf16(v.double())
    assert torch.equal(got, want), (got != want).sum().item()
    assert torch.equal(torch.signbit(got), torch.signbit(want))      # the sign of a zero too
    assert torch.isnan(rne_bf16(torch.tensor([float("nan")], dtype=torch.float64))).all()


def test_rne_bf16_ties_and_single_rounding():
    # bf16 has 8 significant bits: 1 + 2^-8 is a tie between 1 and 1 + 2^-7
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    ulp = 2.0 ** -7
    got = rne_bf16(t(1 + ulp / 2, 1 + 3 * ulp / 2, 1 + 5 * ulp / 2, -(1 + ulp / 2), -(1 + 3 * ulp / 2), 2 - ulp / 2, 255.5, 256.5 * 2))
    assert torch.equal(got, t(1.0, 1 + 2 * ulp, 1 + 2 * ulp, -1.0, -(1 + 2 * ulp), 2.0, 256.0, 512.0))
    # just above / below a tie: float64 carries what a float32 cast would round away first (double rounding)
    eps = 2.0 ** -40
    got = rne_bf16(t(1 + ulp / 2 + eps, 1 + ulp / 2 - eps, 1 + 3 * ulp / 2 - eps))
    assert torch.equal(got, t(1 + ulp, 1.0, 1 + ulp))
    via_f32 = t(1 + ulp / 2 + eps).float().to(torch.bfloat16).double()
    assert via_f32.item() == 1.0                                      # the cast rounds twice and lands on the other side


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:5])))
def test_emulation_passes_at_the_budget(shape):
    *dims, relu = shape
    x, w, s, b, r = _operands(sum(dims), *dims)
    y64, A = ref64(x, w, s, b, r, *dims[6:], relu)
    assert ratio_f32(emulate(x, w, s, b, r, *dims[6:], relu, out_f32=True), y64, A) <= C_BUDGET
    assert interval_violations(emulate(x, w, s, b, r, *dims[6:], relu), y64, A, C_BUDGET) == 0
    y64n, An = ref64(x, w, None, None, None, *dims[6:], relu)
    assert interval_violations(emulate(x, w, None, None, None, *dims[6:], relu), y64n, An, C_BUDGET) == 0


@pytest.mark.parametrize("mistake", ["trunc", "res_after", "zero_tap"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda s: "x".join(map(str, s[:5])))
def test_interval_test_rejects_a_wrong_kernel(shape, mistake):
    *dims, relu = shape
    x, w, s, b, r = _operands(sum(dims), *dims)
    y64, A = ref64(x, w, s, b, r, *dims[6:], relu)
    bad = emulate(x, w, s, b, r, *dims[6:], relu, **{mistake: True})
    n = interval_violations(bad, y64, A, C_BUDGET)
    assert n > 0, mistake
    if mistake == "zero_tap":       # confined to the border column it was planted in
        good = emulate(x, w, s, b, r, *dims[6:], relu)
        assert torch.equal(bad[..., :-1], good[..., :-1]) and interval_violations(bad[..., :-1], y64[..., :-1], A[..., :-1], C_BUDGET) == 0


def test_interval_test_rejects_non_finite_and_accepts_signed_zero():
    y64 = torch.zeros(4, dtype=torch.float64); A = torch.ones(4, dtype=torch.float64)
    assert interval_violations(torch.tensor([0.0, -0.0, 0.0, -0.0]), y64, A, C_BUDGET) == 0
    assert interval_violations(torch.tensor([0.0, float("nan"), float("inf"), 0.0]), y64, A, C_BUDGET) == 2
    assert ratio_f32(torch.tensor([0.0, float("nan"), 0.0, 0.0]), y64, A) == float("inf")
