// cg_mx8.h -- MXFP8 tensors and the block-scaled implicit-GEMM convolution (cg_mx8.hip) of the detector's mxfp8 mode.
//
// Format (include/odam_detr.h, DESIGN.md "MXFP8 backbone mode"): OCP MX v1.0 with e4m3fn elements and one E8M0 scale byte per
// block of 32 values.  A tensor [rows][C] (C % 32 == 0) is stored as elements q [rows][C] (1 byte each) and scales s [rows][C / 32];
// the block of element i is i / 32 in both layouts, so the scale of element i is s[i / 32].  Value = e4m3fn(q) * 2^(s - 127).
// Scale rule: e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127] (all-zero block: -127); elements are
// x * 2^-e rounded to nearest even into e4m3fn, subnormals kept.  No element saturates.  A block holding a NaN or an Inf gets scale
// byte 0xFF (the E8M0 NaN): it dequantizes, and multiplies, to NaN; its element bytes are not specified.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace odam_mx {

__host__ __device__ inline uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ inline float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

// block exponent from the bits of the block's largest |x| (integer max of (bits & 0x7fffffff)); 128 = non-finite block
__host__ __device__ inline int scale_exp(uint32_t ab) {
    if (ab >= 0x7f800000u) return 128;
    if (ab < 0x00800000u) return -127;                 // zero / subnormal amax: below 448 * 2^-127
    const int E = (int)(ab >> 23) - 127;               // amax = 1.f * 2^E; 448 = 1.75 * 2^8
    const int e = E - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// v (|v| <= 448 within the contract) -> e4m3fn byte, round to nearest even, subnormals kept
__host__ __device__ inline uint32_t e4m3(float v) {
    const uint32_t u = f2u(v), s = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return s | 0x7fu;
    if (a < 0x3c800000u) return s | (uint32_t)rintf(u2f(a) * 512.0f);      // below 2^-6: multiples of 2^-9 (8 -> 0x08 = 2^-6)
    uint32_t r = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);   // 3 mantissa bits, exponent bias 127 -> 7
    return s | (r > 0x7eu ? 0x7eu : r);
}

__host__ __device__ inline float e4m3_value(uint32_t b) {
    const uint32_t ex = (b >> 3) & 15u, mn = b & 7u;
    float v;
    if (ex == 0) v = (float)mn * (1.0f / 512.0f);
    else if (ex == 15 && mn == 7) v = u2f(0x7fc00000u);
    else v = u2f(((ex + 120u) << 23) | (mn << 20));
    return (b & 0x80u) ? -v : v;
}

// the scale byte of a block and its elements' multiplier 2^-e
__host__ __device__ inline uint32_t scale_byte(int e) { return e == 128 ? 0xffu : (uint32_t)(e + 127); }

// host: packed filters w [Cout][K] (float32, K % 32 == 0) -> elements q [Cout][K] + scales s [Cout][K / 32]
void quantize_host(const float* w, size_t n, unsigned char* q, unsigned char* s);

// device launchers (cg_mx8.hip).  n % 32 == 0.  src_dtype 0: fp32, 1: bf16.
int launch_quantize(const void* x, int src_dtype, size_t n, unsigned char* q, unsigned char* s, hipStream_t st);
int launch_dequantize(const unsigned char* q, const unsigned char* s, size_t n, float* y, hipStream_t st);

struct ConvArgs {
    const unsigned char *x, *xs;     // NHWC input [B, H, W, Cin] elements + scales [B, H, W, Cin / 32]
    const unsigned char *w, *ws;     // filters [Cout][Kpad] (k = (ky KW + kx) Cin + ci, Kpad = KH KW Cin) + scales [Cout][Kpad / 32]
    const float *scale, *bias;       // [Cout], nullable
    const unsigned short* res;       // bf16 residual [M][Cout], nullable
    unsigned char *y, *ys;           // MXFP8 output [M][Cout] + [M][Cout / 32], nullable (together)
    unsigned short* yb;              // bf16 copy [M][Cout], nullable
    float* yf;                       // fp32 values before quantization [M][Cout], nullable (tests)
    int B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Kpad, relu, M;
};
// checks the shape (Cin % 64 == 0, Cout % 32 == 0, Kpad == KH KW Cin, at least one output), notes "mx8.<BN>x<BM>.w<waves>"
int launch_conv(const ConvArgs& a, hipStream_t st);

}  // namespace odam_mx
