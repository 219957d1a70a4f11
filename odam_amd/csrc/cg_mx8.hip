// cg_mx8.hip -- MXFP8 convolution of the detector's mxfp8 mode on v_mfma_scale_f32_32x32x64_f8f6f4, and the standalone
// quantize / dequantize kernels.  Format: cg_mx8.h.
//
// Implicit GEMM D[n, m] = sum_k W[n, k] X[k, m]: n = output channel (the instruction's A rows), m = output pixel (its B columns),
// k = (tap, ci).  Operand lanes of the 32x32x64 form (measured on the device with one-hot filters and two scales per row): lane l
// holds row (col) l & 31; its bytes 0-15 are k 16 h .. 16 h + 15 and bytes 16-31 are k 32 + 16 h .. 32 + 16 h + 15 (h = l >> 5),
// and its scale byte applies to k 32 h .. 32 h + 31 -- so the two lanes of a row share each 32-k block, and lane half h carries
// the scale of MX block h.  A 64-byte tile row (two MX blocks) is read as [16 h, +16) and [32 + 16 h, +16).  The result
// lane l holds pixel l & 31 and channels (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r, so a 32-channel output block of one
// pixel sits in lanes l and l ^ 32: its amax is one cross-lane max, inside the wave.
//
// Tile 128 channels x 128 pixels x 64 k, four waves (2 x 2 of 64 x 64, 2 x 2 instructions each), operands staged global ->
// registers -> LDS in two LDS stages (the loads of k-tile t + 1 fly under the products of tile t), one barrier per k-tile.
// A k-tile is 64 channels of one tap (Cin % 64 == 0), so a tile row is one contiguous 64-byte read or zeros (padding, ragged M / N).
#include "cg_mx8.h"
#include "conv_gemm.h"
#include "odam_err.h"

#include <algorithm>
#include <cstring>

namespace odam_mx {

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int BN = 128, BM = 128, BK = 64, NTH = 256;
constexpr int ROW = 80;                          // LDS bytes per tile row: 64 + 16 pad (conflict-free 16-byte reads)
constexpr int TILE = 128 * ROW;                  // one operand tile
constexpr int STAGE = 2 * TILE + 2 * 128 * 2;    // W tile, X tile, their scales (2 bytes per row)

__device__ inline uint32_t bf16_rne(float f) {
    const uint32_t u = f2u(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// 32 values of one block -> 32 elements (two 16-byte words) and the scale byte
__device__ inline uint32_t quant32(const float* v, uint4* q) {
    uint32_t ab = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) ab = max(ab, f2u(v[i]) & 0x7fffffffu);
    const int e = scale_exp(ab);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t p = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) p |= e4m3(e == 128 ? v[4 * i + j] : ldexpf(v[4 * i + j], -e)) << (8 * j);
        w[i] = p;
    }
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
    return scale_byte(e);
}

__global__ __launch_bounds__(256) void quantize_kernel(const void* x, int bf, size_t nb, unsigned char* q, unsigned char* s) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    float v[32];
    if (bf) {
        const uint4* p = (const uint4*)((const unsigned short*)x + b * 32);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 u = p[i];
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; j++) { v[8 * i + 2 * j] = u2f(w[j] << 16); v[8 * i + 2 * j + 1] = u2f(w[j] & 0xffff0000u); }
        }
    } else {
        const float4* p = (const float4*)((const float*)x + b * 32);
#pragma unroll
        for (int i = 0; i < 8; i++) { const float4 f = p[i]; v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w; }
    }
    uint4 o[2];
    s[b] = (unsigned char)quant32(v, o);
    ((uint4*)(q + b * 32))[0] = o[0];
    ((uint4*)(q + b * 32))[1] = o[1];
}

__global__ __launch_bounds__(256) void dequantize_kernel(const unsigned char* q, const unsigned char* s, size_t n, float* y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i * 4 >= n) return;
    const uint32_t p = ((const uint32_t*)q)[i];
    const uint32_t sb = s[i / 8];
    float4 o;
    float* f = &o.x;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float d = e4m3_value((p >> (8 * j)) & 0xffu);
        f[j] = sb == 0xffu ? u2f(0x7fc00000u) : ldexpf(d, (int)sb - 127);
    }
    ((float4*)y)[i] = o;
}

__global__ __launch_bounds__(NTH) void conv_kernel(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n0 = blockIdx.y * BN, m0 = blockIdx.x * BM;
    const int cpt = a.Cin / BK, nk = a.Kpad / BK;
    const int q = t & 3;                                  // 16-byte chunk of a tile row this thread stages
    const int HW = a.Ho * a.Wo;

    // the pixels of the X rows this thread stages (rows t / 4 and t / 4 + 64) and of its X-scale row (t - 128)
    int pb[3], py[3], px[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int row = r < 2 ? (t >> 2) + 64 * r : (t & 127);
        const int m = m0 + row;
        if (m < a.M) {
            const int b = m / HW, rem = m - b * HW, oy = rem / a.Wo, ox = rem - oy * a.Wo;
            pb[r] = b * a.H; py[r] = oy * a.stride - a.pad; px[r] = ox * a.stride - a.pad;
        } else {
            pb[r] = 0; py[r] = -(1 << 20); px[r] = 0;     // never inside the image: zeros
        }
    }
    const int sc = a.Kpad / 32, xc = a.Cin / 32;

    uint4 rw[2], rx[2];
    uint32_t rs = 0;
    auto load = [&](int kt) {
        const int tap = kt / cpt, ci0 = (kt - tap * cpt) * BK;
        const int ky = tap / a.KW, kx = tap - ky * a.KW;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int n = n0 + (t >> 2) + 64 * r;
            rw[r] = n < a.Cout ? *(const uint4*)(a.w + (size_t)n * a.Kpad + kt * BK + q * 16) : make_uint4(0, 0, 0, 0);
            const int iy = py[r] + ky, ix = px[r] + kx;
            rx[r] = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                        ? *(const uint4*)(a.x + ((size_t)(pb[r] + iy) * a.W + ix) * a.Cin + ci0 + q * 16) : make_uint4(0, 0, 0, 0);
        }
        if (t < 128) {
            const int n = n0 + t;
            rs = n < a.Cout ? *(const unsigned short*)(a.ws + (size_t)n * sc + kt * 2) : 0x7f7fu;
        } else {
            const int iy = py[2] + ky, ix = px[2] + kx;
            rs = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                     ? *(const unsigned short*)(a.xs + ((size_t)(pb[2] + iy) * a.W + ix) * xc + ci0 / 32) : 0x7f7fu;
        }
    };
    auto store = [&](int st) {
        unsigned char* L = lds + st * STAGE;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int row = (t >> 2) + 64 * r;
            *(uint4*)(L + row * ROW + q * 16) = rw[r];
            *(uint4*)(L + TILE + row * ROW + q * 16) = rx[r];
        }
        *(unsigned short*)(L + 2 * TILE + t * 2) = (unsigned short)rs;     // t < 128: W scales of row t, else X scales of row t - 128
    };

    const int wn = wv >> 1, wm = wv & 1, r32 = lane & 31, h = lane >> 5;
    v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int k = 0; k < 16; k++) acc[i][j][k] = 0.0f;

    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int st = kt & 1;
        if (kt + 1 < nk) load(kt + 1);
        const unsigned char* L = lds + st * STAGE;
        v8i fa[2], fb[2];
        int sa[2], sb[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int ra = wn * 64 + i * 32 + r32, rb = wm * 64 + i * 32 + r32;
            const uint4 a0 = *(const uint4*)(L + ra * ROW + h * 16), a1 = *(const uint4*)(L + ra * ROW + 32 + h * 16);
            const uint4 b0 = *(const uint4*)(L + TILE + rb * ROW + h * 16), b1 = *(const uint4*)(L + TILE + rb * ROW + 32 + h * 16);
            fa[i] = v8i{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
            fb[i] = v8i{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
            sa[i] = L[2 * TILE + ra * 2 + h];
            sb[i] = L[2 * TILE + 256 + rb * 2 + h];
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
        if (kt + 1 < nk) store(st ^ 1);
        __syncthreads();
    }

    // epilogue: * scale + bias (+ bf16 residual), ReLU in fp32; per 32-channel block of a pixel: amax over lanes l, l ^ 32,
    // scale byte, e4m3 elements; optional bf16 / fp32 copies
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int nb = n0 + wn * 64 + i * 32;
        if (nb >= a.Cout) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int m = m0 + wm * 64 + j * 32 + r32;
            const bool ok = m < a.M;
            float v[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int n = nb + 8 * g + 4 * h;
                const float4 scv = a.scale ? *(const float4*)(a.scale + n) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float4 biv = a.bias ? *(const float4*)(a.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
                uint2 rr = make_uint2(0, 0);
                if (a.res && ok) rr = *(const uint2*)(a.res + (size_t)m * a.Cout + n);
                const float sv[4] = {scv.x, scv.y, scv.z, scv.w}, bv[4] = {biv.x, biv.y, biv.z, biv.w};
                const float rv[4] = {u2f(rr.x << 16), u2f(rr.x & 0xffff0000u), u2f(rr.y << 16), u2f(rr.y & 0xffff0000u)};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float x = acc[i][j][4 * g + k] * sv[k] + bv[k];
                    if (a.res) x = x + rv[k];
                    if (a.relu) x = fmaxf(x, 0.0f);
                    v[4 * g + k] = x;
                }
            }
            uint32_t ab = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) ab = max(ab, f2u(v[k]) & 0x7fffffffu);
            ab = max(ab, (uint32_t)__shfl_xor((int)ab, 32));
            const int e = scale_exp(ab);
            if (!ok) continue;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const size_t o = (size_t)m * a.Cout + nb + 8 * g + 4 * h;
                if (a.y) {
                    uint32_t p = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) p |= e4m3(e == 128 ? v[4 * g + k] : ldexpf(v[4 * g + k], -e)) << (8 * k);
                    *(uint32_t*)(a.y + o) = p;
                }
                if (a.yb)
                    *(uint2*)(a.yb + o) = make_uint2(bf16_rne(v[4 * g]) | (bf16_rne(v[4 * g + 1]) << 16),
                                                     bf16_rne(v[4 * g + 2]) | (bf16_rne(v[4 * g + 3]) << 16));
                if (a.yf) *(float4*)(a.yf + o) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
            }
            if (a.y && h == 0) a.ys[(size_t)m * (a.Cout / 32) + nb / 32] = (unsigned char)scale_byte(e);
        }
    }
}

}  // namespace

void quantize_host(const float* w, size_t n, unsigned char* q, unsigned char* s) {
    for (size_t b = 0; b < n / 32; b++) {
        uint32_t ab = 0;
        for (int i = 0; i < 32; i++) ab = std::max(ab, f2u(w[b * 32 + i]) & 0x7fffffffu);
        const int e = scale_exp(ab);
        for (int i = 0; i < 32; i++) q[b * 32 + i] = (unsigned char)e4m3(e == 128 ? w[b * 32 + i] : ldexpf(w[b * 32 + i], -e));
        s[b] = (unsigned char)scale_byte(e);
    }
}

int launch_quantize(const void* x, int src_dtype, size_t n, unsigned char* q, unsigned char* s, hipStream_t st) {
    if (n % 32) return odam_fail(1, "mxfp8 quantize: the element count must be a multiple of 32");
    const size_t nb = n / 32;
    if (!nb) return 0;
    hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, x, src_dtype, nb, q, s);
    ODAM_HIP(hipGetLastError());
    return 0;
}

int launch_dequantize(const unsigned char* q, const unsigned char* s, size_t n, float* y, hipStream_t st) {
    if (n % 32) return odam_fail(1, "mxfp8 dequantize: the element count must be a multiple of 32");
    if (!n) return 0;
    hipLaunchKernelGGL(dequantize_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, q, s, n, y);
    ODAM_HIP(hipGetLastError());
    return 0;
}

int launch_conv(const ConvArgs& a, hipStream_t st) {
    if (!a.x || !a.xs || !a.w || !a.ws) return odam_fail(1, "mxfp8 conv: null operand");
    if (!a.y != !a.ys) return odam_fail(1, "mxfp8 conv: MXFP8 output needs both its elements and its scales");
    if (!a.y && !a.yb && !a.yf) return odam_fail(1, "mxfp8 conv: no output");
    if (a.Cin < 64 || a.Cin % 64 || a.Cout < 32 || a.Cout % 32)
        return odam_fail(1, "mxfp8 conv: Cin must be a multiple of 64 and Cout a multiple of 32");
    if (a.Kpad != a.KH * a.KW * a.Cin) return odam_fail(1, "mxfp8 conv: Kpad must be KH * KW * Cin (tap-major k)");
    if (a.stride < 1 || a.pad < 0 || a.Ho < 1 || a.Wo < 1 || a.M != a.B * a.Ho * a.Wo) return odam_fail(1, "mxfp8 conv: bad geometry");
    if ((long long)a.B * a.H * a.W * a.Cin >= (1LL << 40)) return odam_fail(1, "mxfp8 conv: tensor too large");
    odam_cg::note_path("mx8.%dx%d.w%d", BN, BM, NTH / 64);
    hipLaunchKernelGGL(conv_kernel, dim3((unsigned)((a.M + BM - 1) / BM), (unsigned)((a.Cout + BN - 1) / BN)), dim3(NTH), 0, st, a);
    ODAM_HIP(hipGetLastError());
    return 0;
}

}  // namespace odam_mx
