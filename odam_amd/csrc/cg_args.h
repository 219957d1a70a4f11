// cg_args.h -- the argument block of a contraction launch (conv_gemm.h launch_conv_gemm), free of HIP so that the kernel choice
// (cg_choice.h) compiles and is tested as plain host C++.  The struct is passed to the kernels by value: its layout is theirs.
#pragma once

namespace odam_cg {

constexpr int ODAM_CG_F32 = 0;
constexpr int ODAM_CG_BF16 = 1;

struct ConvGemmArgs {
    const void* A;       // NHWC input [B, H, W, Cin] fp32 or bf16; Cin a power of two >= one 16-byte chunk (4 / 8)
    const void* Wt;      // [Cout][Kpad] same type, k-major, zero padded to a multiple of the k-tile (32 / 64)
    const void* Wt3 = nullptr;   // fp32 layers, optional: the same filters split exactly into three bf16 values per weight,
                         //    [Cout][Kpad / 16][3][16] (hi | mid | lo of every 16-k group; split3_filters); lets the split
                         //    contraction mode (set_f32_mode 2) skip splitting them in registers
    const float* scale;  // [Cout] fp32 or nullptr
    const float* bias;   // [Cout] fp32 or nullptr
    const void* res;     // [M, Cout] activation type, or nullptr
    void* C;             // [M, Cout] activation type (fp32 when out_f32)
    int B, H, W, Cin, log2Cin;
    int Ho, Wo, Cout;
    int KH, KW, stride, pad;
    int Kpad;
    int relu;
    int M;
    int ldc;             // row stride of C / res in elements (>= Cout)
    int dtype;           // ODAM_CG_F32 / ODAM_CG_BF16: v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_bf16, fp32 accumulate
    int out_f32;         // bf16 mode only: write C as fp32
    int lda;             // elements between consecutive input pixels (0 = Cin): reads a column block of a wider buffer
    int k_order;         // 0: k = (tap, ci).  1: k = (ci / kt, tap, ci % kt) with kt = the k-tile (32 fp32 / 64 bf16),
                         //    Cin % kt == 0: the taps of one channel chunk are consecutive k-tiles, so a workgroup re-reads
                         //    its input window from L2 while it is still there (tap-major revisits it 8+ k-tiles later)
    // Fused second layer (optional; conv_gemm_big_kernel with pre-split filters, Cout == 64 only): this layer's output
    // tile -- after scale / bias / ReLU -- is not stored but multiplied on chip by a 1x1 layer with F_N = 256 outputs,
    //   F_C[m, n] = act( (relu(C) F_W^T)[m, n] * F_scale[n] + F_bias[n] + F_res[m, n] ),
    // i.e. a ResNet bottleneck's 3x3 + expand + residual in one launch (detr_forward.hip, layer1).  F_Wt3 = the expand
    // filters split by split3_filters(w, 256, 64, .); fp32 only; C is ignored.
    const void* F_Wt3 = nullptr;
    const float* F_scale = nullptr;
    const float* F_bias = nullptr;
    const float* F_res = nullptr;   // [M, F_ldc] or null
    float* F_C = nullptr;           // [M, F_ldc]
    int F_ldc = 0, F_relu = 0;
    // ... and a third: the NEXT bottleneck's 1x1 reduce (256 -> G_N channels, scale / bias / ReLU) applied to F_C's tile
    // while it is on chip, G_C[m, 0..G_N-1]; G_Wt3 = split3_filters(w, G_N, 256, .).  Optional; needs the F_* layer.
    const void* G_Wt3 = nullptr;
    const float* G_scale = nullptr;
    const float* G_bias = nullptr;
    float* G_C = nullptr;           // [M, G_N]
    int G_N = 64;                   // 64 (the next block of the same stage) or 128 (layer2's first reduce after layer1's last block)
    // bf16 mode (dtype ODAM_CG_BF16), the same two fusions with plain bf16 filters: F_Wt [F_ldc][Cout] (the 1x1 expand, K = this
    // layer's Cout = 64 / 128 / 256), G_Wt [G_N][F_ldc] (the next reduce).  F_res / F_C / G_C then point to bf16 tensors.
    const void* F_Wt = nullptr;
    const void* G_Wt = nullptr;
    int dil = 1;                    // dilation of the taps (both axes): tap (ky, kx) reads input pixel (oy stride - pad + ky dil, ox stride - pad + kx dil);
                                    // the window loop and the bottleneck-on-the-tile launches take dil = 1 only
    // Stem with the max-pool on the tile (conv_gemm_big_kernel, sixteen-wave 512 x 64 tiles only; launch_conv_gemm checks): pool = 1
    // makes a tile a 2-D patch of (2 pool_ph + 1) x (2 pool_pw + 1) <= 512 conv outputs -- the 3 x 3 / stride 2 / pad 1 windows of
    // pool_ph x pool_pw pooled pixels -- instead of 512 consecutive ones; after scale / bias / ReLU the patch is pooled in LDS and C
    // receives the POOLED tensor [B, Hp, Wp, Cout] (ldc = Cout).  Patches overlap by one conv row / column (recomputed).  The
    // ReLU makes zero padding equivalent to the -inf padding of max_pool2d.  M stays B Ho Wo (the conv's own size).
    // pool_ph x pool_pw is fixed at POOL_PH x POOL_PW below (compile-time divisors in the kernel).
    int pool = 0, pool_ph = 0, pool_pw = 0, Hp = 0, Wp = 0;
    int no_pin = 0;                 // 1: odam_config cg.pin does not apply to this call (its M does not depend on the shard a rank holds: the
                                    //    association network runs on the same rows on every rank, and small tiles are what its sizes want)
    int s1_window = 0;              // set by launch_conv_gemm (bf16 ring kernel, 3x3 stride 1): one LDS window per (channel slice, ky)
                                    //    serves the three horizontal taps (odam_config.h cg.s1)
    int a_bf16 = 0;                 // fp32 layer whose activations are exact in ONE bf16 value (the stem's centred uint8 frame): A is bf16 in memory
                                    //    ([B, H, W] pixels of lda bf16, Cin of them per tap), never split; a x (w_hi, w_mid, w_lo) = three products per
                                    //    block instead of six, none dropped (conv_gemm_big_kernel MODE 5: sixteen-wave 512 x 64 tiles, pre-split filters)
};

constexpr int POOL_PH = 8, POOL_PW = 14;      // pooled pixels per patch: (2 * 8 + 1) x (2 * 14 + 1) = 493 conv outputs of a 512-row tile

}  // namespace odam_cg
