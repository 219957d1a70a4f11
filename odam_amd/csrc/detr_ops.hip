// detr_ops.hip -- single-operator entry points of include/odam_detr.h: what tests and tools call to drive one kernel of the
// detector -- a convolution, an attention, a LayerNorm, a pooling / layout / elementwise pass -- through the launchers the forward uses.  Each family of entries
// shares one checked implementation; which checks an entry runs, and the name its error texts begin with, are its own.
#include <hip/hip_runtime.h>

#include "detr_kernels.h"
#include "detr_model.h"

using namespace odam_dm;
using odam_cg::ConvGemmArgs;

namespace {

int fail(int code, const char* who, const char* what) {
    std::snprintf(g_odam_err, sizeof(g_odam_err), "%s: %s", who, what);
    return code;
}

// Split contraction mode: a model keeps its filters pre-split into three bf16 planes (detr_weights.hip upload_w3); the op-level entries
// build them for the one call (download, split on the host, upload), so that the op tests drive the SAME kernels a forward does -- the
// 16x16x32 loop with its ragged last row tile and ragged last columns -- and not only the layer shapes a DETR happens to have.  *d3 = null
// where the mode or the shape takes no pre-split filters; the caller frees *d3 after synchronising the stream.
int split_filters_for_call(const float* w_packed, int Cout, int Kpad, hipStream_t st, unsigned short** d3, const char* who) {
    *d3 = nullptr;
    if (!odam_cg::presplit_applies(Cout, Kpad)) return 0;
    std::vector<float> hw((size_t)Cout * Kpad);
    ODAM_HIP(hipStreamSynchronize(st));
    ODAM_HIP(hipMemcpy(hw.data(), w_packed, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<unsigned short> h3(hw.size() * 3);
    odam_cg::split3_filters(hw.data(), Cout, Kpad, h3.data());
    ODAM_HIP(hipMalloc(d3, h3.size() * 2));
    if (hipMemcpy(*d3, h3.data(), h3.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(*d3); *d3 = nullptr;
        return fail(1, who, "upload of the split filters failed");
    }
    return 0;
}

// a layer described by an entry's arguments, filters as the caller packed them
Conv conv_of(const void* w, const float* scale, const float* bias, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
             int Kpad, int k_order) {
    Conv c;
    c.w = const_cast<void*>(w); c.scale = const_cast<float*>(scale); c.bias = const_cast<float*>(bias);
    c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW; c.stride = stride; c.pad = pad; c.Kpad = Kpad; c.dil = dil;
    c.k_order = k_order;
    return c;
}

// ---- conv2d: odam_op_conv2d_nhwc_ex and _bf16 (odam_op_conv2d_nhwc forwards to _ex) ----
int conv2d_op(const char* who, const void* x, const void* w_packed, const float* scale, const float* bias, const void* residual, void* y,
              int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int Kpad, int relu, int k_order,
              int dtype, int out_f32, void* stream) {
    if (!x || !w_packed || !y) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (dil < 1) return fail(1, who, "dilation must be >= 1");
    if (dtype == 0 && out_f32) return fail(1, who, "out_f32 is for bf16 operands");
    hipStream_t st = (hipStream_t)stream;
    Conv c = conv_of(w_packed, scale, bias, Cin, Cout, KH, KW, stride, pad, dil, Kpad, k_order);
    unsigned short* d3 = nullptr;
    if (dtype == 0) RC(split_filters_for_call((const float*)w_packed, Cout, Kpad, st, &d3, who));
    c.w3 = d3;
    const int rc = run_conv(c, x, B, H, W, residual, relu != 0, y, st, dtype, out_f32);
    if (d3) { (void)hipStreamSynchronize(st); (void)hipFree(d3); }
    return rc;
}

// ---- bottleneck tail as one launch: the 3x3 (P -> P channels, pad 1, filters packed k_order 1) through conv_args, then the
// expand (-> 4 P) and optionally the next reduce (-> PN) on its tile ----
ConvGemmArgs bottleneck_args(int dtype, const void* x, const void* w2, const float* s2, const float* b2, const float* s3, const float* b3,
                             const void* residual, void* y, const float* s1n, const float* b1n, void* y_next, int B, int H, int W, int P,
                             int stride, int PN) {
    ConvGemmArgs a = conv_args(conv_of(w2, s2, b2, P, P, 3, 3, stride, 1, 1, 9 * P, 1), x, B, H, W, dtype);
    a.relu = 1;
    a.F_scale = s3; a.F_bias = b3; a.F_res = (const float*)residual; a.F_C = (float*)y; a.F_ldc = 4 * P; a.F_relu = 1;
    if (PN > 0) { a.G_scale = s1n; a.G_bias = b1n; a.G_C = (float*)y_next; a.G_N = PN; }
    return a;
}

// ---- attention: which of the checks below an entry runs is part of its contract (odam_op_attention: null pointers only) ----
enum AttChecks { ATT_NULLS, ATT_BF16, ATT_EX, ATT_HD };

int attention_op(const char* who, AttChecks checks, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                 int ldo, int B, int H, int Lq, int Lk, int head_dim, int dtype, const unsigned char* key_mask, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!Q || !K || !V || !O) return fail(1, who, "null pointer");
    if (checks == ATT_BF16 && (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4))
        return fail(1, who, "row pitches must be multiples of 8 / 8 / 8 / 4 elements");
    if (checks == ATT_EX || checks == ATT_HD) {
        if (B < 0 || H < 0 || Lq < 0 || Lk < 0) return fail(1, who, "negative extent");
        if (checks == ATT_HD && head_dim != 32 && head_dim != 64) return fail(1, who, "head_dim must be 32 or 64");
        if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
        const int pm = dtype == 1 ? 8 : 4;      // 16-byte rows of Q / K / V (the bf16 kernel's uint4 loads); O in 4-element groups
        if (ldq % pm || ldk % pm || ldv % pm || ldo % 4)
            return fail(1, who, "row pitches must be multiples of 8 / 8 / 8 / 4 (bf16) or 4 (fp32) elements");
        if (H == 0) return 0;
    }
    if (checks == ATT_EX && head_dim != 32) {
        // not launch_attention(.., head_dim = 64): that one takes the split kernel where att.x3 is on, this entry promises the
        // associator's (fp32 matrix instruction, scale 1/8)
        if (head_dim == 64 && dtype == 0 && !key_mask)
            return odam_dk::launch_attention_d64((const float*)Q, ldq, (const float*)K, ldk, (const float*)V, ldv, (float*)O, ldo,
                                                 B, H, Lq, Lk, st);
        return fail(1, who, "head_dim 32 (fp32 / bf16, optional key mask) or 64 (fp32, no mask) only");
    }
    return odam_dk::launch_attention(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, dtype, st, key_mask, head_dim);
}

// ---- residual add + LayerNorm: odam_op_add_layernorm checks null pointers only, _ex and _c everything ----
int layernorm_op(const char* who, bool checked, const void* x, const void* r, const float* gamma, const float* beta, void* y,
                 const float* pos, int L, void* y_pos, int M, int C, int dtype, void* stream) {
    if (!x || !gamma || !beta || !y) return fail(1, who, "null pointer");
    if (checked) {
        if (y_pos && (!pos || L <= 0)) return fail(1, who, "y_pos needs pos and L > 0");
        if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
        if (M < 0) return fail(1, who, "negative M");
        if (C % 64 || C < 128 || C > 1024) return fail(1, who, "C must be a multiple of 64 in 128 .. 1024");
    }
    return odam_dk::launch_add_layernorm(x, r, gamma, beta, y, pos, y_pos ? L : 1, y_pos, M, dtype, (hipStream_t)stream, C);
}

// ---- 3x3 / stride 2 / pad 1 max-pool: odam_op_maxpool3x3s2_nhwc (fp32) and _ex ----
int maxpool_op(const char* who, const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
    if (!x || !y) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (B < 0 || H < 0 || W < 0 || C < 0) return fail(1, who, "negative extent");
    if (C % 4) return fail(1, who, "C must be a multiple of 4");
    if (!B || !H || !W || !C) return 0;
    return odam_dk::launch_maxpool3x3s2(x, y, B, H, W, C, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), dtype, (hipStream_t)stream);
}

}  // namespace

extern "C" int odam_op_conv2d_nhwc_ex(const void* x, const void* w_packed, const float* scale, const float* bias, const void* residual,
                                      void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                                      int Kpad, int relu, int k_order, int dtype, int out_f32, void* stream) {
    return conv2d_op("odam_op_conv2d_nhwc_ex", x, w_packed, scale, bias, residual, y, B, H, W, Cin, Cout, KH, KW, stride, pad, dil, Kpad,
                     relu, k_order, dtype, out_f32, stream);
}

extern "C" int odam_op_conv2d_nhwc(const float* x, const float* w_packed, const float* scale, const float* bias,
                                   const float* residual, float* y, int B, int H, int W, int Cin, int Cout, int KH,
                                   int KW, int stride, int pad, int Kpad, int relu, int k_order, void* stream) {
    if (!x || !w_packed || !y) return odam_fail(1, "odam_op_conv2d_nhwc: null pointer");
    return odam_op_conv2d_nhwc_ex(x, w_packed, scale, bias, residual, y, B, H, W, Cin, Cout, KH, KW, stride, pad, 1, Kpad, relu,
                                  k_order, 0, 0, stream);
}

extern "C" int odam_op_conv2d_nhwc_bf16(const void* x, const void* w_packed, const float* scale, const float* bias,
                                        const void* residual, void* y, int B, int H, int W, int Cin, int Cout, int KH,
                                        int KW, int stride, int pad, int Kpad, int relu, int out_f32, int k_order, void* stream) {
    return conv2d_op("odam_op_conv2d_nhwc_bf16", x, w_packed, scale, bias, residual, y, B, H, W, Cin, Cout, KH, KW, stride, pad, 1, Kpad,
                     relu, k_order, 1, out_f32, stream);
}

// ---- MXFP8 (cg_mx8.h) ----
extern "C" int odam_op_quantize_mxfp8(const void* x, int src_dtype, long long n, void* q, void* s, void* stream) {
    if (!x || !q || !s || n < 0) return odam_fail(1, "odam_op_quantize_mxfp8: null pointer or negative count");
    if (src_dtype != 0 && src_dtype != 1) return odam_fail(1, "odam_op_quantize_mxfp8: src_dtype must be 0 (fp32) or 1 (bf16)");
    return odam_mx::launch_quantize(x, src_dtype, (size_t)n, (unsigned char*)q, (unsigned char*)s, (hipStream_t)stream);
}

extern "C" int odam_op_dequantize_mxfp8(const void* q, const void* s, long long n, float* y, void* stream) {
    if (!q || !s || !y || n < 0) return odam_fail(1, "odam_op_dequantize_mxfp8: null pointer or negative count");
    return odam_mx::launch_dequantize((const unsigned char*)q, (const unsigned char*)s, (size_t)n, y, (hipStream_t)stream);
}

extern "C" int odam_op_conv2d_nhwc_mxfp8(const void* x, const void* xs, const void* w_packed, const void* ws, const float* scale,
                                         const float* bias, const void* residual, void* y, void* ys, void* y_bf16, float* y_f32,
                                         int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                                         int Kpad, int relu, int k_order, void* stream) {
    if (dil != 1) return odam_fail(1, "odam_op_conv2d_nhwc_mxfp8: dilation must be 1");
    if (k_order != 0) return odam_fail(1, "odam_op_conv2d_nhwc_mxfp8: k_order must be 0 (tap-major)");
    if (B < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0) return odam_fail(1, "odam_op_conv2d_nhwc_mxfp8: bad shape");
    Conv c = conv_of(nullptr, scale, bias, Cin, Cout, KH, KW, stride, pad, 1, Kpad, 0);
    c.wq = (unsigned char*)const_cast<void*>(w_packed); c.wqs = (unsigned char*)const_cast<void*>(ws);
    odam_mx::ConvArgs a = mx_args(c, x, xs, B, H, W);
    a.res = (const unsigned short*)residual; a.relu = relu ? 1 : 0;
    a.y = (unsigned char*)y; a.ys = (unsigned char*)ys; a.yb = (unsigned short*)y_bf16; a.yf = y_f32;
    return odam_mx::launch_conv(a, (hipStream_t)stream);
}

// A whole bf16 bottleneck tail as ONE launch (cg_choice.h fused_bf16_ok, cg_fused_bf16.hip): 3x3 (P -> P channels, stride 1 or 2, pad 1; filters
// packed k_order 1) + scale / bias / ReLU, 1x1 expand to 4 P channels + scale / bias + residual + ReLU -> y, and optionally the
// next block's 1x1 reduce (4 P -> PN channels, scale / bias / ReLU) of y -> y_next.  Returns 4 where the fused kernel does
// not apply to the shape (the caller then runs the layers one by one with odam_op_conv2d_nhwc_bf16; results are bit-identical).
extern "C" int odam_op_bottleneck_bf16(const void* x, const void* w2, const float* s2, const float* b2, const void* w3,
                                       const float* s3, const float* b3, const void* residual, void* y, const void* w1n,
                                       const float* s1n, const float* b1n, void* y_next, int B, int H, int W, int P, int stride,
                                       int PN, void* stream) {
    if (!x || !w2 || !w3 || !y) return odam_fail(1, "odam_op_bottleneck_bf16: null pointer");
    ConvGemmArgs a = bottleneck_args(1, x, w2, s2, b2, s3, b3, residual, y, s1n, b1n, y_next, B, H, W, P, stride, w1n ? PN : 0);
    a.F_Wt = w3;
    if (w1n && PN > 0) a.G_Wt = w1n;
    if (!odam_cg::fused_bf16_ok(a)) return odam_fail(4, "odam_op_bottleneck_bf16: the fused kernel does not apply to this shape");
    return odam_cg::launch_conv_gemm(a, (hipStream_t)stream);
}

// The fp32 counterpart (cg_choice.h fused_second_ok, cg_fused_f32.hip launch_big_fused, split mode): 3x3 (P = 64 or 128 channels, stride 1 or 2,
// pad 1; w2 [P][9 P] packed k_order 1) + scale / bias / ReLU, 1x1 expand to 4 P + scale / bias (+ residual) + ReLU -> y, and for
// P = 64 optionally the next reduce (PN = 64 / 128) -> y_next.  The filters come packed in fp32 and are split on the host for the
// call, as odam_op_conv2d_nhwc does.  Returns 4 where fused_second_ok refuses the shape or the configuration.
extern "C" int odam_op_bottleneck_f32(const float* x, const float* w2, const float* s2, const float* b2, const float* w3,
                                      const float* s3, const float* b3, const float* residual, float* y, const float* w1n,
                                      const float* s1n, const float* b1n, float* y_next, int B, int H, int W, int P, int stride,
                                      int PN, void* stream) {
    if (!x || !w2 || !w3 || !y) return odam_fail(1, "odam_op_bottleneck_f32: null pointer");
    if (PN > 0 && (!w1n || !y_next)) return odam_fail(1, "odam_op_bottleneck_f32: PN > 0 needs w1n and y_next");
    if (P != 64 && P != 128) return odam_fail(4, "odam_op_bottleneck_f32: the fused kernel is built for P = 64 and 128");
    hipStream_t st = (hipStream_t)stream;
    ConvGemmArgs a = bottleneck_args(0, x, w2, s2, b2, s3, b3, residual, y, s1n, b1n, y_next, B, H, W, P, stride, PN);
    // what fused_second_ok checks before the filters exist: non-null placeholders, then the real split planes
    a.Wt3 = w2; a.F_Wt3 = w3; a.G_Wt3 = PN > 0 ? w1n : nullptr;
    if (!odam_cg::fused_second_ok(a)) return odam_fail(4, "odam_op_bottleneck_f32: the fused kernel does not apply to this shape");
    unsigned short *d2 = nullptr, *d3 = nullptr, *d1 = nullptr;
    int rc = split_filters_for_call(w2, P, 9 * P, st, &d2, "odam_op_bottleneck_f32");
    if (!rc) rc = split_filters_for_call(w3, 4 * P, P, st, &d3, "odam_op_bottleneck_f32");
    if (!rc && PN > 0) rc = split_filters_for_call(w1n, PN, 4 * P, st, &d1, "odam_op_bottleneck_f32");
    if (!rc) {
        a.Wt3 = d2; a.F_Wt3 = d3; a.G_Wt3 = PN > 0 ? d1 : nullptr;
        rc = odam_cg::launch_conv_gemm(a, st);
    }
    (void)hipStreamSynchronize(st);
    if (d2) (void)hipFree(d2);
    if (d3) (void)hipFree(d3);
    if (d1) (void)hipFree(d1);
    return rc;
}

// ---- the stem from raw frames: a model of nothing but conv1, built for the call ----
extern "C" int odam_op_stem_u8(const unsigned char* rgb, int B, int h, int w, int H, int W, const float* conv1_w, const float* scale,
                               const float* bias, const float* mean, const float* std_dev, float* y, int* path, void* stream) {
    const char* who = "odam_op_stem_u8";
    if (!rgb || !conv1_w || !scale || !bias || !mean || !std_dev || !y) return fail(1, who, "null pointer");
    if (B < 1 || h < 1 || w < 1 || H < 32 || W < 32) return fail(1, who, "bad size");
    hipStream_t st = (hipStream_t)stream;
    odam_detr m{};
    m.cfg.img_h = H; m.cfg.img_w = W; m.cfg.max_batch = B;
    m.H1 = conv_out(H, 7, 2, 3); m.W1 = conv_out(W, 7, 2, 3);
    m.H2 = conv_out(m.H1, 3, 2, 1); m.W2 = conv_out(m.W1, 3, 2, 1);
    auto run = [&]() -> int {
        RC(pack_stem_rows(&m, conv1_w, 64, const_cast<float*>(scale), const_cast<float*>(bias)));
        if (!stem_rows_applies(&m, B)) return fail(4, who, "conv1 does not run as the row convolution here");
        RC(m.dev_alloc(&m.x4, (size_t)B * (H + 6) * (W + 8) * 16));
        RC(m.dev_alloc(&m.stem_out, (size_t)B * m.H1 * m.W1 * 64 * 4));
        m.bufA = reinterpret_cast<char*>(y);
        int p = 0;
        RC(stem_from_u8(&m, rgb, B, h, w, mean, std_dev, st, &p));
        if (path) *path = p;
        return 0;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    for (void* p : m.allocs) (void)hipFree(p);
    return rc;
}

extern "C" long long odam_op_conv_paths(char* buf, int n, int reset) { return odam_cg::read_paths(buf, n, reset); }

// experiment switch of the bf16-native contraction kernel (cg_choice.h set_big_mode): 0 off, 1 auto, 2 whenever eligible
extern "C" int odam_op_conv_bf16_mode(int mode) {
    if (mode < 0 || mode > 2) return odam_fail(1, "odam_op_conv_bf16_mode: mode must be 0, 1 or 2");
    odam_cg::set_big_mode(mode);      // = odam_config_set("cg.ring", mode)
    return 0;
}

// fp32 contraction mode of the 256-row kernel (cg_choice.h set_f32_mode): 0 fp32 matrix instruction on 128x128 tiles,
// 1 the same instruction in the ring kernel, 2 bf16 matrix instruction through the exact three-way split
extern "C" int odam_op_conv_f32_mode(int mode) {
    if (mode != 0 && mode != 2) return odam_fail(1, "odam_op_conv_f32_mode: mode must be 0 or 2");
    odam_cg::set_f32_mode(mode);
    return 0;
}

extern "C" int odam_op_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O,
                                 int ldo, int B, int H, int Lq, int Lk, void* stream) {
    return attention_op("odam_op_attention", ATT_NULLS, Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, 32, 0, nullptr, stream);
}

extern "C" int odam_op_attention_bf16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                                      int ldo, int B, int H, int Lq, int Lk, void* stream) {
    return attention_op("odam_op_attention_bf16", ATT_BF16, Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, 32, 1, nullptr, stream);
}

extern "C" int odam_op_attention_ex(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                    int B, int H, int Lq, int Lk, int head_dim, int dtype, const unsigned char* key_mask,
                                    void* stream) {
    return attention_op("odam_op_attention_ex", ATT_EX, Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, head_dim, dtype, key_mask, stream);
}

// the detector's attention at either head width (the model's own launcher and kernel choice)
extern "C" int odam_op_attention_hd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                    int B, int H, int Lq, int Lk, int head_dim, int dtype, const unsigned char* key_mask,
                                    void* stream) {
    return attention_op("odam_op_attention_hd", ATT_HD, Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, head_dim, dtype, key_mask, stream);
}

extern "C" int odam_op_add_layernorm(const float* x, const float* r, const float* gamma, const float* beta, float* y,
                                     int M, void* stream) {
    return layernorm_op("odam_op_add_layernorm", false, x, r, gamma, beta, y, nullptr, 1, nullptr, M, 256, 0, stream);
}

extern "C" int odam_op_add_layernorm_ex(const void* x, const void* r, const float* gamma, const float* beta, void* y,
                                        const float* pos, int L, void* y_pos, int M, int dtype, void* stream) {
    return layernorm_op("odam_op_add_layernorm_ex", true, x, r, gamma, beta, y, pos, L, y_pos, M, 256, dtype, stream);
}

extern "C" int odam_op_add_layernorm_c(const void* x, const void* r, const float* gamma, const float* beta, void* y,
                                       const float* pos, int L, void* y_pos, int M, int C, int dtype, void* stream) {
    return layernorm_op("odam_op_add_layernorm_c", true, x, r, gamma, beta, y, pos, L, y_pos, M, C, dtype, stream);
}

// ---- the kernels between the contractions: pooling, layouts, position add, convert, sigmoid, post-processing.  Every entry
// checks its arguments before any HIP call and then calls the launcher the forward calls ----
extern "C" int odam_op_maxpool3x3s2_nhwc_ex(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
    return maxpool_op("odam_op_maxpool3x3s2_nhwc_ex", x, y, B, H, W, C, dtype, stream);
}

extern "C" int odam_op_maxpool3x3s2_nhwc(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    return maxpool_op("odam_op_maxpool3x3s2_nhwc", x, y, B, H, W, C, 0, stream);
}

extern "C" int odam_op_nchw_to_nhwc4(const float* in, void* out, int B, int H, int W, int dtype, int framed, void* stream) {
    const char* who = "odam_op_nchw_to_nhwc4";
    if (!in || !out) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (B < 0 || H < 0 || W < 0) return fail(1, who, "negative extent");
    if (!B || !H || !W) return 0;
    return framed ? odam_dk::launch_nchw_to_nhwc4_framed(in, out, B, H, W, dtype, (hipStream_t)stream)
                  : odam_dk::launch_nchw_to_nhwc4(in, out, B, H, W, dtype, (hipStream_t)stream);
}

extern "C" int odam_op_nhwc_to_nchw(const void* in, float* out, int B, int H, int W, int C, int dtype, void* stream) {
    const char* who = "odam_op_nhwc_to_nchw";
    if (!in || !out) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (B < 0 || H < 0 || W < 0 || C < 0) return fail(1, who, "negative extent");
    return odam_dk::launch_nhwc_to_nchw(in, out, B, H, W, C, dtype, (hipStream_t)stream);
}

extern "C" int odam_op_add_pos(const void* x, const float* pos, int L, void* out, int M, int C, int dtype, void* stream) {
    const char* who = "odam_op_add_pos";
    if (!pos || !out) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (M < 0 || C < 0) return fail(1, who, "negative extent");
    if (C % 4) return fail(1, who, "C must be a multiple of 4");
    if (L <= 0) return fail(1, who, "L must be positive");
    if (!M || !C) return 0;
    return odam_dk::launch_add_pos(x, pos, L, out, M, dtype, (hipStream_t)stream, C);
}

extern "C" int odam_op_to_f32(const void* in, float* out, long long n, int dtype, void* stream) {
    const char* who = "odam_op_to_f32";
    if (!in || !out) return fail(1, who, "null pointer");
    if (dtype != 0 && dtype != 1) return fail(1, who, "dtype must be 0 (fp32) or 1 (bf16)");
    if (n < 0) return fail(1, who, "negative extent");
    if (n % 4) return fail(1, who, "n must be a multiple of 4");
    return odam_dk::launch_to_f32(in, out, (size_t)n, dtype, (hipStream_t)stream);
}

extern "C" int odam_op_sigmoid(float* x, int n, void* stream) {
    if (!x) return fail(1, "odam_op_sigmoid", "null pointer");
    if (n < 0) return fail(1, "odam_op_sigmoid", "negative extent");
    return odam_dk::launch_sigmoid(x, n, (hipStream_t)stream);
}

extern "C" int odam_op_postprocess(const float* logits, const float* boxes, const float* angle, const float* offset, const float* size,
                                   const float* depth, int n, int n_cls1, int n_bins, const float* K9, float img_w, float img_h,
                                   float* rows, void* stream) {
    const char* who = "odam_op_postprocess";
    if (!logits || !boxes || !angle || !offset || !size || !depth || !K9 || !rows) return fail(1, who, "null pointer");
    if (n < 0) return fail(1, who, "negative extent");
    if (n_cls1 < 2) return fail(1, who, "n_cls1 must be at least 2 (one class and no-object)");
    if (n_bins < 1) return fail(1, who, "n_bins must be at least 1");
    if (!n) return 0;
    return odam_dk::launch_postprocess(logits, boxes, angle, offset, size, depth, 1, n, n_cls1, n_bins, img_w, img_h, K9[0], K9[4],
                                       K9[2], K9[5], rows, (hipStream_t)stream);
}
