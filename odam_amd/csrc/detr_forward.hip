// detr_forward.hip -- the detector's forward: the schedule of launches over the gfx950 kernels (conv_gemm / cg_mx8 /
// detr_kernels), stage by stage as the reference runs them (src/models/detr.py:59-94, backbone.py:59-94, transformer.py),
// and the optional per-launch timing that bench.py's roofline reads.
#include <hip/hip_runtime.h>

#include <atomic>

#include "detr_kernels.h"
#include "detr_model.h"
#include "odam_config.h"

using namespace odam_dm;
using odam_cg::ConvGemmArgs;

namespace odam_dm {

ConvGemmArgs conv_args(const Conv& c, const void* x, int B, int H, int W, int dtype) {
    ConvGemmArgs a{};
    a.dtype = dtype;
    a.A = x; a.Wt = c.w; a.Wt3 = c.w3; a.scale = c.scale; a.bias = c.bias;
    a.B = B; a.H = H; a.W = W; a.Cin = c.Cin; a.log2Cin = ilog2(c.Cin);
    a.Ho = conv_out(H, (c.KH - 1) * c.dil + 1, c.stride, c.pad); a.Wo = conv_out(W, (c.KW - 1) * c.dil + 1, c.stride, c.pad);
    a.Cout = c.Cout; a.KH = c.KH; a.KW = c.KW; a.stride = c.stride; a.pad = c.pad; a.Kpad = c.Kpad; a.dil = c.dil;
    a.k_order = c.k_order;
    a.M = B * a.Ho * a.Wo; a.ldc = c.Cout;
    return a;
}

odam_mx::ConvArgs mx_args(const Conv& c, const void* x, const void* xs, int B, int H, int W) {
    odam_mx::ConvArgs a{};
    a.x = (const unsigned char*)x; a.xs = (const unsigned char*)xs; a.w = c.wq; a.ws = c.wqs; a.scale = c.scale; a.bias = c.bias;
    a.B = B; a.H = H; a.W = W; a.Cin = c.Cin; a.Ho = conv_out(H, c.KH, c.stride, c.pad); a.Wo = conv_out(W, c.KW, c.stride, c.pad);
    a.Cout = c.Cout; a.KH = c.KH; a.KW = c.KW; a.stride = c.stride; a.pad = c.pad; a.Kpad = c.Kpad;
    a.M = B * a.Ho * a.Wo;
    return a;
}

int run_conv(const Conv& c, const void* x, int B, int H, int W, const void* res, bool relu, void* y, hipStream_t st, int dtype,
             int out_f32) {
    ConvGemmArgs a = conv_args(c, x, B, H, W, dtype);
    a.out_f32 = out_f32; a.res = res; a.C = y; a.relu = relu ? 1 : 0;
    if (c.KH * c.KW == 1 && (c.Cin & (c.Cin - 1))) {
        // one tap whose width is not a power of two (linears of a 192 / 320 / 384 ... wide transformer): the gather splits k into
        // tap and channel with a power-of-two Cin, so give it the next one -- k < Kpad = Cin stays inside tap 0 -- and the real
        // pixel stride in lda
        int p2 = 1;
        while (p2 < c.Cin) p2 <<= 1;
        a.Cin = p2; a.log2Cin = ilog2(p2); a.lda = c.Cin;
    }
    return odam_cg::launch_conv_gemm(a, st);
}

}  // namespace odam_dm

namespace {

// ---- the forward's launches: identical to the untimed ones, bracketed by events when profiling is on (EventLog::timed) ----
int conv_t(odam_detr* m, const Conv& c, const void* x, int B, int H, int W, const void* res, bool relu, void* y,
           hipStream_t st, int out_f32 = 0) {
    const int Ho = conv_out(H, (c.KH - 1) * c.dil + 1, c.stride, c.pad), Wo = conv_out(W, (c.KW - 1) * c.dil + 1, c.stride, c.pad);
    const int Cin_true = (c.KH == 7) ? 3 : c.Cin;  // the stem's 4th input channel is zero padding
    return m->conv_ev.timed(st, 2.0 * B * Ho * Wo * (double)c.Cout * c.KH * c.KW * Cin_true,
                            [&] { return run_conv(c, x, B, H, W, res, relu, y, st, m->dt, out_f32); });
}
int lin_t(odam_detr* m, const Conv& c, const void* x, int M, const void* res, bool relu, void* y, hipStream_t st,
          int out_f32 = 0) {
    return conv_t(m, c, x, 1, 1, M, res, relu, y, st, out_f32);
}

// A bottleneck's 3x3 (c2: 64 channels) and expand + residual + ReLU (c3: 256 channels) as ONE launch where the fused kernel
// of conv_gemm.hip applies (layer1 in fp32 split mode); returns -1 where it does not, and the caller runs the two layers
// next_c1 (nullable) + t_next: also the following bottleneck's 1x1 reduce on the tile, its output (the next 3x3's input) to
// t_next; *chained tells the caller whether that happened
int fused_c2c3_t(odam_detr* m, const Conv& c2, const Conv& c3, const void* x, int B, int H, int W, const void* res, void* y,
                 hipStream_t st, const Conv* next_c1, void* t_next, bool* chained) {
    *chained = false;
    if (m->basic) return -1;         // BasicBlock bodies have no expand layer: nothing of this applies
    if (c2.dil != 1) return -1;      // dilated 3x3 (the DC5 backbone's layer4): the separate launches
    if (c3.KH != 1 || c3.stride != 1 || c3.Kpad != c2.Cout) return -1;
    if (!m->dt && (!c2.w3 || !c3.w3)) return -1;
    ConvGemmArgs a = conv_args(c2, x, B, H, W, m->dt);
    a.relu = 1;
    a.F_scale = c3.scale; a.F_bias = c3.bias; a.F_res = (const float*)res; a.F_C = (float*)y;
    a.F_ldc = c3.Cout; a.F_relu = 1;
    // bf16: 3x3 + expand + residual (+ the next block's reduce where the channel combination is built) as one launch; fp32 the
    // same on the pre-split filters, the next reduce for 256 -> 64 / 128 channels
    const bool bf = m->dt != 0;
    auto fused_ok = [&] { return bf ? odam_cg::fused_bf16_ok(a) : odam_cg::fused_second_ok(a); };
    if (bf) a.F_Wt = c3.w; else a.F_Wt3 = c3.w3;
    const bool next_ok = next_c1 && t_next && next_c1->KH == 1 && next_c1->stride == 1 && next_c1->Kpad == c3.Cout &&
                         (bf || (next_c1->w3 && (next_c1->Cout == 64 || next_c1->Cout == 128) && c3.Cout == 256));
    if (next_ok) {
        if (bf) a.G_Wt = next_c1->w; else a.G_Wt3 = next_c1->w3;
        a.G_scale = next_c1->scale; a.G_bias = next_c1->bias; a.G_C = (float*)t_next; a.G_N = next_c1->Cout;
        *chained = fused_ok();
        if (!*chained) { a.G_Wt = a.G_Wt3 = nullptr; a.G_scale = a.G_bias = nullptr; a.G_C = nullptr; a.G_N = 64; }
    }
    if (!fused_ok()) return -1;
    const double flops3 = *chained ? 2.0 * a.M * (double)next_c1->Cout * c3.Cout : 0.0;
    return m->conv_ev.timed(st, 2.0 * a.M * ((double)c2.Cout * c2.KH * c2.KW * c2.Cin + (double)c3.Cout * c2.Cout) + flops3,
                            [&] { return odam_cg::launch_conv_gemm(a, st); });
}

std::atomic<long long> g_pooled_stem_launches{0};

// conv1 over the framed image (stem): the arguments conv_args cannot derive -- output width from the true image, pixel
// stride smaller than the row length.  Tries the max-pool on the tile (ConvGemmArgs::pool; the output then goes to
// `pooled_out` [B, H2, W2, 64] instead of stem_out); *pooled: whether it ran so
int stem_rows_t(odam_detr* m, int B, hipStream_t st, void* pooled_out, bool* pooled) {
    const Conv& c = m->stem_rows;
    ConvGemmArgs a = conv_args(c, m->x4, B, m->cfg.img_h + 6, m->cfg.img_w + 8, m->dt);
    a.lda = 4; a.Ho = m->H1; a.Wo = m->W1; a.M = B * a.Ho * a.Wo;
    a.relu = 1;
    // patches of 17 x 29 conv outputs = 8 x 14 pooled pixels (493 of the tile's 512 rows; 14 % of the conv recomputed at the seams)
    a.pool = 1; a.pool_ph = odam_cg::POOL_PH; a.pool_pw = odam_cg::POOL_PW; a.Hp = m->H2; a.Wp = m->W2; a.C = pooled_out;
    *pooled = odam_cg::pooled_stem_ok(a);
    if (!*pooled) { a.pool = 0; a.C = m->stem_out; }
    else g_pooled_stem_launches.fetch_add(1);
    return m->conv_ev.timed(st, 2.0 * a.M * (double)c.Cout * 147,      // the algorithmic products, not the 224 issued
                            [&] { return odam_cg::launch_conv_gemm(a, st); });
}

// conv1 on the centred uint8 frame in m->x4 (four bf16 per pixel, preprocess_u8_bf16x4_framed_kernel) with the folded filters w3: the
// row-convolution stem's geometry, the activations as one bf16 plane (ConvGemmArgs::a_bf16); pool: the max-pool on the tile, into bufA
ConvGemmArgs stem_u8_args(odam_detr* m, int B, const void* w3, bool pool) {
    ConvGemmArgs a = conv_args(m->stem_rows, m->x4, B, m->cfg.img_h + 6, m->cfg.img_w + 8, 0);
    a.Wt3 = w3; a.a_bf16 = 1;
    a.lda = 4; a.Ho = m->H1; a.Wo = m->W1; a.M = B * a.Ho * a.Wo;
    a.relu = 1; a.C = m->stem_out;
    if (pool) { a.pool = 1; a.pool_ph = odam_cg::POOL_PH; a.pool_pw = odam_cg::POOL_PW; a.Hp = m->H2; a.Wp = m->W2; a.C = m->bufA; }
    return a;
}

// an mxfp8 body layer: x / xs MXFP8 input, res bf16 (nullable); outputs y / ys MXFP8 and / or yb bf16 (nullable)
int mx_t(odam_detr* m, const Conv& c, const unsigned char* x, const unsigned char* xs, int B, int H, int W, const void* res, bool relu,
         unsigned char* y, unsigned char* ys, void* yb, hipStream_t st) {
    odam_mx::ConvArgs a = mx_args(c, x, xs, B, H, W);
    a.res = (const unsigned short*)res; a.relu = relu ? 1 : 0;
    a.y = y; a.ys = ys; a.yb = (unsigned short*)yb;
    return m->conv_ev.timed(st, 2.0 * a.M * (double)c.Cout * c.Kpad, [&] { return odam_mx::launch_conv(a, st); });
}

int att_t(odam_detr* m, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
          int B, int H, int Lq, int Lk, hipStream_t st, const unsigned char* key_mask = nullptr) {
    const int hd = m->cfg.hidden_dim / m->cfg.nheads;      // 32 or 64 (odam_detr_create)
    return m->att_ev.timed(st, 4.0 * B * H * (double)Lq * Lk * hd,   // QK^T + PV, 2 flop per MAC
                           [&] { return odam_dk::launch_attention(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Lq, Lk, m->dt, st, key_mask, hd); });
}

// ---- the stages of a forward --------------------------------------------------------------------------------

// the activation that runs through the ResNet body: the block input (NHWC, H x W) and the buffer the block writes
struct Act { char *cur, *nxt; int H, W; };

char* off(const odam_detr* m, char* p, size_t n) { return p + n * m->es; }   // element offset in the activation type

// per-stage profile: note where each ResNet stage's launches begin (odam_detr_profile_read_stages); i = the block about to run
void mark_stage(odam_detr* m, size_t i) {
    for (int l = 0, first = 0; l < 4; first += m->cfg.resnet_blocks[l], l++)
        if ((int)i == first) m->stage_ev[l + 1] = m->conv_ev.used;
}

// conv1 + bn1 + ReLU + max-pool (backbone.py:59-94): the pooled map [B, H2, W2, 64] is left in bufA
int stem(odam_detr* m, const float* img, int B, hipStream_t st) {
    // fp32, split contraction mode, enough rows to fill the device: conv1 on the ring kernel.  With Cin = 4 the 7x7
    // filter cannot use its gather (a k-tile must sit inside one tap), but seven consecutive NHWC4 pixels ARE 28
    // contiguous floats: over an image framed with zeros (3 rows above / below, 3 + 5 columns) conv1 is a 7x1
    // convolution with "Cin" = 32 floats per row, pixel stride lda = 4, no padding, K = 224 instead of 147 + pad --
    // a third of the products are zeros, on a path that is 2-3x faster than the 128x64 tiles of the fp32 instruction.
    const int dt = m->dt, ih = m->cfg.img_h, iw = m->cfg.img_w;
    bool pooled = false;
    if (stem_rows_applies(m, B)) {
        RC(odam_dk::launch_nchw_to_nhwc4_framed(img, m->x4, B, ih, iw, dt, st));
        RC(stem_rows_t(m, B, st, m->bufA, &pooled));
    } else {
        RC(odam_dk::launch_nchw_to_nhwc4(img, m->x4, B, ih, iw, dt, st));
        RC(conv_t(m, m->stem, m->x4, B, ih, iw, nullptr, true, m->stem_out, st));
    }
    if (!pooled) RC(odam_dk::launch_maxpool3x3s2(m->stem_out, m->bufA, B, m->H1, m->W1, 64, m->H2, m->W2, dt, st));
    return 0;
}

}  // namespace

namespace odam_dm {

bool stem_rows_applies(const odam_detr* m, int B) {
    const long Mst = (long)B * m->H1 * m->W1;
    const bool rows_mode = m->dt ? (m->stem_rows.w != nullptr && odam_cfg::get(odam_cfg::CG_RING) != 0)
                                 : (m->stem_rows.w3 != nullptr && odam_cg::f32_mode() == 2);
    return odam_cfg::get(odam_cfg::STEM_ROWS) != 0 && rows_mode && (Mst >= 192L * 256 || odam_cfg::get(odam_cfg::CG_PIN));
}

// The stem from raw frames.  Where the model is fp32 in split mode, conv1 runs as the row convolution, the framed row pitch is even
// (every stride-2 output's first pixel on a 16-byte boundary) and stem.u8 is on: ONE producer pass writes the centred integers as the
// framed bf16 image (8 bytes per pixel) and conv1 reads that with three products per block (conv_gemm_big_kernel MODE 5).  Otherwise
// the normalised fp32 image goes to a scratch of the model's and the stem runs as odam_detr_forward runs it: the same bits as
// odam_detr_preprocess_u8 + odam_detr_forward.
int stem_from_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean, const float* stdv, hipStream_t st, int* path) {
    const int ih = m->cfg.img_h, iw = m->cfg.img_w;
    odam_detr::Resample tx{}, ty{};
    RC(resample_tables(m, h, w, &tx, &ty));
    if (path) *path = 0;
    if (odam_cfg::get(odam_cfg::STEM_U8) != 0 && m->dt == 0 && !m->mx && (iw + 8) % 2 == 0 && !m->conv1_w.empty() && stem_rows_applies(m, B)) {
        // (a cheap test first -- the filters are built only where the kernel would take them)
        bool pooled = odam_cg::bf16_plane_ok(stem_u8_args(m, B, m->stem_rows.w3, true));
        if (pooled || odam_cg::bf16_plane_ok(stem_u8_args(m, B, m->stem_rows.w3, false))) {
            const odam_detr::StemU8* f = nullptr;
            RC(stem_u8_filters(m, mean, stdv, &f));
            RC(odam_dk::launch_preprocess_u8_bf16x4_framed(rgb, B, h, w, tx.xmin, tx.cnt, tx.K, tx.ksize, ty.xmin, ty.cnt, ty.K, ty.ksize,
                                                           m->x4, ih, iw, f->centre, st));
            const ConvGemmArgs a = stem_u8_args(m, B, f->w3, pooled);
            if (pooled) g_pooled_stem_launches.fetch_add(1);
            RC(m->conv_ev.timed(st, 2.0 * a.M * (double)a.Cout * 147, [&] { return odam_cg::launch_conv_gemm(a, st); }));
            if (!pooled) RC(odam_dk::launch_maxpool3x3s2(m->stem_out, m->bufA, B, m->H1, m->W1, 64, m->H2, m->W2, 0, st));
            if (path) *path = 1;
            return 0;
        }
    }
    if (!m->u8_img) RC(m->dev_alloc(&m->u8_img, (size_t)m->cfg.max_batch * 3 * ih * iw));
    RC(odam_dk::launch_preprocess_u8(rgb, B, h, w, tx.xmin, tx.cnt, tx.K, tx.ksize, ty.xmin, ty.cnt, ty.K, ty.ksize, m->u8_img, ih, iw, mean,
                                     stdv, st));
    return stem(m, m->u8_img, B, st);
}

}  // namespace odam_dm

namespace {

// mxfp8: every body convolution on MXFP8 operands, one launch per layer (cg_mx8.hip).  Block inputs / outputs are
// written in both forms -- MXFP8 (cq / cs, read by conv1 and the downsample) and bf16 (cur, read as the residual); the
// downsample output is bf16 only (a residual); layer4's last output only bf16 (input_proj reads it)
int body_mxfp8(odam_detr* m, int B, Act& s, hipStream_t st) {
    unsigned char *cq = m->qa, *cs = m->qas, *nq = m->qb, *ns = m->qbs;
    RC(odam_mx::launch_quantize(s.cur, 1, (size_t)B * s.H * s.W * 64, cq, cs, st));      // the pooled stem, bf16 in bufA
    for (size_t i = 0; i < m->blocks.size(); i++) {
        mark_stage(m, i);
        const Bottleneck& b = m->blocks[i];
        const int stride = m->block_stride[i];
        const int Ho = conv_out(s.H, 3, stride, 1), Wo = conv_out(s.W, 3, stride, 1);
        const bool last = i + 1 == m->blocks.size();
        unsigned char* oq = last ? nullptr : nq;
        unsigned char* os = last ? nullptr : ns;
        RC(mx_t(m, b.c1, cq, cs, B, s.H, s.W, nullptr, true, m->qt1, m->qt1s, nullptr, st));
        const char* res = s.cur;
        if (b.has_ds) {
            RC(mx_t(m, b.ds, cq, cs, B, s.H, s.W, nullptr, false, nullptr, nullptr, m->dsb, st));
            res = m->dsb;
        }
        if (m->basic) {
            RC(mx_t(m, b.c2, m->qt1, m->qt1s, B, Ho, Wo, res, true, oq, os, s.nxt, st));
        } else {
            RC(mx_t(m, b.c2, m->qt1, m->qt1s, B, s.H, s.W, nullptr, true, m->qt2, m->qt2s, nullptr, st));
            RC(mx_t(m, b.c3, m->qt2, m->qt2s, B, Ho, Wo, res, true, oq, os, s.nxt, st));
        }
        std::swap(s.cur, s.nxt); std::swap(cq, nq); std::swap(cs, ns);
        s.H = Ho; s.W = Wo;
    }
    return 0;
}

// BasicBlock: conv1 (3x3 / stride) + bn1 + ReLU -> t1; conv2 (3x3) + bn2 + identity or downsample + ReLU in conv2's epilogue
int body_basic(odam_detr* m, int B, Act& s, hipStream_t st) {
    for (size_t i = 0; i < m->blocks.size(); i++) {
        mark_stage(m, i);
        const Bottleneck& b = m->blocks[i];
        const int stride = m->block_stride[i];
        const int Ho = conv_out(s.H, 3, stride, 1), Wo = conv_out(s.W, 3, stride, 1);
        RC(conv_t(m, b.c1, s.cur, B, s.H, s.W, nullptr, true, m->t1, st));
        const char* res = s.cur;
        if (b.has_ds) {
            RC(conv_t(m, b.ds, s.cur, B, s.H, s.W, nullptr, false, m->dsb, st));
            res = m->dsb;
        }
        RC(conv_t(m, b.c2, m->t1, B, Ho, Wo, res, true, s.nxt, st));
        std::swap(s.cur, s.nxt);
        s.H = Ho; s.W = Wo;
    }
    return 0;
}

// Bottleneck: 1x1 reduce -> 3x3 (stride) -> 1x1 expand + identity or downsample + ReLU; the last two, and the next block's
// reduce, as one launch where fused_c2c3_t can
int body_bottleneck(odam_detr* m, int B, Act& s, hipStream_t st) {
    char* tin = m->t1;          // where this block's 1x1 reduce output lives (the 3x3's input)
    char* tout = m->t2;         // the other small buffer: the 3x3's output, or -- chained -- the NEXT block's reduce output
    bool have_c1 = false;       // the previous block's launch already computed this block's reduce
    for (size_t i = 0; i < m->blocks.size(); i++) {
        mark_stage(m, i);
        const Bottleneck& b = m->blocks[i];
        const int stride = m->block_stride[i];
        const int Ho = conv_out(s.H, 3, stride, 1), Wo = conv_out(s.W, 3, stride, 1);
        if (!have_c1) RC(conv_t(m, b.c1, s.cur, B, s.H, s.W, nullptr, true, tin, st));
        have_c1 = false;
        const char* res = s.cur;
        if (b.has_ds) {
            RC(conv_t(m, b.ds, s.cur, B, s.H, s.W, nullptr, false, m->dsb, st));
            res = m->dsb;
        }
        // the next block's reduce rides along where that block keeps the resolution and the channel counts (layer1's 2nd, 3rd)
        // (layer2's first reduce after layer1's last block included: a bottleneck's stride sits on its 3x3)
        const Conv* next_c1 = (i + 1 < m->blocks.size()) ? &m->blocks[i + 1].c1 : nullptr;
        bool chained = false;
        const int frc = fused_c2c3_t(m, b.c2, b.c3, tin, B, s.H, s.W, res, s.nxt, st, next_c1, tout, &chained);
        if (frc > 0) return frc;
        if (frc < 0) {
            RC(conv_t(m, b.c2, tin, B, s.H, s.W, nullptr, true, tout, st));
            RC(conv_t(m, b.c3, tout, B, Ho, Wo, res, true, s.nxt, st));
        } else if (chained) {
            std::swap(tin, tout);      // the next block reads its 3x3 input from where this launch put it
            have_c1 = true;
        }
        std::swap(s.cur, s.nxt);
        s.H = Ho; s.W = Wo;
    }
    return 0;
}

// encoder (transformer.py:154-188) over src / srcpos = src + pos; leaves the memory where m->memory_out says and
// memory + pos (the cross-attention keys' input) in srcpos.  Row r of the batch reads pos[r % Lp]
int encoder(odam_detr* m, int B, const float* pos, int Lp, const unsigned char* key_mask, hipStream_t st) {
    const int E = m->cfg.hidden_dim, Hh = m->cfg.nheads, dt = m->dt, L = m->L, M = B * L;
    for (const EncLayer& e : m->enc) {
        if (m->cfg.pre_norm) {
            // forward_pre (transformer.py:169-183): src2 = norm1(src); q = k = src2 + pos; src += attn(q, k, src2);
            //                                       src2 = norm2(src); src += linear2(relu(linear1(src2)))
            RC(odam_dk::launch_add_layernorm(m->src, nullptr, e.n1.g, e.n1.b, m->tmp, pos, Lp, m->srcpos, M, dt, st, E));
            RC(lin_t(m, e.qk, m->srcpos, M, nullptr, false, m->qk, st));
            RC(lin_t(m, e.v, m->tmp, M, nullptr, false, m->v, st));
            RC(att_t(m, m->qk, 2 * E, off(m, m->qk, E), 2 * E, m->v, E, m->att, E, B, Hh, L, L, st, key_mask));
            RC(lin_t(m, e.out, m->att, M, m->src, false, m->src, st));                  // residual added in place
            RC(odam_dk::launch_add_layernorm(m->src, nullptr, e.n2.g, e.n2.b, m->tmp, nullptr, L, nullptr, M, dt, st, E));
            RC(lin_t(m, e.l1, m->tmp, M, nullptr, true, m->ffn, st));
            RC(lin_t(m, e.l2, m->ffn, M, m->src, false, m->src, st));
            continue;
        }
        RC(lin_t(m, e.qk, m->srcpos, M, nullptr, false, m->qk, st));
        RC(lin_t(m, e.v, m->src, M, nullptr, false, m->v, st));
        RC(att_t(m, m->qk, 2 * E, off(m, m->qk, E), 2 * E, m->v, E, m->att, E, B, Hh, L, L, st, key_mask));
        RC(lin_t(m, e.out, m->att, M, m->src, false, m->tmp, st));
        RC(odam_dk::launch_add_layernorm(m->tmp, nullptr, e.n1.g, e.n1.b, m->src, nullptr, L, nullptr, M, dt, st, E));
        RC(lin_t(m, e.l1, m->src, M, nullptr, true, m->ffn, st));
        RC(lin_t(m, e.l2, m->ffn, M, m->src, false, m->tmp, st));
        RC(odam_dk::launch_add_layernorm(m->tmp, nullptr, e.n2.g, e.n2.b, m->src, pos, Lp, m->srcpos, M, dt, st, E));
    }
    m->memory_out = m->src;
    if (m->cfg.pre_norm) {      // memory = encoder.norm(src) (transformer.py:82-83), memory + pos for the cross-attention keys
        RC(odam_dk::launch_add_layernorm(m->src, nullptr, m->enc_norm.g, m->enc_norm.b, m->tmp, pos, Lp, m->srcpos, M, dt, st, E));
        m->memory_out = m->tmp;
    }
    return 0;
}

// the decoder's final norm (transformer.py:120-121) and the heads on its output (detr.py:73-88), fp32 in every mode
int heads(odam_detr* m, int B, float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
          float* obj_features, hipStream_t st) {
    const int E = m->cfg.hidden_dim, Q = m->cfg.num_queries, dt = m->dt, Mq = B * Q;
    // fp32 mode: the final norm can write straight into the caller's obj_features buffer
    void* hs = (obj_features && dt == 0) ? (void*)obj_features : (void*)m->hs;
    RC(odam_dk::launch_add_layernorm(m->tgt, nullptr, m->dec_norm.g, m->dec_norm.b, hs, nullptr, Q, nullptr, Mq, dt, st, E));
    if (obj_features && dt != 0) RC(odam_dk::launch_to_f32(m->hs, obj_features, (size_t)Mq * E, dt, st));
    RC(lin_t(m, m->class_embed, hs, Mq, nullptr, false, logits, st, 1));
    float* outs[5] = {boxes, offset, angle, size, depth};
    for (int k = 0; k < 5; k++) {
        RC(lin_t(m, m->mlp[k][0], hs, Mq, nullptr, true, m->h1, st));
        RC(lin_t(m, m->mlp[k][1], m->h1, Mq, nullptr, true, m->h2, st));
        RC(lin_t(m, m->mlp[k][2], m->h2, Mq, nullptr, false, outs[k], st, 1));
    }
    return odam_dk::launch_sigmoid(boxes, Mq * 4, st);
}

// where odam_detr_forward_aux puts every decoder layer's outputs: blocks [L][fpl][Q][.], layer l of frame b at (l * fpl + b) * Q * n
struct LayerOut { float *logits, *boxes, *angle, *offset, *size, *depth, *obj_features; int fpl; };

// norm + heads of decoder layer l (transformer.py:117-118: every intermediate goes through the decoder's final norm) into slot l:
// heads() as it stands, on the same B * Q rows, so that slot L-1 holds the bits of the plain forward
int layer_heads(odam_detr* m, int B, const LayerOut& o, size_t l, hipStream_t st) {
    const size_t row = l * (size_t)o.fpl * m->cfg.num_queries;
    return heads(m, B, o.logits + row * m->cfg.num_classes1, o.boxes + row * 4, o.angle + row * m->cfg.angle_bins, o.offset + row * 2,
                 o.size + row * 3, o.depth + row, o.obj_features ? o.obj_features + row * m->cfg.hidden_dim : nullptr, st);
}

// decoder layers (transformer.py:217-262) over the stacked cross-attention keys / values kc / vc; leaves their output in tgt.
// `each` (nullable): the heads run after every layer into that layer's slot (hs / h1 / h2 are no layer's own: reused on the one stream)
int decoder(odam_detr* m, int B, const unsigned char* key_mask, hipStream_t st, const LayerOut* each = nullptr) {
    const int E = m->cfg.hidden_dim, Hh = m->cfg.nheads, Q = m->cfg.num_queries, dt = m->dt, L = m->L, Mq = B * Q;
    ODAM_HIP(hipMemsetAsync(m->tgt, 0, (size_t)m->es * Mq * E, st));
    RC(odam_dk::launch_add_pos(nullptr, m->query_pos, Q, m->tgtpos, Mq, dt, st, E));
    const int ldkv = m->cfg.dec_layers * E;
    for (size_t i = 0; i < m->dec.size(); i++) {
        const DecLayer& d = m->dec[i];
        if (m->cfg.pre_norm) {
            // forward_pre (transformer.py:240-262): every sub-block normalises its INPUT and adds its output to tgt
            RC(odam_dk::launch_add_layernorm(m->tgt, nullptr, d.n1.g, d.n1.b, m->dtmp, m->query_pos, Q, m->tgtpos, Mq, dt, st, E));
            RC(lin_t(m, d.qk, m->tgtpos, Mq, nullptr, false, m->dqk, st));
            RC(lin_t(m, d.v, m->dtmp, Mq, nullptr, false, m->dv, st));
            RC(att_t(m, m->dqk, 2 * E, off(m, m->dqk, E), 2 * E, m->dv, E, m->datt, E, B, Hh, Q, Q, st));
            RC(lin_t(m, d.out, m->datt, Mq, m->tgt, false, m->tgt, st));
            RC(odam_dk::launch_add_layernorm(m->tgt, nullptr, d.n2.g, d.n2.b, m->dtmp, m->query_pos, Q, m->tgtpos, Mq, dt, st, E));
            RC(lin_t(m, d.cq, m->tgtpos, Mq, nullptr, false, m->dq, st));
            RC(att_t(m, m->dq, E, off(m, m->kc, i * E), ldkv, off(m, m->vc, i * E), ldkv, m->datt, E, B, Hh, Q, L, st, key_mask));
            RC(lin_t(m, d.cout, m->datt, Mq, m->tgt, false, m->tgt, st));
            RC(odam_dk::launch_add_layernorm(m->tgt, nullptr, d.n3.g, d.n3.b, m->dtmp, nullptr, Q, nullptr, Mq, dt, st, E));
            RC(lin_t(m, d.l1, m->dtmp, Mq, nullptr, true, m->dffn, st));
            RC(lin_t(m, d.l2, m->dffn, Mq, m->tgt, false, m->tgt, st));
            if (each) RC(layer_heads(m, B, *each, i, st));
            continue;
        }
        RC(lin_t(m, d.qk, m->tgtpos, Mq, nullptr, false, m->dqk, st));
        RC(lin_t(m, d.v, m->tgt, Mq, nullptr, false, m->dv, st));
        RC(att_t(m, m->dqk, 2 * E, off(m, m->dqk, E), 2 * E, m->dv, E, m->datt, E, B, Hh, Q, Q, st));
        RC(lin_t(m, d.out, m->datt, Mq, m->tgt, false, m->dtmp, st));
        RC(odam_dk::launch_add_layernorm(m->dtmp, nullptr, d.n1.g, d.n1.b, m->tgt, m->query_pos, Q, m->tgtpos, Mq, dt, st, E));
        RC(lin_t(m, d.cq, m->tgtpos, Mq, nullptr, false, m->dq, st));
        RC(att_t(m, m->dq, E, off(m, m->kc, i * E), ldkv, off(m, m->vc, i * E), ldkv, m->datt, E, B, Hh, Q, L, st, key_mask));
        RC(lin_t(m, d.cout, m->datt, Mq, m->tgt, false, m->dtmp, st));
        RC(odam_dk::launch_add_layernorm(m->dtmp, nullptr, d.n2.g, d.n2.b, m->tgt, nullptr, Q, nullptr, Mq, dt, st, E));
        RC(lin_t(m, d.l1, m->tgt, Mq, nullptr, true, m->dffn, st));
        RC(lin_t(m, d.l2, m->dffn, Mq, m->tgt, false, m->dtmp, st));
        RC(odam_dk::launch_add_layernorm(m->dtmp, nullptr, d.n3.g, d.n3.b, m->tgt, m->query_pos, Q, m->tgtpos, Mq, dt, st, E));
        if (each) RC(layer_heads(m, B, *each, i, st));
    }
    return 0;
}

struct RawFrames { const unsigned char* rgb; int h, w; const float *mean, *stdv; };      // odam_detr_forward_u8: the stem reads these, not img

// key_mask / pos_b: null for same-size batches (no padding: the mask is all false and one position table serves every
// image).  Otherwise key_mask [B][L] marks padded tokens (backbone.py:79) and pos_b [B][L][E] is each image's own sine
// embedding, which depends on its mask (position_encoding.py:26-46).
int forward_impl(odam_detr* m, const float* img, int B, const unsigned char* key_mask, const float* pos_b,
                 float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
                 float* obj_features, void* stream, int frames_per_layer = 0, const RawFrames* raw = nullptr) {
    if (!m || (!img && !raw) || !logits || !boxes || !angle || !offset || !size || !depth)
        return odam_fail(1, "odam_detr_forward: null pointer");
    if (!m->finalized) return odam_fail(1, "odam_detr_forward: call odam_detr_finalize first");
    if (B < 1 || B > m->cfg.max_batch) return odam_fail(3, "odam_detr_forward: batch outside 1..max_batch");
    hipStream_t st = (hipStream_t)stream;
    m->conv_ev.used = m->att_ev.used = 0;

    // ---- backbone (backbone.py:59-94) ----
    if (raw) RC(stem_from_u8(m, raw->rgb, B, raw->h, raw->w, raw->mean, raw->stdv, st, nullptr));
    else RC(stem(m, img, B, st));
    std::fill(m->stage_ev, m->stage_ev + 6, m->conv_ev.used);
    m->stage_ev[0] = 0;
    Act s{m->bufA, m->bufB, m->H2, m->W2};
    RC(m->mx ? body_mxfp8(m, B, s, st) : m->basic ? body_basic(m, B, s, st) : body_bottleneck(m, B, s, st));
    m->layer4 = s.cur;
    m->stage_ev[5] = m->conv_ev.used;

    // ---- input_proj + positions (detr.py:70), encoder, the cross-attention keys / values of every decoder layer ----
    const int E = m->cfg.hidden_dim, M = B * m->L;
    RC(conv_t(m, m->input_proj, s.cur, B, s.H, s.W, nullptr, false, m->src, st));
    const float* pos = pos_b ? pos_b : m->pos;
    const int Lp = pos_b ? M : m->L;
    RC(odam_dk::launch_add_pos(m->src, pos, Lp, m->srcpos, M, m->dt, st, E));
    RC(encoder(m, B, pos, Lp, key_mask, st));
    RC(lin_t(m, m->cross_k_all, m->srcpos, M, nullptr, false, m->kc, st));
    RC(lin_t(m, m->cross_v_all, m->memory_out, M, nullptr, false, m->vc, st));

    // ---- decoder + heads ----
    if (frames_per_layer > 0) {      // every layer's heads inside the decoder, the last layer's included (slot L-1)
        const LayerOut each{logits, boxes, angle, offset, size, depth, obj_features, frames_per_layer};
        return decoder(m, B, key_mask, st, &each);
    }
    RC(decoder(m, B, key_mask, st));
    return heads(m, B, logits, boxes, angle, offset, size, depth, obj_features, st);
}

}  // namespace

extern "C" int odam_detr_forward(odam_detr* m, const float* img, int B, float* logits, float* boxes, float* angle,
                                 float* offset, float* size, float* depth, float* obj_features, void* stream) {
    return forward_impl(m, img, B, nullptr, nullptr, logits, boxes, angle, offset, size, depth, obj_features, stream);
}

extern "C" int odam_detr_forward_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean, const float* stdv,
                                    float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
                                    float* obj_features, void* stream) {
    if (!rgb || !mean || !stdv) return odam_fail(1, "odam_detr_forward_u8: null pointer");
    if (h < 1 || w < 1) return odam_fail(1, "odam_detr_forward_u8: bad size");
    const RawFrames raw{rgb, h, w, mean, stdv};
    return forward_impl(m, nullptr, B, nullptr, nullptr, logits, boxes, angle, offset, size, depth, obj_features, stream, 0, &raw);
}

extern "C" int odam_detr_forward_masked(odam_detr* m, const float* img, int B, const unsigned char* key_mask,
                                        const float* pos, float* logits, float* boxes, float* angle, float* offset,
                                        float* size, float* depth, float* obj_features, void* stream) {
    if (!key_mask || !pos) return odam_fail(1, "odam_detr_forward_masked: null mask / position table");
    return forward_impl(m, img, B, key_mask, pos, logits, boxes, angle, offset, size, depth, obj_features, stream);
}

extern "C" int odam_detr_forward_aux(odam_detr* m, const float* img, int B, const unsigned char* key_mask, const float* pos,
                                     float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
                                     float* obj_features, int frames_per_layer, void* stream) {
    if (!m || !img || !logits || !boxes || !angle || !offset || !size || !depth) return odam_fail(1, "odam_detr_forward_aux: null pointer");
    if ((key_mask == nullptr) != (pos == nullptr))
        return odam_fail(1, "odam_detr_forward_aux: mask and position table go together (both null for a same-size batch)");
    if (frames_per_layer < 1 || frames_per_layer < B) return odam_fail(1, "odam_detr_forward_aux: frames_per_layer below the batch");
    if (!m->finalized) return odam_fail(1, "odam_detr_forward_aux: call odam_detr_finalize first");
    return forward_impl(m, img, B, key_mask, pos, logits, boxes, angle, offset, size, depth, obj_features, stream, frames_per_layer);
}

extern "C" int odam_detr_debug_read(odam_detr* m, int B, float* layer4_nchw, float* memory, void* stream) {
    if (!m || !m->finalized || !m->layer4) return odam_fail(1, "odam_detr_debug_read: no forward has run");
    hipStream_t st = (hipStream_t)stream;
    if (layer4_nchw) RC(odam_dk::launch_nhwc_to_nchw(m->layer4, layer4_nchw, B, m->fh, m->fw, m->l4_ch, m->dt, st));
    if (memory) RC(odam_dk::launch_to_f32(m->memory_out ? m->memory_out : m->src, memory, (size_t)B * m->L * m->cfg.hidden_dim, m->dt, st));
    return 0;
}

extern "C" int odam_detr_postprocess(odam_detr* m, const float* logits, const float* boxes, const float* angle,
                                     const float* offset, const float* size, const float* depth, int B,
                                     const float* K9, float img_w, float img_h, float* rows, void* stream) {
    if (!m || !logits || !boxes || !angle || !offset || !size || !depth || !K9 || !rows)
        return odam_fail(1, "odam_detr_postprocess: null pointer");
    return odam_dk::launch_postprocess(logits, boxes, angle, offset, size, depth, B, m->cfg.num_queries,
                                       m->cfg.num_classes1, m->cfg.angle_bins, img_w, img_h, K9[0], K9[4], K9[2],
                                       K9[5], rows, (hipStream_t)stream);
}

extern "C" long long odam_op_pooled_stem_launches(void) { return g_pooled_stem_launches.load(); }

// ---- per-launch timing of the contraction and attention kernels (roofline measurement) ------------------------
extern "C" int odam_detr_profile_enable(odam_detr* m, int on) {
    if (!m) return odam_fail(1, "odam_detr_profile_enable: null model");
    m->conv_ev.on = m->att_ev.on = on != 0;
    m->conv_ev.used = m->att_ev.used = 0;
    return 0;
}

extern "C" int odam_detr_profile_read(odam_detr* m, int* n_launches, double* total_ms, double* total_flops) {
    if (!m || !n_launches || !total_ms || !total_flops) return odam_fail(1, "odam_detr_profile_read: null argument");
    return m->conv_ev.sum(0, m->conv_ev.used, n_launches, total_ms, total_flops);
}

extern "C" int odam_detr_profile_read_stages(odam_detr* m, int n, int* launches, double* ms, double* flops) {
    if (!m || n < 6 || !launches || !ms || !flops) return odam_fail(1, "odam_detr_profile_read_stages: null argument or n < 6");
    for (int s = 0; s < 6; s++)      // stage s: the launches from where it began to where the next one did
        RC(m->conv_ev.sum(s ? m->stage_ev[s] : 0, s < 5 ? m->stage_ev[s + 1] : m->conv_ev.used, &launches[s], &ms[s], &flops[s]));
    return 0;
}

extern "C" int odam_detr_profile_read_attention(odam_detr* m, int* n_launches, double* total_ms, double* total_flops) {
    if (!m || !n_launches || !total_ms || !total_flops) return odam_fail(1, "odam_detr_profile_read_attention: null argument");
    return m->att_ev.sum(0, m->att_ev.used, n_launches, total_ms, total_flops);
}
