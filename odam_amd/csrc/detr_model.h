// detr_model.h -- the detector's host-side model and what its units (detr_weights / detr_forward / detr_ops / detr_input .hip) share.
// Reference (likojack/ODAM): src/models/detr.py:18-94 (DETR), src/models/backbone.py:21-110 (FrozenBN,
// ResNet body = torchvision ResNet v1.5 bottlenecks, stride on the 3x3), src/models/transformer.py
// (post-norm encoder/decoder), src/models/position_encoding.py (sine embedding, passed in precomputed).
// Layout: activations NHWC / [B*L, C] batch-major rows; every contraction runs on conv_gemm.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/odam_detr.h"
#include "cg_mx8.h"
#include "conv_gemm.h"
#include "odam_err.h"

namespace odam_dm {

struct HostTensor {
    std::vector<long long> shape;
    std::vector<float> data;
};

struct Conv {          // packed convolution / linear layer on device
    void* w = nullptr;       // [Cout][Kpad], fp32 or bf16
    void* w3 = nullptr;      // fp32 models: the same filters split into three bf16 planes (conv_gemm.h Wt3), or null
    float* scale = nullptr;  // [Cout] or null
    float* bias = nullptr;   // [Cout] or null
    int Cin = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0, Kpad = 0, dil = 1;
    int k_order = 0;         // conv_gemm.h: 1 = channel-chunk-major K (multi-tap filters with Cin % k-tile == 0)
    unsigned char* wq = nullptr;    // mxfp8 body layers: MXFP8 filters [Cout][Kpad] (k = tap * Cin + ci) and their scales
    unsigned char* wqs = nullptr;   //    [Cout][Kpad / 32] (cg_mx8.h); w is then null
};

struct Bottleneck {     // one residual block: Bottleneck c1 1x1, c2 3x3 (stride), c3 1x1 + residual; BasicBlock (odam_detr::basic)
    Conv c1, c2, c3, ds;   //   c1 3x3 (stride), c2 3x3 + residual, c3 unused
    bool has_ds = false;
};

struct LN { float* g = nullptr; float* b = nullptr; };

struct EncLayer { Conv qk, v, out, l1, l2; LN n1, n2; };
struct DecLayer { Conv qk, v, out, cq, cout, l1, l2; LN n1, n2, n3; };

inline int ilog2(int x) { int l = 0; while ((1 << l) < x) l++; return l; }
inline int conv_out(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }

// Optional per-launch timing (bench.py roofline): event pairs around the launches of one kind during a forward, read back
// by odam_detr_profile_read*.  Pair i brackets launch i; flops[i] is that launch's algorithmic work.
struct EventLog {
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<double> flops;
    size_t used = 0;               // events of the current forward (two per launch)

    // launch() -- bracketed by an event pair when timing is on.  The callable is a template parameter: a forward issues a few
    // hundred of these from the host, and nothing here may allocate per launch
    template <typename F>
    int timed(hipStream_t st, double fl, F&& launch) {
        if (!on) return launch();
        if (used + 2 > ev.size()) {
            for (int k = 0; k < 2; k++) {
                hipEvent_t e;
                ODAM_HIP(hipEventCreate(&e));
                ev.push_back(e);
            }
            flops.resize(ev.size() / 2);
        }
        flops[used / 2] = fl;
        ODAM_HIP(hipEventRecord(ev[used], st));
        const int rc = launch();
        ODAM_HIP(hipEventRecord(ev[used + 1], st));
        used += 2;
        return rc;
    }
    // *n / *ms / *fl = the launches whose first event lies in [lo, hi) (clipped to `used`), summed; waits for each to finish
    int sum(size_t lo, size_t hi, int* n, double* ms, double* fl) const {
        *n = 0; *ms = 0.0; *fl = 0.0;
        for (size_t i = lo; i < std::min(hi, used); i += 2) {
            ODAM_HIP(hipEventSynchronize(ev[i + 1]));
            float t = 0.0f;
            ODAM_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            *n += 1;
            *ms += t;
            *fl += flops[i / 2];
        }
        return 0;
    }
};

}  // namespace odam_dm

struct odam_detr {
    odam_detr_cfg cfg;
    std::map<std::string, odam_dm::HostTensor> host;
    bool finalized = false;
    std::vector<void*> allocs;

    odam_dm::Conv stem;
    bool basic = false;          // cfg.basic_block: the blocks are torchvision BasicBlocks
    int l4_ch = 2048;            // channels of the layer4 map (512 for BasicBlock bodies), from the packed weights
    std::vector<odam_dm::Bottleneck> blocks;
    std::vector<int> block_stride;
    odam_dm::Conv input_proj;
    std::vector<odam_dm::EncLayer> enc;
    std::vector<odam_dm::DecLayer> dec;
    odam_dm::Conv cross_k_all, cross_v_all;
    odam_dm::LN dec_norm;
    odam_dm::LN enc_norm;        // pre_norm only: the encoder's final LayerNorm (transformer.py:27-28)
    const void* memory_out = nullptr;      // where the last forward left the encoder's output (odam_detr_debug_read)
    odam_dm::Conv class_embed;
    odam_dm::Conv mlp[5][3];  // bbox, offset, angle, size, depth
    odam_dm::Conv stem_rows;     // conv1 as a 7x1 convolution over 32-float rows of the framed NHWC4 image (detr_forward.hip, stem)
    float* pos = nullptr;        // [L, hidden_dim]
    float* query_pos = nullptr;  // [Q, hidden_dim]

    // geometry
    int H1, W1, H2, W2, fh, fw, L;

    // workspace (activations: fp32 or bf16 according to cfg.dtype; sizes in bytes = elements * es)
    char *x4 = nullptr, *stem_out = nullptr, *bufA = nullptr, *bufB = nullptr, *t1 = nullptr, *t2 = nullptr,
         *dsb = nullptr;
    char *src = nullptr, *srcpos = nullptr, *qk = nullptr, *v = nullptr, *att = nullptr, *tmp = nullptr, *ffn = nullptr;
    char *kc = nullptr, *vc = nullptr;
    char *tgt = nullptr, *tgtpos = nullptr, *dqk = nullptr, *dv = nullptr, *datt = nullptr, *dq = nullptr,
         *dtmp = nullptr, *dffn = nullptr, *hs = nullptr, *h1 = nullptr, *h2 = nullptr;
    const char* layer4 = nullptr;  // where the last forward left the layer4 map (NHWC)
    int es = 4;                    // bytes per activation / weight element
    int dt = 0;                    // 0 fp32, 1 bf16 (also the mxfp8 mode's: everything outside the ResNet body runs as in bf16)
    bool mx = false;               // cfg.dtype 2: the body's convolutions on MXFP8 operands (cg_mx8.h)
    // mxfp8 workspace: block inputs / outputs (elements + scales; their bf16 forms live in bufA / bufB), the 1x1 reduce
    // and 3x3 outputs; the downsample output (a residual only) is bf16 in dsb
    unsigned char *qa = nullptr, *qas = nullptr, *qb = nullptr, *qbs = nullptr, *qt1 = nullptr, *qt1s = nullptr, *qt2 = nullptr,
                  *qt2s = nullptr;

    odam_dm::EventLog conv_ev;     // every conv_gemm / cg_mx8 launch of a forward
    odam_dm::EventLog att_ev;      // every fused attention launch
    size_t stage_ev[6] = {};       // conv_ev.used where the stem, layer1 .. layer4 and the rest (input_proj .. heads) began

    // input-transform resampling tables per (source length, output length): device [xmin | cnt | K]
    struct Resample { int* xmin; int* cnt; int* K; int ksize; };
    std::map<std::pair<int, int>, Resample> resample;

    // conv1 on raw uint8 frames (detr_forward.hip stem_from_u8, odam_config stem.u8): conv1's fp32 filters as loaded, and per (mean, std)
    // pair seen the integer centres and the folded, pre-split filters (detr_weights.hip stem_u8_filters)
    struct StemU8 { float mean[3], stdv[3]; int centre[3]; void* w3; };
    std::vector<float> conv1_w;
    std::vector<StemU8> stem_u8;
    float* u8_img = nullptr;       // where that path does not apply: the normalised fp32 image [max_batch, 3, img_h, img_w], allocated on first use

    template <typename T>
    int dev_alloc(T** p, size_t n) {
        ODAM_HIP(hipMalloc((void**)p, n * sizeof(T)));
        allocs.push_back((void*)*p);
        return 0;
    }
};

namespace odam_dm {

#define RC(call)                 \
    do {                         \
        int rc_ = (call);        \
        if (rc_) return rc_;     \
    } while (0)

// What every conv_gemm launch of layer `c` over an NHWC input x [B, H, W, c.Cin] has in common: operands, scale / bias,
// geometry (output size with dilation), K layout, M, ldc = Cout.  No residual, no ReLU, no output: the caller sets those.
odam_cg::ConvGemmArgs conv_args(const Conv& c, const void* x, int B, int H, int W, int dtype);
// the same for an mxfp8 body layer (cg_mx8.h); the caller sets the residual, the outputs and the ReLU
odam_mx::ConvArgs mx_args(const Conv& c, const void* x, const void* xs, int B, int H, int W);

// detr_weights.hip: conv1 [Cout][3][7][7] as the row-convolution stem (m->stem_rows); the filters of the uint8 stem for one (mean, std) pair
int pack_stem_rows(odam_detr* m, const float* w, int Cout, float* scale, float* bias);
int stem_u8_filters(odam_detr* m, const float* mean, const float* stdv, const odam_detr::StemU8** out);
// detr_input.hip: the two resampling tables of an h x w frame for this model's input size
int resample_tables(odam_detr* m, int h, int w, odam_detr::Resample* tx, odam_detr::Resample* ty);
// detr_forward.hip: conv1 + bn1 + ReLU + max-pool from raw uint8 frames [B, h, w, 3] into m->bufA [B, H2, W2, 64]: on the centred bf16 frame
// where that applies (*path = 1; path nullable), else through the normalised fp32 image and the stem as odam_detr_forward runs it (*path = 0)
int stem_from_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean, const float* stdv, hipStream_t st, int* path);
// ... and whether conv1 would run as the row convolution at all for B frames (the op-level entry has no other stem to fall back to)
bool stem_rows_applies(const odam_detr* m, int B);

// one layer on conv_gemm: y = act(conv(x) * scale + bias + res)
int run_conv(const Conv& c, const void* x, int B, int H, int W, const void* res, bool relu, void* y, hipStream_t st,
             int dtype = 0, int out_f32 = 0);

}  // namespace odam_dm
